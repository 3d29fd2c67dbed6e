"""Pins tests/learner_reference.py (the float64 restatements the GPU learner-kernel tests compare against) to the modules
and optimiser it restates, on the CPU: the history and privileged encoders against the ActorCritic modules cast to
float64, GAE against the reference's known-answer fixture and the CPU port's recurrence, clip + Adam against
nn.utils.clip_grad_norm_ + torch.optim.Adam in float64."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import golden_procedure as gp
import learner_reference as lr
from wbc_amd.rsl_rl.modules import ActorCritic
from wbc_amd.rsl_rl.storage import RolloutStorage

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_reference.npz"))


@pytest.fixture(scope="module")
def ac64():
    torch.manual_seed(1)
    return copy.deepcopy(ActorCritic(76, 76, 18, **gp.POLICY_KW)).double()


def test_encoders_match_the_modules_in_float64(ac64):
    g = torch.Generator().manual_seed(0)
    obs = 2.0 * torch.randn(301, 860, generator=g, dtype=torch.float64)
    with torch.no_grad():
        hist_mod = ac64.actor.history_encoder(obs[:, 100:].reshape(-1, 10, 76))
        priv_mod = ac64.actor.priv_encoder(obs[:, 76:100])
        hist = lr.hist_latent(lr.hist_weights(ac64), obs)
        priv = lr.priv_latent(lr.priv_weights(ac64), obs)
    assert hist.dtype == priv.dtype == torch.float64 and hist.shape == priv.shape == (301, 20)
    assert (hist - hist_mod).abs().max().item() < 1e-12
    assert (priv - priv_mod).abs().max().item() < 1e-12
    assert hist.std().item() > 0.05 and priv.std().item() > 0.05          # not a saturated / constant output


def test_gae_matches_the_reference_known_answer():
    rew, val, dones, last = gp.gae_known_answer_inputs()
    ret, adv = lr.gae(rew.numpy(), val.numpy(), dones.numpy(), last.numpy(), 0.99, 0.95)
    np.testing.assert_allclose(ret, GOLD["gae_returns"], rtol=1e-6, atol=1e-6)
    z, _, _ = lr.normalize(adv)
    np.testing.assert_allclose(z, GOLD["gae_advantages"], rtol=1e-5, atol=1e-6)
    n, s, q = lr.gae_stats(adv)
    assert n == 16 and s == pytest.approx(adv.sum(), abs=1e-15) and q == pytest.approx((adv ** 2).sum(), rel=1e-15)


@pytest.mark.parametrize("N,T,lam", [(37, 24, 0.95), (5, 1, 1.0), (64, 40, 0.95)])
def test_gae_matches_the_cpu_port(N, T, lam):
    g = torch.Generator().manual_seed(N * T)
    rew = 0.05 * torch.randn(T, N, 2, generator=g)
    val = torch.randn(T, N, 2, generator=g)
    dones = (torch.rand(T, N, 1, generator=g) < 0.1).to(torch.uint8)
    last = torch.randn(N, 2, generator=g)
    st = RolloutStorage(N, T, [3], [None], [1])
    st.rewards.copy_(rew); st.values.copy_(val); st.dones.copy_(dones)
    st._compute_returns_torch(last, 0.99, lam)
    ret, adv = lr.gae(rew.numpy(), val.numpy(), dones.numpy(), last.numpy(), 0.99, lam)
    # the port runs in float32: each of the T steps rounds a few values of the size of the return
    tol = 8 * T * 2.0 ** -24 * (np.abs(ret).max() + 1)
    assert np.abs(st.returns.numpy() - ret).max() <= tol
    if N * T > 1:
        z, _, _ = lr.normalize(adv)
        assert np.abs(st.advantages.numpy() - z).max() <= tol / adv.std() * 4


def test_rollout_store_matches_the_eager_process_env_step():
    g = torch.Generator().manual_seed(2)
    n = 300
    rew, arm, values = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, 2, generator=g)
    to = torch.rand(n, generator=g) < 0.3
    dones = torch.randint(-1, 3, (n,), generator=g)
    eager = torch.stack([rew.clone(), arm.clone()], -1)             # PPO.process_env_step's unfused branch (PPO:133-134)
    eager += 0.99 * torch.squeeze(values * to.unsqueeze(1), 1)
    r, d = lr.rollout_store(rew.numpy(), arm.numpy(), dones.numpy(), to.numpy(), values.numpy(), 0.99)
    assert np.abs(eager.numpy() - r).max() <= 2 * 2.0 ** -24 * (np.abs(r).max() + 1)
    np.testing.assert_array_equal(d, (dones != 0).numpy().astype(np.uint8))
    r32 = lr.rollout_store_fp32(rew.numpy(), arm.numpy(), to.numpy(), values.numpy(), 0.99)
    assert np.abs(r32.astype(np.float64) - r).max() <= 2.0 ** -23 * (np.abs(r).max() + 1)
    np.testing.assert_array_equal(lr.rollout_store_fp32(rew.numpy(), arm.numpy(), None, values.numpy(), 0.99),
                                  torch.stack([rew, arm], -1).numpy())


@pytest.mark.parametrize("clip_active", [True, False])
@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clip_adam_matches_torch(clip_active, t, grad_scale):
    g = torch.Generator().manual_seed(t + int(clip_active))
    shapes = [(64, 24), (64,), (20, 64), (20,), (18,)]
    params = [torch.nn.Parameter(0.1 * torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    grads = [1e-2 * torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    flat_g = torch.cat([x.reshape(-1) for x in grads]).numpy()
    norm = grad_scale * np.linalg.norm(flat_g)
    max_norm = 0.5 * norm if clip_active else 2.0 * norm
    m0 = [1e-3 * torch.randn(s, generator=g, dtype=torch.float64) for s in shapes] if t > 1 else [torch.zeros(s, dtype=torch.float64) for s in shapes]
    v0 = [1e-5 * torch.rand(s, generator=g, dtype=torch.float64) for s in shapes] if t > 1 else [torch.zeros(s, dtype=torch.float64) for s in shapes]
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs]).numpy()     # noqa: E731
    p_ref, g_ref, m_ref, v_ref, n_ref = lr.clip_adam(flat(params), flat_g, flat(m0), flat(v0), t, 1e-3, max_norm, grad_scale=grad_scale)
    assert n_ref == pytest.approx(norm, rel=1e-14)
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for p, gr, m, v in zip(params, grads, m0, v0):
        p.grad = gr.clone() * grad_scale                               # the 1 / world_size division the kernels fold in
        if t > 1:
            opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    assert np.abs(flat([p.grad for p in params]) - g_ref).max() <= 1e-15
    assert np.abs(flat([opt.state[p]["exp_avg"] for p in params]) - m_ref).max() <= 1e-16
    assert np.abs(flat([opt.state[p]["exp_avg_sq"] for p in params]) - v_ref).max() <= 1e-18
    assert np.abs(flat(params) - p_ref).max() <= 1e-15
    assert float(opt.state[params[0]]["step"]) == t
    assert (np.abs(g_ref) < np.abs(flat_g) * grad_scale).all() if clip_active else np.array_equal(g_ref, flat_g * grad_scale)


def test_clip_adam_without_clip_keeps_the_scaled_gradient():
    g = np.linspace(-3.0, 3.0, 101)
    for max_norm in (0.0, -1.0):
        _, g_out, _, _, norm = lr.clip_adam(np.zeros(101), g, np.zeros(101), np.zeros(101), 1, 1e-3, max_norm, grad_scale=0.5)
        assert np.array_equal(g_out, 0.5 * g) and norm == pytest.approx(0.5 * math.sqrt((g * g).sum()), rel=1e-15)
