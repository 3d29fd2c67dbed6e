"""The learner-side HIP kernels, each through its C-ABI, against the float64 restatements of tests/learner_reference.py
(pinned on the CPU by tests/test_learner_reference.py), at the dispatch edges where they could go wrong unnoticed:

  wbc_hist_latent     one group per workgroup up to 512 groups of 24 rows, a persistent 768-workgroup grid above
                      (idle workgroups, a second 1-row group, the cross-group prefetch); guard rows past `rows`
  wbc_priv_latent     the same row counts
  wbc_gae_compute     2N around the 256-lane block, T = 1, dones at the first / last step, the fp64 statistics buffer
   + _normalize       and its workspace bound, the grid-stride normalisation beyond 2048 x 256 elements
  wbc_rollout_store   ragged n, no time-outs, done values other than 0 / 1
  wbc_ppo_clip_adam   clip active / inactive / off, grad_scale, bias correction at t = 1000, the recomputed norm
  wbc_hist_clip_adam  the same, with the norm from wbc_hist_train_grad's squares or recomputed after a reduction

u = 2^-24 (float32 unit round-off) below. Each bound is derived from the operation; the docstrings give the largest
error measured on the MI355X as a fraction of that bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_procedure as gp
import learner_reference as lr
from wbc_amd.native import check, lib
from wbc_amd.rsl_rl.modules import ActorCritic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_reference.npz"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _new_ac(seed=1):
    torch.manual_seed(seed)
    return ActorCritic(76, 76, 18, **gp.POLICY_KW).to(DEV)


def _hist_params(ac):
    he = ac.actor.history_encoder
    return [he.encoder[0].weight, he.encoder[0].bias, he.conv_layers[0].weight, he.conv_layers[0].bias,
            he.conv_layers[2].weight, he.conv_layers[2].bias, he.linear_output[0].weight, he.linear_output[0].bias]


def _priv_params(ac):
    pe = ac.actor.priv_encoder
    return [pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias]


def _table(ps):
    return (C.c_void_p * len(ps))(*[p.data_ptr() for p in ps])


# ---------------------------------------------------------------------------------------------------------------------
# history / privileged encoder latents
# 12288 rows = 512 groups: the last one-group-per-workgroup launch; 12289: the first persistent one (513 groups on 768
# workgroups, 255 idle); 18432 = 768 groups: one each; 18433: workgroup 0 takes a second, 1-row group; 163840: the rows of
# one PPO update at the bench shape.
HIST_ROWS = [1, 23, 24, 25, 12288, 12289, 18432, 18433, 40960, 163840]
GUARD = 48


@pytest.fixture(scope="module")
def enc():
    ac = _new_ac()
    g = torch.Generator(device=DEV).manual_seed(11)
    obs = torch.randn(max(HIST_ROWS), 860, generator=g, device=DEV)
    return dict(ac=ac, obs=obs, hw=lr.hist_weights(ac), pw=lr.priv_weights(ac))


def _run_latent(fn, ps, obs, rows):
    out = torch.full((rows + GUARD, 20), float("nan"), device=DEV)
    check(fn(_table(ps), obs.data_ptr(), out.data_ptr(), rows, _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out[rows:]).all(), "a write past the last row"
    return out[:rows]


@pytest.mark.parametrize("rows", HIST_ROWS)
def test_hist_and_priv_latent_match_fp64(enc, rows):
    """Both latents vs float64 at |err| <= 2e-6 + 1e-5 |ref| (the bound of test_fused_history_encoder_matches_torch, here
    against fp64 instead of the fp32 modules). The fp32 chains are 76 + 120 + 40 + 30 (history) and 24 + 64 (privileged)
    products deep with O(1) activations: a few hundred u. Achieved on MI355X over all ten row counts: history 2.3e-7 abs
    (0.068 of the bound), privileged 5.1e-7 abs (0.13)."""
    obs = enc["obs"][:rows]
    L = lib()
    for fn, ps, ref_fn, w in ((L.wbc_hist_latent, _hist_params(enc["ac"]), lr.hist_latent, enc["hw"]),
                              (L.wbc_priv_latent, _priv_params(enc["ac"]), lr.priv_latent, enc["pw"])):
        got = _run_latent(fn, ps, obs, rows).double()
        ref = ref_fn(w, obs)
        excess = ((got - ref).abs() - (2e-6 + 1e-5 * ref.abs())).max().item()
        assert excess <= 0.0, (fn.__name__, rows, (got - ref).abs().max().item())
        del got, ref


@pytest.mark.parametrize("rows,shift", [(163840, 7), (40960, 13), (12288, 5)])
def test_hist_latent_does_not_depend_on_row_position(enc, rows, shift):
    """Within one launch variant a row's latent is the same bits wherever it sits: rolling the input rows by a shift that is
    not a multiple of 24 moves every row to another group and slot (and, in the persistent grid, across the cross-group
    prefetch) and must roll the outputs bit for bit."""
    L = lib()
    ps = _hist_params(enc["ac"])
    obs = enc["obs"][:rows]
    a = _run_latent(L.wbc_hist_latent, ps, obs, rows)
    b = _run_latent(L.wbc_hist_latent, ps, torch.roll(obs, shift, 0).contiguous(), rows)
    assert torch.equal(torch.roll(a, shift, 0), b)


# ---------------------------------------------------------------------------------------------------------------------
# GAE: wbc_gae_compute, a copy of the raw advantages, wbc_gae_normalize
SENTINEL = -1.2345e300


def _gae_kernel(rew, val, dones, last, gamma, lam):
    T, N = rew.shape[0], rew.shape[1]
    L = lib()
    nws = L.wbc_gae_workspace_doubles(N)
    ws = torch.full((nws + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    r, v, lv = (torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV) for x in (rew, val, last))
    d = torch.from_numpy(np.ascontiguousarray(dones, np.uint8)).to(DEV)
    ret = torch.full((T * N * 2 + 64,), float("nan"), device=DEV)
    adv = torch.full((T * N * 2 + 64,), float("nan"), device=DEV)
    s = _stream()
    check(lib().wbc_gae_compute(r.data_ptr(), v.data_ptr(), d.data_ptr(), lv.data_ptr(), ret.data_ptr(), adv.data_ptr(), ws.data_ptr(),
                                T, N, float(gamma), float(lam), s), "wbc_gae_compute")
    raw = adv.clone()
    stats = ws[:3].clone()
    check(L.wbc_gae_normalize(adv.data_ptr(), ws.data_ptr(), T * N * 2, s), "wbc_gae_normalize")
    torch.cuda.synchronize()
    n = T * N * 2
    assert (ws[nws:] == SENTINEL).all(), "workspace written past wbc_gae_workspace_doubles(N)"
    for buf in (ret, raw, adv):
        assert torch.isnan(buf[n:]).all(), "a write past T * N * 2"
    shape = (T, N, 2)
    return (ret[:n].view(shape).cpu().numpy().astype(np.float64), raw[:n].view(shape).cpu().numpy().astype(np.float64),
            stats.cpu().numpy(), adv[:n].view(shape).cpu().numpy().astype(np.float64), (nws - 3) // 2)


def _check_normalized(z, raw, T, nblocks):
    """The normalisation of the kernel's own fp32 advantages vs float64. The one-pass variance (q - s^2 / n) / (n - 1) in
    float64 loses K 2^-53 (1 + mean^2 / var) relatively (K: the sums' depth, T + 8 + nblocks); the fp32 (a - mean_f32) inv
    adds u |mean| / std (the rounded mean), u |a - mean| / std and one rounding of z."""
    ref, mean, std = lr.normalize(raw)
    var_rel = (T + 8 + nblocks + 4) * 2.0 ** -53 * (1 + mean * mean / max(std * std, 1e-300))
    bound = 2 * (U * (abs(mean) + 2 * np.abs(raw - mean)) / (std + 1e-8) + np.abs(ref) * (var_rel + 2 * U))
    err = np.abs(z - ref)
    assert (err <= bound).all(), (err.max(), (err / bound).max())


def _dones(kind, T, N, rng):
    d = np.zeros((T, N), np.uint8)
    if kind == "all":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "last":
        d[T - 1] = 1
    elif kind == "random":
        d = (rng.random((T, N)) < 0.03).astype(np.uint8)
    return d


@pytest.mark.parametrize("N,T", [(1, 1), (1, 40), (127, 5), (128, 5), (129, 5), (4096, 40), (8192, 40)])
@pytest.mark.parametrize("kind", ["none", "all", "first", "last", "random"])
@pytest.mark.parametrize("lam", [0.95, 1.0])
def test_gae_matches_fp64(N, T, kind, lam):
    """Returns and raw advantages vs the float64 recurrence: each of T steps rounds a few fp32 values no larger than
    M = max|r| + 2 max|v| + max|ret|, and the error carries over with factor gamma lam <= 1: bound 4 T u M. The statistics
    (count, sum a, sum a^2) vs correctly rounded float64 sums of the kernel's own fp32 advantages: 1e-12 of sum |a| and of
    sum a^2 (the kernel's fixed-order fp64 sums are (T + 8 + blocks) 2^-53 deep). 8192 x 40 is 655360 elements: the
    normalisation's grid-stride loop takes a second pass. Achieved on MI355X over the 70 cases: returns and raw
    advantages 0.18 of the bound (1.6e-6 abs), sum a exact, sum a^2 5e-16 relative, normalised 0.42 of its bound."""
    rng = np.random.default_rng(N * 1000 + T + (kind == "random"))
    rew = 0.05 * rng.standard_normal((T, N, 2))
    val = rng.standard_normal((T, N, 2))
    last = rng.standard_normal((N, 2))
    dones = _dones(kind, T, N, rng)
    rew, val, last = (x.astype(np.float32) for x in (rew, val, last))
    ret, raw, stats, z, nblocks = _gae_kernel(rew, val, dones, last, 0.99, lam)
    g32 = float(np.float32(0.99))
    ret_ref, adv_ref = lr.gae(rew, val, dones, last, g32, float(np.float32(lam)))
    M = np.abs(rew).max() + 2 * max(np.abs(val).max(), np.abs(last).max()) + np.abs(ret_ref).max()
    bound = 4 * T * U * M
    assert np.abs(ret - ret_ref).max() <= bound, np.abs(ret - ret_ref).max() / bound
    assert np.abs(raw - adv_ref).max() <= bound + U * np.abs(adv_ref).max()
    n, s, q = lr.gae_stats(raw)
    assert stats[0] == n == 2 * T * N
    assert abs(stats[1] - s) <= 1e-12 * np.abs(raw).sum()
    assert abs(stats[2] - q) <= 1e-12 * q
    _check_normalized(z, raw, T, nblocks)


def test_gae_kernel_matches_the_reference_known_answer():
    """The reference's own 4-step x 2-env fixture (GOLD gae_returns / gae_advantages), on the kernel."""
    rew, val, dones, last = gp.gae_known_answer_inputs()
    ret, _, _, z, _ = _gae_kernel(rew.numpy(), val.numpy(), dones.numpy().reshape(4, 2), last.numpy(), 0.99, 0.95)
    np.testing.assert_allclose(ret, GOLD["gae_returns"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(z, GOLD["gae_advantages"], rtol=1e-5, atol=1e-6)


def test_gae_constant_advantages_normalise_to_zero():
    """Every step terminal, values 0: the advantage is the reward, here one constant. Its fp64 sums are exact, so the mean
    is the constant and (a - mean) is 0; whatever variance the one-pass formula leaves, the result is 0, finite."""
    T, N = 8, 300
    rew = np.full((T, N, 2), 0.37, np.float32)
    ret, raw, stats, z, _ = _gae_kernel(rew, np.zeros_like(rew), np.ones((T, N), np.uint8), np.zeros((N, 2), np.float32), 0.99, 0.95)
    assert (raw == np.float32(0.37)).all()
    assert np.isfinite(z).all() and (z == 0.0).all()


def test_gae_large_common_offset_normalises():
    """Advantages 50 + 0.01 N(0, 1): the one-pass variance cancels mean^2 / var = 2.5e7 of its magnitude in float64, and the
    float32 mean alone is off by up to u 50 = 3e-6, i.e. 3e-4 of a standard deviation (see _check_normalized).
    Achieved on MI355X: 1.9e-4 abs, 0.32 of the bound."""
    T, N = 40, 4096
    rng = np.random.default_rng(9)
    rew = (50.0 + 0.01 * rng.standard_normal((T, N, 2))).astype(np.float32)
    _, raw, _, z, nblocks = _gae_kernel(rew, np.zeros_like(rew), np.ones((T, N), np.uint8), np.zeros((N, 2), np.float32), 0.99, 0.95)
    ref, mean, std = lr.normalize(raw)
    assert 49.9 < mean < 50.1 and 0.009 < std < 0.011
    _check_normalized(z, raw, T, nblocks)
    assert abs(z.mean()) < 1e-3 and abs(z.std(ddof=1) - 1.0) < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# rollout store
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
@pytest.mark.parametrize("with_time_outs", [True, False])
def test_rollout_store_matches_process_env_step(n, with_time_outs):
    """Against the formula of PPO.process_env_step evaluated in float32 in the kernel's order: bit-exact. (Not bit-exact
    against the eager two-rounding order r + fl(gamma (v t)): hipcc contracts the kernel's r += gamma * (v * t) into one
    fused multiply-add, 1 ulp apart at most -- checked as such.) Done values 2 and -1 store as 1."""
    g = torch.Generator(device=DEV).manual_seed(n)
    rew, arm = torch.randn(n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)
    values = torch.randn(n, 2, generator=g, device=DEV)
    dones = torch.tensor([0, 1, 2, -1], device=DEV)[torch.randint(0, 4, (n,), generator=g, device=DEV)].contiguous()
    to = (torch.rand(n, generator=g, device=DEV) < 0.3) if with_time_outs else None
    out_r = torch.full((n + 64, 2), float("nan"), device=DEV)
    out_d = torch.full((n + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    check(lib().wbc_rollout_store(rew.data_ptr(), arm.data_ptr(), dones.data_ptr(), to.data_ptr() if to is not None else None,
                                  values.data_ptr(), 0.99, out_r.data_ptr(), out_d.data_ptr(), n, _stream()), "wbc_rollout_store")
    torch.cuda.synchronize()
    assert torch.isnan(out_r[n:]).all() and (out_d[n:] == 0xAB).all()
    got = out_r[:n].cpu().numpy()
    to_np = to.cpu().numpy() if to is not None else None
    np.testing.assert_array_equal(got, lr.rollout_store_fp32(rew.cpu().numpy(), arm.cpu().numpy(), to_np, values.cpu().numpy(), 0.99))
    r64, d = lr.rollout_store(rew.cpu().numpy(), arm.cpu().numpy(), dones.cpu().numpy(), to_np, values.cpu().numpy(), 0.99)
    np.testing.assert_array_equal(out_d[:n].cpu().numpy(), d)
    scale = np.abs(np.stack([rew.cpu().numpy(), arm.cpu().numpy()], -1)).astype(np.float64)
    if to is not None:
        scale += 0.99 * np.abs(values.cpu().numpy()) * to_np[:, None]
    assert (np.abs(got - r64) <= 2 * U * scale).all()
    eager = torch.stack([rew.clone(), arm.clone()], -1)
    if to is not None:
        eager += 0.99 * torch.squeeze(values * to.unsqueeze(1), 1)
    eager = eager.cpu().numpy()
    gap = np.spacing(np.abs(eager))
    if to is not None:
        gap = gap + np.spacing(np.abs(np.float32(0.99) * values.cpu().numpy() * to_np[:, None]))    # the rounding fl(gamma (v t))
    assert (np.abs(got - eager) <= gap).all()


# ---------------------------------------------------------------------------------------------------------------------
# clip + Adam
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3


def _adam_case(nparam, clip, grad_scale, t, g_flat, seed):
    """Moments for step t (zero at t = 1) and the max_norm of the case, from the norm of the scaled gradient."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    if t == 1:
        m, v = torch.zeros(nparam, device=DEV), torch.zeros(nparam, device=DEV)
    else:
        m = 1e-3 * torch.randn(nparam, generator=gen, device=DEV)
        v = 1e-5 * torch.rand(nparam, generator=gen, device=DEV) + 1e-9
    norm = grad_scale * g_flat.double().norm().item()
    max_norm = {"active": 0.5 * norm, "inactive": 2.0 * norm, "off": 0.0}[clip]
    return m, v, max_norm


def _check_adam(p_new, g_new, m_new, v_new, p0, g0, m0, v0, t, max_norm, grad_scale, clip):
    """Kernel vs lr.clip_adam with the moments at the float32 betas the C-ABI receives and the bias corrections at the
    caller's float64 betas (ppo.py computes step_size and bc2_sqrt in double). That is not exactly torch.optim.Adam: the
    kernels' 1 - beta2 is 1 - fl32(0.999) = 0.00099998713 where torch's fp32 step uses fl32(1 - 0.999), so at t = 1 the
    kernels' step is 6.4e-6 longer relatively (a fraction that decays with t). Bounds per element, from the fp32
    operations: the clip coefficient (an fp32 sum of squares <= 40 deep, sqrt, divide) <= 24 u relative, exact without
    clip (scale 1 or 0.5, coefficient 1: achieved bit-exact); m, v: a few u of their terms; the step: the errors of m / (sqrt(v) / bc2 + eps)
    and of the fp32 step_size; the parameter: one more rounding. The check is |err| <= 2 x that."""
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    p_ref, g_ref, m_ref, v_ref, _ = lr.clip_adam(p0, g0, m0, v0, t, LR, max_norm, beta1=b1, beta2=b2, eps=EPS, grad_scale=grad_scale,
                                                 bias_betas=(B1, B2))
    cg = 48 if clip == "active" else 0
    err_g = cg * U * np.abs(g_ref)
    err_m = (1 - b1) * err_g + 4 * U * (np.abs(m0) + (1 - b1) * np.abs(g_ref) + np.abs(m_ref))
    err_v = 2 * (1 - b2) * np.abs(g_ref) * err_g + 4 * U * (np.abs(v0) + (1 - b2) * g_ref * g_ref + np.abs(v_ref))
    bc2 = np.sqrt(1 - B2 ** t)
    step_size = LR / (1 - B1 ** t)
    sv = np.sqrt(v_ref)
    denom = sv / bc2 + EPS
    err_denom = np.divide(err_v, 2 * sv, out=np.zeros_like(sv), where=sv > 0) / bc2 + 3 * U * denom
    step = step_size * m_ref / denom
    err_p = step_size * (err_m / denom + np.abs(m_ref) * err_denom / denom ** 2) + 4 * U * np.abs(step) + U * np.abs(p_ref)
    ratios = []
    for name, got, ref, err in (("grad", g_new, g_ref, err_g), ("exp_avg", m_new, m_ref, err_m), ("exp_avg_sq", v_new, v_ref, err_v),
                                ("param", p_new, p_ref, err_p)):
        d = np.abs(got - ref)
        assert (d <= 2 * err).all(), (name, d.max(), (d / np.maximum(2 * err, 1e-300)).max())
        ratios.append((d / np.maximum(2 * err, 1e-300)).max())
    moved = np.abs(p_ref - p0)
    assert moved.max() > 0.1 * LR                      # a real step was taken
    return ratios


@pytest.mark.parametrize("clip", ["active", "inactive", "off"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("t", [1, 1000])
def test_ppo_clip_adam_matches_fp64(clip, grad_scale, t):
    """wbc_ppo_clip_adam on the policy's 33 parameters (fused_param_table layout), synthetic flat gradient, sq_partials =
    None (the norm recomputed by ppo_sqnorm_kernel). Achieved on MI355X, with the clip + Adam cases of the history
    encoder below: gradient 0.033, exp_avg 0.10, exp_avg_sq 0.12, parameters 0.49 of the (2 x) bounds of _check_adam."""
    L = lib()
    ac = _new_ac()
    params = ac.fused_params()
    nparam = sum(p.numel() for p in params)
    ng = L.wbc_ppo_grad_floats()
    assert nparam == ng - 3
    gen = torch.Generator(device=DEV).manual_seed(100 + t)
    g = 1e-2 * torch.randn(nparam, generator=gen, device=DEV)
    grad = torch.zeros(ng, device=DEV)
    grad[:nparam] = g
    m, v, max_norm = _adam_case(nparam, clip, grad_scale, t, g, 200 + t)
    p0 = torch.cat([p.detach().reshape(-1) for p in params]).double().cpu().numpy()
    g0, m0, v0 = (x.double().cpu().numpy() for x in (g, m, v))
    ws = torch.empty(int(L.wbc_ppo_clip_adam_workspace_floats()), device=DEV)
    check(L.wbc_ppo_clip_adam(ac.fused_param_table(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), max_norm, B1, B2, EPS,
                              LR / (1 - B1 ** t), (1 - B2 ** t) ** 0.5, grad_scale, None, ws.data_ptr(), _stream()), "wbc_ppo_clip_adam")
    torch.cuda.synchronize()
    p_new = torch.cat([p.detach().reshape(-1) for p in params]).double().cpu().numpy()
    _check_adam(p_new, grad[:nparam].double().cpu().numpy(), m.double().cpu().numpy(), v.double().cpu().numpy(), p0, g0, m0, v0, t,
                max_norm, grad_scale, clip)


@pytest.mark.parametrize("clip", ["active", "inactive", "off"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("reduced", [0, 1])
def test_hist_clip_adam_matches_fp64(clip, grad_scale, t, reduced):
    """wbc_hist_clip_adam on the history encoder's 8 tensors. grad_was_reduced = 0: the gradient and the squares the norm
    reads are the ones a preceding wbc_hist_train_grad left; 1: a synthetic gradient whose squares hist_sq_kernel
    recomputes. Achieved on MI355X: see test_ppo_clip_adam_matches_fp64 (the figures cover both kernels)."""
    L = lib()
    ac = _new_ac()
    hp = _hist_params(ac)
    nparam = sum(p.numel() for p in hp)
    ng = L.wbc_hist_train_grad_floats()
    assert nparam == ng - 1
    grad = torch.zeros(ng, device=DEV)
    ws = torch.empty(L.wbc_hist_train_workspace_floats(), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(300 + t)
    if reduced:
        grad[:nparam] = 1e-2 * torch.randn(nparam, generator=gen, device=DEV)
    else:
        rows = 2000
        obs = torch.randn(rows, 860, generator=gen, device=DEV)
        target = torch.randn(rows, 20, generator=gen, device=DEV)
        idx = torch.arange(rows, device=DEV)
        check(L.wbc_hist_train_grad(_table(hp), obs.data_ptr(), target.data_ptr(), idx.data_ptr(), rows, ws.data_ptr(), grad.data_ptr(),
                                    _stream()), "wbc_hist_train_grad")
    torch.cuda.synchronize()
    g = grad[:nparam].clone()
    assert g.abs().max().item() > 0
    m, v, max_norm = _adam_case(nparam, clip, grad_scale, t, g, 400 + t)
    p0 = torch.cat([p.detach().reshape(-1) for p in hp]).double().cpu().numpy()
    g0, m0, v0 = (x.double().cpu().numpy() for x in (g, m, v))
    check(L.wbc_hist_clip_adam(_table(hp), grad.data_ptr(), m.data_ptr(), v.data_ptr(), max_norm, B1, B2, EPS, LR / (1 - B1 ** t),
                               (1 - B2 ** t) ** 0.5, grad_scale, reduced, ws.data_ptr(), _stream()), "wbc_hist_clip_adam")
    torch.cuda.synchronize()
    p_new = torch.cat([p.detach().reshape(-1) for p in hp]).double().cpu().numpy()
    _check_adam(p_new, grad[:nparam].double().cpu().numpy(), m.double().cpu().numpy(), v.double().cpu().numpy(), p0, g0, m0, v0, t,
                max_norm, grad_scale, clip)
