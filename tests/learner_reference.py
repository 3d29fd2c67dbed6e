"""Plain float64 restatements of the learner-side operations the HIP kernels implement, for the tests. Nothing here calls
a project module on the compute path: torch is used as an fp64 array library (CPU or GPU), numpy for the scans.

  hist_latent          StateHistoryEncoder, tsteps = 10 (AC:39-84)       <-> wbc_hist_latent   (csrc/wbc_hist_kernel.hip)
  priv_latent          privileged encoder 24 -> 64 -> 20 (AC:129-141)    <-> wbc_priv_latent   (csrc/wbc_hist_train_kernel.hip)
  gae / normalize      RolloutStorage.compute_returns (RS:136-150)       <-> wbc_gae_compute + wbc_gae_normalize
  rollout_store        PPO.process_env_step's bootstrap + done cast      <-> wbc_rollout_store (csrc/wbc_gae_kernel.hip)
  clip_adam            clip_grad_norm_ + Adam.step (PPO:243-246)         <-> wbc_ppo_clip_adam / wbc_hist_clip_adam
  policy_act           ActorCritic forward, sampling, log-density        <-> wbc_policy_act    (csrc/wbc_policy_kernel.hip)
  ppo_minibatch        the gradient of one PPO.update minibatch          <-> wbc_ppo_minibatch_grad (csrc/wbc_ppo_kernel.hip)
  hist_train           the gradient of one PPO.update_dagger minibatch   <-> wbc_hist_train_grad (csrc/wbc_hist_train_kernel.hip)
  kink_free_batch      PPO minibatch inputs no row of which is near a kink of the piecewise losses

The two gradient functions run float64 autograd over the restated forward and read the gradient dZ at every layer's
pre-activation off the tape: the weight gradient is then formed here as dZ^T A, next to its element-wise error scale
S = |dZ|^T |A| -- the sum of the absolute values of the terms of each element's sum over the rows, which is what the
float32 round-off of that sum, in any order, is proportional to.
"""
import math

import numpy as np
import torch

HIST_OFF, PRIV_OFF, N_PROP, T_HIST = 100, 76, 76, 10


def _elu(x):
    return torch.where(x > 0, x, torch.expm1(x))


def hist_weights(ac, device=None):
    """The eight history-encoder tensors in the kernels' table order, as float64."""
    he = ac.actor.history_encoder
    ps = [he.encoder[0].weight, he.encoder[0].bias, he.conv_layers[0].weight, he.conv_layers[0].bias,
          he.conv_layers[2].weight, he.conv_layers[2].bias, he.linear_output[0].weight, he.linear_output[0].bias]
    return [p.detach().to(device=device or p.device, dtype=torch.float64) for p in ps]


def priv_weights(ac, device=None):
    pe = ac.actor.priv_encoder
    ps = [pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias]
    return [p.detach().to(device=device or p.device, dtype=torch.float64) for p in ps]


def hist_latent(w, obs, rec=None):
    """obs [B, >= 860] -> [B, 20]: Linear 76->30 + ELU per step; Conv1d 30->20 (k4 s2) + ELU; Conv1d 20->10 (k2 s1) + ELU;
    channel-major flatten; Linear 30->20 + ELU. The convolutions are written out as sums over (tap, channel).
    rec(layer, A, z) -> z, if given, sees every pre-activation z with the input A it was formed from (hist_train's tape)."""
    rec = rec or (lambda layer, a, z: z)
    enc_w, enc_b, c1_w, c1_b, c2_w, c2_b, lin_w, lin_b = w
    x = obs[:, HIST_OFF:HIST_OFF + T_HIST * N_PROP].to(torch.float64).reshape(-1, T_HIST, N_PROP)
    h1 = _elu(rec(0, x, x @ enc_w.T + enc_b))                                                 # [B, 10, 30]
    h2 = torch.stack([rec(1, h1[:, 2 * l:2 * l + 4], torch.einsum("bkc,ock->bo", h1[:, 2 * l:2 * l + 4], c1_w) + c1_b) for l in range(4)], 1)
    h2 = _elu(h2)                                                                             # [B, 4, 20]
    h3 = torch.stack([rec(2, h2[:, l:l + 2], torch.einsum("bkc,ock->bo", h2[:, l:l + 2], c2_w) + c2_b) for l in range(3)], 1)
    h3 = _elu(h3)                                                                             # [B, 3 positions, 10 channels]
    flat = h3.permute(0, 2, 1).reshape(-1, 30)                                                # index = channel * 3 + position
    return _elu(rec(3, flat, flat @ lin_w.T + lin_b))


def priv_latent(w, obs):
    w0, b0, w1, b1 = w
    x = obs[:, PRIV_OFF:PRIV_OFF + 24].to(torch.float64)
    return _elu(_elu(x @ w0.T + b0) @ w1.T + b1)


def gae(rewards, values, dones, last_values, gamma, lam):
    """RS:136-149 in float64. rewards, values [T, N, 2]; dones [T, N] or [T, N, 1] (any integer values: not_terminal =
    1 - done as in the reference); last_values [N, 2]. Returns (returns, advantages = returns - values), un-normalised."""
    r = np.asarray(rewards, np.float64)
    v = np.asarray(values, np.float64)
    d = np.asarray(dones, np.float64).reshape(r.shape[0], r.shape[1], 1)
    ret = np.empty_like(r)
    adv = np.zeros_like(r[0])
    next_v = np.asarray(last_values, np.float64)
    for t in range(r.shape[0] - 1, -1, -1):
        nt = 1.0 - d[t]
        delta = r[t] + nt * gamma * next_v - v[t]
        adv = delta + nt * gamma * lam * adv
        ret[t] = adv + v[t]
        next_v = v[t]
    return ret, ret - v


def gae_stats(adv):
    """(count, sum a, sum a^2) of an advantage array, in float64 (math.fsum: correctly rounded sums)."""
    a = np.asarray(adv, np.float64).ravel()
    return np.array([float(a.size), math.fsum(a), math.fsum(a * a)])


def normalize(adv):
    """RS:150: (a - mean) / (std + 1e-8), unbiased std, two-pass in float64."""
    a = np.asarray(adv, np.float64)
    mean = a.mean()
    std = math.sqrt(math.fsum(((a - mean) ** 2).ravel()) / (a.size - 1))
    return (a - mean) / (std + 1e-8), mean, std


def rollout_store(rew, arm_rew, dones, time_outs, values, gamma):
    """PPO.process_env_step (PPO:129-141): rewards [n, 2] = (rew, arm_rew) + gamma * values * time_out (float64), dones cast
    to 0 / 1 as RolloutStorage.add_transitions does (RS:70-72)."""
    r = np.stack([np.asarray(rew, np.float64), np.asarray(arm_rew, np.float64)], -1)
    if time_outs is not None:
        r = r + gamma * np.asarray(values, np.float64) * np.asarray(time_outs, np.float64)[:, None]
    return r, (np.asarray(dones) != 0).astype(np.uint8)


def rollout_store_fp32(rew, arm_rew, time_outs, values, gamma):
    """The same bootstrap evaluated in float32, in the fused kernel's operation order: t = v * time_out (exact for a 0 / 1
    time-out), then ONE rounding of r + gamma_f32 * t (the kernel's fused multiply-add). gamma_f32 * t is exact in
    float64 (24 x 24 bits) and the float64 sum rounds once more before the cast, so this equals the fused multiply-add
    except when that sum lands exactly on a float32 tie (probability ~2^-29 per element)."""
    g32 = np.float64(np.float32(gamma))
    r = np.stack([np.asarray(rew, np.float32), np.asarray(arm_rew, np.float32)], -1).astype(np.float64)
    if time_outs is not None:
        t = np.asarray(values, np.float32).astype(np.float64) * np.asarray(time_outs, np.float64)[:, None]
        r = r + g32 * t
    return r.astype(np.float32)


def clip_adam(param, grad, exp_avg, exp_avg_sq, step, lr, max_norm, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, bias_betas=None):
    """One nn.utils.clip_grad_norm_ + torch.optim.Adam.step (no weight decay, no amsgrad) on flat float64 arrays, `step` =
    the step number t after the increment. grad_scale is folded in first, as the kernels document it (the 1 / world_size
    of a SUM all-reduce): the norm is that of the scaled gradient. max_norm <= 0 means no clipping (the kernels'
    convention; clip_grad_norm_ itself would zero the gradient). Returns (param, grad after scale and clip, exp_avg,
    exp_avg_sq, total_norm). bias_betas: the (beta1, beta2) of the bias corrections, if not the moments' ones."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (param, grad, exp_avg, exp_avg_sq))
    g = g * grad_scale
    norm = math.sqrt(math.fsum(g * g))
    if max_norm > 0:
        g = g * min(max_norm / (norm + 1e-6), 1.0)
    m = m + (g - m) * (1.0 - beta1)                       # exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    c1, c2 = bias_betas or (beta1, beta2)
    step_size = lr / (1.0 - c1 ** step)
    denom = np.sqrt(v) / math.sqrt(1.0 - c2 ** step) + eps
    return p - step_size * m / denom, g, m, v, norm


# ---------------------------------------------------------------------------------------------------------------------
# policy inference and the two fused gradient kernels
U32 = 2.0 ** -24                                       # float32 unit round-off
N_LEG, HALF_LOG_2PI = 12, 0.5 * math.log(2.0 * math.pi)
# the 16 Linear layers in the kernels' table order (struct PolicyParams): index l -> weight 2 l, bias 2 l + 1 of `w`
POLICY_LAYERS = ("actor.priv_encoder.0", "actor.priv_encoder.2", "actor.actor_backbone.0",
                 "actor.actor_leg_control_head.0", "actor.actor_leg_control_head.2", "actor.actor_leg_control_head.4",
                 "actor.actor_arm_control_head.0", "actor.actor_arm_control_head.2", "actor.actor_arm_control_head.4",
                 "critic.critic_backbone.0",
                 "critic.critic_leg_control_head.0", "critic.critic_leg_control_head.2", "critic.critic_leg_control_head.4",
                 "critic.critic_arm_control_head.0", "critic.critic_arm_control_head.2", "critic.critic_arm_control_head.4")


def policy_weights(ac, device=None):
    """(w, std): the 32 weight / bias tensors of POLICY_LAYERS and std [18], as float64."""
    sd = dict(ac.named_parameters())
    cast = lambda p: p.detach().to(device=device or p.device, dtype=torch.float64)     # noqa: E731
    w = []
    for name in POLICY_LAYERS:
        w += [cast(sd[name + ".weight"]), cast(sd[name + ".bias"])]
    return w, cast(sd["std"]).reshape(-1)


def policy_grad_floats(w):
    return sum(x.numel() for x in w) + 18 + 3


def _ident(x):
    return x


def _policy_net(layer, x, latent=None):
    """The network's wiring (AC:204-217, 281-286), for any layer(l, input, activation) -> output whose tensors keep the
    features in the last dimension. x [..., 100] = proprioception 76 + privileged 24. Returns mean [..., 18], values
    [..., 2] and the latent [..., 20] the actor backbone saw."""
    lat = layer(1, layer(0, x[..., PRIV_OFF:PRIV_OFF + 24], _elu), _elu) if latent is None else latent
    trunk = layer(2, torch.cat([x[..., :N_PROP], lat], -1), _elu)
    ctrunk = layer(9, x, _elu)
    heads = [layer(l0 + 2, layer(l0 + 1, layer(l0, t, _elu), _elu), last)
             for l0, t, last in ((3, trunk, torch.tanh), (6, trunk, torch.tanh), (10, ctrunk, _ident), (13, ctrunk, _ident))]
    return torch.cat(heads[:2], -1), torch.cat(heads[2:], -1), lat


def _log_prob2(mean, std, actions):
    """Normal(mean, std).log_prob(actions) summed over the 12 leg and the 6 arm dimensions (AC:341-345) -> [B, 2]."""
    lp = -((actions - mean) ** 2) / (2.0 * std * std) - torch.log(std) - HALF_LOG_2PI
    return torch.stack([lp[:, :N_LEG].sum(-1), lp[:, N_LEG:].sum(-1)], -1)


def policy_act(w, std, obs, eps, latent=None):
    """obs [B, >= 100], eps [B, 18] standard normals or None (act on the mean), latent [B, 20] or None (privileged
    encoder). Returns (mean, actions, logp [B, 2], values [B, 2]) in float64 and, in the same order, the running
    forward error scales E of a float32 evaluation: E_0 = u |x|, E_l = |W_l| E_{l-1} + u (|W_l| |a_{l-1}| + |b_l| + |a_l|)
    through the 1-Lipschitz activations; actions + u (|mu| + |std eps|); log-probabilities: sum over the group's
    dimensions of |d| / std^2 E_action + u (d^2 / (2 std^2) + |log std| + log(2 pi) / 2), d = std eps."""
    def layer(l, ae, act):                             # ae[0] the activations, ae[1] their error scale
        W, b = w[2 * l], w[2 * l + 1]
        out = act(ae[0] @ W.T + b)
        e = ae[1] @ W.abs().T + U32 * (ae[0].abs() @ W.abs().T + b.abs() + out.abs())
        return torch.stack([out, e])
    x = obs[:, :100].to(torch.float64)
    lat = None
    if latent is not None:
        lat = latent.to(torch.float64)
        lat = torch.stack([lat, U32 * lat.abs()])
    mean, values, _ = _policy_net(layer, torch.stack([x, U32 * x.abs()]), lat)
    (mean, e_mean), (values, e_values) = mean, values
    d = std * eps.to(torch.float64) if eps is not None else torch.zeros_like(mean)
    actions = mean + d
    e_act = e_mean + U32 * (mean.abs() + d.abs())
    logp = _log_prob2(mean, std.expand_as(mean), actions)
    t = d.abs() / (std * std) * e_act + U32 * (d * d / (2.0 * std * std) + torch.log(std).abs() + HALF_LOG_2PI)
    e_logp = torch.stack([t[:, :N_LEG].sum(-1), t[:, N_LEG:].sum(-1)], -1)
    return (mean, actions, logp, values), (e_mean, e_act, e_logp, e_values)


class _Tape:
    """Every pre-activation z of a forward pass with the input A it was formed from; after backward(), z.grad is dZ."""

    def __init__(self):
        self.items = []

    def __call__(self, layer, a, z):
        z.retain_grad()
        self.items.append((layer, a.detach(), z))
        return z

    def layer_grads(self, layer, conv=False):
        """(dW, S_W, db, S_b) of one layer, summed over its records (a convolution has one per output position).
        Linear: A [..., in], dZ [..., out]; convolution: A [B, tap, channel], dZ [B, out] -> weight [out, channel, tap]."""
        eq = "bo,bkc->ock" if conv else "bo,bi->oi"
        out = None
        for lay, a, z in self.items:
            if lay != layer:
                continue
            dz = z.grad
            if not conv:
                a, dz = a.reshape(-1, a.shape[-1]), dz.reshape(-1, dz.shape[-1])
            terms = [torch.einsum(eq, dz, a), torch.einsum(eq, dz.abs(), a.abs()), dz.sum(0), dz.abs().sum(0)]
            out = terms if out is None else [p + q for p, q in zip(out, terms)]
        return out


def _flat(tape, layers, convs=()):
    g, s = [], []
    for l in layers:
        dw, sw, db, sb = tape.layer_grads(l, conv=l in convs)
        g += [dw.reshape(-1), db]
        s += [sw.reshape(-1), sb]
    return g, s


def ppo_minibatch(w, std, batch, idx, clip=0.2, value_coef=1.0, mixing=0.5, roa_coef=0.1, use_clipped_value_loss=True):
    """One PPO.update minibatch (PPO:166-221, teacher path, no entropy term) in float64: loss = mean surrogate (Advantage
    Mixing, ratio clip) + value_coef * mean value loss (clipped or plain) + roa_coef * mean ||priv_latent - hist_latent||
    with the GIVEN history latent. batch: dict of flat [TN, ...] tensors obs, actions, old_values, advantages, returns,
    old_logp, hist_latent; idx [B] the minibatch's rows. Returns (flat, S) in the layout of wbc_ppo_grad_floats(): 16 x
    (weight, bias), std [18], then the three loss SUMS (surrogate and value over 2 B terms, regulariser over B)."""
    w = [x.detach().clone().requires_grad_(True) for x in w]
    obs, actions, old_v, adv, ret, old_logp, hist = (batch[k][idx].to(torch.float64) for k in
                                                     ("obs", "actions", "old_values", "advantages", "returns", "old_logp", "hist_latent"))
    B = obs.shape[0]
    std_rows = std.detach().expand(B, 18).clone().requires_grad_(True)      # a copy per row: its gradient holds std's per-row terms
    tape = _Tape()
    mean, value, priv = _policy_net(lambda l, a, act: act(tape(l, a, a @ w[2 * l].T + w[2 * l + 1])), obs[:, :100])
    logp = _log_prob2(mean, std_rows, actions)
    mixed = torch.stack([adv[:, 0] + mixing * adv[:, 1], adv[:, 1] + mixing * adv[:, 0]], -1)
    ratio = torch.exp(logp - old_logp)
    surr = torch.max(-mixed * ratio, -mixed * ratio.clamp(1.0 - clip, 1.0 + clip))
    if use_clipped_value_loss:
        vclip = old_v + (value - old_v).clamp(-clip, clip)
        vl = torch.max((value - ret) ** 2, (vclip - ret) ** 2)
    else:
        vl = (ret - value) ** 2
    reg = (priv - hist).norm(p=2, dim=1)
    (surr.sum() / (2 * B) + value_coef * vl.sum() / (2 * B) + roa_coef * reg.sum() / B).backward()
    g, s = _flat(tape, range(16))
    c = std_rows.grad
    sums = torch.stack([surr.sum(), vl.sum(), reg.sum()]).detach()
    s_sums = torch.stack([surr.abs().sum(), vl.abs().sum(), reg.abs().sum()]).detach()
    return torch.cat(g + [c.sum(0), sums]), torch.cat(s + [c.abs().sum(0), s_sums])


def hist_train(w, obs, target, idx):
    """One PPO.update_dagger minibatch (PPO:265-291) in float64: loss = mean over the rows idx of ||target - hist_latent||_2.
    Returns (flat, S) in the layout of wbc_hist_train_grad_floats(): the eight tensors of hist_weights, then the loss SUM."""
    w = [x.detach().clone().requires_grad_(True) for x in w]
    tape = _Tape()
    rows = (target[idx].to(torch.float64) - hist_latent(w, obs[idx], rec=tape)).norm(p=2, dim=1)
    (rows.sum() / rows.shape[0]).backward()
    g, s = _flat(tape, range(4), convs=(1, 2))
    total = rows.sum().detach().reshape(1)
    return torch.cat(g + [total]), torch.cat(s + [total])


RATIO_BANDS = ((0.55, 0.79), (0.81, 1.19), (1.21, 1.6))


def kink_free_batch(w, std, obs, seed, clip=0.2):
    """PPO minibatch inputs for the observations obs [B, >= 100], built from the float64 forward so that no row is near a
    kink of the piecewise losses -- a float32 kernel and the float64 reference then take the same branch in every row, and
    no test needs to leave a row out:
      actions    mu64 + std N(0, 1)
      old_logp   logp64 - log r, r uniform in one of RATIO_BANDS drawn per (row, channel): below, inside and above the
                 ratio clip, each with both signs of the N(0, 1) advantages
      old_values v64 - s f, s from {-0.5, -0.1, 0.1, 0.5}, f uniform in [0.6, 0.9]: |v - v_old| in [0.06, 0.09] or [0.30, 0.45]
      returns    (v64 + vclip64) / 2 +- (0.05 + |N(0, 1)|): the l1 = l2 kink of a clipped row sits at that midpoint
      hist_latent an independent N(0, 1) draw
    Everything is cast to float32 and the margins are evaluated, in float64, on the cast values; the function ASSERTS them
    (ratio 5e-3 from 1 -+ clip, v - v_old 1e-2 from +-clip, |l1 - l2| >= 1e-3 on clipped rows, ||priv - hist|| >= 0.1, and
    for B >= 1000 at least 10 % of the (row, channel) entries in every branch). Returns (batch dict of float32 tensors,
    margins dict)."""
    assert clip == 0.2, "the bands above are laid out around clip = 0.2"
    dev = obs.device
    g = torch.Generator(device=dev).manual_seed(seed)
    B = obs.shape[0]
    randn = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float64)      # noqa: E731
    rand = lambda *s: torch.rand(*s, generator=g, device=dev, dtype=torch.float64)        # noqa: E731
    with torch.no_grad():
        mean, value, priv = _policy_net(lambda l, a, act: act(a @ w[2 * l].T + w[2 * l + 1]), obs[:, :100].to(torch.float64))
        actions = (mean + std * randn(B, 18)).float()
        logp = _log_prob2(mean, std.expand_as(mean), actions.double())
        bands = torch.tensor(RATIO_BANDS, dtype=torch.float64, device=dev)
        band = torch.randint(0, 3, (B, 2), generator=g, device=dev)
        r = bands[band, 0] + (bands[band, 1] - bands[band, 0]) * rand(B, 2)
        old_logp = (logp - torch.log(r)).float()
        adv = randn(B, 2).float()
        s = torch.tensor([-0.5, -0.1, 0.1, 0.5], dtype=torch.float64, device=dev)[torch.randint(0, 4, (B, 2), generator=g, device=dev)]
        old_v = (value - s * (0.6 + 0.3 * rand(B, 2))).float()
        dv = value - old_v.double()
        vclip = old_v.double() + dv.clamp(-clip, clip)
        sign = torch.where(rand(B, 2) < 0.5, -1.0, 1.0)
        ret = (0.5 * (value + vclip) + sign * (0.05 + randn(B, 2).abs())).float()
        hist = randn(B, 20).float()
        # the margins, on the cast values
        ratio = torch.exp(logp - old_logp.double())
        clipped = dv.abs() > clip
        l1, l2 = (value - ret.double()) ** 2, (vclip - ret.double()) ** 2
        gap = torch.where(clipped, (l1 - l2).abs(), torch.full_like(l1, float("inf")))
        m = dict(ratio=torch.minimum((ratio - (1.0 - clip)).abs(), (ratio - (1.0 + clip)).abs()).min().item(),
                 value_clip=(dv.abs() - clip).abs().min().item(), l1_l2=gap.min().item(),
                 latent=(priv - hist.double()).norm(p=2, dim=1).min().item())
        n = float(2 * B)
        m["shares"] = dict(ratio_low=(ratio < 1.0 - clip).sum().item() / n, ratio_in=((ratio > 1.0 - clip) & (ratio < 1.0 + clip)).sum().item() / n,
                           ratio_high=(ratio > 1.0 + clip).sum().item() / n, clipped=clipped.sum().item() / n, unclipped=(~clipped).sum().item() / n,
                           l1_gt_l2=(clipped & (l1 > l2)).sum().item() / n, l1_lt_l2=(clipped & (l1 < l2)).sum().item() / n)
    assert m["ratio"] >= 5e-3 and m["value_clip"] >= 1e-2 and m["l1_l2"] >= 1e-3 and m["latent"] >= 0.1, m
    if B >= 1000:
        assert min(m["shares"].values()) >= 0.10, m
    return dict(actions=actions, old_values=old_v, advantages=adv, returns=ret, old_logp=old_logp, hist_latent=hist), m


# ---------------------------------------------------------------------------------------------------------------------
# The eager module path. NOT part of the float64 reference above: these run the ActorCritic they are handed (in whatever
# precision it is in) exactly as PPO.act / PPO.update / PPO.update_dagger do. In float64 they are what the restatements
# are pinned against; in float32 on the GPU they are the arithmetic the GPU tests' constants are measured on.
def eager_act(ac, obs, eps, latent=None):
    """PPO.act's policy side on the modules -> (mean, actions, logp, values); latent: the student path's given latent."""
    a = ac.actor
    lat = a.infer_priv_latent(obs) if latent is None else latent
    trunk = a.actor_backbone(torch.cat([obs[:, :N_PROP], lat], dim=1))
    mean = torch.cat([a.actor_leg_control_head(trunk), a.actor_arm_control_head(trunk)], dim=-1)
    ac.distribution = torch.distributions.Normal(mean, mean * 0. + ac.std)
    actions = mean + ac.std * eps if eps is not None else mean
    return mean, actions, ac.get_actions_log_prob(actions), ac.evaluate(obs)


def eager_ppo_grad(ac, batch, idx, clip=0.2, value_coef=1.0, mixing=0.5, roa_coef=0.1, use_clipped_value_loss=True):
    """The eager update's loss (PPO.update, teacher path, no entropy term) on the modules, the given history latent as the
    regulariser's target; autograd. Flat gradient in the layout of wbc_ppo_grad_floats(), the three loss sums last."""
    obs, actions, old_v, adv, ret, old_logp, hist = (batch[k][idx] for k in ("obs", "actions", "old_values", "advantages", "returns", "old_logp", "hist_latent"))
    ac.zero_grad()
    ac.update_distribution(obs, False)
    logp, value = ac.get_actions_log_prob(actions), ac.evaluate(obs)
    reg = (ac.actor.infer_priv_latent(obs) - hist).norm(p=2, dim=1)
    mixed = torch.stack([adv[..., 0] + mixing * adv[..., 1], adv[..., 1] + mixing * adv[..., 0]], dim=-1)
    ratio = torch.exp(logp - old_logp)
    surr = torch.max(-mixed * ratio, -mixed * torch.clamp(ratio, 1.0 - clip, 1.0 + clip))
    if use_clipped_value_loss:
        vclip = old_v + (value - old_v).clamp(-clip, clip)
        vl = torch.max((value - ret).pow(2), (vclip - ret).pow(2))
    else:
        vl = (ret - value).pow(2)
    (surr.mean() + value_coef * vl.mean() + roa_coef * reg.mean()).backward()
    sd = dict(ac.named_parameters())
    gs = []
    for name in POLICY_LAYERS:
        gs += [sd[name + ".weight"].grad.reshape(-1), sd[name + ".bias"].grad.reshape(-1)]
    flat = torch.cat(gs + [ac.std.grad.reshape(-1), torch.stack([surr.sum(), vl.sum(), reg.sum()]).detach()])
    ac.zero_grad()
    ac.distribution = None                             # (it holds the graph: the module would not deepcopy)
    return flat


def eager_hist_grad(ac, obs, target, idx):
    """PPO.update_dagger's loss on the history-encoder module; autograd. Layout of wbc_hist_train_grad_floats()."""
    he = ac.actor.history_encoder
    he.zero_grad()
    rows = (target[idx] - he(obs[idx][:, HIST_OFF:].reshape(-1, T_HIST, N_PROP))).norm(p=2, dim=1)
    rows.mean().backward()
    flat = torch.cat([p.grad.reshape(-1) for p in he.parameters()] + [rows.sum().detach().reshape(1)])
    he.zero_grad()
    return flat
