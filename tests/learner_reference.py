"""Plain float64 restatements of the learner-side operations the HIP kernels implement, for the tests. Nothing here calls
a project module on the compute path: torch is used as an fp64 array library (CPU or GPU), numpy for the scans.

  hist_latent          StateHistoryEncoder, tsteps = 10 (AC:39-84)       <-> wbc_hist_latent   (csrc/wbc_hist_kernel.hip)
  priv_latent          privileged encoder 24 -> 64 -> 20 (AC:129-141)    <-> wbc_priv_latent   (csrc/wbc_hist_train_kernel.hip)
  gae / normalize      RolloutStorage.compute_returns (RS:136-150)       <-> wbc_gae_compute + wbc_gae_normalize
  rollout_store        PPO.process_env_step's bootstrap + done cast      <-> wbc_rollout_store (csrc/wbc_gae_kernel.hip)
  clip_adam            clip_grad_norm_ + Adam.step (PPO:243-246)         <-> wbc_ppo_clip_adam / wbc_hist_clip_adam
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


def hist_latent(w, obs):
    """obs [B, >= 860] -> [B, 20]: Linear 76->30 + ELU per step; Conv1d 30->20 (k4 s2) + ELU; Conv1d 20->10 (k2 s1) + ELU;
    channel-major flatten; Linear 30->20 + ELU. The convolutions are written out as sums over (tap, channel)."""
    enc_w, enc_b, c1_w, c1_b, c2_w, c2_b, lin_w, lin_b = w
    x = obs[:, HIST_OFF:HIST_OFF + T_HIST * N_PROP].to(torch.float64).reshape(-1, T_HIST, N_PROP)
    h1 = _elu(x @ enc_w.T + enc_b)                                                            # [B, 10, 30]
    h2 = torch.stack([torch.einsum("bkc,ock->bo", h1[:, 2 * l:2 * l + 4], c1_w) for l in range(4)], 1)
    h2 = _elu(h2 + c1_b)                                                                      # [B, 4, 20]
    h3 = torch.stack([torch.einsum("bkc,ock->bo", h2[:, l:l + 2], c2_w) for l in range(3)], 1)
    h3 = _elu(h3 + c2_b)                                                                      # [B, 3 positions, 10 channels]
    flat = h3.permute(0, 2, 1).reshape(-1, 30)                                                # index = channel * 3 + position
    return _elu(flat @ lin_w.T + lin_b)


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
