"""Time of wbc_sim_slip_detect (wbc_slip_detect_kernel) next to the same computation in torch ops, in one session:
  * the launch with every output, and with prob + slip alone;
  * the torch route: refresh_rigid_body_state() for the foot origins' world velocities, the common-mode mean, the tangential speed, the
    evidence through torch.erf, the hysteresis and the friction recursions as torch.where, the fusion and every output as tensor
    expressions.

  python tools/profile_slip.py [--envs 4096]       device-event times of every mode, back to back calls after warm-up, two rounds

The other lane mapping (lane = env, the four legs walked in sequence) is timed by running this script on a library whose
wbc_slip_kernel.hip was compiled with -DSL_EPW=64 (python tools/build_variant.py sl64 -DSL_EPW=64;
WBC_AMD_LIB=<that library> python tools/profile_slip.py --mode hip)."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", choices=["every", "hip"], default="every")
a = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import torch  # noqa: E402

from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
env.reset_buf.zero_()
n, sim, dev = a.envs, env.sim, env.device
slip = env.slip_detector(common_mode=0.5)
c = slip.cfg
gen = torch.Generator(device="cuda"); gen.manual_seed(3)
contact = torch.rand(n, 4, device="cuda", generator=gen).contiguous()
force = (torch.rand(n, 4, 3, device="cuda", generator=gen) * torch.tensor([20.0, 20.0, 60.0], device="cuda") -
         torch.tensor([10.0, 10.0, 0.0], device="cuda")).contiguous()
for _ in range(3):                                                                  # a state with flags, timers and weights of several ages
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
    env.reset_buf.zero_()
    slip.update(torch.rand(n, 4, device="cuda", generator=gen), foot_force=force)
state0 = slip.state.clone()
state = state0.clone()
feet = env.feet_indices
SQRT2 = math.sqrt(2.0)


def hip_all():
    sim.slip_detect(c, state, contact, foot_force=force, prob=slip.prob, slip=slip.slip, weight=slip.weight, foot_vel=slip.foot_vel,
                    speed=slip.speed, distance=slip.distance, mu=slip.mu, mu_lower=slip.mu_lower, mu_env=slip.mu_env, info=slip.info)


def hip_flag():
    sim.slip_detect(c, state, contact, foot_force=force, prob=slip.prob, slip=slip.slip)


def torch_route(st):
    """(state, prob, slip, weight, foot_vel, speed, distance, mu, mu_lower, mu_env) of one call from `st` [N, 4, 8], torch ops only."""
    sim.refresh_rigid_body_state()
    u = env.rigid_body_state[:, feet, 7:10]
    p, s, t, cp, d, mu, w, m = [st[:, :, k] for k in range(8)]
    s, cp = s != 0, cp != 0
    cc = contact.clamp(0.0, 1.0)
    stand = cc >= c.c_on
    d = torch.where(stand & ~cp, torch.zeros_like(d), d)
    cw = torch.where(stand, cc, torch.zeros_like(cc))
    S = cw.sum(1)
    cm = (stand.sum(1) >= 2) & (S > 0)
    ub = torch.where(cm[:, None], (cw[:, :, None] * u).sum(1) / S.clamp_min(1e-30)[:, None], torch.zeros(n, 3, device=dev))
    g = u - c.common_mode * ub[:, None, :]
    sp = g[:, :, 0:2].norm(dim=-1)                                                       # the normal is world z
    P = torch.where(stand, cc * 0.5 * (1 + torch.erf((sp - c.v_slip) / (c.sigma_v * SQRT2))), torch.zeros_like(cc))
    p = p + c.alpha * (P - p)
    t = t + c.dt
    lift = ~stand & s
    start = ~lift & stand & ~s & (p >= c.p_on) & (t >= c.t_dwell)
    stop = ~lift & ~start & s & (p <= c.p_off) & (t >= c.t_dwell)
    s = torch.where(start, torch.ones_like(s), torch.where(lift | stop, torch.zeros_like(s), s))
    t = torch.where(start | lift | stop, torch.zeros_like(t), t)
    d = d + torch.where(s, sp * c.dt, torch.zeros_like(sp))
    fn = force[:, :, 2]
    ft = force[:, :, 0:2].norm(dim=-1)
    valid = stand & (fn >= c.fn_min)
    rho = ft / fn
    m = c.gamma * m
    m = torch.where(valid & ~s, torch.maximum(m, rho), m)
    w = c.gamma * w
    slide = valid & s & (p > 0)
    wn = torch.where(slide, w + p, w)
    mu = torch.where(slide, mu + (p / wn.clamp_min(1e-30)) * (rho - mu), mu)
    W = wn.sum(1)
    mue = torch.where(W >= c.w_min, (wn * mu).sum(1) / W.clamp_min(1e-30), torch.full_like(W, c.mu_prior))
    mraw = torch.where(wn >= c.w_min, mu, mue[:, None].expand(n, 4))
    new = torch.stack([p, s.float(), t, stand.float(), d, mu, wn, m], dim=-1)
    return (new, p, s.to(torch.uint8), cc * (1 - p), u, sp, d, (c.mu_scale * mraw).clamp(c.mu_min, c.mu_max), m, torch.stack([mue, W], dim=-1))


if a.mode == "every":                                                                  # the two routes compute the same thing
    tn, tp, ts, tw, tu, tsp, td, tmu, tm, tme = torch_route(state0)
    hip_all()
    torch.cuda.synchronize()
    diff = lambda x, y: float((x.float() - y.float()).abs().max())                  # noqa: E731
    print(f"torch route against the kernel: largest difference in the state {diff(tn, state):.3g}, prob {diff(tp, slip.prob):.3g}, slip "
          f"{diff(ts, slip.slip):.3g}, weight {diff(tw, slip.weight):.3g}, foot_vel {diff(tu, slip.foot_vel):.3g}, speed {diff(tsp, slip.speed):.3g}, "
          f"distance {diff(td, slip.distance):.3g}, mu {diff(tmu, slip.mu):.3g}, mu_lower {diff(tm, slip.mu_lower):.3g}, mu_env "
          f"{diff(tme, slip.mu_env):.3g}; flagged feet {int(slip.slip.sum())} of {4 * n}; MU_VALID feet {int((state[:, :, 6] >= c.w_min).sum())}", flush=True)
calls = {"hip every output": hip_all, "hip prob and slip": hip_flag}
if a.mode == "every":
    calls["torch"] = lambda: torch_route(state0)
times = {}
for rnd in range(a.rounds):
    for mode, call in calls.items():
        iters = a.iters if mode.startswith("hip") else max(a.iters // 10, 5)
        state.copy_(state0)
        for _ in range(10 if mode.startswith("hip") else 3):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        times.setdefault(mode, []).append(t0.elapsed_time(t1) * 1e3 / iters)
        print(f"round {rnd} {mode:20s} N={n}: {times[mode][-1]:.2f} us per call (device events, back to back)", flush=True)
second = {m: v[-1] for m, v in times.items()}
line = ", ".join(f"{m} {v:.2f} us" for m, v in second.items())
print(f"second round: {line}" + (f"; torch / hip every output = {second['torch'] / second['hip every output']:.1f}" if "torch" in second else ""), flush=True)
