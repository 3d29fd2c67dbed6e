"""Time of wbc_sim_ground_estimate (wbc_ground_estimate_kernel) next to the same plane fit in torch ops, in one session:
  * the launch with every output (five query points per env) and with the state alone;
  * the torch route: refresh_rigid_body_state() for the foot origins, the latch and the ages as torch.where, the weighted sums about
    foot 0's point, torch.linalg.cholesky and cholesky_solve on the 2 x 2 system, the clamp and every output as tensor expressions.

  python tools/profile_ground.py [--envs 4096]       device-event times of every mode, back to back calls after warm-up, two rounds

The other lane mapping (lane = env, the four legs walked in sequence) is timed by running this script on a library whose
wbc_ground_kernel.hip was compiled with -DGE_EPW=64 (python tools/build_variant.py ge64 -DGE_EPW=64;
WBC_AMD_LIB=<that library> python tools/profile_ground.py --mode hip)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--queries", type=int, default=5)
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
gnd = env.ground_estimator()
c = gnd.cfg
lam = float(getattr(c, "lambda"))
gen = torch.Generator(device="cuda"); gen.manual_seed(3)
contact = (torch.rand(n, 4, device="cuda", generator=gen) < 0.5).float().contiguous()
for _ in range(3):                                                                  # contact points of several ages, a slope to remember
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
    env.reset_buf.zero_()
    gnd.update((torch.rand(n, 4, device="cuda", generator=gen) < 0.5).float())
query = (env.root_states[:, None, 0:2] + torch.rand(n, a.queries, 2, device="cuda", generator=gen) - 0.5).contiguous()
state0 = gnd.state.clone()
state = state0.clone()
query_z = torch.zeros(n, a.queries, device=dev)
feet = env.feet_indices


def hip_all():
    sim.ground_estimate(c, state, contact, query_xy=query, normal=gnd.normal, ground=gnd.ground, residual=gnd.residual, trunk=gnd.trunk,
                        theta_ref=gnd.theta_ref, query_z=query_z, info=gnd.info)


def hip_state():
    sim.ground_estimate(c, state, contact, query_xy=query)


def torch_route(st):
    """(state, normal, ground, residual, trunk, theta_ref, query_z) of one call from `st` [N, 32], torch ops only."""
    sim.refresh_rigid_body_state()
    p = env.rigid_body_state[:, feet, 0:3]
    root = env.root_states
    b, qt = root[:, 0:3], root[:, 3:7]
    feet_st = st[:, :20].view(n, 4, 5)
    stand = contact >= c.c_on
    m = torch.where(stand[:, :, None], p, feet_st[:, :, 0:3])
    t = torch.where(stand, torch.zeros_like(contact), feet_st[:, :, 3] + c.dt)
    w = torch.exp(-(t - t.min(dim=1, keepdim=True).values) / c.tau_age)
    W = w.sum(1)
    m0 = m[:, 0]
    e = m - m0[:, None]
    r = (w[:, :, None] * e).sum(1) / W[:, None]
    d = e - r[:, None]
    S = torch.einsum("nf,nfu,nfv->nuv", w, d[:, :, 0:2], d[:, :, 0:2]) + (lam * W)[:, None, None] * torch.eye(2, device=dev)
    rhs = torch.einsum("nf,nfu,nf->nu", w, d[:, :, 0:2], d[:, :, 2]) + (lam * W)[:, None] * st[:, 23:25]
    sl = torch.cholesky_solve(rhs[:, :, None], torch.linalg.cholesky(S))[:, :, 0]
    norm = sl.norm(dim=1, keepdim=True)
    sl = torch.where(norm > c.slope_max, sl * (c.slope_max / norm.clamp_min(1e-30)), sl)
    a0 = m0[:, 2] + r[:, 2]
    plane = lambda xy: a0[:, None] + (sl[:, None, :] * ((xy - m0[:, None, 0:2]) - r[:, None, 0:2])).sum(-1)   # noqa: E731
    s2 = (sl * sl).sum(1)
    s = s2.sqrt()
    ninv = torch.rsqrt(1 + s2)
    normal = torch.stack([-sl[:, 0] * ninv, -sl[:, 1] * ninv, ninv], dim=-1)[:, None, :].expand(n, 4, 3)
    ground = plane(p[:, :, 0:2])
    residual = d[:, :, 2] - (sl[:, None, :] * d[:, :, 0:2]).sum(-1)
    zb = plane(b[:, None, 0:2])[:, 0]
    x, y, z, wq = qt.unbind(-1)
    hx, hy = 1 - 2 * (y * y + z * z), 2 * (x * y + wq * z)
    hn = (hx * hx + hy * hy).sqrt()
    ch, sh = hx / hn, hy / hn
    zero = torch.zeros_like(zb)
    trunk = torch.stack([zb, (b[:, 2] - zb) * ninv, sl[:, 0] * ch + sl[:, 1] * sh, sl[:, 1] * ch - sl[:, 0] * sh, zero, zero], dim=-1)
    g = c.tilt_gain * torch.where(s < 1e-4, 1 - s2 / 3, torch.atan(s) / s.clamp_min(1e-30))
    theta = torch.stack([g * sl[:, 1], -g * sl[:, 0], zero], dim=-1)
    new = torch.cat([torch.cat([m, t[:, :, None], torch.zeros(n, 4, 1, device=dev)], dim=-1).view(n, 20), m0[:, 0:2] + r[:, 0:2], a0[:, None], sl,
                     torch.zeros(n, 7, device=dev)], dim=-1)
    return new, normal, ground, residual, trunk, theta, plane(query)


if a.mode == "every":                                                                  # the two routes compute the same thing
    tn, tnormal, tground, tres, ttrunk, ttheta, tq = torch_route(state0)
    hip_all()
    torch.cuda.synchronize()
    diff = lambda u, v: float((u - v).abs().max())                                   # noqa: E731
    print(f"torch route against the kernel: largest difference in the state {diff(tn, state):.3g}, normal {diff(tnormal, gnd.normal):.3g}, ground "
          f"{diff(tground, gnd.ground):.3g}, residual {diff(tres, gnd.residual):.3g}, trunk {diff(ttrunk, gnd.trunk):.3g}, theta_ref "
          f"{diff(ttheta, gnd.theta_ref):.3g}, query_z {diff(tq, query_z):.3g}; largest |a| {float(state[:, 23:25].norm(dim=1).max()):.3g}; info words "
          f"{sorted(set(gnd.info.cpu().tolist()))[:8]}", flush=True)
calls = {"hip every output": hip_all, "hip state only": hip_state}
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
