"""Time of wbc_sim_contact_detect (wbc_contact_detect_kernel) at the bench's env count next to the same detection in torch ops, in one
session:
  * the launch with every output and with prob alone (tau_ext from an observer state's residual plane, ground, phase from a planner state);
  * the torch route: refresh_jacobian_tensors(), a gather of the four 3 x 3 leg blocks, torch.linalg.solve on J^T J + delta^2 I,
    torch.erf for the three terms, the fusion, the low-pass and the flag logic as tensor expressions.

  python tools/profile_contact.py        device-event times of every mode, back to back calls after warm-up, two rounds, alternating

The layout -- lane = (env, foot), 16 envs per wavefront -- was chosen against the estimator's (two envs per wavefront, the feet on lanes
0..3 of each 32-lane group) by running this script on a library whose wbc_contact_kernel.hip was compiled with -DCT_EPW=2
(python tools/build_variant.py ct2 -DCT_EPW=2; WBC_AMD_LIB=<that library> python tools/profile_contact.py --mode hip)."""
import argparse
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
planner = env.gait_planner("trot", period=0.5, duty=0.5, horizon=0)
gen = torch.Generator(device="cuda"); gen.manual_seed(3)
planner.reset(phase=torch.rand(n, device="cuda", generator=gen))
det = env.contact_detector(planner=planner)
for _ in range(3):                                                                  # a residual worth solving for
    det.update()
c = det.cfg
state0 = (torch.rand(n, 4, 4, device="cuda", generator=gen) * torch.tensor([1.0, 1.0, 0.1, 0.0], device="cuda")).contiguous()
state0[:, :, 1] = (state0[:, :, 1] > 0.5).float()
state0 = state0.view(n, 16).contiguous()
ground = det._plane_ground
phase = planner.state[:, 0]
tau_ext = det.tau_ext
feet = env.feet_indices
leg_dofs = None


def hip_all():
    sim.contact_detect(c, det.state, tau_ext=tau_ext, ground=ground, phase=phase, prob=det.prob, contact=det.contact, stance=det.stance,
                       force=det.foot_forces, terms=det.terms, info=det.info)


def hip_prob():
    sim.contact_detect(c, det.state, tau_ext=tau_ext, ground=ground, phase=phase, prob=det.prob)


def Phi(x):
    return 0.5 * (1 + torch.erf(x * 0.7071067811865476))


def torch_route(state):
    """(p, c, t, force) of one detector step from `state` [N, 16], torch ops only."""
    global leg_dofs
    sim.refresh_jacobian_tensors()
    sim.refresh_rigid_body_state()
    Jw = env.jacobian_whole[:, feet, 0:3, :]                                           # [N, 4, 3, 26]
    if leg_dofs is None:                                                               # the three joint columns that move each foot
        nz = (Jw[0, :, :, 6:].abs().sum(1) > 0)
        leg_dofs = torch.stack([torch.nonzero(nz[f])[:3, 0] for f in range(4)]) + 6   # [4, 3]
    J = torch.gather(Jw, 3, leg_dofs[None, :, None, :].expand(n, 4, 3, 3))             # [N, 4, 3, 3]
    tau = tau_ext[:, leg_dofs]                                                         # [N, 4, 3]
    A = J.transpose(-1, -2) @ J + (c.damping ** 2) * torch.eye(3, device=dev)
    y = torch.linalg.solve(A, tau.unsqueeze(-1))
    force = (J @ y).squeeze(-1)
    Pf = Phi((force[..., 2] - c.mu_f) / c.sigma_f)
    pz = env.rigid_body_state[:, feet, 2]
    Pz = Phi((c.mu_z - (pz - ground)) / c.sigma_z)
    offset = torch.tensor(list(c.offset), device=dev)
    phi = torch.remainder(phase[:, None] + offset[None], 1.0)
    sched = phi < c.duty
    s = torch.where(sched, phi / c.duty, (phi - c.duty) / (1 - c.duty))
    k = c.sigma_phase * 2 ** 0.5
    G = 0.5 * (torch.erf(s / k) + torch.erf((1 - s) / k))
    Pphi = torch.where(sched, G, 1 - G)
    P = (Pphi / c.var_phase + Pz / c.var_z + Pf / c.var_f) / (1 / c.var_phase + 1 / c.var_z + 1 / c.var_f)
    st = state.view(n, 4, 4)
    p = st[:, :, 0] + c.alpha * (P - st[:, :, 0])
    on = st[:, :, 1] != 0
    t = st[:, :, 2] + c.dt
    td = ~on & (p >= c.p_on) & (t >= c.t_dwell)
    lo = on & (p <= c.p_off) & (t >= c.t_dwell)
    on = torch.where(td, torch.ones_like(on), torch.where(lo, torch.zeros_like(on), on))
    t = torch.where(td | lo, torch.zeros_like(t), t)
    early = ~sched & (s >= c.early_min) & on
    late = sched & (s >= c.late_min) & ~on
    stance = (sched | early) & ~late
    return p, on, t, force, stance


if a.mode == "every":                                                                  # the two routes compute the same thing
    det.state.copy_(state0)
    p, on, t, force, stance = torch_route(state0)
    hip_all()
    torch.cuda.synchronize()
    print(f"torch route against the kernel: largest |p| difference {float((p - det.prob).abs().max()):.3g}, contact equal in "
          f"{float((on == det.contact.bool()).float().mean()):.4f} of the feet, stance equal in {float((stance == det.stance.bool()).float().mean()):.4f}, "
          f"largest force difference {float((force - det.foot_forces).abs().max()):.3g} N (largest |force| {float(det.foot_forces.abs().max()):.3g} N)", flush=True)
calls = {"hip every output": hip_all, "hip prob only": hip_prob}
if a.mode == "every":
    calls["torch"] = lambda: torch_route(state0)
times = {}
for rnd in range(a.rounds):
    for mode, call in calls.items():
        iters = a.iters if mode.startswith("hip") else max(a.iters // 10, 5)
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
