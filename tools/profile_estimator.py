"""Time of wbc_sim_leg_odometry (wbc_leg_odometry_kernel) at the bench's env count next to the route it replaces, in one session and one build:
  * the launch with height rows (m = 28) and without (m = 24), every optional output asked for;
  * the torch route: refresh_jacobian_tensors + refresh_rigid_body_state, the feet's rows gathered from them, A P A^T + Q, a dense C,
    torch.linalg.cholesky and cholesky_solve, on the same inputs.

  python tools/profile_estimator.py        device-event times of every mode, back to back calls after warm-up, two rounds, alternating

The packing of two envs per wavefront was chosen against one env per wavefront by running this script on a library whose
wbc_estimator_kernel.hip was compiled with -DEST_EPW=1 (WBC_AMD_LIB=<that library> python tools/profile_estimator.py --mode hip)."""
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
n, sim = a.envs, env.sim
est = env.base_state_estimator()
c = est.cfg
gen = torch.Generator(device="cuda"); gen.manual_seed(3)
G = torch.randn(n, 18, 18, device="cuda", generator=gen) * 0.05
P0 = G @ G.transpose(1, 2) + 0.01 * torch.eye(18, device="cuda")
P0 = (torch.tril(P0) + torch.tril(P0, -1).transpose(1, 2)).contiguous()
x0 = est.x.clone()
x0[:, 3:6] = env.root_states[:, 7:10]
contact = (torch.rand(n, 4, device="cuda", generator=gen) < 0.5).float()
accel = torch.randn(n, 3, device="cuda", generator=gen) + torch.tensor([0.0, 0.0, 9.81], device="cuda")
height = torch.zeros(n, 4, device="cuda")
gravity = torch.tensor(list(env.tcfg.gravity), device="cuda")
x, P = x0.clone(), P0.clone()
vel, nis, status = torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")

# ---- the torch route's tables ---------------------------------------------------------------------------------------------------------
feet = env.feet_indices
rows = [(a_, 6 + 3 * f + a_) for f in range(4) for a_ in range(3)] + [(3 + a_, -1) for f in range(4) for a_ in range(3)] + [(8 + 3 * f, -1) for f in range(4)]
foot_of = [f for f in range(4) for _ in range(3)] * 2 + list(range(4))
group_of = [0] * 12 + [1] * 12 + [2] * 4
C28 = torch.zeros(28, 18, device="cuda")
for k, (c1, c2) in enumerate(rows):
    C28[k, c1] = 1.0
    if c2 >= 0:
        C28[k, c2] = -1.0
A = torch.eye(18, device="cuda"); A[0:3, 3:6] = c.dt * torch.eye(3, device="cuda")
sig2 = torch.tensor([c.sigma_r ** 2, c.sigma_rdot ** 2, c.sigma_z ** 2], device="cuda")[torch.tensor(group_of, device="cuda")]
foot_idx = torch.tensor(foot_of, device="cuda")


def quat_to_mat(q):
    q = q / q.norm(dim=-1, keepdim=True)
    x_, y_, z_, w_ = q.unbind(-1)
    return torch.stack([1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ - w_ * z_), 2 * (x_ * z_ + w_ * y_), 2 * (x_ * y_ + w_ * z_), 1 - 2 * (x_ * x_ + z_ * z_),
                        2 * (y_ * z_ - w_ * x_), 2 * (x_ * z_ - w_ * y_), 2 * (y_ * z_ + w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)], -1).view(-1, 3, 3)


def torch_route(xin, Pin, m):
    sim.refresh_jacobian_tensors(); sim.refresh_rigid_body_state()
    root = env.root_states
    R = quat_to_mat(root[:, 3:7])
    r = env.rigid_body_state[:, feet, 0:3] - root[:, None, 0:3]
    nu = torch.cat([root[:, 10:13], env.dof_vel], dim=1)                              # the root's angular velocity and the joint rates
    rdot = torch.einsum("nfic,nc->nfi", env.jacobian_whole[:, feet, 0:3, 3:], nu)
    s = 1 + c.kappa * (1 - contact.clamp(0, 1))
    acc = torch.einsum("nij,nj->ni", R, accel) + gravity
    xm = xin.clone()
    xm[:, 0:3] = xin[:, 0:3] + xin[:, 3:6] * c.dt + 0.5 * acc * c.dt ** 2
    xm[:, 3:6] = xin[:, 3:6] + acc * c.dt
    q = torch.cat([torch.full((n, 3), c.dt * c.sigma_p ** 2, device="cuda"), torch.full((n, 3), c.dt * c.sigma_v ** 2, device="cuda"),
                   (c.dt * c.sigma_f ** 2 * s).repeat_interleave(3, dim=1)], dim=1)
    Pm = A @ Pin @ A.T + torch.diag_embed(q)
    e = torch.cat([(-r - (xm[:, None, 0:3] - xm[:, 6:].view(n, 4, 3))).reshape(n, 12), (-rdot - xm[:, None, 3:6]).reshape(n, 12),
                   height - xm[:, 8::3]], dim=1)[:, :m]
    Cm = C28[:m]
    CP = Cm @ Pm
    S = CP @ Cm.T + torch.diag_embed(sig2[:m] * s[:, foot_idx[:m]])
    Lc = torch.linalg.cholesky(S)
    sol = torch.cholesky_solve(torch.cat([CP, e.unsqueeze(-1)], dim=2), Lc)         # S^-1 [C P-, e]
    xp = xm + torch.einsum("nkj,nk->nj", CP, sol[:, :, 18])
    Pp = Pm - CP.transpose(1, 2) @ sol[:, :, :18]
    return xp, Pp, torch.einsum("nji,nj->ni", R, xp[:, 3:6])


def hip(m):
    x.copy_(x0); P.copy_(P0)
    sim.leg_odometry(c, x, P, contact, accel=accel, foot_height=height if m == 28 else None, vel_body=vel, nis=nis, status=status)


def hip_bare(m):                                                                    # what is timed: the call alone, on whatever x and P hold
    sim.leg_odometry(c, x, P, contact, accel=accel, foot_height=height if m == 28 else None, vel_body=vel, nis=nis, status=status)


if a.mode == "every":                                                              # the two routes compute the same thing
    for m in (28, 24):
        hip(m)
        tx, tP, tv = torch_route(x0, P0, m)
        torch.cuda.synchronize()
        print(f"m = {m}: torch route against the kernel: largest difference in x {float((tx - x).abs().max()):.3g}, in P {float((tP - P).abs().max()):.3g}, "
              f"in vel_body {float((tv - vel).abs().max()):.3g}; {int((status != 0).sum())} envs not updated", flush=True)
calls = {"hip m=28": lambda: hip_bare(28), "hip m=24": lambda: hip_bare(24)}
if a.mode == "every":
    calls.update({"torch m=28": lambda: torch_route(x0, P0, 28), "torch m=24": lambda: torch_route(x0, P0, 24)})
times = {}
for rnd in range(a.rounds):
    for mode, call in calls.items():
        x.copy_(x0); P.copy_(P0)
        iters = a.iters if mode.startswith("hip") else max(a.iters // 10, 5)
        for _ in range(10 if mode.startswith("hip") else 3):
            call()
        x.copy_(x0); P.copy_(P0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        times.setdefault(mode, []).append(t0.elapsed_time(t1) * 1e3 / iters)
        print(f"round {rnd} {mode:10s} N={n}: {times[mode][-1]:.2f} us per call (device events, back to back)", flush=True)
if a.mode == "every":
    for m in (28, 24):
        h, t = min(times[f"hip m={m}"]), min(times[f"torch m={m}"])
        print(f"m = {m}: HIP {h:.2f} us, torch route {t:.2f} us, ratio {t / h:.1f}", flush=True)
