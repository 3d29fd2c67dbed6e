"""Time of wbc_sim_centroidal_mpc (wbc_centroidal_mpc_kernel) at the bench's env count next to a batched-torch restatement of the same
iteration, in one session and one build: H = 10 on rollout states with a trot schedule,
  * iters = 40 from a cold start and iters = 10 from a warm start (shifted), every output asked for, the sim's own state (NULL inputs:
    the call includes the centroidal launch) and explicit tensors (the MPC kernel alone);
  * the torch route: the same Riccati factorisation (torch.linalg.cholesky / cholesky_solve) and ADMM iteration in bmm / einsum on the same
    explicit tensors.

  python tools/profile_mpc.py        device-event times of every mode, back to back calls after warm-up, two rounds, alternating

One env per wavefront was chosen against two (one per 32-lane group) by running this script on a library whose wbc_mpc_kernel.hip was
compiled with -DMPC_EPW=2 (WBC_AMD_LIB=<that library> python tools/profile_mpc.py --mode hip)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=10)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", choices=["every", "hip"], default="every")
a = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import torch  # noqa: E402

from wbc_amd import abi  # noqa: E402
from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import CentroidalMPC, WidowGo1, trot_schedule  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n, H, sim, dev = a.envs, a.horizon, env.sim, "cuda"
mpc = env.centroidal_mpc(horizon=H)
gen = torch.Generator(device="cuda"); gen.manual_seed(3)
contact = trot_schedule(torch.rand(n, device="cuda", generator=gen), 0.4, 0.5, H, mpc.cfg.dt)
vel_cmd = torch.rand(n, 2, device="cuda", generator=gen) - 0.5
mpc.solve(contact, vel_cmd=vel_cmd, height=0.3)
x_ref = mpc.x_ref.clone()

# the explicit tensors NULL stands for
com, _, _, inr = sim.centroidal()
sim.refresh_rigid_body_state()
root = env.root_states
yaw = CentroidalMPC._yaw(env.base_quat)
x0 = torch.cat([CentroidalMPC._heading_rotvec(env.base_quat, yaw), root[:, 0:3] + com[:, 0:3], root[:, 10:13], com[:, 3:6]], dim=-1).contiguous()
mass = inr[:, 0].contiguous()
inertia = inr[:, [1, 4, 5, 4, 2, 6, 5, 6, 3]].view(-1, 3, 3).contiguous()
feet = env.rigid_body_state[:, env.feet_indices, 0:3].reshape(n, 1, 4, 3).contiguous()
gravity = torch.tensor(list(env.tcfg.gravity), device=dev)


def make_cfg(iters):
    c = mpc.cfg
    return abi.WbcMpcCfg(H, iters, c.dt, c.rho, c.mu, c.fz_min, c.fz_max, c.q, c.r, c.tol)


CFG = {10: make_cfg(10), 40: make_cfg(40)}
outs = dict(forces=torch.empty(n, 4, 3, device=dev), u=torch.empty(n, H, 12, device=dev), x_pred=torch.empty(n, H, 12, device=dev),
            base_acc=torch.empty(n, 6, device=dev), res=torch.empty(n, 2, device=dev), status=torch.empty(n, dtype=torch.int32, device=dev))
warm = torch.zeros(n, 2, H, 20, device=dev)
ws = torch.empty(16 * n, device=dev)


def hip(iters, cold, explicit):
    kw = dict(x0=x0, mass=mass, inertia=inertia, foot_pos=feet) if explicit else {}
    sim.centroidal_mpc(CFG[iters], contact, x_ref, warm=warm, cold=cold, shift=not cold, workspace=ws, **outs, **kw)


# ---- the torch route: the same factorisation and iteration, batched ---------------------------------------------------------------------
def skew(r):
    z = torch.zeros_like(r[..., 0])
    return torch.stack([torch.stack([z, -r[..., 2], r[..., 1]], -1), torch.stack([r[..., 2], z, -r[..., 0]], -1), torch.stack([-r[..., 1], r[..., 0], z], -1)], -2)


c = mpc.cfg
dt, rho, mu = float(c.dt), float(c.rho), float(c.mu)
q = torch.tensor(list(c.q), device=dev); rr = torch.tensor(list(c.r), device=dev)
A = torch.eye(12, device=dev); A[0:3, 6:9] = dt * torch.eye(3, device=dev); A[3:6, 9:12] = dt * torch.eye(3, device=dev)
c5 = torch.tensor([[-1, 0, mu], [1, 0, mu], [0, -1, mu], [0, 1, mu], [0, 0, 1]], device=dev)
Cm = torch.block_diag(c5, c5, c5, c5)
lo = torch.tensor([0, 0, 0, 0, float(c.fz_min)] * 4, device=dev); hi = torch.tensor([float("inf")] * 4 + [float(c.fz_max)], device=dev).repeat(4)
Rt = rr.repeat(4) + rho * torch.tensor([2.0, 2.0, 4 * mu * mu + 1], device=dev).repeat(4)
eye3 = torch.eye(3, device=dev)


def torch_route(iters, z, y):
    d = torch.cat([torch.zeros(3, device=dev), 0.5 * dt * dt * gravity, torch.zeros(3, device=dev), dt * gravity])
    pbar = torch.cat([x0[:, None, 3:6], x_ref[:, :H - 1, 3:6]], 1)
    r = feet.expand(n, H, 4, 3) - pbar[:, :, None]
    W = torch.linalg.inv(inertia)[:, None, None] @ skew(r)
    im = (1.0 / mass)[:, None, None, None, None] * eye3
    on = (contact != 0).float()[..., None, None]
    blocks = torch.cat([0.5 * dt * dt * W, (0.5 * dt * dt * im).expand_as(W), dt * W, (dt * im).expand_as(W)], -2) * on
    B = torch.cat([blocks[:, :, f] for f in range(4)], -1)                                        # [n, H, 12, 12]
    stance = (contact != 0).repeat_interleave(5, dim=-1)
    P = torch.diag(q).expand(n, 12, 12)
    K, Gi, Pd = [None] * H, [None] * H, [None] * H
    for k in range(H - 1, -1, -1):
        Bk = B[:, k]
        Pd[k] = P @ d
        PB = P @ Bk
        G = Bk.transpose(1, 2) @ PB + torch.diag(Rt)
        L = torch.linalg.cholesky(G)
        sol = torch.cholesky_solve(torch.cat([PB.transpose(1, 2) @ A, torch.eye(12, device=dev).expand(n, 12, 12)], 2), L)
        K[k], Gi[k] = sol[:, :, :12], sol[:, :, 12:]
        Pn = A.T @ (P @ (A - Bk @ K[k])) + (torch.diag(q) if k > 0 else 0)
        P = 0.5 * (Pn + Pn.transpose(1, 2))
    qx = -q * x_ref
    u = torch.zeros(n, H, 12, device=dev)
    xs = [x0] + [None] * H
    kap = [None] * H
    for _ in range(iters):
        rt = -rho * ((z - y) @ Cm)
        p = qx[:, H - 1]
        for k in range(H - 1, -1, -1):
            s = p + Pd[k]
            v = torch.einsum("nij,ni->nj", B[:, k], s) + rt[:, k]
            kap[k] = torch.einsum("nij,nj->ni", Gi[k], v)
            p = s @ A - torch.einsum("nji,nj->ni", K[k], v)
            if k > 0:
                p = p + qx[:, k - 1]
        us = []
        for k in range(H):
            uk = -torch.einsum("nij,nj->ni", K[k], xs[k]) - kap[k]
            xs[k + 1] = xs[k] @ A.T + torch.einsum("nij,nj->ni", B[:, k], uk) + d
            us.append(uk)
        u = torch.stack(us, 1)
        Cu = u @ Cm.T
        zn = torch.where(stance, torch.minimum(torch.maximum(Cu + y, lo), hi), torch.zeros_like(Cu))
        y = torch.where(stance, y + Cu - zn, torch.zeros_like(Cu))
        z = zn
    return u, torch.stack(xs[1:], 1), z, y


if a.mode == "every":                                                                # the two routes compute the same thing
    hip(40, True, True)
    tu, tx, tz, ty = torch_route(40, torch.zeros(n, H, 20, device=dev), torch.zeros(n, H, 20, device=dev))
    torch.cuda.synchronize()
    scale = float(tu.abs().max())
    print(f"torch route against the kernel, 40 cold iterations: largest difference in u {float((tu - outs['u']).abs().max()):.3g} of {scale:.3g}, in x_pred "
          f"{float((tx - outs['x_pred']).abs().max()):.3g}; statuses {torch.bincount(outs['status'], minlength=3).tolist()}", flush=True)
hip(40, True, True)
warm0 = warm.clone()
calls = {"hip 40 cold, sim state": lambda: hip(40, True, False), "hip 40 cold, explicit": lambda: hip(40, True, True),
         "hip 10 warm, sim state": lambda: hip(10, False, False), "hip 10 warm, explicit": lambda: hip(10, False, True)}
if a.mode == "every":
    z0, y0 = warm0[:, 0].clone(), warm0[:, 1].clone()
    calls.update({"torch 40 cold": lambda: torch_route(40, torch.zeros_like(z0), torch.zeros_like(y0)), "torch 10 warm": lambda: torch_route(10, z0, y0)})
times = {}
for rnd in range(a.rounds):
    for mode, call in calls.items():
        is_hip = mode.startswith("hip")
        calls_n = a.calls if is_hip else max(a.calls // 10, 3)
        for _ in range(5 if is_hip else 2):
            call()
        warm.copy_(warm0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls_n):
            call()
        t1.record()
        torch.cuda.synchronize()
        times.setdefault(mode, []).append(t0.elapsed_time(t1) * 1e3 / calls_n)
        print(f"round {rnd} {mode:24s} N={n} H={H}: {times[mode][-1]:.1f} us per call (device events, back to back)", flush=True)
if a.mode == "every":
    for k, hk in (("torch 40 cold", "hip 40 cold, explicit"), ("torch 10 warm", "hip 10 warm, explicit")):
        print(f"{k}: {min(times[k]):.0f} us against {min(times[hk]):.1f} us, ratio {min(times[k]) / min(times[hk]):.1f}", flush=True)
