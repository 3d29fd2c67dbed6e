"""Time of wbc_sim_attitude_filter (wbc_attitude_filter_kernel) next to the same filter in torch ops, in one session:
  * the launch with every output and with the state alone (gyro, accelerometer and one heading vector given);
  * the torch route: the predict as batched 6 x 6 matmuls with Phi, then per measurement H P H^T + r I, torch.linalg.cholesky on the
    3 x 3, two triangular solves, the quaternion composition and P - W^T W as tensor expressions.

  python tools/profile_attitude.py [--envs 4096]     device-event times of every mode, back to back calls after warm-up, two rounds

The layout variant (the same lane = env code on 16 lanes of four times as many wavefronts) is timed by running this script on a library
whose wbc_attitude_kernel.hip was compiled with -DAT_EPW=16 (python tools/build_variant.py at16 -DAT_EPW=16;
WBC_AMD_LIB=<that library> python tools/profile_attitude.py --mode hip)."""
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
att = env.attitude_estimator()
imu = env.imu(gyro_bias=0.02, gyro_noise=0.002, accel_noise=0.05, heading_noise=0.01, seed=3)
c = att.cfg
gyro, accel, heading = imu.read()
for _ in range(3):                                                                  # a covariance with every block filled
    att.update(gyro=gyro, accel=accel, aux=(heading, imu.heading_world, 0.05))
aux_body = heading.reshape(n, 1, 3).contiguous()
aux_world = imu.heading_world.expand(n, 1, 3).contiguous()
aux_sigma = torch.full((n, 1), 0.05, device=dev)
q0, b0, P0 = att.quat.clone(), att.bias.clone(), att.P.clone()
q, b, P = q0.clone(), b0.clone(), P0.clone()
gravity = torch.tensor(list(env.tcfg.gravity), dtype=torch.float32, device=dev)
gn = gravity.norm()
up = -gravity / gn
eye3, eye6 = torch.eye(3, device=dev), torch.eye(6, device=dev)


def hip_all():
    sim.attitude_filter(c, q, b, P, gyro=gyro, accel=accel, aux_body=aux_body, aux_world=aux_world, aux_sigma=aux_sigma, gyro_out=att.gyro,
                        gravity_body=att.gravity_body, nis=att.nis, status=att.status)


def hip_state():
    sim.attitude_filter(c, q, b, P, gyro=gyro, accel=accel, aux_body=aux_body, aux_world=aux_world, aux_sigma=aux_sigma)


def quat_mul(x, y):
    xv, xw, yv, yw = x[:, :3], x[:, 3:], y[:, :3], y[:, 3:]
    return torch.cat([xw * yv + yw * xv + torch.linalg.cross(xv, yv, dim=-1), xw * yw - (xv * yv).sum(-1, keepdim=True)], dim=-1)


def quat_to_mat(x):
    v, w = x[:, :3], x[:, 3]
    S = skew(v)
    return eye3 + 2 * w[:, None, None] * S + 2 * S @ S


def skew(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], dim=-1).view(-1, 3, 3)


def exp_quat(phi):
    ang = phi.norm(dim=-1, keepdim=True)
    small = ang < 1e-4
    s = torch.where(small, 0.5 * (1 - ang * ang / 24), torch.sin(0.5 * ang) / ang.clamp_min(1e-30))
    return torch.cat([phi * s, torch.where(small, 1 - ang * ang / 8, torch.cos(0.5 * ang))], dim=-1)


def compose(x, phi):
    o = quat_mul(x, exp_quat(phi))
    return o / o.norm(dim=-1, keepdim=True)


def torch_route(q, b, P):
    """(q, b, P, nis) of one filter step, torch ops only."""
    dt = c.dt
    dq = exp_quat((gyro - b) * dt)
    q = quat_mul(q, dq); q = q / q.norm(dim=-1, keepdim=True)
    F = eye6.repeat(n, 1, 1)
    F[:, :3, :3] = quat_to_mat(dq).transpose(1, 2)
    F[:, :3, 3:] = -dt * eye3
    Q = torch.diag(torch.tensor([dt * c.sigma_g ** 2] * 3 + [dt * c.sigma_b ** 2] * 3, device=dev))
    P = F @ P @ F.transpose(1, 2) + Q
    x = (accel.norm(dim=-1) - gn) / gn
    nis = []
    for w, u, r in ((up.expand(n, 3), accel, c.sigma_a ** 2 * (1 + c.kappa_a * x * x)), (aux_world[:, 0], aux_body[:, 0], aux_sigma[:, 0] ** 2)):
        m = u / u.norm(dim=-1, keepdim=True)
        mh = (quat_to_mat(q).transpose(1, 2) @ (w / w.norm(dim=-1, keepdim=True)).unsqueeze(-1)).squeeze(-1)
        H = torch.cat([skew(mh), torch.zeros(n, 3, 3, device=dev)], dim=-1)
        HP = H @ P
        L = torch.linalg.cholesky(HP @ H.transpose(1, 2) + r[:, None, None] * eye3)
        W = torch.linalg.solve_triangular(L, HP, upper=False)
        y = torch.linalg.solve_triangular(L, (m - mh).unsqueeze(-1), upper=False)
        dx = (W.transpose(1, 2) @ y).squeeze(-1)
        q, b, P = compose(q, dx[:, :3]), b + dx[:, 3:], P - W.transpose(1, 2) @ W
        nis.append((y * y).sum(dim=(1, 2)))
    return q, b, P, torch.stack(nis, dim=1)


if a.mode == "every":                                                                  # the two routes compute the same thing
    tq, tb, tP, tnis = torch_route(q0, b0, P0)
    hip_all()
    torch.cuda.synchronize()
    print(f"torch route against the kernel: largest difference in q {float((tq - q).abs().max()):.3g}, in b {float((tb - b).abs().max()):.3g} "
          f"(largest |b| {float(b.abs().max()):.3g}), in P {float((tP - P).abs().max()):.3g} (largest |P| {float(P.abs().max()):.3g}), in nis "
          f"{float((tnis - att.nis).abs().max()):.3g} (largest nis {float(att.nis.max()):.3g}); status words {sorted(set(att.status.cpu().tolist()))}", flush=True)
calls = {"hip every output": hip_all, "hip state only": hip_state}
if a.mode == "every":
    calls["torch"] = lambda: torch_route(q0, b0, P0)
times = {}
for rnd in range(a.rounds):
    for mode, call in calls.items():
        iters = a.iters if mode.startswith("hip") else max(a.iters // 10, 5)
        q.copy_(q0); b.copy_(b0); P.copy_(P0)
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
