"""Time of wbc_sim_footstep_plan (wbc_footstep_plan_kernel) at the bench's env count next to the same plan in torch ops, in one session
and one build:
  * the launch with search_radius 0 and 3, on the plane and on the training heightfield, every output asked for (H = 10);
  * the torch route: refresh_rigid_body_state for the feet, the clock and the nominal footholds as tensor expressions, the candidates'
    heights and probes by gathers on the int16 height samples, argmin, the swing polynomial (the per-stage outputs are left out of it).

  python tools/profile_footstep.py        device-event times of every mode, back to back calls after warm-up, two rounds, alternating

The layout -- the searching feet in sequence, lane = candidate -- was chosen against four feet at once on 16 lanes each by running this
script on a library whose wbc_footstep_kernel.hip was compiled with -DFS_LPF=16 (WBC_AMD_LIB=<that library> python
tools/profile_footstep.py --mode hip)."""
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

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
assert env.height_samples is not None, "the default config trains on a heightfield"
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n, sim, dev = a.envs, env.sim, env.device
terrain = env.terrain
hf = dict(heights=terrain.heightsamples, hs=float(terrain.horizontal_scale), vs=float(terrain.vertical_scale), t=[float(v) for v in terrain.transform])
planners = {R: env.gait_planner("trot", period=0.5, duty=0.5, horizon=10, search_radius=R) for R in (0, 3)}
gen = torch.Generator(device="cuda"); gen.manual_seed(3)
phase0 = torch.rand(n, device="cuda", generator=gen)
cmd = (torch.rand(n, 2, device="cuda", generator=gen) - 0.5)
wz = (torch.rand(n, device="cuda", generator=gen) - 0.5)
for p in planners.values():
    p.reset(phase=phase0)
state0 = {R: p.state.clone() for R, p in planners.items()}
feet = env.feet_indices
H16 = env.height_samples.to(torch.float32)


def set_terrain(name):
    if name == "plane":
        sim.set_heightfield(None)
    else:
        sim.set_heightfield(hf["heights"], hf["hs"], hf["vs"], *hf["t"])


def query(x, y, plane):
    """terrain_query in torch ops: (h, n_z)."""
    if plane:
        return torch.zeros_like(x), torch.ones_like(x)
    rows, cols = H16.shape
    fx, fy = (x - hf["t"][0]) / hf["hs"], (y - hf["t"][1]) / hf["hs"]
    ix, iy = fx.trunc().clamp(0, rows - 2).long(), fy.trunc().clamp(0, cols - 2).long()
    u, v = (fx - ix).clamp(0, 1), (fy - iy).clamp(0, 1)
    flat = H16.reshape(-1)
    h00, h10 = flat[ix * cols + iy] * hf["vs"], flat[(ix + 1) * cols + iy] * hf["vs"]
    h01, h11 = flat[ix * cols + iy + 1] * hf["vs"], flat[(ix + 1) * cols + iy + 1] * hf["vs"]
    low = u >= v
    dhdx, dhdy = torch.where(low, h10 - h00, h11 - h01), torch.where(low, h11 - h10, h01 - h00)
    h = h00 + u * dhdx + v * dhdy + hf["t"][2]
    gx, gy = dhdx / hf["hs"], dhdy / hf["hs"]
    return h, torch.rsqrt(gx * gx + gy * gy + 1)


def torch_route(R, plane, state):
    c = planners[R].cfg
    sim.refresh_rigid_body_state()
    root = env.root_states
    p = env.rigid_body_state[:, feet, 0:3]
    pd = env.rigid_body_state[:, feet, 7:10]
    offset = torch.tensor(list(c.offset), device=dev)
    so = torch.tensor([[c.stance_offset[i][0], c.stance_offset[i][1]] for i in range(4)], device=dev)
    phase = state[:, 0]
    phi = torch.remainder(phase[:, None] + offset[None], 1.0)
    stand = phi < c.duty
    s = torch.where(stand, torch.zeros_like(phi), (phi - c.duty) / (1 - c.duty))
    fs = state[:, 4:].view(n, 4, 7)
    flag = fs[:, :, 6]
    lifted, touched = ~stand & (flag == 0), stand & (flag != 0)
    lift = torch.where(lifted[..., None], p, fs[:, :, 0:3])
    target = torch.where(touched[..., None], p, fs[:, :, 3:6])
    Tst, Tsw = c.duty * c.period, (1 - c.duty) * c.period
    t = torch.where(stand, (c.duty - phi) * c.period + Tsw, (1 - s) * Tsw)
    x, y, z, w = root[:, 3:7].unbind(-1)
    yaw = torch.atan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))
    ch, sh = torch.cos(yaw), torch.sin(yaw)
    vc = torch.stack([ch * cmd[:, 0] - sh * cmd[:, 1], sh * cmd[:, 0] + ch * cmd[:, 1]], -1)
    yt = yaw[:, None] + wz[:, None] * t
    ct, st = torch.cos(yt), torch.sin(yt)
    hip = root[:, None, 0:2] + vc[:, None] * t[..., None] + torch.stack([ct * so[:, 0] - st * so[:, 1], st * so[:, 0] + ct * so[:, 1]], -1)
    v = root[:, 7:10]
    kc = 0.5 * (c.com_height / 9.81) ** 0.5
    add = 0.5 * Tst * v[:, 0:2] + c.k_v * (v[:, 0:2] - vc) + kc * torch.stack([v[:, 1] * wz, -v[:, 0] * wz], -1)
    ln = add.norm(dim=-1, keepdim=True)
    add = torch.where(ln > c.max_reach, add * (c.max_reach / ln.clamp_min(1e-12)), add)
    nom = hip + add[:, None]
    ar = torch.arange(-R, R + 1, device=dev, dtype=torch.float32) * c.search_step
    d = torch.stack(torch.meshgrid(ar, ar, indexing="ij"), -1).reshape(-1, 2)                              # [K, 2]
    cand = nom[:, :, None, :] + d
    h, nz = query(cand[..., 0], cand[..., 1], plane)
    rough = torch.zeros_like(h)
    for dx, dy in ((c.probe_radius, 0.0), (-c.probe_radius, 0.0), (0.0, c.probe_radius), (0.0, -c.probe_radius)):
        hp, _ = query(cand[..., 0] + dx, cand[..., 1] + dy, plane)
        rough = torch.maximum(rough, (hp - h).abs())
    cost = c.w_dist * (d * d).sum(-1) + c.w_rough * rough * rough + c.w_slope * (1 - nz)
    cost = torch.where((rough > c.rough_max) | (nz < c.nz_min), torch.full_like(cost, float("inf")), cost)
    best = cost.argmin(-1, keepdim=True)
    none = torch.isinf(cost.gather(-1, best))[..., 0]
    hn, _ = query(nom[..., 0], nom[..., 1], plane)
    found = torch.stack([cand[..., 0].gather(-1, best)[..., 0], cand[..., 1].gather(-1, best)[..., 0], h.gather(-1, best)[..., 0]], -1)
    found = torch.where(none[..., None], torch.cat([nom, hn[..., None]], -1), found)
    search = ~stand & (s < c.latch)
    target = torch.where(search[..., None], found, target)
    bump = lambda q: (q ** 3 * (10 - 15 * q + 6 * q * q), 30 * q * q * (1 - q) ** 2, 60 * q * (1 - q) * (1 - 2 * q))    # noqa: E731
    sd = 1 / Tsw
    b0, b1, b2 = bump(s)
    dxy = target[..., 0:2] - lift[..., 0:2]
    za = torch.maximum(lift[..., 2], target[..., 2]) + c.swing_height
    up = s < 0.5
    z0, z1, z2 = bump(torch.where(up, 2 * s, 2 * s - 1))
    zs, dz = torch.where(up, lift[..., 2], za), torch.where(up, za - lift[..., 2], target[..., 2] - za)
    pos = torch.cat([lift[..., 0:2] + dxy * b0[..., None], (zs + dz * z0)[..., None]], -1)
    vel = torch.cat([dxy * (b1 * sd)[..., None], (dz * z1 * 2 * sd)[..., None]], -1)
    acc = torch.cat([dxy * (b2 * sd * sd)[..., None], (dz * z2 * 4 * sd * sd)[..., None]], -1)
    sacc = torch.where(stand[..., None], torch.zeros_like(acc), acc + c.kp * (pos - p) + c.kd * (vel - pd))
    foothold = torch.where(stand[..., None], torch.cat([nom, hn[..., None]], -1), target)
    return stand, foothold, sacc


def hip(R):
    planners[R]._launch(vel_cmd=cmd, yaw_rate=wz, hold=True)                       # the launch alone, the clock held


if a.mode == "every":                                                              # the two routes compute the same thing
    for name in ("heightfield", "plane"):
        set_terrain(name)
        for R in (0, 3):
            planners[R].state.copy_(state0[R])
            stand, fh, sacc = torch_route(R, name == "plane", state0[R])
            hip(R)
            torch.cuda.synchronize()
            p = planners[R]
            same = (stand == p.stance.bool()).all(dim=1) & ((fh - p.footholds).abs().amax(dim=(1, 2)) < 1e-3)
            print(f"{name} R={R}: torch route against the kernel: stance equal in {float((stand == p.stance.bool()).float().mean()):.4f} of the feet, "
                  f"envs with every foothold within 1 mm {float(same.float().mean()):.4f}, largest swing_acc difference there "
                  f"{float((sacc - p.swing_acc)[same].abs().max()) if bool(same.any()) else float('nan'):.3g}", flush=True)
calls = {}
for name in ("heightfield", "plane"):
    for R in (0, 3):
        calls[f"hip {name} R={R}"] = (name, lambda R=R: hip(R))
        if a.mode == "every":
            calls[f"torch {name} R={R}"] = (name, lambda R=R, name=name: torch_route(R, name == "plane", state0[R]))
times = {}
for rnd in range(a.rounds):
    for mode, (name, call) in calls.items():
        set_terrain(name)
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
        print(f"round {rnd} {mode:28s} N={n}: {times[mode][-1]:.2f} us per call (device events, back to back)", flush=True)
for name in ("heightfield", "plane"):
    for R in (0, 3):
        h = min(times[f"hip {name} R={R}"])
        if a.mode == "every":
            t = min(times[f"torch {name} R={R}"])
            print(f"{name} R={R}: HIP {h:.2f} us, torch route {t:.2f} us, ratio {t / h:.1f}", flush=True)
        else:
            print(f"{name} R={R}: HIP {h:.2f} us", flush=True)
