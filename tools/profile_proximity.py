"""Time of wbc_sim_proximity (wbc_proximity_kernel) at the bench's env count, next to its yardstick and to the route it replaces, in one
session and one build:
  * the launch with every output, with gap + nearest only and with gap + jac, against the M-only launch of wbc_body_dynamics_kernel;
  * the torch route: refresh_rigid_body_state + refresh_jacobian_tensors (69 MB of J at 4096 envs) + the same geometry in torch ops
    (the nine feature pairs of the 44 limb pairs, the three spheres against the trunk box, the rows from the rigid bodies' Jacobians).

  python tools/profile_proximity.py                     device-event times of every mode, back to back launches, two rounds, alternating
  python tools/profile_proximity.py --rocprof DIR       one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child
                                                        process each, under its own time limit; the first failure ends the
                                                        session) and the kernels' average times from the stats files

Modes: all (every output), gapnear (gap and nearest, k = 4), gapjac (gap and jac), mm (the M-only body_dynamics launch), torch (the torch
route, device events only)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["all", "gapnear", "gapjac", "mm"]
MODES = KERNEL_MODES + ["torch"]
KERNELS = {m: "wbc_proximity_kernel" for m in ("all", "gapnear", "gapjac")}
KERNELS.update(mm="wbc_body_dynamics_kernel")

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", choices=MODES + ["every"], default="every")
ap.add_argument("--rocprof", metavar="DIR", help="profile every kernel mode under rocprofv3, outputs below DIR")
ap.add_argument("--limit", type=int, default=240, help="seconds each profiled child may take")
a = ap.parse_args()

if a.rocprof:
    os.makedirs(a.rocprof, exist_ok=True)
    for mode in (KERNEL_MODES if a.mode == "every" else [a.mode]):
        out = os.path.join(a.rocprof, mode)
        cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--iters", str(a.iters), "--rounds", "1", "--mode", mode]
        rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
        if rc != 0:
            sys.exit(f"{mode}: the profiled run ended with status {rc}; nothing more is started")
        rows = [r for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
        hit = [r for r in rows if r["Name"].startswith(KERNELS[mode])]
        if not hit:
            sys.exit(f"{mode}: {KERNELS[mode]} is not in the kernel statistics under {out}")
        r = hit[0]
        print(f"{mode:8s} N={a.envs}: {KERNELS[mode]} {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
              f"min {float(r['MinNs']) / 1e3:.2f} us, max {float(r['MaxNs']) / 1e3:.2f} us", flush=True)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import torch  # noqa: E402

from wbc_amd import abi  # noqa: E402
from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n = a.envs
sim, L = env.sim, env.sim.L
P = len(sim.proximity_pair_ids)
new = lambda *shape: torch.empty(*shape, device="cuda")  # noqa: E731
gap, normal, witness, jac, near = new(n, P), new(n, P, 3), new(n, P, 2, 3), new(n, P, 26), torch.empty(n, 4, dtype=torch.int32, device="cuda")
mm = new(n, 26, 26)

# ---- the torch route's tables: rigid bodies of the limbs' ends and of the limbs themselves, the nine features' radii -----------------------
cps, limbs, _ = abi.collision_set(env.robot_model)
sph_rb = {c["sph"]: c["rb"] for c in cps if c["kind"] == abi.CP_TERRAIN and c["sph"] >= 0 and c["body"] != abi.BOX_BODY}
ids = sim.proximity_pair_ids
lp = ids[ids[:, 0] == abi.PR_LIMBS]
idx = lambda v: torch.tensor(v, device="cuda", dtype=torch.long)  # noqa: E731
A0, A1 = idx([sph_rb[limbs[p]["s0"]] for p in lp[:, 1]]), idx([sph_rb[limbs[p]["s1"]] for p in lp[:, 1]])
B0, B1 = idx([sph_rb[limbs[p]["s0"]] for p in lp[:, 2]]), idx([sph_rb[limbs[p]["s1"]] for p in lp[:, 2]])
RA, RB = idx([limbs[p]["rb"] for p in lp[:, 1]]), idx([limbs[p]["rb"] for p in lp[:, 2]])
rad = lambda col, keys: torch.tensor([[limbs[p][k] for k in keys] for p in lp[:, col]], device="cuda")  # noqa: E731
# feature f: A's part (0 shaft, 1 / 2 an end sphere), B's part, in the kernel's order
FA, FB = [0, 1, 2, 0, 0, 1, 1, 2, 2], [0, 0, 0, 1, 2, 1, 2, 1, 2]
ra, rb = rad(1, ("radius", "cap0", "cap1"))[:, FA], rad(2, ("radius", "cap0", "cap1"))[:, FB]          # [44, 9]
missing = (ra <= 0) | (rb <= 0)
missing[:, 0] = False
sp = ids[ids[:, 0] == abi.PR_STATIC]
SB = idx([sph_rb[s] for s in sp[:, 1]])
sb_r = torch.tensor([next(c["radius"] for c in cps if c["sph"] == s and c["kind"] == abi.CP_TERRAIN) for s in sp[:, 1]], device="cuda")
trunk_rb = env.robot_model.rb_names.index("trunk")
half = torch.tensor(abi.TRUNK_HALF, device="cuda")
clamp01 = lambda x: x.clamp(0.0, 1.0)  # noqa: E731
dot = lambda u, v: (u * v).sum(-1)  # noqa: E731


def point_rows(J, rbs, c, x, nrm):
    """n . (linear point Jacobian at c riding on rigid bodies rbs): [N, K, 26]."""
    Jb = J[:, rbs]                                                              # [N, K, 6, 26]
    r = c - x[:, rbs]
    return torch.einsum("nkj,nkjc->nkc", nrm, Jb[:, :, 0:3]) + torch.einsum("nkj,nkjc->nkc", torch.cross(r, nrm, dim=-1), Jb[:, :, 3:6])


def torch_route():
    sim.refresh_rigid_body_state(); sim.refresh_jacobian_tensors()
    x, J = env.rigid_body_state[:, :, :3], sim.acquire_jacobian_tensor()
    a0, a1, b0, b1 = x[:, A0], x[:, A1], x[:, B0], x[:, B1]
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    aa, ee, f, c, b = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
    den = aa * ee - b * b
    s = torch.where(den > 1e-7 * aa * ee, clamp01((b * f - c * ee) / den.clamp_min(1e-30)), torch.zeros_like(den))
    t = (b * s + f) / ee
    s = torch.where(t < 0, clamp01(-c / aa), torch.where(t > 1, clamp01((b - c) / aa), s))
    t = clamp01(t)
    on_b = lambda pnt: clamp01(dot(pnt - b0, d2) / ee)  # noqa: E731
    on_a = lambda pnt: clamp01(dot(pnt - a0, d1) / aa)  # noqa: E731
    zero, one = torch.zeros_like(s), torch.ones_like(s)
    S = torch.stack([s, zero, one, on_a(b0), on_a(b1), zero, zero, one, one], -1)      # [N, 44, 9]
    T = torch.stack([t, on_b(a0), on_b(a1), zero, one, zero, one, zero, one], -1)
    pa, pb = a0.unsqueeze(2) + d1.unsqueeze(2) * S.unsqueeze(-1), b0.unsqueeze(2) + d2.unsqueeze(2) * T.unsqueeze(-1)
    dist = (pa - pb).norm(dim=-1)
    g = torch.where(missing, torch.full_like(dist, 3e38), dist - ra - rb)
    w = g.argmin(-1, keepdim=True)
    take = lambda v: v.gather(2, w.unsqueeze(-1).expand(-1, -1, -1, 3)).squeeze(2)  # noqa: E731
    ca, cb, gl = take(pa), take(pb), g.gather(2, w).squeeze(2)
    nl = (ca - cb) / dist.gather(2, w)
    rows_l = point_rows(J, RA, ca, x, nl) - point_rows(J, RB, cb, x, nl)
    # the spheres against the trunk box
    q = env.rigid_body_state[:, trunk_rb, 3:7]
    qv, qw = q[:, None, :3], q[:, None, 3:4]
    rot = lambda v, sgn: v + 2 * torch.cross(sgn * qv.expand_as(v), torch.cross(sgn * qv.expand_as(v), v, dim=-1) + qw * v, dim=-1)  # noqa: E731
    cs = x[:, SB]
    loc = rot(cs - x[:, trunk_rb:trunk_rb + 1], -1.0)
    cl = torch.minimum(torch.maximum(loc, -half), half)
    inside = (loc.abs() <= half).all(-1, keepdim=True)
    depth = half - loc.abs()
    face = torch.nn.functional.one_hot(depth.argmin(-1), 3).to(loc.dtype) * torch.where(loc < 0, -1.0, 1.0)
    dv = loc - cl
    dn = dv.norm(dim=-1, keepdim=True)
    ns = rot(torch.where(inside, face, dv / dn.clamp_min(1e-30)), 1.0)
    gs = torch.where(inside.squeeze(-1), -depth.min(-1).values, dn.squeeze(-1)) - sb_r
    rows_s = point_rows(J, SB, cs, x, ns)                                          # the box rides on the root: no joint moves it
    rows = torch.cat([rows_l, rows_s], 1)
    rows[:, :, :6] = 0
    return torch.cat([gl, gs], 1), torch.cat([nl, ns], 1), rows


def kernel(**outs):
    """The C-ABI call with NULL for the outputs that are not asked for."""
    ptrs = [outs[k].data_ptr() if k in outs else None for k in ("gap", "normal", "witness", "jac", "nearest")]
    rc = L.wbc_sim_proximity(sim.h, *ptrs, 4, sim._stream())
    assert rc == 0, L.wbc_last_error()


calls = {"all": lambda: kernel(gap=gap, normal=normal, witness=witness, jac=jac, nearest=near), "gapnear": lambda: kernel(gap=gap, nearest=near),
         "gapjac": lambda: kernel(gap=gap, jac=jac), "mm": lambda: sim.body_dynamics(mm=mm), "torch": torch_route}
if a.mode in ("every", "torch"):                                                   # the two routes compute the same thing
    kernel(gap=gap, jac=jac)
    tg, _, tj = torch_route()
    torch.cuda.synchronize()
    print(f"torch route against the kernel: largest |gap| difference {float((tg - gap).abs().max()):.3g} m, "
          f"largest |jac| difference {float((tj - jac).abs().max()):.3g}", flush=True)
for rnd in range(a.rounds):
    for mode in (MODES if a.mode == "every" else [a.mode]):
        call = calls[mode]
        iters = a.iters
        for _ in range(3 if mode == "torch" else 10):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        print(f"round {rnd} {mode:8s} N={n}: {t0.elapsed_time(t1) * 1e3 / iters:.2f} us per call (device events, back to back)", flush=True)
