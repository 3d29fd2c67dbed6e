"""Time of wbc_sim_centroidal (wbc_centroidal_kernel) at the bench's env count, next to its yardstick (the h-only launch of
wbc_inverse_dynamics_kernel) and to the route that existed before it, in one session and one build: refresh_mass_matrix_tensors(),
two inverse-dynamics launches (tau and g) and the torch algebra that picks m and m c x out of M's root block and moves the angular
rows of M and of tau - g from the root origin to the centre of mass.

  python tools/profile_centroidal.py                      device-event times of every mode, back to back launches, two rounds
  python tools/profile_centroidal.py --rocprof DIR        one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child
                                                          process each, under its own time limit; the first failure ends the
                                                          session) and the kernels' average times from the stats files

Modes: all (the four outputs, nudot given), all0 (nudot NULL), mom (mom alone), cmm (A_G alone), com (com alone), h (the h-only
inverse-dynamics launch), composed (the earlier route, device events only; it prints its largest difference from the kernel once).
WBC_AMD_LIB selects a variant library (tools/build_variant.py cm_epw1 -DCM_EPW=1: one env per wavefront)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["all", "all0", "mom", "cmm", "com", "h"]
MODES = KERNEL_MODES + ["composed"]
KERNELS = {m: "wbc_centroidal_kernel" for m in KERNEL_MODES}
KERNELS["h"] = "wbc_inverse_dynamics_kernel"

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

from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n = a.envs
sim, L = env.sim, env.sim.L
nudot = torch.randn(n, 26, device="cuda") * 5.0
com, mom, cmm, inr = sim.centroidal(nudot)
tau, grav, mm = torch.empty(n, 26, device="cuda"), torch.empty(n, 26, device="cuda"), env.mm_whole


def kernel(nd, **outs):
    """The C-ABI call with NULL for the outputs that are not asked for."""
    ptr = [outs[k].data_ptr() if k in outs else None for k in ("com", "mom", "cmm", "inertia")]
    rc = L.wbc_sim_centroidal(sim.h, nd.data_ptr() if nd is not None else None, *ptr, sim._stream())
    assert rc == 0, L.wbc_last_error()


def hat(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], 1).view(-1, 3, 3)


def composed():
    """What a user had before: (c - p_root, h_G, hdot_G, A_G, m, I_G) from mm_whole and two inverse-dynamics launches."""
    env.refresh_mass_matrix_tensors()
    sim.inverse_dynamics(nudot=nudot, tau=tau)
    sim.inverse_dynamics(grav=grav)
    mass = mm[:, 0, 0]
    mcx = mm[:, 3:6, 0:3]                                                          # m [c]x
    c = torch.stack([mcx[:, 2, 1], mcx[:, 0, 2], mcx[:, 1, 0]], 1) / mass[:, None]
    cx = hat(c)
    A = torch.cat([mm[:, 0:3], mm[:, 3:6] - cx @ mm[:, 0:3]], 1)
    nu = torch.cat([env.root_states[:, 7:13], env.dof_vel], 1)
    h = (A @ nu[:, :, None])[:, :, 0]
    w = tau - grav
    hd = torch.cat([w[:, 0:3], w[:, 3:6] - (cx @ w[:, 0:3, None])[:, :, 0]], 1)
    return c, h, hd, A, mass, A[:, 3:6, 3:6]


calls = {"all": lambda: kernel(nudot, com=com, mom=mom, cmm=cmm, inertia=inr), "all0": lambda: kernel(None, com=com, mom=mom, cmm=cmm, inertia=inr),
         "mom": lambda: kernel(nudot, mom=mom), "cmm": lambda: kernel(nudot, cmm=cmm), "com": lambda: kernel(nudot, com=com),
         "h": lambda: sim.inverse_dynamics(tau=tau), "composed": composed}
if a.mode in ("every", "composed"):
    kernel(nudot, com=com, mom=mom, cmm=cmm, inertia=inr)
    c, h, hd, A, mass, IG = composed()
    torch.cuda.synchronize()
    diffs = {"c": (c - com[:, 0:3]).abs().max(), "h_G": (h - mom[:, 0:6]).abs().max(), "hdot_G": (hd - mom[:, 6:12]).abs().max(),
             "A_G": (A - cmm).abs().max(), "m": (mass - inr[:, 0]).abs().max()}
    print("composed route vs kernel, largest absolute difference: " + ", ".join(f"{k} {float(v):.3g}" for k, v in diffs.items()), flush=True)
for rnd in range(a.rounds):
    for mode in (MODES if a.mode == "every" else [a.mode]):
        call = calls[mode]
        for _ in range(10):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        print(f"round {rnd} {mode:8s} N={n}: {t0.elapsed_time(t1) * 1e3 / a.iters:.2f} us per call (device events, back to back)", flush=True)
