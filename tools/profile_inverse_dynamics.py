"""Time of the whole-body inverse dynamics (wbc_inverse_dynamics_kernel) at the bench's env count, next to its yardstick, the
mass-matrix-only launch of wbc_body_dynamics_kernel, in one session and one build.

  python tools/profile_inverse_dynamics.py                      device-event times of every mode, back to back launches
  python tools/profile_inverse_dynamics.py --rocprof DIR        one `rocprofv3 --kernel-trace --stats` run per mode (a fresh child
                                                                process each, under its own time limit; the first failure ends
                                                                the session) and the kernels' average times from the stats files

Modes: h (tau only, nudot = NULL), h+grav (both outputs), nudot (tau with an acceleration input), grav (g(q) only), mm (M only)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["h", "h+grav", "nudot", "grav", "mm"]
KERNEL = {m: "wbc_inverse_dynamics_kernel" for m in MODES}
KERNEL["mm"] = "wbc_body_dynamics_kernel"

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--mode", choices=MODES + ["all"], default="all")
ap.add_argument("--rocprof", metavar="DIR", help="profile every mode under rocprofv3, outputs below DIR")
ap.add_argument("--limit", type=int, default=240, help="seconds each profiled child may take")
a = ap.parse_args()

if a.rocprof:
    os.makedirs(a.rocprof, exist_ok=True)
    for mode in (MODES if a.mode == "all" else [a.mode]):
        out = os.path.join(a.rocprof, mode.replace("+", "_"))
        cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--iters", str(a.iters), "--mode", mode]
        rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
        if rc != 0:
            sys.exit(f"{mode}: the profiled run ended with status {rc}; nothing more is started")
        rows = [r for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
        hit = [r for r in rows if r["Name"].startswith(KERNEL[mode])]
        if not hit:
            sys.exit(f"{mode}: {KERNEL[mode]} is not in the kernel statistics under {out}")
        r = hit[0]
        print(f"{mode:7s} N={a.envs}: {KERNEL[mode]} {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
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
tau, grav, mm = env.bias_forces, torch.empty_like(env.bias_forces), env.mm_whole
nudot = torch.randn_like(tau) * 10
calls = {"h": lambda: env.sim.inverse_dynamics(tau=tau), "h+grav": lambda: env.sim.inverse_dynamics(tau=tau, grav=grav),
         "nudot": lambda: env.sim.inverse_dynamics(nudot=nudot, tau=tau), "grav": lambda: env.sim.inverse_dynamics(grav=grav),
         "mm": lambda: env.sim.body_dynamics(mm=mm)}
for mode in (MODES if a.mode == "all" else [a.mode]):
    call = calls[mode]
    for _ in range(10):
        call()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        call()
    t1.record()
    torch.cuda.synchronize()
    print(f"{mode:7s} N={a.envs}: {t0.elapsed_time(t1) * 1e3 / a.iters:.2f} us per launch (device events, back to back)")
