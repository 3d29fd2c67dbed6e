"""Time of the mass-matrix solves and of forward dynamics (wbc_mass_solve_kernel) at the bench's env count, next to their yardsticks
(the M-only launch of wbc_body_dynamics_kernel, the h-only launch of wbc_inverse_dynamics_kernel) and to the route that existed
before them (refresh_mass_matrix_tensors() + torch.linalg.solve on the gathered 24x24 live block), in one session and one build.

  python tools/profile_mass_solve.py                      device-event times of every mode, back to back launches, two rounds
  python tools/profile_mass_solve.py --rocprof DIR        one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child
                                                          process each, under its own time limit; the first failure ends the
                                                          session) and the kernels' average times from the stats files

Modes: solve1 / solve6 / solve32 (nrhs right-hand sides; solve6 takes the strided view jacobian_whole[:, gripper]), fd (forward
dynamics: the h launch and the solve launch), mm (M only), h (h only), torch1 / torch6 (the earlier route, device events only).
WBC_AMD_LIB selects a variant library (tools/build_variant.py ms_epw1 -DMS_EPW=1: one env per wavefront)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["solve1", "solve6", "solve32", "fd", "mm", "h"]
MODES = KERNEL_MODES + ["torch1", "torch6"]
KERNELS = {"solve1": ["wbc_mass_solve_kernel"], "solve6": ["wbc_mass_solve_kernel"], "solve32": ["wbc_mass_solve_kernel"],
           "fd": ["wbc_inverse_dynamics_kernel", "wbc_mass_solve_kernel"], "mm": ["wbc_body_dynamics_kernel"],
           "h": ["wbc_inverse_dynamics_kernel"]}

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", choices=MODES + ["all"], default="all")
ap.add_argument("--rocprof", metavar="DIR", help="profile every kernel mode under rocprofv3, outputs below DIR")
ap.add_argument("--limit", type=int, default=240, help="seconds each profiled child may take")
a = ap.parse_args()

if a.rocprof:
    os.makedirs(a.rocprof, exist_ok=True)
    for mode in (KERNEL_MODES if a.mode == "all" else [a.mode]):
        out = os.path.join(a.rocprof, mode)
        cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--iters", str(a.iters), "--rounds", "1", "--mode", mode]
        rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
        if rc != 0:
            sys.exit(f"{mode}: the profiled run ended with status {rc}; nothing more is started")
        rows = [r for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
        for kernel in KERNELS[mode]:
            hit = [r for r in rows if r["Name"].startswith(kernel)]
            if not hit:
                sys.exit(f"{mode}: {kernel} is not in the kernel statistics under {out}")
            r = hit[0]
            print(f"{mode:8s} N={a.envs}: {kernel} {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
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
tau, mm = env.bias_forces, env.mm_whole
env.refresh_jacobian_tensors()
grip = env.robot_model.rb_names.index("wx250s/ee_gripper_link")
b1, b32 = torch.randn(n, 1, 26, device="cuda"), torch.randn(n, 32, 26, device="cuda")
b6 = env.jacobian_whole[:, grip]                                                   # [N, 6, 26], env stride 27 * 156
o1, o6, o32, nd = torch.empty(n, 1, 26, device="cuda"), torch.empty(n, 6, 26, device="cuda"), torch.empty_like(b32), torch.empty_like(tau)
live = torch.tensor([c for c in range(26) if c not in (24, 25)], device="cuda")


def torch_route(b):
    """What a user had before: the mass-matrix tensor, its live 24x24 block, a batched dense solve."""
    env.refresh_mass_matrix_tensors()
    M = mm[:, live][:, :, live]
    return torch.linalg.solve(M, b[:, :, live].transpose(1, 2))


calls = {"solve1": lambda: env.sim.mass_solve(b1, out=o1), "solve6": lambda: env.sim.mass_solve(b6, out=o6),
         "solve32": lambda: env.sim.mass_solve(b32, out=o32), "fd": lambda: env.sim.forward_dynamics(b1[:, 0], out=nd),
         "mm": lambda: env.sim.body_dynamics(mm=mm), "h": lambda: env.sim.inverse_dynamics(tau=tau),
         "torch1": lambda: torch_route(b1), "torch6": lambda: torch_route(b6)}
for rnd in range(a.rounds):
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
        print(f"round {rnd} {mode:8s} N={n}: {t0.elapsed_time(t1) * 1e3 / a.iters:.2f} us per call (device events, back to back)", flush=True)
