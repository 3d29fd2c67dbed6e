"""Time of the whole-body Jacobian / mass-matrix refresh (wbc_body_dynamics_kernel) at the bench's env count, and the bytes it
writes. Run alone for device-event times, or under `rocprofv3 --kernel-trace --stats` with one --mode for the kernel time of that
mode (both: J + M, 80.1 MB at 4096 envs; mm: M only, 11.1 MB; jac: J only)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import torch  # noqa: E402

from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--mode", choices=["both", "mm", "jac", "all"], default="all")
a = ap.parse_args()
cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
jac, mm = env.jacobian_whole, env.mm_whole
outs = {"both": dict(jac=jac, mm=mm), "mm": dict(mm=mm), "jac": dict(jac=jac)}
for mode in (["both", "mm", "jac"] if a.mode == "all" else [a.mode]):
    kw = outs[mode]
    nbytes = sum(t.numel() * 4 for t in kw.values())
    for _ in range(10):
        env.sim.body_dynamics(**kw)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        env.sim.body_dynamics(**kw)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / a.iters
    print(f"{mode:4s} N={a.envs}: {nbytes / 1e6:.1f} MB per refresh, {us:.2f} us per launch (device events, back to back), "
          f"{nbytes / us / 1e6:.2f} TB/s")
