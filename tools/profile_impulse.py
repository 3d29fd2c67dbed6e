"""Time of contact impulses and post-impact velocities (wbc_sim_impulse_dynamics: wbc_impulse_rhs_kernel, the mass solve,
wbc_impulse_solve_kernel or its map variant) at the bench's env count, next to wbc_sim_constrained_dynamics on the same bodies (the
same chain plus the h launch) and to the only route to the same result that existed before, in one session and one build.

  python tools/profile_impulse.py                  device-event times of every mode, back to back calls, two rounds, the new call, the
                                                   sibling and the torch route alternating in one process
  python tools/profile_impulse.py --rocprof DIR    one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child process
                                                   each, under its own time limit; the first failure ends the session) and the kernels'
                                                   average times from the stats files

Modes: imp4 / imp5 (four feet; feet and gripper, 15 rows; nu+, impulses and the energy), map4 / map5 (the same with dnu_dnu), cd4 / cd5
(wbc_sim_constrained_dynamics), old4 / old5 (the torch route, device events only): refresh_jacobian_tensors(), mass_solve on the gathered
rows, bmm, torch.linalg.cholesky / cholesky_solve on [N, 3K, 3K], nu+ = nu + Y^T Lambda."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["imp4", "imp5", "map4", "map5", "cd4", "cd5"]
MODES = KERNEL_MODES + ["old4", "old5"]
IMP = ["wbc_impulse_rhs_kernel", "wbc_mass_solve_kernel", "wbc_impulse_solve_kernel"]
MAP = IMP[:2] + ["wbc_impulse_solve_map_kernel"]
CD = ["wbc_inverse_dynamics_kernel", "wbc_constraint_rhs_kernel", "wbc_mass_solve_kernel", "wbc_constraint_solve_kernel"]
KERNELS = {"imp4": IMP, "imp5": IMP, "map4": MAP, "map5": MAP, "cd4": CD, "cd5": CD}

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
        total = 0.0
        for kernel in KERNELS[mode]:
            hit = [r for r in rows if r["Name"].startswith(kernel)]
            if not hit:
                sys.exit(f"{mode}: {kernel} is not in the kernel statistics under {out}")
            r = hit[0]
            total += float(r["AverageNs"]) / 1e3
            print(f"{mode:5s} N={a.envs}: {kernel} {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
                  f"min {float(r['MinNs']) / 1e3:.2f} us, max {float(r['MaxNs']) / 1e3:.2f} us", flush=True)
        print(f"{mode:5s} N={a.envs}: sum of the kernels' averages {total:.2f} us", flush=True)
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
env.refresh_jacobian_tensors()
grip = env.robot_model.rb_names.index("wx250s/ee_gripper_link")
feet = [int(i) for i in env.feet_indices.tolist()]
tau = torch.randn(n, 26, device="cuda")
sets = {4: feet, 5: feet + [grip]}
outs = {k: (torch.empty(n, 26, device="cuda"), torch.empty(n, k, 3, device="cuda")) for k in sets}
index = {k: torch.tensor(sets[k], device="cuda") for k in sets}
live = torch.ones(26, device="cuda"); live[-2:] = 0.0


def state_nu():
    return torch.cat([env.sim.tensor("ROOT_STATES")[:, 0, 7:13], env.sim.tensor("DOF_STATE")[..., 1]], 1) * live


def old_route(k):
    """What a user had before: the Jacobian tensor, M^-1 Jc^T from mass_solve, a batched dense Cholesky (a plastic impact)."""
    env.refresh_jacobian_tensors()
    nu = state_nu()
    Jc = env.jacobian_whole[:, index[k], :3].reshape(n, 3 * k, 26)
    Y = env.sim.mass_solve(Jc)
    A = torch.bmm(Jc, Y.transpose(1, 2))
    c = -torch.bmm(Jc, nu.unsqueeze(2)).squeeze(2)
    lam = torch.cholesky_solve(c.unsqueeze(2), torch.linalg.cholesky(A)).squeeze(2)
    return nu + torch.bmm(Y.transpose(1, 2), lam.unsqueeze(2)).squeeze(2), lam


def impulse(k, want_map):
    r = env.sim.impulse_dynamics(sets[k], want_map=want_map, want_energy=True)
    return r["nu_plus"], r["impulse"]


calls = {"imp4": lambda: impulse(4, False), "imp5": lambda: impulse(5, False), "map4": lambda: impulse(4, True), "map5": lambda: impulse(5, True),
         "cd4": lambda: env.sim.constrained_dynamics(sets[4], tau=tau, out=outs[4]),
         "cd5": lambda: env.sim.constrained_dynamics(sets[5], tau=tau, out=outs[5]),
         "old4": lambda: old_route(4), "old5": lambda: old_route(5)}
if a.mode == "all":                                                                # the two routes give the same answer
    for k in sets:
        nu_new, lam_new = calls[f"imp{k}"]()
        nu_old, lam_old = old_route(k)
        torch.cuda.synchronize()
        print(f"K={k}: largest |nu+_new - nu+_old| {float((nu_new - nu_old).abs().max()):.3g} of {float(nu_new.abs().max()):.3g}, "
              f"|Lambda_new - Lambda_old| {float((lam_new.reshape(n, -1) - lam_old).abs().max()):.3g} of {float(lam_new.abs().max()):.3g}", flush=True)
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
        print(f"round {rnd} {mode:5s} N={n}: {t0.elapsed_time(t1) * 1e3 / a.iters:.2f} us per call (device events, back to back)", flush=True)
