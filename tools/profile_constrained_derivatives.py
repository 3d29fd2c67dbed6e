"""Time of wbc_sim_constrained_dynamics_derivatives at the bench's env count, four stance feet, next to the route that existed before it,
in one session and one build: central differences of wbc_sim_constrained_dynamics through set_root_state / set_dof_state over the 42 live
directions of q and nu (3 root rotations, 3 root angular velocities, 18 joints and their velocities: 84 calls of four launches each and
86 state uploads per linearisation, the sim's state restored at the end). The perturbed states are built once, outside the timed
window, so the composed figure is its launches and uploads alone.

  python tools/profile_constrained_derivatives.py                 device-event times of every mode, back to back calls, two rounds with
                                                                  the modes alternating
  python tools/profile_constrained_derivatives.py --rocprof DIR   one `rocprofv3 --kernel-trace --stats` run of the full call (a fresh child
                                                                  process under its own time limit) and the two new kernels' average
                                                                  times from the stats files

Modes: full (all six outputs, conventional layout), fullt (WBC_DERIV_TRANSPOSED), qnu (the four q / nu outputs), tau (the two tau outputs),
cd (the sibling wbc_sim_constrained_dynamics alone, the unit of the composed route), composed (it prints its largest difference from the
analytic call once)."""
import argparse
import csv
import glob
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["full", "fullt", "qnu", "tau", "cd", "composed"]
KERNELS = ("wbc_constraint_tangent_kernel", "wbc_constraint_derivatives_solve_kernel")

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", choices=MODES + ["every"], default="every")
ap.add_argument("--rocprof", metavar="DIR", help="profile the full call under rocprofv3, outputs below DIR")
ap.add_argument("--limit", type=int, default=240, help="seconds the profiled child may take")
a = ap.parse_args()

if a.rocprof:
    os.makedirs(a.rocprof, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "--",
           sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--iters", str(a.iters), "--rounds", "1", "--mode", "full"]
    rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
    if rc != 0:
        sys.exit(f"the profiled run ended with status {rc}")
    rows = [r for f in glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
    for kernel in KERNELS:
        hit = [r for r in rows if r["Name"].startswith(kernel)]
        if not hit:
            sys.exit(f"{kernel} is not in the kernel statistics under {a.rocprof}")
        r = hit[0]
        print(f"N={a.envs}: {kernel} {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
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
sim = env.sim
feet = [int(i) for i in env.feet_indices.tolist()]
tau = torch.randn(n, 26, device="cuda")
QNU = ("dnudot_dq", "dnudot_dnu", "dlambda_dq", "dlambda_dnu")
TAU = ("dnudot_dtau", "dlambda_dtau")
full = sim.constrained_dynamics_derivatives(feet, tau=tau)
fullt = sim.constrained_dynamics_derivatives(feet, tau=tau, transposed=True)
cd_out = sim.constrained_dynamics(feet, tau=tau)
sub = lambda names: {k: full[k] for k in ("nudot", "lambda") + names}  # noqa: E731

# ---- the composed route: central differences through the state setters
STEP = 1e-3
root0, dof0 = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()


def rotated(root, j, h):
    """The root turned by the WORLD rotation vector h e_j: quaternion (xyzw) dq * q."""
    out = root.clone()
    d = [0.0, 0.0, 0.0, math.cos(h / 2)]
    d[j] = math.sin(h / 2)
    x, y, z, w = out[:, 0, 3], out[:, 0, 4], out[:, 0, 5], out[:, 0, 6]
    ax, ay, az, aw = d
    out[:, 0, 3:7] = torch.stack([aw * x + ax * w + ay * z - az * y, aw * y - ax * z + ay * w + az * x,
                                  aw * z + ax * y - ay * x + az * w, aw * w - ax * x - ay * y - az * z], 1)
    return out


states = []                                                     # (output, column, which tensor, +state, -state)
for j in range(3):
    states.append((0, 3 + j, "root", rotated(root0, j, STEP), rotated(root0, j, -STEP)))
    plus, minus = root0.clone(), root0.clone()
    plus[:, 0, 10 + j] += STEP; minus[:, 0, 10 + j] -= STEP
    states.append((1, 3 + j, "root", plus, minus))
for d in range(18):
    for out, slot in ((0, 0), (1, 1)):
        plus, minus = dof0.clone(), dof0.clone()
        plus[:, d, slot] += STEP; minus[:, d, slot] -= STEP
        states.append((out, 6 + d, "dof", plus, minus))
fd = [torch.zeros(n, 26, 26, device="cuda") for _ in range(2)]
fl = [torch.zeros(n, 12, 26, device="cuda") for _ in range(2)]
outs_p = (torch.empty(n, 26, device="cuda"), torch.empty(n, 4, 3, device="cuda"))
outs_m = (torch.empty(n, 26, device="cuda"), torch.empty(n, 4, 3, device="cuda"))


def composed():
    for out, col, which, plus, minus in states:
        setter = sim.set_root_state if which == "root" else sim.set_dof_state
        setter(plus); sim.constrained_dynamics(feet, tau=tau, out=outs_p)
        setter(minus); sim.constrained_dynamics(feet, tau=tau, out=outs_m)
        fd[out][:, :, col] = (outs_p[0] - outs_m[0]) / (2 * STEP)
        fl[out][:, :, col] = (outs_p[1] - outs_m[1]).view(n, 12) / (2 * STEP)
        if which == "root" and col == 5 and out == 1:
            sim.set_root_state(root0)                           # the root directions are done: back to the unperturbed root
    sim.set_dof_state(dof0)


calls = {"full": lambda: sim.constrained_dynamics_derivatives(feet, tau=tau, out=full),
         "fullt": lambda: sim.constrained_dynamics_derivatives(feet, tau=tau, transposed=True, out=fullt),
         "qnu": lambda: sim.constrained_dynamics_derivatives(feet, tau=tau, want=QNU, out=sub(QNU)),
         "tau": lambda: sim.constrained_dynamics_derivatives(feet, tau=tau, want=TAU, out=sub(TAU)),
         "cd": lambda: sim.constrained_dynamics(feet, tau=tau, out=cd_out), "composed": composed}
if a.mode in ("every", "composed"):
    calls["full"]()
    composed()
    torch.cuda.synchronize()
    assert torch.equal(sim.tensor("ROOT_STATES"), root0) and torch.equal(sim.tensor("DOF_STATE"), dof0)
    for name, got, want in (("dnudot_dq", fd[0], full["dnudot_dq"]), ("dnudot_dnu", fd[1], full["dnudot_dnu"]),
                            ("dlambda_dq", fl[0], full["dlambda_dq"]), ("dlambda_dnu", fl[1], full["dlambda_dnu"])):
        err = (got - want).abs().flatten(1).max(1).values / want.abs().flatten(1).max(1).values
        print(f"composed route (fp32 central differences, step {STEP:g}) vs the analytic call, {name}: per-env largest |difference| / largest "
              f"|entry|: median {float(err.median()):.3g}, largest {float(err.max()):.3g}", flush=True)
for rnd in range(a.rounds):
    for mode in (MODES if a.mode == "every" else [a.mode]):
        call = calls[mode]
        iters = a.iters if mode != "composed" else max(1, a.iters // 20)
        for _ in range(10 if mode != "composed" else 1):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        print(f"round {rnd} {mode:8s} N={n}: {t0.elapsed_time(t1) * 1e3 / iters:.2f} us per call (device events, back to back, {iters} calls)", flush=True)
