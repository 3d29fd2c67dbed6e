"""Time of wbc_sim_inverse_dynamics_derivatives (wbc_dynamics_derivatives_kernel) and of wbc_sim_forward_dynamics_derivatives at the bench's
env count, next to the route that existed before them, in one session and one build: central differences of wbc_sim_inverse_dynamics
through set_root_state / set_dof_state over every live direction (3 root rotations and 18 joints of dq, 3 root angular velocities and 18
joint velocities of dnu: 84 inverse-dynamics launches and 86 state uploads per linearisation, the sim's state restored at the end). The
perturbed states are built once, outside the timed window, so the composed figure is its launches and uploads alone.

  python tools/profile_dynamics_derivatives.py                 device-event times of every mode, back to back calls, two rounds
  python tools/profile_dynamics_derivatives.py --rocprof DIR   one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child
                                                               process each, under its own time limit; the first failure ends the
                                                               session) and the kernel's average time from the stats files

Modes: both (dtau_dq and dtau_dnu, nudot given), dq, dnu (one output alone), fdd (the full forward-dynamics-derivative call, conventional
layout: seven launches), fddt (the same with WBC_DERIV_TRANSPOSED: six), id (one inverse-dynamics launch, the unit of the composed route),
composed (device events only; it prints its largest difference from the kernel once)."""
import argparse
import csv
import glob
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["both", "dq", "dnu"]
MODES = KERNEL_MODES + ["fdd", "fddt", "id", "composed"]
KERNEL = "wbc_dynamics_derivatives_kernel"

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
        hit = [r for r in rows if r["Name"].startswith(KERNEL)]
        if not hit:
            sys.exit(f"{mode}: {KERNEL} is not in the kernel statistics under {out}")
        r = hit[0]
        print(f"{mode:8s} N={a.envs}: {KERNEL} {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
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
gen_tau = torch.randn(n, 26, device="cuda")
dq, dnu = sim.inverse_dynamics_derivatives(nudot)
fd_outs = sim.forward_dynamics_derivatives(gen_tau)
tau = torch.empty(n, 26, device="cuda")


def kernel(**outs):
    """The C-ABI call with NULL for the output that is not asked for."""
    rc = L.wbc_sim_inverse_dynamics_derivatives(sim.h, nudot.data_ptr(), outs["dq"].data_ptr() if "dq" in outs else None,
                                                outs["dnu"].data_ptr() if "dnu" in outs else None, 0, sim._stream())
    assert rc == 0, L.wbc_last_error()


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
fd_q, fd_nu = torch.zeros(n, 26, 26, device="cuda"), torch.zeros(n, 26, 26, device="cuda")
tau_p, tau_m = torch.empty(n, 26, device="cuda"), torch.empty(n, 26, device="cuda")


def composed():
    for out, col, which, plus, minus in states:
        setter = sim.set_root_state if which == "root" else sim.set_dof_state
        setter(plus); sim.inverse_dynamics(nudot=nudot, tau=tau_p)
        setter(minus); sim.inverse_dynamics(nudot=nudot, tau=tau_m)
        (fd_q if out == 0 else fd_nu)[:, :, col] = (tau_p - tau_m) / (2 * STEP)
        if which == "root" and col == 5 and out == 1:
            sim.set_root_state(root0)                           # the root directions are done: back to the unperturbed root
    sim.set_dof_state(dof0)


calls = {"both": lambda: kernel(dq=dq, dnu=dnu), "dq": lambda: kernel(dq=dq), "dnu": lambda: kernel(dnu=dnu),
         "fdd": lambda: sim.forward_dynamics_derivatives(gen_tau, *fd_outs), "fddt": lambda: sim.forward_dynamics_derivatives(gen_tau, *fd_outs, transposed=True),
         "id": lambda: sim.inverse_dynamics(nudot=nudot, tau=tau), "composed": composed}
if a.mode in ("every", "composed"):
    kernel(dq=dq, dnu=dnu)
    composed()
    torch.cuda.synchronize()
    assert torch.equal(sim.tensor("ROOT_STATES"), root0) and torch.equal(sim.tensor("DOF_STATE"), dof0)
    print(f"composed route (fp32 central differences, step {STEP:g}) vs kernel, largest absolute difference: dtau_dq {float((fd_q - dq).abs().max()):.3g} "
          f"(largest entry {float(dq.abs().max()):.3g}), dtau_dnu {float((fd_nu - dnu).abs().max()):.3g} (largest entry {float(dnu.abs().max()):.3g})", flush=True)
for rnd in range(a.rounds):
    for mode in (MODES if a.mode == "every" else [a.mode]):
        call = calls[mode]
        iters = a.iters
        for _ in range(10):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        print(f"round {rnd} {mode:8s} N={n}: {t0.elapsed_time(t1) * 1e3 / iters:.2f} us per call (device events, back to back, {iters} calls)", flush=True)
