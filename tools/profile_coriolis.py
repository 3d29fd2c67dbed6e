"""Time of wbc_sim_coriolis (wbc_coriolis_kernel, wbc_momentum_kernel) and wbc_sim_momentum_observer at the bench's env count, next to
their yardsticks and to the route they replace, in one session and one build:
  * the matrix call against the M-only launch of wbc_body_dynamics_kernel, which stores the same bytes for C alone;
  * the vector kernel against the h-only launch of wbc_inverse_dynamics_kernel;
  * the finite-difference route to dM/dt and C^T nu: two body_dynamics (M-only) and two inverse_dynamics launches (the state write-backs
    between them are not even counted).

  python tools/profile_coriolis.py                      device-event times of every mode, back to back launches, two rounds
  python tools/profile_coriolis.py --rocprof DIR        one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child
                                                        process each, under its own time limit; the first failure ends the
                                                        session) and the kernels' average times from the stats files

Modes: cmat (C alone), mdot (dM/dt alone), mats (C and dM/dt), all (both and vec), vec (the vector kernel), observer (the update: the
gravity launch and the vector kernel with its epilogue), mm (the M-only body_dynamics launch), h (the h-only inverse-dynamics launch),
fd (the finite-difference route, device events only)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["cmat", "mdot", "mats", "all", "vec", "observer", "mm", "h"]
MODES = KERNEL_MODES + ["fd"]
KERNELS = {m: "wbc_coriolis_kernel" for m in ("cmat", "mdot", "mats", "all")}
KERNELS.update(vec="wbc_momentum_kernel", observer="wbc_momentum_kernel", mm="wbc_body_dynamics_kernel", h="wbc_inverse_dynamics_kernel")

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
new = lambda *shape: torch.empty(*shape, device="cuda")  # noqa: E731
cmat, mdot, vec, state = new(n, 26, 26), new(n, 26, 26), new(n, 2, 26), torch.zeros(n, 2, 26, device="cuda")
mm, mm2, tau, tau2 = new(n, 26, 26), new(n, 26, 26), new(n, 26), new(n, 26)
torques = torch.randn(n, 26, device="cuda")
sim.momentum_observer(torques, 10.0, 0.02, state=state, reset=True)


def kernel(**outs):
    """The C-ABI call with NULL for the outputs that are not asked for."""
    rc = L.wbc_sim_coriolis(sim.h, *[outs[k].data_ptr() if k in outs else None for k in ("cmat", "mdot", "vec")], sim._stream())
    assert rc == 0, L.wbc_last_error()


def finite_difference():
    """The launches of the route by differences: M and h at two states (what moves the state between them is left out)."""
    sim.body_dynamics(mm=mm); sim.inverse_dynamics(tau=tau)
    sim.body_dynamics(mm=mm2); sim.inverse_dynamics(tau=tau2)


calls = {"cmat": lambda: kernel(cmat=cmat), "mdot": lambda: kernel(mdot=mdot), "mats": lambda: kernel(cmat=cmat, mdot=mdot),
         "all": lambda: kernel(cmat=cmat, mdot=mdot, vec=vec), "vec": lambda: kernel(vec=vec),
         "observer": lambda: sim.momentum_observer(torques, 10.0, 0.02, state=state), "mm": lambda: sim.body_dynamics(mm=mm),
         "h": lambda: sim.inverse_dynamics(tau=tau), "fd": finite_difference}
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
