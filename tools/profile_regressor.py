"""Time of wbc_sim_inverse_dynamics_regressor (wbc_inverse_dynamics_regressor_kernel) and of wbc_sim_forward_dynamics_sensitivity at the
bench's env count, next to the route that existed before them, in one session and one build: central differences of
wbc_sim_inverse_dynamics, in two forms. `setenv` goes through wbc_sim_set_env_params, the setter a caller has: it takes the five
randomisation inputs (base_dmass, base_dcom xyz, gripper_dmass), copies them from the host and synchronises, so this form reaches five
directions of the 20-column WBC_T_BODY_PARAMS: 10 setter calls, 10 inverse-dynamics launches and one setter call to restore. `composed`
writes the perturbed [N, 20] tensor that setter fills with a device copy instead, which reaches all 20 columns (root composite and gripper
body) and is the cheaper setter: 40 launches and 41 copies, the parameters restored at the end. The perturbed arrays of both are built
once, outside the timed window.

  python tools/profile_regressor.py                 device-event times of every mode, back to back calls, two alternating rounds
  python tools/profile_regressor.py --rocprof DIR   one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child process each,
                                                    under its own time limit; the first failure ends the session)

Modes: id (one inverse-dynamics launch, the session's yardstick and the unit of the composed route), all (the regressor for all nineteen
bodies, linear columns: the 81 MB output at 4096 envs), allt (the same, transposed), rg (root + gripper, native: [N, 26, 20]), sens2 and
sens19 (the sensitivity call for two and for nineteen bodies), store (a fill of the `all` output: the HBM store rate of the session),
setenv, composed (the latter prints its deviation and the kernel's from the fp64 restatement on a few envs once)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["all", "allt", "rg"]
MODES = ["id"] + KERNEL_MODES + ["sens2", "sens19", "store", "setenv", "composed"]
KERNEL = "wbc_inverse_dynamics_regressor_kernel"

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

for d in ("deep-whole-body-control_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n = a.envs
sim = env.sim
gb = int(env.robot_model.gripper_piece["body"])
nudot = torch.randn(n, 26, device="cuda") * 5.0
gen_tau = torch.randn(n, 26, device="cuda")
tau = torch.empty(n, 26, device="cuda")
Y = sim.inverse_dynamics_regressor(nudot=nudot)
Yt = sim.inverse_dynamics_regressor(nudot=nudot, transposed=True)
Yrg = sim.inverse_dynamics_regressor([0, gb], nudot=nudot, native=True)
s2 = sim.forward_dynamics_sensitivity([0, gb], gen_tau, native=True)
s19 = sim.forward_dynamics_sensitivity(None, gen_tau)

# ---- the composed route: central differences over the columns of BODY_PARAMS
bp = sim.tensor("BODY_PARAMS")
bp0 = bp.clone()
STEP = [1e-2] + [1e-3] * 3 + [1e-4] * 6 + [1e-3] + [1e-3] * 3 + [1e-5] * 6      # per column: masses, centres of mass, inertias
perturbed = []
for k in range(20):
    plus, minus = bp0.clone(), bp0.clone()
    plus[:, k] += STEP[k]; minus[:, k] -= STEP[k]
    perturbed.append((plus, minus, (plus[:, k] - minus[:, k]).unsqueeze(1)))         # the step the fp32 parameters really took
fd = torch.zeros(n, 26, 20, device="cuda")
tau_p, tau_m = torch.empty(n, 26, device="cuda"), torch.empty(n, 26, device="cuda")


def composed():
    for k, (plus, minus, h) in enumerate(perturbed):
        bp.copy_(plus); sim.inverse_dynamics(nudot=nudot, tau=tau_p)
        bp.copy_(minus); sim.inverse_dynamics(nudot=nudot, tau=tau_m)
        fd[:, :, k] = (tau_p - tau_m) / h
    bp.copy_(bp0)


# ---- the same through wbc_sim_set_env_params: the five inputs it takes
mp0 = sim.tensor("MASS_PARAMS").cpu().numpy().copy()                                  # (base_dmass, base_dcom xyz, gripper_dmass) per env
ENV_STEP = [1e-2, 1e-3, 1e-3, 1e-3, 1e-3]
env_inputs = []
for k in range(5):
    for sign in (1.0, -1.0):
        mp = mp0.copy(); mp[:, k] += sign * ENV_STEP[k]
        env_inputs.append(dict(base_dmass=mp[:, 0].copy(), base_dcom=mp[:, 1:4].copy(), gripper_dmass=mp[:, 4].copy()))
env_restore = dict(base_dmass=mp0[:, 0].copy(), base_dcom=mp0[:, 1:4].copy(), gripper_dmass=mp0[:, 4].copy())
fd_env = torch.zeros(n, 26, 5, device="cuda")


def setenv():
    for k in range(5):
        sim.set_env_params(**env_inputs[2 * k]); sim.inverse_dynamics(nudot=nudot, tau=tau_p)
        sim.set_env_params(**env_inputs[2 * k + 1]); sim.inverse_dynamics(nudot=nudot, tau=tau_m)
        fd_env[:, :, k] = (tau_p - tau_m) / (2 * ENV_STEP[k])
    sim.set_env_params(**env_restore)


calls = {"id": lambda: sim.inverse_dynamics(nudot=nudot, tau=tau), "all": lambda: sim.inverse_dynamics_regressor(nudot=nudot, out=Y),
         "allt": lambda: sim.inverse_dynamics_regressor(nudot=nudot, out=Yt, transposed=True),
         "rg": lambda: sim.inverse_dynamics_regressor([0, gb], nudot=nudot, out=Yrg, native=True),
         "sens2": lambda: sim.forward_dynamics_sensitivity([0, gb], gen_tau, native=True, nudot=s2[0], out=s2[1]),
         "sens19": lambda: sim.forward_dynamics_sensitivity(None, gen_tau, nudot=s19[0], out=s19[1]),
         "store": lambda: Y.fill_(1.0), "setenv": setenv, "composed": composed}
if a.mode in ("every", "setenv"):
    setenv()
    torch.cuda.synchronize()
    if not torch.equal(bp, bp0):                                                   # parameters that did not come from the setter's inputs
        print("set_env_params does not reproduce the BODY_PARAMS the env held; they are written back", flush=True)
        bp.copy_(bp0)
if a.mode in ("every", "composed"):
    import regressor_reference as rr
    composed()
    torch.cuda.synchronize()
    assert torch.equal(bp, bp0)
    kern = sim.inverse_dynamics_regressor([0, gb], nudot=nudot, native=True).view(n, 26, 20)
    root = sim.tensor("ROOT_STATES").cpu().numpy().astype(np.float64)
    dof = sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64)
    worst = {"composed": 0.0, "kernel": 0.0}
    absw = {"composed": 0.0, "kernel": 0.0}
    for e in range(0, n, max(1, n // 8)):
        nu = np.r_[root[e, 0, 7:13], dof[e, :, 1]]
        Yr, mag = rr.regressor(env.robot_model, root[e, 0, 3:7], dof[e, :, 0], nu, nudot[e].cpu().numpy().astype(np.float64),
                               [float(x) for x in env.tcfg.gravity])
        Yn, magn = rr.native(Yr, mag, rr.theta_of(env.robot_model, bp0[e].cpu().numpy().astype(np.float64)))
        ref, mg = Yn[:, [0, gb]].reshape(26, 20), magn[:, [0, gb]].reshape(26, 20)
        for name, got in (("composed", fd[e]), ("kernel", kern[e])):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            worst[name] = max(worst[name], float((err[mg > 0] / (2.0 ** -24 * mg[mg > 0])).max()))
            absw[name] = max(absw[name], float(err.max()))
    print(f"deviation from the fp64 restatement over {len(range(0, n, max(1, n // 8)))} envs, largest |x - ref| / (2^-24 mag) and largest absolute: "
          f"composed route (fp32 central differences) {worst['composed']:.3g}, {absw['composed']:.3g}; kernel {worst['kernel']:.3g}, {absw['kernel']:.3g}",
          flush=True)
print(f"output of `all`: {Y.numel() * 4 / 1e6:.1f} MB", flush=True)
for rnd in range(a.rounds):
    for mode in (MODES if a.mode == "every" else [a.mode]):
        call = calls[mode]
        iters = a.iters
        for _ in range(10 if mode not in ("composed", "setenv") else 2):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / iters
        extra = f", {Y.numel() * 4 / us / 1e3:.0f} GB/s" if mode in ("all", "allt", "store") else ""
        print(f"round {rnd} {mode:8s} N={n}: {us:.2f} us per call (device events, back to back, {iters} calls){extra}", flush=True)
