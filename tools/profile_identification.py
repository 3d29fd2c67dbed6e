"""Time of wbc_sim_identification_accumulate (wbc_identification_accumulate_kernel) and wbc_sim_identification_solve
(wbc_identification_solve_kernel) at the bench's env count, next to the route a user had before them, in one session and one build:
inverse_dynamics_regressor(bodies) writing Y to HBM, inverse_dynamics for the torque of all bodies, the target and the normal equations
in torch (one baddbmm each for Phi^T Phi and Phi^T z on the decayed accumulators), and torch.linalg.cholesky_ex / cholesky_solve for the
estimate.

  python tools/profile_identification.py                 device-event times of every mode, back to back calls, two alternating rounds
  python tools/profile_identification.py --rocprof DIR   one `rocprofv3 --kernel-trace --stats` run per kernel mode (a fresh child process
                                                         each, under its own time limit; the first failure ends the session)

Modes: acc1, acc2, acc3 (the fused accumulate call for the gripper body, root + gripper body and root + gripper body + one more),
solve (every output, P = 20), solve_pi (pi_hat only), old_acc1 / old_acc2 / old_acc3 (the torch route's update for the same lists: three
launches of this library and the torch kernels behind two baddbmm, the weighting and the subtraction), old_solve (cholesky_ex and
cholesky_solve on the [N, 20, 20] accumulators). With every mode, the tool first prints how far the two routes' A are apart after eight
updates."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODES = ["acc1", "acc2", "acc3", "solve", "solve_pi"]
MODES = KERNEL_MODES + ["old_acc1", "old_acc2", "old_acc3", "old_solve"]

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
        kernel = "wbc_identification_solve_kernel" if mode.startswith("solve") else "wbc_identification_accumulate_kernel"
        out = os.path.join(a.rocprof, mode)
        cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--iters", str(a.iters), "--rounds", "1", "--mode", mode]
        rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
        if rc != 0:
            sys.exit(f"{mode}: the profiled run ended with status {rc}; nothing more is started")
        rows = [r for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
        hit = [r for r in rows if r["Name"].startswith(kernel)]
        if not hit:
            sys.exit(f"{mode}: {kernel} is not in the kernel statistics under {out}")
        r = hit[0]
        print(f"{mode:8s} N={a.envs}: {kernel} {int(r['Calls'])} launches (the set-up's included), average {float(r['AverageNs']) / 1e3:.2f} us, "
              f"min {float(r['MinNs']) / 1e3:.2f} us, max {float(r['MaxNs']) / 1e3:.2f} us", flush=True)
    sys.exit(0)

for d in ("deep-whole-body-control_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import torch  # noqa: E402

from wbc_amd import abi  # noqa: E402
from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n, sim = a.envs, env.sim
gb = int(env.robot_model.gripper_piece["body"])
LISTS = {1: [gb], 2: [0, gb], 3: [0, gb, 3]}
FORGET = 0.98
nudot = torch.randn(n, 26, device="cuda") * 5.0
tau_gen = env.inverse_dynamics(nudot)
live = torch.ones(26, device="cuda")
live[24:] = 0.0
pi_all = torch.tensor(abi.linear_body_params(env.robot_model, sim.tensor("BODY_PARAMS").cpu().numpy()), dtype=torch.float32, device="cuda")

new = {k: sim.identification_accumulate(b, tau_gen, nudot=nudot) for k, b in LISTS.items()}                 # (A, b, stat, target), reset
old = {k: (torch.zeros(n, 10 * k, 10 * k, device="cuda"), torch.zeros(n, 10 * k, 1, device="cuda")) for k in LISTS}
Y = {k: torch.empty(n, 26, k, 10, device="cuda") for k in LISTS}
tau = torch.empty(n, 26, device="cuda")
prior = env.parameter_identifier().prior
out_all = sim.identification_solve(*new[2][:3], prior=prior)
out_pi = sim.identification_solve(*new[2][:2], want=("pi_hat",))


def fused(k):
    A, b, st, tgt = new[k]
    return lambda: sim.identification_accumulate(LISTS[k], tau_gen, nudot=nudot, forget=FORGET, info_mat=A, info_vec=b, stat=st, target=tgt)


def torch_route(k):
    bodies, (A, b) = LISTS[k], old[k]

    def run():
        sim.inverse_dynamics_regressor(bodies, nudot=nudot, out=Y[k])
        sim.inverse_dynamics(nudot=nudot, tau=tau)                                         # what the listed bodies contribute to it is Phi pi_S
        Phi = Y[k].view(n, 26, 10 * k)
        z = tau_gen - (tau - torch.bmm(Phi, pi_all[:, bodies].reshape(n, 10 * k, 1)).squeeze(-1))   # the route a user had: it cancels
        Pw = Phi * live[None, :, None]
        A.baddbmm_(Pw.transpose(1, 2), Phi, beta=FORGET)
        b.baddbmm_(Pw.transpose(1, 2), z.unsqueeze(-1), beta=FORGET)
    return run


def torch_solve():
    A, b = old[2]
    L, info = torch.linalg.cholesky_ex(A)
    return torch.cholesky_solve(b, L), info


calls = {"solve": lambda: sim.identification_solve(*new[2][:3], prior=prior, out=out_all),
         "solve_pi": lambda: sim.identification_solve(*new[2][:2], want=("pi_hat",), out=out_pi), "old_solve": torch_solve}
for k in LISTS:
    calls[f"acc{k}"], calls[f"old_acc{k}"] = fused(k), torch_route(k)

if a.mode == "every":                                                                      # both routes see the same eight updates
    for k in LISTS:
        new[k][0].zero_(); new[k][1].zero_(); new[k][2].zero_()
        for _ in range(8):
            calls[f"acc{k}"](); calls[f"old_acc{k}"]()
    torch.cuda.synchronize()
    dA = float((new[2][0] - old[2][0]).abs().max() / old[2][0].abs().max())
    print(f"root + gripper body after 8 updates: fused A against the torch route's, largest difference / largest entry {dA:.3g}", flush=True)

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
        print(f"round {rnd} {mode:9s} N={n}: {t0.elapsed_time(t1) * 1e3 / a.iters:.2f} us per call (device events, back to back, {a.iters} calls)",
              flush=True)
