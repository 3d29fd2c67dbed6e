"""Time of wbc_sim_task_inverse_dynamics_qp (the sibling's three launches and wbc_taskqp_solve_kernel) at 4096 envs with 4 stance feet
and 6 tasks on rollout states, next to wbc_sim_task_inverse_dynamics in the same session and build. There is no torch route for the
inequality-constrained problem, so the unconstrained call is the yardstick. Three routes, alternating:

  never     the new call with limits that never bind where the feet push (tau_limit = FLT_MAX, fn_min = -FLT_MAX, mu = 1e6)
  nominal   the new call with mu = 0.6, fn_min = 2 N and the config's torque limits
  sibling   wbc_sim_task_inverse_dynamics
then, with every velocity of those states set to zero and gentle trunk and gripper targets (robots at rest: their feet push, so no row
binds and the new call takes no step), `never` and `sibling` once more as `never@rest` and `sibling@rest`: the cost of the new call
where it does nothing but check.

  python tools/profile_task_qp.py      device-event times, back to back calls, two rounds; then, for `never` and `nominal`, the share of
                                       envs with an active row, the statuses and the histogram of iterations
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["never", "nominal", "sibling"]
FLT_MAX = 3.4028234663852886e38

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2)
a = ap.parse_args()

sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import torch  # noqa: E402

from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n, dev = a.envs, "cuda"
sim = env.sim
feet = [int(i) for i in env.feet_indices.tolist()]
tasks = [0, int(env.gripper_idx)] + feet
WP, WF, WT = 1e-2, 1e-4, 1e-3
acc = torch.randn(n, 6, 6, device=dev) * 2.0
w = torch.ones(n, 6, 6, device=dev)
w[:, 2:] = 0.0                                                                   # the four feet stand: their tasks carry no weight
huge = torch.full((n, 18), FLT_MAX, device=dev)
kw = dict(posture=WP, force=WF, torque=WT)
outs = sim.task_inverse_dynamics(feet, tasks, acc, w, **kw)
qp = {m: sim.task_inverse_dynamics_qp(feet, tasks, acc, w, **kw) for m in ("never", "nominal")}
flat = lambda o: tuple(o[:3]) + (o[3]["status"], o[3]["active_set"], o[3]["iterations"])
calls = {
    "never": lambda: sim.task_inverse_dynamics_qp(feet, tasks, acc, w, mu=1e6, fn_min=-FLT_MAX, tau_limit=huge, out=flat(qp["never"]), **kw),
    "nominal": lambda: sim.task_inverse_dynamics_qp(feet, tasks, acc, w, mu=0.6, fn_min=2.0, out=flat(qp["nominal"]), **kw),
    "sibling": lambda: sim.task_inverse_dynamics(feet, tasks, acc, w, out=outs, **kw),
}


def measure(rnd, modes, tag=""):
    for mode in modes:
        call = calls[mode]
        for _ in range(10):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        print(f"round {rnd} {mode + tag:12s} N={n}: {t0.elapsed_time(t1) * 1e3 / a.iters:.2f} us per call (device events, back to back)", flush=True)


def report(modes, tag=""):
    for mode in modes:
        info = qp[mode][3]
        it = info["iterations"].cpu()
        hist = torch.bincount(it, minlength=1).tolist()
        print(f"{mode + tag:12s} N={n}: envs with an active row {float((info['active_set'] != 0).float().mean()):.3f}, statuses (0, 1, 2) "
              f"{torch.bincount(info['status'].cpu(), minlength=3).tolist()}, iterations mean {float(it.float().mean()):.2f} max {int(it.max())}, "
              f"histogram {dict((k, v) for k, v in enumerate(hist) if v)}", flush=True)
    idle = qp["never"][3]["iterations"] == 0
    same = all(torch.equal(x[idle], y[idle]) for x, y in zip(qp["never"][:3], outs))
    print(f"{'never' + tag:12s} N={n}: the {int(idle.sum())} envs without an iteration carry the sibling's bits: {same}", flush=True)


for rnd in range(a.rounds):
    measure(rnd, MODES)
report(("never", "nominal"))
root, dof = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
root[..., 7:13] = 0.0
dof[..., 1] = 0.0
sim.set_root_state(root.contiguous()); sim.set_dof_state(dof.contiguous())
acc.mul_(0.1)
for rnd in range(a.rounds):
    measure(rnd, ("never", "sibling"), "@rest")
report(("never",), "@rest")
