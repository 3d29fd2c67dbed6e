"""Time of whole-body inverse kinematics (wbc_sim_inverse_kinematics: one launch of wbc_ik_kernel) at the bench's env count, next to the
only route to the same result that existed before, in one session and one build.

  python tools/profile_ik.py                  device-event times, back to back calls, two rounds, the call and the torch route alternating
  python tools/profile_ik.py --rocprof DIR    one `rocprofv3 --kernel-trace --stats` run of the call (a fresh child process under its own
                                              time limit) and the kernel's average time from the stats file
  WBC_AMD_LIB=<a build with -DIK_EPW=1> python tools/profile_ik.py --mode ik      the one-env-per-workgroup variant (wbc_amd/native.py)

The problem is the tests' reachable case at the Python defaults (posture 1e-2, damping 1e-3, step_tol 1e-4): the four feet and the gripper
(position and orientation) at the poses of the sim's own state q*, q_ref = q*, from q* perturbed by +-0.1 rad on every joint (clamped) and
on the root, +-2.5 cm on the root position. Modes: ik (the call), torch (the route built from the parent's public calls, one iteration =
set_root_state / set_dof_state, refresh_rigid_body_state, refresh_jacobian_tensors (wbc_sim_body_dynamics), gather, H and g,
torch.linalg.cholesky_ex / cholesky_solve, the same accept / reject rule per env, for the call's mean number of iterations; the sim's
state is restored afterwards)."""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["ik", "torch"]

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", choices=MODES + ["all"], default="all")
ap.add_argument("--rocprof", metavar="DIR", help="profile the call under rocprofv3, outputs below DIR")
ap.add_argument("--limit", type=int, default=240, help="seconds the profiled child may take")
a = ap.parse_args()

if a.rocprof:
    os.makedirs(a.rocprof, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "--",
           sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--iters", str(a.iters), "--rounds", "1", "--mode", "ik"]
    rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
    if rc != 0:
        sys.exit(f"the profiled run ended with status {rc}")
    rows = [r for f in glob.glob(os.path.join(a.rocprof, "**", "*kernel_stats.csv"), recursive=True) for r in csv.DictReader(open(f))]
    hit = [r for r in rows if r["Name"].startswith("wbc_ik_kernel")]
    if not hit:
        sys.exit(f"wbc_ik_kernel is not in the kernel statistics under {a.rocprof}")
    r = hit[0]
    print(f"N={a.envs}: wbc_ik_kernel {int(r['Calls'])} launches, average {float(r['AverageNs']) / 1e3:.2f} us, "
          f"min {float(r['MinNs']) / 1e3:.2f} us, max {float(r['MaxNs']) / 1e3:.2f} us", flush=True)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, "deep-whole-body-control_amd"))
import torch  # noqa: E402

from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

cfg = WidowGo1RoughCfg(); cfg.env.num_envs = a.envs; cfg.terrain.mesh_type = "plane"
env = WidowGo1(cfg, sim_device="cuda:0", seed=1)
torch.manual_seed(1)
for _ in range(5):
    env.step(torch.randn(a.envs, 18, device="cuda") * 0.5)
n, sim = a.envs, env.sim
grip = env.robot_model.rb_names.index("wx250s/ee_gripper_link")
feet = [int(i) for i in env.feet_indices.tolist()]
bodies = feet + [grip]
idx = torch.tensor(bodies, device="cuda")
POSTURE, LAMBDA0, TOL = 1e-2, 1e-3, 1e-4

# the problem: targets at the poses of the sim's own state, a perturbed start
sim.refresh_rigid_body_state()
root0, dof0 = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
tpos = env.rigid_body_state[:, idx, 0:3].clone().contiguous()
tquat = env.rigid_body_state[:, idx, 3:7].clone().contiguous()
w_ori = torch.zeros(n, 5, device="cuda"); w_ori[:, 4] = 1.0
g = torch.Generator(device="cuda"); g.manual_seed(3)
sign = lambda *shape: (torch.randint(0, 2, shape, device="cuda", generator=g).float() * 2 - 1)   # noqa: E731
lo, hi = env.dof_pos_limits[:, 0], env.dof_pos_limits[:, 1]
limited = ~((lo == 0) & (hi == 0))
q_star = dof0[..., 0].clone().contiguous()
dof_init = q_star.clone()
dof_init[:, :18] += 0.1 * sign(n, 18)
dof_init = torch.where(limited, torch.minimum(torch.maximum(dof_init, lo), hi), dof_init).contiguous()


def quat_mul(p, q):
    px, py, pz, pw = p.unbind(-1)
    qx, qy, qz, qw = q.unbind(-1)
    return torch.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                        pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz], -1)


def quat_exp(v):
    an = v.norm(dim=-1, keepdim=True)
    k = torch.where(an > 1e-6, torch.sin(0.5 * an) / an.clamp_min(1e-12), torch.full_like(an, 0.5))
    return torch.cat([v * k, torch.cos(0.5 * an)], -1)


def quat_log(q):
    q = q * torch.where(q[..., 3:4] < 0, -1.0, 1.0)
    nv = q[..., :3].norm(dim=-1, keepdim=True)
    k = torch.where(nv > 1e-6, 2 * torch.atan2(nv, q[..., 3:4]) / nv.clamp_min(1e-12), 2 / q[..., 3:4])
    return q[..., :3] * k


axis = torch.randn(n, 3, device="cuda", generator=g)
axis = axis / axis.norm(dim=-1, keepdim=True)
root_init = root0[:, 0, :7].clone()
root_init[:, :3] += 0.025 * sign(n, 3)
root_init[:, 3:7] = quat_mul(quat_exp(0.1 * axis), root_init[:, 3:7])
root_init = root_init.contiguous()
kw = dict(target_quat=tquat, w_ori=w_ori, root_init=root_init, dof_init=dof_init, q_ref=q_star, posture=POSTURE, damping=LAMBDA0, step_tol=TOL)

root, dof, info = sim.inverse_kinematics(bodies, tpos, **kw)
torch.cuda.synchronize()
status, iters = info["status"].cpu(), info["iterations"].float().cpu()
mean_it = float(iters.mean())
print(f"N={n}: status 0 on {int((status == 0).sum())} envs, iterations mean {mean_it:.2f} max {int(iters.max())}, "
      f"largest |gripper position residual| {float(info['residual'][:, 4, :3].abs().max()):.3g} m", flush=True)
NIT = max(1, round(mean_it))
live = torch.tensor([0, 1, 2, 3, 4, 5] + list(range(6, 24)), device="cuda")
W = torch.ones(n, 5, 6, device="cuda"); W[:, :4, 3:] = 0.0
Wf = W.reshape(n, 30)
conj = torch.tensor([-1.0, -1.0, -1.0, 1.0], device="cuda")


def torch_route():
    """The same projected Levenberg-Marquardt loop from the parent's public calls, NIT candidate evaluations; no second solve."""
    pos, quat, q = root_init[:, :3].clone(), root_init[:, 3:7].clone(), dof_init.clone()
    cpos, cquat, cq = pos.clone(), quat.clone(), q.clone()
    lam = torch.full((n,), LAMBDA0, device="cuda")
    cost = torch.full((n,), float("inf"), device="cuda")
    H = gvec = fixed = None
    rs, ds = root0.clone(), dof0.clone()
    for trip in range(NIT + 1):
        rs[:, 0, :3], rs[:, 0, 3:7], ds[..., 0] = cpos, cquat, cq
        sim.set_root_state(rs); sim.set_dof_state(ds)
        sim.refresh_rigid_body_state()
        env.refresh_jacobian_tensors()
        x, xq = env.rigid_body_state[:, idx, 0:3], env.rigid_body_state[:, idx, 3:7]
        r = torch.cat([tpos - x, quat_log(quat_mul(tquat, xq * conj))], -1).reshape(n, 30)
        dq = cq[:, :18] - q_star[:, :18]
        cc = 0.5 * (Wf * r * r).sum(1) + 0.5 * POSTURE * (dq * dq).sum(1)
        acc = cc <= cost
        if trip > 0:
            lam = torch.where(acc, (lam / 8).clamp_min(1e-9), lam * 8)
        J = env.jacobian_whole[:, idx][..., live].reshape(n, 30, 24)
        JW = J * Wf.unsqueeze(2)
        Hn = torch.bmm(JW.transpose(1, 2), J)
        Hn[:, 6:, 6:] += POSTURE * torch.eye(18, device="cuda")
        gn = -torch.bmm(JW.transpose(1, 2), r.unsqueeze(2)).squeeze(2)
        gn[:, 6:] += POSTURE * dq
        at = limited[:18] & (((cq[:, :18] <= lo[:18]) & (gn[:, 6:] > 0)) | ((cq[:, :18] >= hi[:18]) & (gn[:, 6:] < 0)))
        fn = torch.cat([torch.zeros(n, 6, dtype=torch.bool, device="cuda"), at], 1)
        if H is None:
            H, gvec, fixed = Hn, gn, fn
        else:
            m3 = acc.view(n, 1, 1)
            H, gvec, fixed = torch.where(m3, Hn, H), torch.where(acc.view(n, 1), gn, gvec), torch.where(acc.view(n, 1), fn, fixed)
        pos, quat, q = torch.where(acc.view(n, 1), cpos, pos), torch.where(acc.view(n, 1), cquat, quat), torch.where(acc.view(n, 1), cq, q)
        cost = torch.where(acc, cc, cost)
        free = (~fixed).float()
        A = H * free.unsqueeze(1) * free.unsqueeze(2) + torch.diag_embed(free * (lam.view(n, 1) * torch.diagonal(H, dim1=1, dim2=2) + 1e-9) + (1 - free))
        L, _ = torch.linalg.cholesky_ex(A)
        d = torch.cholesky_solve((-gvec * free).unsqueeze(2), L).squeeze(2)
        cpos = pos + d[:, :3]
        cquat = quat_mul(quat_exp(d[:, 3:6]), quat)
        cquat = cquat / cquat.norm(dim=-1, keepdim=True)
        cq = q.clone()
        cq[:, :18] = q[:, :18] + d[:, 6:]
        cq = torch.where(limited, torch.minimum(torch.maximum(cq, lo), hi), cq)
    sim.set_root_state(root0); sim.set_dof_state(dof0)
    return pos, quat, q


calls = {"ik": lambda: sim.inverse_kinematics(bodies, tpos, **kw), "torch": torch_route}
if a.mode == "all":                                                                # the two routes end near the same point
    pos, quat, q = torch_route()
    torch.cuda.synchronize()
    print(f"largest |q_call - q_torch| {float((dof - q).abs().max()):.3g} rad, |root position| {float((root[:, :3] - pos).abs().max()):.3g} m "
          f"(the torch route stops after {NIT} candidates whatever an env needs)", flush=True)
for rnd in range(a.rounds):
    for mode in (MODES if a.mode == "all" else [a.mode]):
        call = calls[mode]
        reps = a.iters if mode == "ik" else max(3, a.iters // 20)
        for _ in range(3):
            call()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            call()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / reps
        print(f"round {rnd} {mode:5s} N={n}: {us:.1f} us per call, {us / mean_it:.1f} us per iteration (mean {mean_it:.2f}; device events, "
              f"back to back)", flush=True)
assert torch.equal(sim.tensor("ROOT_STATES"), root0) and torch.equal(sim.tensor("DOF_STATE"), dof0)
