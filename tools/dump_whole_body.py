"""Every output of every entry point of csrc/wbc_arm_kernel.hip at seeded states, saved to one .npz. A change that must leave those
kernels' results bit-identical is checked by dumping once per library build (WBC_AMD_LIB selects the library; each dump in a process of
its own) and comparing the two files as raw 32-bit integers.

  WBC_AMD_LIB=/path/libwbc_amd.so python tools/dump_whole_body.py OUT.npz      dump
  python tools/dump_whole_body.py --compare A.npz B.npz                         exit status 1 unless every array is equal, bit for bit
  python tools/dump_whole_body.py --compare A.npz B.npz --allow-new             the same, but arrays that B alone holds are listed, not
                                                                                counted: an older build's dump against a newer one's

Envs n = 1, 13, 64 (13: the idle half-workgroup of the two-envs-per-workgroup kernels is live), and n = 273 for
wbc_sim_constrained_dynamics_derivatives alone (arrays that only one of the two dumps holds count as differences, unless --allow-new
lets the second, newer dump hold more); states and body parameters from the
generators of tests/test_mass_solve.py. Every array is float32: of task_inverse_dynamics_qp's integer outputs, status and iterations are
stored by value (exact below 2^24, asserted) and the int64 active_set as its two 32-bit words, reinterpreted and not converted.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if sys.argv[1:2] == ["--compare"]:
    A, B = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = sorted(set(A.files) ^ set(B.files))
    if sys.argv[4:5] == ["--allow-new"]:
        print(f"arrays of {sys.argv[3]} alone: {sorted(set(B.files) - set(A.files))}")
        bad = sorted(set(A.files) - set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        a, b = A[k], B[k]
        if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            bad.append(k)
            if a.shape == b.shape:
                print(f"{k}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} words differ, largest |difference| {np.nanmax(np.abs(a - b)):.3g}")
    print(f"{len(A.files)} arrays, {sum(A[k].size for k in A.files)} words: " + ("every array bit-identical" if not bad else f"DIFFERENT: {bad}"))
    sys.exit(1 if bad else 0)

for d in ("deep-whole-body-control_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import torch  # noqa: E402

import test_mass_solve as tms  # noqa: E402
from wbc_amd.config import WidowGo1RoughCfg  # noqa: E402
from wbc_amd.envs import WidowGo1  # noqa: E402

out = {}


def keep(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        a = t.detach().cpu().numpy()
        assert a.dtype == np.float32, name
        if not np.isfinite(a).all():
            print(f"{name}.{i}: {int((~np.isfinite(a)).sum())} non-finite values")
        out[f"{name}.{i}"] = a


def keep_qp(name, tau, nudot, lam, info):
    """The QP entry point's outputs; prints how many envs ended in each status and how many hold a torque-limit row."""
    keep(name, tau, nudot, lam)
    status, iters, aset = (info[k].cpu().numpy() for k in ("status", "iterations", "active_set"))
    assert status.dtype == np.int32 and iters.dtype == np.int32 and aset.dtype == np.int64
    for tag, a in (("status", status), ("iterations", iters)):
        out[f"{name}.{tag}"] = a.astype(np.float32)
        assert np.array_equal(out[f"{name}.{tag}"].astype(np.int32), a), tag
    out[name + ".active_set"] = np.ascontiguousarray(aset).view(np.float32).reshape(-1, 2)        # the words' bits, not their values
    print(f"{name}: status counts {np.bincount(status, minlength=3).tolist()}, box rows held in {int((aset & (2 ** 36 - 1) != 0).sum())} of "
          f"{len(aset)} envs, contact rows in {int((aset >> 36 != 0).sum())}")


def keep_cdd(sim, name, feet, grip, tau, g):
    """wbc_sim_constrained_dynamics_derivatives: feet masked; feet + gripper with damping; armature + transposed."""
    n = sim.num_envs
    act = (torch.rand(n, 4, device="cuda", generator=g) < 0.6)
    order = ("nudot", "lambda") + sim.CDD_OUTPUTS
    r = sim.constrained_dynamics_derivatives(feet, tau=tau, active=act)
    keep(name + "cdd.4", *[r[k] for k in order])
    r = sim.constrained_dynamics_derivatives(feet + [grip], tau=tau, damping=1e-3)
    keep(name + "cdd.5", *[r[k] for k in order])
    r = sim.constrained_dynamics_derivatives(feet, tau=None, armature=True, transposed=True)
    keep(name + "cdd.4.a1.t1", *[r[k] for k in order])


def keep_impulse(sim, name, feet, grip):
    """wbc_sim_impulse_dynamics (a generator of its own: the other entry points' draws stay what they were): feet all active; feet
    masked; feet + gripper with vel_des, restitution and impulse_ext; no active body."""
    n = sim.num_envs
    g = torch.Generator(device="cuda"); g.manual_seed(7000 + n)
    rnd = lambda *shape, scale=1.0: ((torch.rand(*shape, device="cuda", generator=g) * 2 - 1) * scale).contiguous()  # noqa: E731
    order = ("nu_plus", "impulse", "denergy", "dnu_dnu")
    both = dict(want_map=True, want_energy=True)
    keep(name + "imp.4", *[sim.impulse_dynamics(feet, **both)[k] for k in order])
    act = (torch.rand(n, 4, device="cuda", generator=g) < 0.6)
    keep(name + "imp.4.masked", *[sim.impulse_dynamics(feet, active=act, restitution=0.5, armature=True, **both)[k] for k in order])
    r = sim.impulse_dynamics(feet + [grip], restitution=torch.rand(n, 5, device="cuda", generator=g).contiguous(), vel_des=rnd(n, 5, 3),
                             impulse_ext=rnd(n, 26, scale=2.0), damping=1e-3, **both)
    keep(name + "imp.5", *[r[k] for k in order])
    r = sim.impulse_dynamics(feet, active=torch.zeros(n, 4, dtype=torch.bool, device="cuda"), impulse_ext=rnd(n, 26, scale=2.0), **both)
    keep(name + "imp.4.none", *[r[k] for k in order])
    r = sim.impulse_dynamics([grip], restitution=1.0)
    keep(name + "imp.1.plain", r["nu_plus"], r["impulse"])


def keep_ik(sim, name, feet, grip):
    """wbc_sim_inverse_kinematics (a generator of its own): the feet and the gripper at the poses of the sim's own state from a start
    perturbed by +-0.1 rad with q_ref the state's joints (reachable), and the same with the gripper's target 2 m from the trunk
    (unreachable); status and iterations are stored by value."""
    n = sim.num_envs
    g = torch.Generator(device="cuda"); g.manual_seed(8000 + n)
    sign = lambda *shape: (torch.randint(0, 2, shape, device="cuda", generator=g).float() * 2 - 1)   # noqa: E731
    sim.refresh_rigid_body_state()
    rb = sim.tensor("RIGID_BODY_STATE")
    bodies = feet + [grip]
    tpos, tquat = rb[:, bodies, 0:3].clone().contiguous(), rb[:, bodies, 3:7].clone().contiguous()
    w_ori = torch.zeros(n, 5, device="cuda"); w_ori[:, 4] = 1.0
    root = sim.tensor("ROOT_STATES")[:, 0, :7].clone().contiguous()
    q = sim.tensor("DOF_STATE")[..., 0].clone().contiguous()
    dof_init = q.clone(); dof_init[:, :18] += 0.1 * sign(n, 18)
    root_init = root.clone(); root_init[:, :3] += 0.025 * sign(n, 3)
    for tag, tp in (("reach", tpos), ("far", tpos.clone())):
        if tag == "far":
            d = tp[:, 4] - root[:, :3]
            tp[:, 4] = root[:, :3] + 2.0 * d / d.norm(dim=-1, keepdim=True)
        r, dof, info = sim.inverse_kinematics(bodies, tp.contiguous(), tquat, None, w_ori, root_init, dof_init.contiguous(), q)
        torch.cuda.synchronize()
        print(f"{name}ik.{tag}: status counts {torch.bincount(info['status'], minlength=4).tolist()}, most iterations {int(info['iterations'].max())}")
        keep(name + "ik." + tag, r, dof, info["residual"], info["cost"], info["status"].float(), info["iterations"].float())


def keep_coriolis(sim, name, tau):
    """wbc_sim_coriolis (all three outputs; vec alone: the vector kernel) and wbc_sim_momentum_observer: a reset, then two updates with
    tau and one with a NULL tau at the same state."""
    n = sim.num_envs
    keep(name + "coriolis", *sim.coriolis())
    keep(name + "coriolis.vec_only", *sim.coriolis(vec=torch.empty(n, 2, 26, device="cuda")))
    state = torch.zeros(n, 2, 26, device="cuda")
    keep(name + "observer.reset", sim.momentum_observer(tau, 30.0, 0.02, state=state, reset=True).clone())
    sim.momentum_observer(tau, 30.0, 0.02, state=state)
    keep(name + "observer.2", sim.momentum_observer(tau, 30.0, 0.02, state=state).clone())
    keep(name + "observer.null", sim.momentum_observer(None, 30.0, 0.02, state=state).clone())


for n in (1, 13, 64, 273):
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    env = WidowGo1(cfg, sim_device="cuda:0", seed=5)
    sim, m, dev = env.sim, env.robot_model, "cuda"
    root, dof = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
    bps = []
    for e in range(n):
        rng = np.random.default_rng(1000 * n + e)
        pos, quat, q, nu = tms._random_state(rng)
        bps.append(tms._random_body_params(m, rng))
        root[e, 0] = torch.tensor(np.concatenate([pos, quat, nu[0:6]]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q, nu[6:]], -1), dtype=torch.float32)
    sim.set_root_state(root.contiguous()); sim.set_dof_state(dof.contiguous())
    sim.tensor("BODY_PARAMS").copy_(torch.tensor(np.array(bps), dtype=torch.float32))
    g = torch.Generator(device=dev); g.manual_seed(n)
    rnd = lambda *shape, scale=1.0: ((torch.rand(*shape, device=dev, generator=g) * 2 - 1) * scale).contiguous()  # noqa: E731
    nudot = rnd(n, 26, scale=20.0)
    tau = rnd(n, 26, scale=10.0)
    feet, grip = [int(i) for i in env.feet_indices.tolist()], int(env.gripper_idx)
    T = f"n{n}."
    if n == 273:                                   # the new call alone at a size with a partial last workgroup of every two-env kernel
        keep_cdd(sim, T, feet, grip, tau, g)
        continue

    keep(T + "arm", *sim.arm_dynamics(env._arm_link_rb, m.rb_mass[-9:]))
    jac, mm = torch.empty(n, 27, 6, 26, device=dev), torch.empty(n, 26, 26, device=dev)
    sim.body_dynamics(jac=jac, mm=mm); keep(T + "body", jac, mm)
    mm1 = torch.empty_like(mm); sim.body_dynamics(mm=mm1); keep(T + "body.mm_only", mm1)
    for tag, nd in (("nudot", nudot), ("null", None)):
        t, gv = torch.empty(n, 26, device=dev), torch.empty(n, 26, device=dev)
        sim.inverse_dynamics(nudot=nd, tau=t, grav=gv); keep(T + "id." + tag, t, gv)
        keep(T + "accel." + tag, sim.body_accelerations(nd))
        keep(T + "centroidal." + tag, *sim.centroidal(nudot=nd))
        for tr in (False, True):
            keep(T + f"idd.{tag}.t{int(tr)}", *sim.inverse_dynamics_derivatives(nudot=nd, transposed=tr))
    gv = torch.empty(n, 26, device=dev); sim.inverse_dynamics(grav=gv); keep(T + "id.grav_only", gv)
    cm = torch.empty(n, 9, device=dev)
    check = sim.L.wbc_sim_centroidal(sim.h, None, cm.data_ptr(), None, None, None, sim._stream())
    assert check == 0
    keep(T + "centroidal.com_only", cm)
    dq = torch.empty(n, 26, 26, device=dev)
    assert sim.L.wbc_sim_inverse_dynamics_derivatives(sim.h, nudot.data_ptr(), dq.data_ptr(), None, 0, sim._stream()) == 0
    keep(T + "idd.dq_only", dq)
    for arm in (False, True):
        A = f".a{int(arm)}"
        keep(T + "solve1" + A, sim.mass_solve(tau, armature=arm))
        keep(T + "solve32" + A, sim.mass_solve(rnd(n, 32, 26, scale=5.0), armature=arm))
        keep(T + "solve.jac_view" + A, sim.mass_solve(jac[:, grip], armature=arm))
        keep(T + "fd" + A, sim.forward_dynamics(tau, armature=arm))
        keep(T + "fd.null" + A, sim.forward_dynamics(None, armature=arm))
        for tr in (False, True):
            keep(T + f"fdd.t{int(tr)}" + A, *sim.forward_dynamics_derivatives(tau=tau, armature=arm, transposed=tr))
        act = (torch.rand(n, 4, device=dev, generator=g) < 0.6)
        ades = rnd(n, 4, 3, scale=3.0)
        keep(T + "cd.1" + A, *sim.constrained_dynamics([grip], tau=tau, armature=arm))
        keep(T + "cd.4" + A, *sim.constrained_dynamics(feet, tau=tau, active=act, acc_des=ades, damping=1e-3, armature=arm))
        keep(T + "cd.5" + A, *sim.constrained_dynamics(feet + [grip], tau=None, damping=1e-4, armature=arm))
        keep(T + "tid.0_0" + A, *sim.task_inverse_dynamics(armature=arm))
        tasks = [0, grip] + feet
        w = torch.ones(n, 6, 6, device=dev); w[:, 2:] = 0.0
        full = dict(stance_bodies=feet, task_bodies=tasks, task_acc=rnd(n, 6, 6, scale=2.0), task_weight=w, active=act, stance_acc=ades,
                    nudot_ref=rnd(n, 26), damping=1e-4, armature=arm)
        free = sim.task_inverse_dynamics(**full)
        keep(T + "tid.4_6" + A, *free)
        keep(T + "tid.4_6.plain" + A, *sim.task_inverse_dynamics(feet, tasks, rnd(n, 6, 6, scale=2.0), armature=arm))
        # the same problem with inequalities: the config's limits; limits at half of what the sibling asks for, so that box rows bind;
        # no stance body (torque limits alone)
        keep_qp(T + "tqp.4_6" + A, *sim.task_inverse_dynamics_qp(**full, mu=0.6, fn_min=2.0))
        half = (0.5 * free[0][:, 6:24].abs() + 0.05).contiguous()
        keep_qp(T + "tqp.4_6.box" + A, *sim.task_inverse_dynamics_qp(**full, mu=0.6, fn_min=2.0, tau_limit=half))
        keep_qp(T + "tqp.0_6" + A, *sim.task_inverse_dynamics_qp((), tasks, full["task_acc"], w, nudot_ref=full["nudot_ref"], armature=arm,
                                                                 tau_limit=half))
    # the body-parameter regressor: full, a subset, native, transposed; the sensitivity call for two bodies and for all
    gb = int(m.gripper_piece["body"])
    keep(T + "reg.full", sim.inverse_dynamics_regressor(nudot=nudot), sim.inverse_dynamics_regressor())
    keep(T + "reg.subset", sim.inverse_dynamics_regressor([gb, 3, 0, 17, 9], nudot=nudot))
    keep(T + "reg.native", sim.inverse_dynamics_regressor(nudot=nudot, native=True), env.randomised_parameter_sensitivity(nudot))
    keep(T + "reg.t1", sim.inverse_dynamics_regressor(nudot=nudot, transposed=True), sim.inverse_dynamics_regressor([0, gb], native=True, transposed=True))
    for arm in (False, True):
        keep(T + f"sens.2.a{int(arm)}", *sim.forward_dynamics_sensitivity([0, gb], tau, armature=arm, native=True))
        keep(T + f"sens.19.a{int(arm)}", *sim.forward_dynamics_sensitivity(None, tau, armature=arm))
    md = torch.empty(n, 26, 26, device=dev)
    fd = sim.forward_dynamics_derivatives(tau=None, minv=md)
    keep(T + "fdd.tau_null", *fd)
    keep_cdd(sim, T, feet, grip, tau, g)           # last of the shared generator: its earlier draws stay what they were
    keep_impulse(sim, T, feet, grip)
    keep_ik(sim, T, feet, grip)
    keep_coriolis(sim, T, tau)

np.savez(sys.argv[1], **out)
print(f"{len(out)} arrays, {sum(a.size for a in out.values())} words -> {sys.argv[1]}")
