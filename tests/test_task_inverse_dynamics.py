"""Whole-body inverse dynamics for task-space accelerations (wbc_sim_task_inverse_dynamics; wbc_taskid_rhs_kernel and
wbc_taskid_solve_kernel in csrc/wbc_arm_kernel.hip, definition in include/wbc_sim.h). The CPU tests pin the fp64 Karush-Kuhn-Tucker
reference of tests/task_inverse_dynamics_reference.py to its own residuals, to inverse dynamics, to constrained forward dynamics and to
a standing robot's closed form, and measure the fp32 yardstick; the GPU tests hold the kernels to the four tiers of that module for
every env and row, to the sibling entry point and to their own invariances.

Bounds: residual <= C 2^-24 scale (+ C_ID 2^-24 mag(h) on the dynamics rows, + C_A 2^-24 mag(gamma) on the stance rows; the reduced
gradient has no allowance). K_ref is the fp32 yardstick's largest ratio against the scale over the 60 members of _family
below (asserted <= C / 16 on the CPU), C the smallest power of two >= 16 K_ref and no less than the siblings' C_S = 128 (dynamics rows)
and C_K = 32 (stance rows), and the last column the kernel's largest ratio on an MI355X (n = 1, 13, 64,
every case of test_every_env_and_row):

    rows                     K_ref     C        kernel's largest ratio
    dynamics, root rows      2.90      128      8.17
    dynamics, joint rows     13.2      256      14.7
    stance rows              41.4      1024     37.6
    reduced gradient         401       8192     6088 (the case without tasks; 138 over the cases with tasks)

C = 128 for the root rows is the siblings' C_S restated (the rule alone would give 64); the joint and stance rows exceed the siblings'
C_S = 128 and C_K = 32 because the optimal internal forces are large where w_force = 0 (|lambda| of several hundred N at |nudot| of
a few tens) and the stance rows' scale does not contain |lambda|: their C follows the rule. The least-squares solve is the square-root
form (Householder reflections of the stacked sqrt(weight)-scaled rows); C for the reduced gradient may be at most 16384. Without
tasks the posture term pins the light wrist joints' accelerations to nudot_ref (G_a's diagonal is 1 / inertia there), so the gradient
is a difference far below the sizes the scale sums and every fp32 chain sits one to two orders above its ratio with tasks; those
families always carry a nudot_ref of the size of the accelerations at play (see _family).
On the GPU case's own rollout states (arm near its zero pose, joint speeds of 20-30 rad/s) the yardstick itself reaches 3.6e4 without
tasks (median 1.9e3; the kernel: 6088, median 520, its tree solve is the more accurate): that regime is outside the CPU families.
Reported per case and never asserted: |tau - tau_64| / max |tau|, the same for nudot, and the relative objective excess: at most
7.9e-3, 6.1e-5 and 1.1e-5 for the yardstick over the CPU families; 3.6e-2, 1.4e-4 and 3.3e-5 for the kernel over the GPU cases.
The largest condition number of the diagonally scaled Delassus matrix is 96.9 over the CPU families and 4.16 over the GPU cases
(asserted <= 1000 on both).
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import constrained_dynamics_reference as cdr
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import task_inverse_dynamics_reference as tir
import arm_codegen
import whole_body_reference as wb
from wbc_amd import abi

FINGERS, LIVE, JOINTS, EPS = tir.FINGERS, tir.LIVE, tir.JOINTS, tir.EPS
C_ID, C_A = tir.C_ID, tir.C_A
C_TIER = {"root": tir.C_ROOT, "joint": tir.C_JOINT, "stance": tir.C_STANCE, "grad": tir.C_GRAD}
COND_MAX = 1000.0
SENTINEL = 12345.0
LDS_CAP = 20 * 1024
W_CHOICES = np.array([0.0, 0.5, 1.0, 2.0, 4.0])


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _bodies(model):
    """(feet [4], gripper, trunk) rigid-body indices."""
    feet = [i for i, name in enumerate(model.rb_names) if "foot" in name]
    assert len(feet) == 4 and model.rb_body[0] == 0
    return feet, model.rb_names.index("wx250s/ee_gripper_link"), 0


def _task_arrays(rng, shape, stance_on):
    """Targets and weights [..., 6, 6] of the six tasks (trunk, gripper, four feet): trunk and gripper rows with random weights from
    W_CHOICES (zeros included), a foot's linear rows weighted where it swings (stance_on [..., 4] False) and its angular rows never."""
    acc = _f32(rng.uniform(-5, 5, tuple(shape) + (6, 6)))
    w = np.zeros(tuple(shape) + (6, 6))
    w[..., :2, :] = W_CHOICES[rng.integers(0, len(W_CHOICES), tuple(shape) + (2, 6))]
    w[..., 2:, 0:3] = (W_CHOICES[rng.integers(1, len(W_CHOICES), tuple(shape) + (4,))] * ~np.asarray(stance_on, dtype=bool))[..., None]
    return acc, w


def _weights(seed):
    """(posture, force, torque, damping) of family member / GPU case `seed`."""
    return ([1e-2, 1e-1][seed % 2], [1e-4, 0.0, 1e-3][seed % 3], [1e-3, 1e-2][(seed // 2) % 2], 1e-3 if seed % 5 == 4 else 0.0)


def _problem(M, h, J, jd, stance, on_bodies, a_stance, tasks, acc, w, ref, weights):
    """tir.Problem from the fp64 system (M, h, J [27, 6, 26], Jdot nu [27, 6]) and the call's arguments."""
    on = np.repeat(np.asarray(on_bodies, dtype=bool), 3)
    Jc = np.concatenate([J[r, 0:3] for r in stance]) if len(stance) else np.zeros((0, 26))
    gamma = np.concatenate([jd[r, 0:3] for r in stance]) if len(stance) else np.zeros(0)
    Jt, gt, _ = tir.task_rows(J, jd, jd, tasks)
    a_s = np.zeros(len(on)) if a_stance is None else np.asarray(a_stance, dtype=np.float64).reshape(-1)
    return tir.Problem(M, h, Jc, gamma, a_s, on, Jt, gt, np.asarray(acc).reshape(-1), np.asarray(w).reshape(-1), ref, weights)


def _family(m, seed, arm_vec):
    """One member of the families the GPU tests use: (Problem, mag(h), kind). kind 0: four feet with 0..4 active (every count) and six
    tasks; 1: four feet active, stance accelerations, six tasks; 2: airborne (no stance bodies), six tasks; 3: four feet, no tasks."""
    import test_mass_solve as tms
    rng = np.random.default_rng(700 + seed)
    pos, quat, q, nu = tms._random_state(rng)
    bp = tms._random_body_params(m, rng)
    feet, grip, trunk = _bodies(m)
    kind = seed % 4
    M = msr.mass_matrix(m, pos, quat, q, bp, arm_vec if seed % 2 else None)
    h, magh = idr.bias_forces(m, pos, quat, q, nu, bp)
    J = wb.jacobian(m, pos, quat, q)
    jd, _ = cdr.body_accelerations(m, pos, quat, q, nu)
    stance = [] if kind == 2 else feet
    on = np.ones(len(stance), dtype=bool)
    if kind in (0, 3):
        on[:] = False
        on[rng.permutation(4)[:(seed // 4) % 5]] = True
    a_s = _f32(rng.uniform(-2, 2, 3 * len(stance))) if kind == 1 else None
    tasks = [] if kind == 3 else [trunk, grip] + feet
    acc, w = _task_arrays(rng, (), on if len(stance) else np.zeros(4, dtype=bool))
    if kind == 3:
        acc, w = np.zeros((0, 6)), np.zeros((0, 6))
    # without tasks the posture term is the only target, and with nudot_ref = 0 its residual nudot - nudot_ref is a small difference of
    # a_0 = -M^-1 h and G_a tau_j that the gradient's scale (|nudot| + |nudot_ref|) does not see: no fp32 evaluation is proportional to
    # it. The no-task members therefore always carry a reference of the size of the accelerations at play.
    ref = _f32(np.r_[rng.uniform(-2, 2, 6), rng.uniform(-5, 5, 20)]) if (seed % 3 or kind == 3) else None
    return _problem(M, h, J, jd, stance, on, a_s, tasks, acc, w, ref, _weights(seed)), magh, kind


# ------------------------------------------------------------------------------------------------------------ CPU
def test_abi_refusals_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    idx = (C.c_int32 * 4)(3, 7, 11, 15)
    w = abi.WbcTaskIdWeights(1e-2, 1e-4, 1e-3, 0.0)
    assert L.wbc_sim_task_inverse_dynamics(None, idx, 4, None, None, idx, 2, p, None, None, C.byref(w), 0, p, p, p, p, None) == -1
    assert b"NULL" in L.wbc_last_error()
    ws = L.wbc_sim_task_inverse_dynamics_workspace_floats
    assert ws(10, 4, 6) == 10 * (2 * 31 * 26 + 16 + 36 * 26 + 36) and ws(10, 0, 0) == 10 * (2 * 19 * 26 + 16 + 36)
    assert ws(0, 4, 6) == 0 and ws(10, 5, 6) == 0 and ws(10, -1, 6) == 0 and ws(10, 4, 7) == 0 and ws(10, 4, -1) == 0


def test_new_kernels_codegen():
    """No scratch, no flat memory instructions, the launch's workgroup size, static LDS within the 20 kB the derivatives kernel lives under."""
    for kernel in ("wbc_taskid_rhs_kernel", "wbc_taskid_solve_kernel"):
        assert arm_codegen.meta(kernel, "private_segment_fixed_size") == 0, kernel
        assert arm_codegen.meta(kernel, "max_flat_workgroup_size") == 64, kernel
        assert arm_codegen.meta(kernel, "group_segment_fixed_size") <= LDS_CAP, kernel
        body = arm_codegen.body(kernel)
        assert "s_endpgm" in body and re.search(r"\bglobal_store_dword", body), kernel
        assert not re.search(r"\bflat_", body) and "scratch_" not in body, kernel


def test_kkt_reference_satisfies_its_own_tiers_and_constrained_forward_dynamics(robot):
    m = robot["model"]
    A = msr.armature_vector(robot["tcfg"])
    for seed in range(16):
        P, _, _ = _family(m, seed, A)
        tau, nudot, lam = tir.kkt_reference(P)
        assert np.all(tau[:6] == 0) and np.all(tau[FINGERS] == 0) and np.all(nudot[FINGERS] == 0) and np.all(lam[~P.on] == 0)
        for k, (r, s) in tir.tiers(P, tau, nudot, lam).items():
            assert np.all(r <= 1e-10 * s), (seed, k, float((r / s).max()))
        # the optimum's torques through constrained forward dynamics: the same (nudot, lambda)
        nd2, lam2 = cdr.solve_with_mask(P.M, P.h, tau, P.Jc, P.gamma, P.a_stance, P.damping, P.on)
        assert np.abs(nd2 - nudot).max() <= 1e-9 * max(1.0, np.abs(nudot).max()) and np.abs(lam2 - lam).max(initial=0.0) <= 1e-9 * max(1.0, np.abs(lam).max(initial=0.0))
        # it is a minimum: every feasible neighbour costs more
        Z, x0, mm = tir.null_space(P)
        rng = np.random.default_rng(seed)
        f0 = tir.objective(P, tau, nudot, lam)
        for _ in range(4):
            tj = tau[JOINTS] + rng.normal(size=18)
            t2, n2, l2 = tir._unpack(P, x0 + Z @ tj, mm)
            assert tir.objective(P, t2, n2, l2) > f0


def test_reference_without_stance_and_tasks_is_inverse_dynamics_of_the_projected_posture(robot):
    """nstance = 0, ntasks = 0 and a huge posture weight: nudot is the Euclidean projection of nudot_ref on the feasible set
    {a : (M a + h)[0:6] = 0} (the root rows carry no actuation) up to O(torque / posture), and tau = inverse dynamics of it."""
    import test_mass_solve as tms
    m = robot["model"]
    for seed in range(6):
        rng = np.random.default_rng(40 + seed)
        pos, quat, q, nu = tms._random_state(rng)
        M = msr.mass_matrix(m, pos, quat, q)
        h, _ = idr.bias_forces(m, pos, quat, q, nu)
        ref = np.r_[rng.uniform(-2, 2, 6), rng.uniform(-5, 5, 20)]
        ref[FINGERS] = 0.0
        P = tir.Problem(M, h, np.zeros((0, 26)), np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool), np.zeros((0, 26)), np.zeros(0),
                        np.zeros(0), np.zeros(0), ref, (1e9, 0.0, 1e-3, 0.0))
        tau, nudot, lam = tir.kkt_reference(P)
        B = M[np.ix_(range(6), LIVE)]
        a = np.zeros(26)
        a[LIVE] = ref[LIVE] - B.T @ np.linalg.solve(B @ B.T, B @ ref[LIVE] + h[:6])
        want, _ = idr.inverse_dynamics(m, pos, quat, q, nu, a)
        assert np.abs(want[:6]).max() <= 1e-9 * np.abs(h[:6]).max()
        assert np.abs(nudot - a).max() <= 1e-6 * max(1.0, np.abs(a).max())
        assert np.abs(tau[JOINTS] - want[JOINTS]).max() <= 1e-6 * max(1.0, np.abs(want).max())


def test_standing_closed_form(robot):
    """nu = 0, four feet active, the trunk asked for zero acceleration, nudot_ref = 0: as posture / torque grows the optimum tends
    to nudot = 0 (every task and posture term is 0 there, and what the force and torque terms could gain by moving is O(torque /
    posture)), and then the foot forces carry the robot's weight: sum lambda = h[0:3] (h = -(m g) on the root's linear rows)."""
    import test_mass_solve as tms
    m = robot["model"]
    feet, grip, trunk = _bodies(m)
    rng = np.random.default_rng(7)
    pos, quat, q, _ = tms._random_state(rng)
    q = 0.3 * q
    quat = np.array([0.0, 0.0, 0.0, 1.0])
    nu = np.zeros(26)
    M = msr.mass_matrix(m, pos, quat, q)
    h, _ = idr.bias_forces(m, pos, quat, q, nu)
    J = wb.jacobian(m, pos, quat, q)
    jd, _ = cdr.body_accelerations(m, pos, quat, q, nu)
    assert np.all(jd == 0)
    P = _problem(M, h, J, jd, feet, np.ones(4, dtype=bool), None, [trunk], np.zeros((1, 6)), np.ones((1, 6)), None, (1e6, 0.0, 1e-3, 0.0))
    tau, nudot, lam = tir.kkt_reference(P)
    assert np.abs(nudot).max() <= 1e-6
    total = lam.reshape(4, 3).sum(0)
    assert np.abs(total - h[0:3]).max() <= 1e-5 * np.abs(h[0:3]).max(), (total, h[0:3])
    assert total[2] > 0 and abs(total[2] - 9.81 * sum(float(x) for x in m.mass)) <= 1e-3 * total[2]


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref of the four tiers, the largest scaled Delassus condition number and the reported errors, over 60 members of _family."""
    from wbc_amd.config import WidowGo1RoughCfg
    m = abi.load_default_model()
    A = msr.armature_vector(abi.fill_task_cfg(WidowGo1RoughCfg(), m))
    worst = {k: 0.0 for k in C_TIER}
    rep = {"tau": 0.0, "nudot": 0.0, "excess": 0.0}
    cond, kinds = 0.0, set()
    for seed in range(60):
        P, _, kind = _family(m, seed, A)
        kinds.add((kind, int(P.on.sum()) // 3))
        cond = max(cond, cdr.delassus_condition(P.M, P.Jc, P.damping, P.on))
        tau, nudot, lam = tir.yardstick_f32(P)
        for k, v in tir.ratios(P, tau, nudot, lam).items():
            worst[k] = max(worst[k], v)
        t64, n64, l64 = tir.kkt_reference(P)
        f64 = tir.objective(P, t64, n64, l64)
        rep["tau"] = max(rep["tau"], float(np.abs(tau - t64).max() / np.abs(t64).max()))
        rep["nudot"] = max(rep["nudot"], float(np.abs(nudot - n64).max() / np.abs(n64).max()))
        rep["excess"] = max(rep["excess"], float((tir.objective(P, tau, nudot, lam) - f64) / f64))
    assert {(0, k) for k in range(5)} <= kinds and (1, 4) in kinds and (2, 0) in kinds and {(3, k) for k in range(5)} <= kinds
    return worst, cond, rep


def test_fp32_yardsticks_sit_well_inside_the_bounds():
    worst, cond, rep = _yardsticks()
    print(f"yardsticks: K_ref = {worst} against C = {C_TIER}; largest scaled Delassus condition number {cond:.3g}; reported (never "
          f"asserted) largest |tau - tau64| / max|tau| = {rep['tau']:.3g}, nudot {rep['nudot']:.3g}, relative objective excess {rep['excess']:.3g}")
    for k, c in C_TIER.items():
        assert worst[k] <= c / 16, (k, worst[k])
    assert C_TIER["grad"] <= 16384 and C_TIER["grad"] == 2.0 ** np.ceil(np.log2(16 * worst["grad"]))
    # the dynamics and stance rows keep the siblings' constants where the rule gives no more
    assert C_TIER["root"] == max(cdr.C_S, 2.0 ** np.ceil(np.log2(16 * worst["root"])))
    assert C_TIER["joint"] == max(cdr.C_S, 2.0 ** np.ceil(np.log2(16 * worst["joint"])))
    assert C_TIER["stance"] == max(cdr.C_K, 2.0 ** np.ceil(np.log2(16 * worst["stance"])))


def test_delassus_conditioning_of_the_families():
    assert _yardsticks()[1] <= COND_MAX


# ------------------------------------------------------------------------------------------------------------ GPU
def _case(n):
    """test_constrained_dynamics._case(n): (env, M_ref, h_ref, mag(h), state, J [n, 27, 6, 26], Jdot nu [n, 27, 6], its magnitude),
    computed once, shared with that module and left unchanged."""
    import test_constrained_dynamics as tcd
    return tcd._case(n)


def _masks(n, K):
    import test_constrained_dynamics as tcd
    return tcd._masks(n, K)


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda").contiguous()


def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


_WORST = {"root": 0.0, "joint": 0.0, "stance": 0.0, "grad": 0.0, "cond": 0.0, "tau": 0.0, "nudot": 0.0, "excess": 0.0}


def _check(n, stance, active, a_stance, tasks, acc, w, ref, weights, armature, tau, nudot, lam):
    """All four tiers for every env and row from the kernel's own (tau, nudot, lam) against the fp64 system; the reported errors."""
    env, M, h, magh, _, J, jd, jmag = _case(n)
    if armature:
        M = M + np.diag(msr.armature_vector(env.tcfg))
    K, T = len(stance), len(tasks)
    t64, nd, lm = (x.double().cpu().numpy() for x in (tau, nudot, lam.reshape(n, 3 * K)))
    assert np.isfinite(t64).all() and np.isfinite(nd).all() and np.isfinite(lm).all()
    # tier 3, exact: the root rows and the fingers of tau, the fingers of nudot, the inactive bodies' lambda
    assert np.all(t64[:, :6] == 0) and np.all(t64[:, FINGERS] == 0) and np.all(nd[:, FINGERS] == 0)
    act = np.ones((n, K), dtype=bool) if active is None else active.cpu().numpy().astype(bool)
    worst = {k: 0.0 for k in C_TIER}
    for e in range(n):
        P = _problem(M[e], h[e], J[e], jd[e], stance, act[e], None if a_stance is None else np.nan_to_num(a_stance[e]), tasks,
                     np.zeros((0, 6)) if T == 0 else np.nan_to_num(acc[e]), np.zeros((0, 6)) if T == 0 else w[e], None if ref is None else ref[e], weights)
        assert np.all(lm[e][~P.on] == 0)
        cond = cdr.delassus_condition(P.M, P.Jc, P.damping, P.on)
        assert cond <= COND_MAX, (e, cond)
        _WORST["cond"] = max(_WORST["cond"], cond)
        magg = np.concatenate([jmag[e, r, 0:3] for r in stance])[P.on] if K else np.zeros(0)
        extra = {"root": C_ID * EPS * magh[e][:6], "joint": C_ID * EPS * magh[e][JOINTS], "stance": C_A * EPS * magg, "grad": 0.0}
        for k, (r, s) in tir.tiers(P, t64[e], nd[e], lm[e]).items():
            assert np.all(s > 0), (k, e)
            bound = C_TIER[k] * EPS * s + extra[k]
            assert np.all(r <= bound), (k, e, float((r / bound).max()), float((r / (EPS * s)).max()))
            if len(r):
                worst[k] = max(worst[k], float((r / (EPS * s)).max()))
        tq, nq, lq = tir.kkt_reference(P)
        fq = tir.objective(P, tq, nq, lq)
        _WORST["tau"] = max(_WORST["tau"], float(np.abs(t64[e] - tq).max() / np.abs(tq).max()))
        _WORST["nudot"] = max(_WORST["nudot"], float(np.abs(nd[e] - nq).max() / np.abs(nq).max()))
        _WORST["excess"] = max(_WORST["excess"], float((tir.objective(P, t64[e], nd[e], lm[e]) - fq) / fq))
    for k in worst:
        _WORST[k] = max(_WORST[k], worst[k])
    return worst


def _raw_call(env, stance, active, a_stance, tasks, acc, w, ref, weights, armature, want_nudot=True, want_lam=True):
    """The C-ABI call into sentinel-filled buffers: (tau [n, 26], nudot or None, lam or None); the tails stay untouched."""
    n, K, T = env.num_envs, len(stance), len(tasks)
    L, sim = env.sim.L, env.sim
    nws = int(L.wbc_sim_task_inverse_dynamics_workspace_floats(n, K, T))
    assert nws == n * (2 * (3 * K + 19) * 26 + 16 + 6 * T * 26 + 36)
    tb, nb, lb, ws = _sentinel_buffer(n * 26), _sentinel_buffer(n * 26), _sentinel_buffer(n * 3 * K), _sentinel_buffer(nws)
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    wt = abi.WbcTaskIdWeights(*weights)
    rc = L.wbc_sim_task_inverse_dynamics(sim.h, (C.c_int32 * max(K, 1))(*stance), K, ptr(active), ptr(a_stance), (C.c_int32 * max(T, 1))(*tasks), T,
                                         ptr(acc), ptr(w), ptr(ref), C.byref(wt), 1 if armature else 0, tb.data_ptr(),
                                         nb.data_ptr() if want_nudot else None, lb.data_ptr() if want_lam and K else None, ws.data_ptr(), None)
    assert rc == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    assert bool((tb[n * 26:] == SENTINEL).all()) and bool((nb[n * 26:] == SENTINEL).all()) and bool((lb[n * 3 * K:] == SENTINEL).all())
    assert bool((ws[nws:] == SENTINEL).all())
    if not want_nudot:
        assert bool((nb == SENTINEL).all())
    if not want_lam:
        assert bool((lb == SENTINEL).all())
    return tb[:n * 26].view(n, 26), nb[:n * 26].view(n, 26) if want_nudot else None, lb[:n * 3 * K].view(n, K, 3) if want_lam else None


CASES = ["masks16", "airborne", "no_tasks", "stance_acc", "damping", "force0", "armature", "nudot_null", "lambda_null", "both_null"]


def _arguments(env, n, case):
    """(stance, active, a_stance, tasks, acc, w, ref, weights, armature) of a case: numpy arrays (NaN where nothing may be read) and
    the u8 mask tensor."""
    feet, grip, trunk = _bodies(env.robot_model)
    rng = np.random.default_rng(1100 + CASES.index(case))
    stance, tasks, active, a_s, armature = feet, [trunk, grip] + feet, None, None, False
    weights = _weights({"damping": 4, "force0": 1, "no_tasks": 3}.get(case, 0))
    on = np.ones((n, 4), dtype=bool)
    if case == "masks16":
        active = _masks(n, 4)
        on = active.cpu().numpy().astype(bool)
    if case in ("masks16", "stance_acc"):
        a_s = _f32(rng.uniform(-2, 2, (n, 4, 3)))
        a_s[~on] = np.nan                                                          # never read where inactive
    if case == "airborne":
        stance, on = [], np.zeros((n, 4), dtype=bool)
    acc, w = _task_arrays(rng, (n,), on)
    acc[w == 0] = np.nan                                                           # never read where the weight is 0
    if case == "no_tasks":
        tasks, acc, w = [], None, None
    ref = _f32(np.concatenate([rng.uniform(-2, 2, (n, 6)), rng.uniform(-5, 5, (n, 20))], 1)) if case in ("no_tasks", "force0", "damping", "masks16") else None
    return stance, active, a_s, tasks, acc, w, ref, weights, case == "armature"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_and_row(n, case):
    env = _case(n)[0]
    stance, active, a_s, tasks, acc, w, ref, weights, armature = _arguments(env, n, case)
    d_as, d_acc, d_w, d_ref = _dev(a_s), _dev(acc), _dev(w), _dev(ref)
    tau, nudot, lam = _raw_call(env, stance, active, d_as, tasks, d_acc, d_w, d_ref, weights, armature,
                                want_nudot=case not in ("nudot_null", "both_null"), want_lam=case not in ("lambda_null", "both_null"))
    # the Python entry point is the same call
    t2, n2, l2 = env.sim.task_inverse_dynamics(stance, tasks, d_acc, d_w, active=None if active is None else active.bool(), stance_acc=d_as,
                                               nudot_ref=d_ref, posture=weights[0], force=weights[1], torque=weights[2], damping=weights[3],
                                               armature=armature)
    torch.cuda.synchronize()
    assert l2.shape == (n, len(stance), 3) and torch.equal(t2, tau)
    assert (nudot is None or torch.equal(n2, nudot)) and (lam is None or torch.equal(l2, lam))
    worst = _check(n, stance, active, a_s, tasks, acc, w, ref, weights, armature, tau, n2, l2)
    print(f"task inverse dynamics n={n} {case}: largest residual / (2^-24 scale) = {worst}; running maxima {_WORST}")
    if case == "masks16":
        # WidowGo1.whole_body_inverse_dynamics is the same call with the feet's weights taken from the stance mask
        wts = dict(posture=weights[0], force=weights[1], torque=weights[2], damping=weights[3])
        w_env = torch.zeros(n, 6, 6, device="cuda")
        w_env[:, :2] = 1.0
        w_env[:, 2:, :3] = (~active.bool()).float().unsqueeze(-1)
        clean = torch.nan_to_num(d_acc, nan=0.0)
        t3, n3, l3 = env.sim.task_inverse_dynamics(stance, tasks, clean, w_env, active=active.bool(), **wts)
        tq, nq, lq = env.whole_body_inverse_dynamics(clean[:, 0], clean[:, 1], clean[:, 2:, :3].contiguous(), stance=active.bool(), weights=wts)
        assert tq.shape == (n, 20) and tq.is_contiguous() and torch.equal(tq, t3[:, 6:]) and torch.equal(nq, n3) and torch.equal(lq, l3)


@pytest.mark.gpu
def test_nan_where_nothing_is_read_leaves_every_output_bit_identical():
    n = 64
    env = _case(n)[0]
    stance, active, a_s, tasks, acc, w, ref, weights, armature = _arguments(env, n, "masks16")
    assert np.isnan(a_s).any() and np.isnan(acc).any()
    dirty = env.sim.task_inverse_dynamics(stance, tasks, _dev(acc), _dev(w), active=active, stance_acc=_dev(a_s), nudot_ref=_dev(ref))
    clean = env.sim.task_inverse_dynamics(stance, tasks, _dev(np.nan_to_num(acc, nan=3.0)), _dev(w), active=active,
                                          stance_acc=_dev(np.nan_to_num(a_s, nan=-7.0)), nudot_ref=_dev(ref))
    torch.cuda.synchronize()
    for x, y in zip(dirty, clean):
        assert bool(torch.isfinite(x).all()) and bool(x.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    feet, grip, trunk = _bodies(robot["model"])
    rng = np.random.default_rng(1201)
    acc, w = _task_arrays(rng, (n,), _masks(n, 4).cpu().numpy().astype(bool))
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        out = env.sim.task_inverse_dynamics(feet, [trunk, grip] + feet, _dev(acc), _dev(w), active=_masks(n, 4), damping=1e-3)
        torch.cuda.synchronize()
        outs.append([x.clone() for x in out])
    for x, y in zip(*outs):
        assert bool(x.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13, 64])
def test_returned_torques_through_constrained_dynamics(n):
    """wbc_sim_constrained_dynamics with the returned tau and the same stance, mask, stance accelerations and damping: its (nudot,
    lambda) must satisfy the dynamics and stance rows within THAT call's own bounds, C_S 2^-24 scale + C_ID 2^-24 mag(h) and
    C_K 2^-24 scale + C_A 2^-24 mag(gamma) (tests/test_constrained_dynamics.py), with the scales taken at the NEW call's outputs.
    As an extra, the two pairs' difference satisfies the homogeneous rows within the sum of the two calls' bounds.
    Measured on an MI355X (w_force = 0, damping 1e-3, the 16 mask patterns): the sibling's residual / (2^-24 scale) reaches 14.1 on the
    dynamics rows and 15.8 on the stance rows (n = 13 and 64), at most 0.44 of its bound."""
    env, M, h, magh, _, J, jd, jmag = _case(n)
    stance, active, a_s, tasks, acc, w, ref, weights, armature = _arguments(env, n, "masks16")
    weights = _weights(4)                                                         # damping > 0, w_force = 0
    clean_as = _dev(np.nan_to_num(a_s))
    tau, nudot, lam = env.sim.task_inverse_dynamics(stance, tasks, _dev(acc), _dev(w), active=active, stance_acc=clean_as, nudot_ref=_dev(ref),
                                                    posture=weights[0], force=weights[1], torque=weights[2], damping=weights[3])
    nd2, lam2 = env.sim.constrained_dynamics(stance, tau=tau, active=active, acc_des=clean_as, damping=weights[3])
    torch.cuda.synchronize()
    t64, a1, l1, a2, l2 = (x.double().cpu().numpy().reshape(n, -1) for x in (tau, nudot, lam, nd2, lam2))
    act = active.cpu().numpy().astype(bool)
    own, ratio, extra = [], {"dynamics": 0.0, "stance": 0.0}, []
    for e in range(n):
        P = _problem(M[e], h[e], J[e], jd[e], stance, act[e], np.nan_to_num(a_s[e]), [], np.zeros((0, 6)), np.zeros((0, 6)), None, weights)
        magg = np.concatenate([jmag[e, r, 0:3] for r in stance]) * P.on
        assert np.all(l2[e][~P.on] == 0) and np.all(l1[e][~P.on] == 0)
        _, s1 = cdr.dynamics_residual_and_scale(P.M, P.h, t64[e], P.Jc, a1[e], l1[e])
        r2, s2 = cdr.dynamics_residual_and_scale(P.M, P.h, t64[e], P.Jc, a2[e], l2[e])
        bound = cdr.C_S * EPS * s1 + C_ID * EPS * magh[e]
        own.append(("dynamics", e, float((r2[LIVE] / bound[LIVE]).max())))
        ratio["dynamics"] = max(ratio["dynamics"], float((r2[LIVE] / (EPS * s1[LIVE])).max()))
        c1 = np.where(np.arange(26) < 6, C_TIER["root"], C_TIER["joint"])
        diff = np.abs(P.M @ (a2[e] - a1[e]) - P.Jc.T @ (l2[e] - l1[e]))
        both = EPS * (c1 * s1 + cdr.C_S * s2) + 2 * C_ID * EPS * magh[e]
        extra.append(float((diff[LIVE] / both[LIVE]).max()))
        if P.on.any():
            _, s1 = cdr.constraint_residual_and_scale(P.M, P.Jc, P.gamma, P.a_stance, P.damping, a1[e], l1[e])
            r2, s2 = cdr.constraint_residual_and_scale(P.M, P.Jc, P.gamma, P.a_stance, P.damping, a2[e], l2[e])
            bound = cdr.C_K * EPS * s1 + C_A * EPS * magg
            own.append(("stance", e, float((r2[P.on] / bound[P.on]).max())))
            ratio["stance"] = max(ratio["stance"], float((r2[P.on] / (EPS * s1[P.on])).max()))
            diff = np.abs(P.Jc @ (a2[e] - a1[e]) + P.damping * (l2[e] - l1[e]))
            both = EPS * (C_TIER["stance"] * s1 + cdr.C_K * s2) + 2 * C_A * EPS * magg
            extra.append(float((diff[P.on] / both[P.on]).max()))
    worst = max(own, key=lambda x: x[2])
    print(f"returned torques through wbc_sim_constrained_dynamics n={n}: its residual / (2^-24 scale at the new call's outputs) = {ratio} "
          f"against C_S = {cdr.C_S}, C_K = {cdr.C_K}; largest residual / its own bound = {worst}; largest difference / summed bound = {max(extra):.3g}")
    assert worst[2] <= 1.0, worst
    assert max(extra) <= 1.0


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env = _case(n)[0]
    stance, active, a_s, tasks, acc, w, ref, weights, armature = _arguments(env, n, "masks16")
    args = (stance, tasks, _dev(acc), _dev(w))
    kw = dict(active=active, stance_acc=_dev(a_s), nudot_ref=_dev(ref), damping=1e-3)
    want = [x.clone() for x in env.sim.task_inverse_dynamics(*args, **kw)]
    outs = tuple(torch.zeros_like(x) for x in want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream (the workspace exists already)
        env.sim.task_inverse_dynamics(*args, out=outs, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for x in outs:
        x.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.task_inverse_dynamics(*args, out=outs, **kw)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, want):
        assert bool(y.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env = _case(n)[0]
    m = env.robot_model
    feet, grip, trunk = _bodies(m)
    L, h = env.sim.L, env.sim.h
    tb, nb, lb = _sentinel_buffer(n * 26), _sentinel_buffer(n * 26), _sentinel_buffer(n * 12)
    ws = _sentinel_buffer(int(L.wbc_sim_task_inverse_dynamics_workspace_floats(n, 4, 6)))
    acc = torch.ones(n, 6, 6, device="cuda")
    sidx, tidx = (C.c_int32 * 4)(*feet), (C.c_int32 * 6)(trunk, grip, *feet)
    good = abi.WbcTaskIdWeights(1e-2, 1e-4, 1e-3, 0.0)
    same_body = next(r for r in range(27) if r != feet[0] and m.rb_body[r] == m.rb_body[feet[0]])   # e.g. the calf the foot is fixed to
    W = lambda *a: C.byref(abi.WbcTaskIdWeights(*a))
    call = lambda **kw: L.wbc_sim_task_inverse_dynamics(*[kw.get(k, d) for k, d in (
        ("sim", h), ("srb", sidx), ("ns", 4), ("active", None), ("a_s", None), ("trb", tidx), ("nt", 6), ("acc", acc.data_ptr()), ("w", None),
        ("ref", None), ("weights", C.byref(good)), ("flags", 0), ("tau", tb.data_ptr()), ("nudot", nb.data_ptr()), ("lam", lb.data_ptr()),
        ("ws", ws.data_ptr()), ("stream", None))])
    inf, nan = float("inf"), float("nan")
    refusals = [
        (dict(sim=None), b"NULL"), (dict(tau=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(weights=None), b"NULL"), (dict(acc=None), b"NULL"),
        (dict(srb=None), b"NULL"), (dict(trb=None), b"NULL"),
        (dict(ns=-1), b"nstance"), (dict(ns=5), b"nstance"), (dict(nt=-1), b"ntasks"), (dict(nt=7), b"ntasks"),
        (dict(srb=(C.c_int32 * 4)(feet[0], feet[1], 27, feet[3])), b"index"), (dict(srb=(C.c_int32 * 4)(feet[0], -1, feet[2], feet[3])), b"index"),
        (dict(trb=(C.c_int32 * 6)(trunk, grip, feet[0], 27, feet[2], feet[3])), b"index"), (dict(trb=(C.c_int32 * 6)(trunk, -1, *feet)), b"index"),
        (dict(srb=(C.c_int32 * 4)(feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(srb=(C.c_int32 * 4)(feet[0], feet[1], same_body, feet[3])), b"same moving body"),
        (dict(trb=(C.c_int32 * 6)(trunk, grip, feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(trb=(C.c_int32 * 6)(trunk, grip, feet[0], same_body, feet[2], feet[3])), b"same moving body"),
        (dict(weights=W(1e-2, 1e-4, 0.0, 0.0)), b"torque"), (dict(weights=W(1e-2, 1e-4, -1e-3, 0.0)), b"torque"),
        (dict(weights=W(1e-2, 1e-4, inf, 0.0)), b"torque"), (dict(weights=W(1e-2, 1e-4, nan, 0.0)), b"torque"),
        (dict(weights=W(-1e-2, 1e-4, 1e-3, 0.0)), b"posture"), (dict(weights=W(nan, 1e-4, 1e-3, 0.0)), b"posture"),
        (dict(weights=W(1e-2, -1e-4, 1e-3, 0.0)), b"force"), (dict(weights=W(1e-2, inf, 1e-3, 0.0)), b"force"),
        (dict(weights=W(1e-2, 1e-4, 1e-3, -1e-3)), b"damping"), (dict(weights=W(1e-2, 1e-4, 1e-3, nan)), b"damping"),
        (dict(flags=2), b"flag"), (dict(flags=4), b"flag"),
        (dict(a_s=acc.data_ptr() + 2), b"aligned"), (dict(acc=acc.data_ptr() + 1), b"aligned"), (dict(w=acc.data_ptr() + 3), b"aligned"),
        (dict(ref=acc.data_ptr() + 2), b"aligned"), (dict(tau=tb.data_ptr() + 2), b"aligned"), (dict(nudot=nb.data_ptr() + 1), b"aligned"),
        (dict(lam=lb.data_ptr() + 3), b"aligned"), (dict(ws=ws.data_ptr() + 2), b"aligned"),
    ]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for t in (tb, nb, lb, ws):
        assert bool((t == SENTINEL).all())
    # a stance body may be a task body too, and 4-byte alignment is all that is needed: outputs one float into their buffers
    want = env.sim.task_inverse_dynamics(feet, [trunk, grip] + feet, acc, posture=1e-2, force=1e-4, torque=1e-3)
    assert call(tau=tb.data_ptr() + 4, nudot=nb.data_ptr() + 4, lam=lb.data_ptr() + 4, ws=ws.data_ptr() + 4) == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    for buf, x in zip((tb, nb, lb), want):
        assert float(buf[0]) == SENTINEL and torch.equal(buf[1:1 + x.numel()].view(x.shape), x)
    assert float(ws[0]) == SENTINEL


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_call():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        a = torch.ones(n, 6, device="cuda")
        for _ in range(5):
            if use:
                env.whole_body_inverse_dynamics(base_acc=a, ee_acc=a, stance=env.get_foot_contacts())
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.whole_body_inverse_dynamics(base_acc=a, swing_acc=torch.ones(n, 4, 3, device="cuda"), stance=env.get_foot_contacts(),
                                                armature=True, weights=dict(damping=1e-3))
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for x, y in zip(*finals):
        assert torch.equal(x, y)
