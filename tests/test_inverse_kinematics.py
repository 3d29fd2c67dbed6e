"""Whole-body inverse kinematics with joint limits (wbc_sim_inverse_kinematics; wbc_ik_kernel of csrc/wbc_arm_kernel.hip, definitions in
include/wbc_sim.h). The CPU tests pin the fp64 statement of tests/ik_reference.py to itself (gradient against Richardson differences
through the retraction, the orientation gradient identity, convergence of the family) and measure the fp32 yardstick; the GPU tests
never replay the kernel's path: they judge the point it returned, its reported values, its exact guarantees and its invariances.

The family (ik_reference.member): the four feet (position rows) and the gripper (position and orientation) at the fp64 poses of a
configuration q* drawn inside the joint limits with a random root pose, from q* perturbed by +-0.1 rad (even seeds) or +-0.3 rad (odd
seeds), the root accordingly. Cases (_problem):
    reach       q_ref = q*, posture 1e-2, step_tol 1e-5: the minimum is residual 0
    tradeoff2   q_ref = the start, posture 1e-2, step_tol 1e-4 (the Python defaults)
    tradeoff3   q_ref = the start, posture 1e-3, step_tol 1e-4
    limits      the targets taken at a posture 0.15 rad BEYOND two joints' limits (a front calf's upper, a rear hip's lower), q_ref that
                posture clamped, step_tol 1e-4: the limits are strictly active at the minimum, so the joints end on them
    twice       reach, the gripper listed twice: once for its position, once for its orientation (two targets on one body)
    stance      reach, a per-env subset of the feet switched off by weight 0, their targets NaN
The family stays at posture >= 1e-3 or q_ref = q*: with posture 1e-4 and step_tol 1e-4 the fp32 loop runs to the cap on some members
(a step of step_tol along a direction of curvature `posture` changes the cost by less than fp32 resolves). The fp32 yardstick ends
with status 0 on all 64 members of every case (27 iterations at most); the convergence test speaks about status 0, asks it of every
member where the minimum is residual 0 and of at least 3 in 4 members of the tradeoff cases, where an accept / reject decision at
fp32 resolution may end a member with status 1 or 2 instead.

The step's second pass (a free joint whose step would leave its limits goes onto the limit and the others solve again) is what makes
the limits case converge: without it the yardstick ran 16 of its 64 members to the cap, a joint hovering 3e-4 rad inside its limit
while the clamped step, no longer a descent step of the model, was rejected trip after trip.

Constants (EPS = 2^-24). K_ref is the fp32 yardstick's largest ratio over the 64 members of every case (asserted on the CPU), and the
last column the kernel's largest ratio on an MI355X over n = 1, 13, 64:

    quantity                                                     K_ref    C                      kernel's largest ratio
    projected fp64 step at a status-0 output / step_tol (C_S)    0.990    4  (>= 4 K_ref)        0.989
    reach: |position residual| / (EPS scale) (C_R)               129      4096 (>= 16 K_ref)     127
    reported residual and cost against fp64 at the output (C_V)  0.5      32 (the floor)         6.98 (position), 0.58 (orientation)

C_S: the factor 4 stands for accept / reject decisions that differ from the yardstick's at rounding level, not for a rounding count.
C_R is large because the loop stops BEFORE the step it judges small enough: K_ref is the size of that last, untaken step (up to
step_tol = 1e-5 rad on a lever of half a metre), not an accumulation of roundings. C_V: the yardstick rounds the fp64 residual once
(ratio 0.5), the floor of the project's rule, 32, applies; the reported cost stays within 0.029 of its allowance (_allowance).

The Python layer (test_reach_configuration_and_goal_reachability, _facade_member) is held to the family's goals at its defaults:
reach_configuration's first solve towards default_dof_pos misses them by up to 5 cm in the yardstick, its two proximal solves bring
them to 9e-8 m there (asserted on the CPU) and to 3.6e-7 m = 8.4 EPS scale on an MI355X, against the reach bound C_R.

Translation (test_translation_leaves_every_other_output_bit_identical): start and targets on a 2^-10 grid within +-4 m, shifted by (64, -64, 32) m. Every output but root_out[:, 0:3] is
bit-identical. root_out[:, 0:3] = fl(p0 + d) with the same bits of d = the relative position in both runs, and fl(p0 + S + d) is not
fl(p0 + d) + S in general (the shifted sum rounds on a grid 16 to 32 times coarser): the two differ by at most half an ulp of each, so
the test holds |root_out' - (root_out + S)| to one ulp of the shifted value.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import ik_reference as ik
import whole_body_reference as wbr
from wbc_amd import abi

EPS = ik.EPS
C_S, C_R, C_V = 4.0, 4096.0, 32.0
NFAM = 64
CASES = ("reach", "tradeoff2", "tradeoff3", "limits", "twice", "stance")
SETTINGS = dict(reach=(1e-2, 1e-5), tradeoff2=(1e-2, 1e-4), tradeoff3=(1e-3, 1e-4), limits=(1e-2, 1e-4), twice=(1e-2, 1e-5), stance=(1e-2, 1e-5))
LAMBDA0 = 1e-3
BEYOND = 0.15


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _limit_joints(m):
    """(DoF, side) of the two joints the limits case drives onto a limit: a front calf's upper and a rear hip's lower."""
    names = list(m.dof_names)
    calf = next(i for i, s in enumerate(names) if "calf" in s)
    hip = [i for i, s in enumerate(names) if "hip" in s][-1]
    return (calf, +1), (hip, -1)


@functools.lru_cache(maxsize=None)
def _problem(case, seed):
    """(Problem, start, step_tol) of member `seed` of `case`; every number handed to the kernel is an fp32 value."""
    m = _model()
    posture, tol = SETTINGS[case]
    P, start, star = ik.member(m, seed, "tradeoff" if case.startswith("tradeoff") else "reach", posture)
    feet, grip = ik.bodies(m)
    if case == "limits":
        lo, hi, _ = ik.limits(m)
        q = np.array(star[2])
        for d, side in _limit_joints(m):
            q[d] = (hi[d] if side > 0 else lo[d]) + side * BEYOND
        pos, rot = wbr.rigid_body_poses(m, star[0], ik.quat_unit(star[1]), q)
        tq = np.tile([0.0, 0.0, 0.0, 1.0], (5, 1))
        tq[4] = ik.mat_to_quat(rot[grip])
        qc = ik.f32(np.clip(q, np.where(P.limited, lo, -np.inf), np.where(P.limited, hi, np.inf)))
        P = ik.Problem(m, P.rbs, ik.f32(pos[P.rbs]), ik.f32(tq), None, P.wori, q_ref=qc, posture=posture)
    elif case == "twice":
        tp, tq = np.concatenate([P.tpos, P.tpos[4:5]]), np.concatenate([np.tile([0.0, 0.0, 0.0, 1.0], (5, 1)), [[0.0, 0.0, 0.0, 1.0]]])
        tq[5] = ik.mat_to_quat(P.trot[4])
        wp = np.ones((6, 3)); wp[5] = 0.0
        P = ik.Problem(m, P.rbs + [grip], tp, ik.f32(tq), wp, np.array([0, 0, 0, 0, 0, 1.0]), q_ref=P.q_ref, posture=posture)
    elif case == "stance":
        rng = np.random.default_rng(77 + seed)
        off = rng.random(4) < 0.5
        wp = np.ones((5, 3)); wp[:4][off] = 0.0
        tp = P.tpos.copy(); tp[:4][off] = np.nan
        tq = np.tile([0.0, 0.0, 0.0, 1.0], (5, 1)); tq[4] = ik.mat_to_quat(P.trot[4])
        P = ik.Problem(m, P.rbs, tp, ik.f32(tq), wp, P.wori, q_ref=P.q_ref, posture=posture)
    return P, start, tol


def _fresh(case, seed):
    """A copy whose q_ref the caller may let clamp_start fill."""
    P, start, tol = _problem(case, seed)
    Q = ik.Problem.__new__(ik.Problem)
    Q.__dict__.update(P.__dict__)
    return Q, start, tol


def _allowance(P, state, origin, r=None):
    """What fp32 may leave of the objective at `state`: the residual rows' bound (C_V EPS scale; orientation rows: EPS per composed
    rotation, 8 at most) carried to first order through w r^2 / 2, and C_V EPS of the sum of the terms for the additions."""
    r = ik.kinematics(P, state, jac=False)[0] if r is None else r
    sc = np.concatenate([ik.position_scales(P, state, origin), np.full((P.K, 3), 8.0)], 1)
    w = ik.weights(P)
    return float(C_V * EPS * (np.where(w != 0, w * np.abs(r), 0.0) * sc).sum() + C_V * EPS * ik.objective_terms(P, state, r).sum())


# ------------------------------------------------------------------------------------------------------------ CPU
def test_gradient_matches_richardson_differences_through_the_retraction():
    for case, seed in (("reach", 1), ("tradeoff2", 2), ("twice", 3), ("stance", 5)):
        P, start, _ = _fresh(case, seed)
        state = ik.clamp_start(P, start)
        g, H, _ = ik.gradient_hessian(P, state)
        assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max() and np.linalg.eigvalsh(H).min() > -1e-12
        f = lambda d: ik.objective(P, ik.retract(P, state, d, clamp=False)[0])   # noqa: E731
        for c in range(ik.NLIVE):
            e = np.zeros(ik.NLIVE); e[c] = 1.0
            D = lambda h: (f(h * e) - f(-h * e)) / (2 * h)                         # noqa: E731
            num = (4 * D(5e-4) - D(1e-3)) / 3
            assert abs(num - g[c]) <= 1e-8 * max(1.0, np.abs(g).max()), (case, seed, c, num, g[c])


def test_orientation_gradient_identity():
    """d/d eps 1/2 |log(R_t (exp(eps [w]x) R)^T)|^2 = -phi . w: phi is an eigenvector of the log map's Jacobian with eigenvalue 1."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        Rt, R = [ik.ao.quat_to_mat(ik.quat_unit(rng.normal(size=4))) for _ in range(2)]
        w = rng.normal(size=3)
        phi = ik.rot_log(Rt @ R.T)
        f = lambda e: 0.5 * np.sum(ik.rot_log(Rt @ (ik.ao.quat_to_mat(ik.quat_from_rotvec(e * w)) @ R).T) ** 2)   # noqa: E731
        D = lambda h: (f(h) - f(-h)) / (2 * h)                                     # noqa: E731
        num = (4 * D(5e-4) - D(1e-3)) / 3
        assert abs(num + phi @ w) <= 1e-8 * max(1.0, abs(phi @ w)), (num, phi @ w)
    v = np.array([0.3, -0.2, 0.5])                                                 # rot_log inverts the exponential, also near pi
    for a in (1e-10, 0.5, 3.0, np.pi - 1e-7, np.pi):
        u = v / np.linalg.norm(v) * a
        back = ik.rot_log(ik.ao.quat_to_mat(ik.quat_from_rotvec(u)))
        assert min(np.abs(back - u).max(), np.abs(back + u).max() if a >= np.pi - 1e-6 else 1.0) <= 1e-7


@functools.lru_cache(maxsize=None)
def _yardstick():
    """Over every case and member: the fp64 loop and the fp32 yardstick. Returns per case (status counts fp64, status counts fp32,
    K_S over the status-0 outputs of the fp32 loop, K_R, most iterations fp32)."""
    out = {}
    for case in CASES:
        st64, st32, ks, kr, its = [], [], 0.0, 0.0, 0
        for seed in range(NFAM):
            for dtype in (np.float64, np.float32):
                P, start, tol = _fresh(case, seed)
                o = ik.solve(P, start, LAMBDA0, tol, 0, dtype)
                (st64 if dtype == np.float64 else st32).append(o["status"])
                assert o["cost"] <= o["cost0"]
                if dtype == np.float32:
                    its = max(its, o["iterations"])
                    if o["status"] == 0:
                        ks = max(ks, ik.projected_step(P, o["state"], LAMBDA0) / tol)
                        r = ik.kinematics(P, o["state"], jac=False)[0]
                        kr = max(kr, float((np.abs(r[:, :3]) / (EPS * ik.position_scales(P, o["state"], start[0]))).max()))
        out[case] = (st64, st32, ks, kr, its)
    return out


def test_family_converges_and_the_yardstick_sets_the_constants():
    y = _yardstick()
    for case in CASES:
        st64, st32, ks, kr, its = y[case]
        print(case, "fp64 status 0:", st64.count(0), "fp32 status:", {s: st32.count(s) for s in set(st32)}, "K_S %.3f" % ks, "K_R %.3g" % kr,
              "most iterations", its)
        assert st64.count(0) == NFAM, (case, st64)                                 # the fp64 statement converges on every member
        assert st32.count(0) >= (NFAM if not case.startswith("tradeoff") else 3 * NFAM // 4), (case, st32)
        assert 4 * ks <= C_S, (case, ks)
        if not case.startswith("tradeoff") and case != "limits":
            assert 16 * kr <= C_R, (case, kr)
    ks = max(v[2] for v in y.values())
    kr = max(v[3] for c, v in y.items() if not c.startswith("tradeoff") and c != "limits")
    assert C_S == max(4.0, 2.0 ** np.ceil(np.log2(4 * ks))) and C_R == max(32.0, 2.0 ** np.ceil(np.log2(16 * kr))), (ks, kr)


def test_limits_case_ends_on_the_limits_in_the_reference():
    m = _model()
    for seed in range(8):
        P, start, tol = _fresh("limits", seed)
        o = ik.solve(P, start, LAMBDA0, tol)
        g, _, _ = ik.gradient_hessian(P, o["state"])
        for d, side in _limit_joints(m):
            assert o["state"][2][d] == (P.hi32[d] if side > 0 else P.lo32[d])
            assert g[6 + P.live.index(d)] * side < 0                                # -g points outward


def test_null_and_bad_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 2)(3, 7)
    p = (C.addressof(buf) + 15) & ~15
    good = abi.WbcIkOpts(1e-2, 1e-3, 1e-4, 0)
    order = ("sim", "rb", "k", "tpos", "tquat", "wpos", "wori", "root", "dof", "qref", "opts", "root_out", "dof_out", "res", "cost", "status",
             "iters", "stream")
    base = dict(sim=None, rb=idx, k=2, tpos=p, opts=C.addressof(good), root_out=p, dof_out=p)
    call = lambda **kw: L.wbc_sim_inverse_kinematics(*[{**base, **kw}.get(k) for k in order])   # noqa: E731
    assert call() == -1
    assert b"wbc_sim_inverse_kinematics: sim is NULL" in L.wbc_last_error()
    opt = lambda *a: C.addressof(keep.setdefault(a, abi.WbcIkOpts(*a)))            # noqa: E731
    keep = {}
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(rb=None), b"NULL"), (dict(tpos=None), b"NULL"), (dict(opts=None), b"NULL"), (dict(root_out=None), b"NULL"),
                     (dict(dof_out=None), b"NULL"), (dict(k=0), b"ntargets"), (dict(k=7), b"ntargets"),
                     (dict(rb=(C.c_int32 * 2)(3, 27)), b"index"), (dict(rb=(C.c_int32 * 2)(-1, 3)), b"index"),
                     (dict(wori=p), b"w_ori"), (dict(tquat=p, wori=p + 2), b"4-byte"),
                     (dict(opts=opt(-1.0, 1e-3, 1e-4, 0)), b"posture"), (dict(opts=opt(nan, 1e-3, 1e-4, 0)), b"posture"),
                     (dict(opts=opt(1e-2, 0.0, 1e-4, 0)), b"damping"), (dict(opts=opt(1e-2, inf, 1e-4, 0)), b"damping"),
                     (dict(opts=opt(1e-2, 1e-3, 0.0, 0)), b"step_tol"), (dict(opts=opt(1e-2, 1e-3, nan, 0)), b"step_tol"),
                     (dict(opts=opt(1e-2, 1e-3, 1e-4, -1)), b"max_iter"), (dict(opts=opt(1e-2, 1e-3, 1e-4, 65)), b"max_iter"),
                     (dict(tpos=p + 2), b"4-byte"), (dict(tquat=p + 1), b"4-byte"), (dict(wpos=p + 3), b"4-byte"), (dict(root=p + 2), b"4-byte"),
                     (dict(dof=p + 2), b"4-byte"), (dict(qref=p + 1), b"4-byte"), (dict(root_out=p + 2), b"4-byte"), (dict(dof_out=p + 1), b"4-byte"),
                     (dict(res=p + 2), b"4-byte"), (dict(cost=p + 2), b"4-byte"), (dict(status=p + 2), b"4-byte"), (dict(iters=p + 2), b"4-byte")):
        assert call(**kw) == -1, kw
        msg = L.wbc_last_error()
        assert msg.startswith(b"wbc_sim_inverse_kinematics: ") and word in msg, (kw, msg)
    assert all(v == 0 for v in buf)                                               # nothing written


def test_kernel_metadata():
    """Metadata only: no scratch, a single wavefront, static LDS within the 20 kB that keep eight workgroups per CU."""
    assert arm_codegen.meta("wbc_ik_kernel", "private_segment_fixed_size") == 0
    assert arm_codegen.meta("wbc_ik_kernel", "max_flat_workgroup_size") == 64
    assert arm_codegen.meta("wbc_ik_kernel", "group_segment_fixed_size") <= 20 * 1024


# ------------------------------------------------------------------------------------------------------------ GPU
def _np(t):
    return t.detach().cpu().numpy().astype(np.float64) if t.dtype.is_floating_point else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _env(n):
    import test_inverse_dynamics as tid
    return tid._env(n, seed=11, steps=3)


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda").contiguous()


def _arrays(problems):
    """The kernel's inputs of a list of (Problem, start, tol) with one list of bodies."""
    Ps, starts = [p[0] for p in problems], [p[1] for p in problems]
    quat = Ps[0].tquat is not None
    tq = np.stack([P.tquat for P in Ps]) if quat else None
    return dict(bodies=Ps[0].rbs, target_pos=_dev(np.stack([P.tpos for P in Ps])), target_quat=_dev(tq) if quat else None,
                w_pos=_dev(np.stack([P.wpos for P in Ps])), w_ori=_dev(np.stack([P.wori for P in Ps])) if quat else None,
                root_init=_dev(np.stack([np.r_[s[0], s[1]] for s in starts])), dof_init=_dev(np.stack([s[2] for s in starts])),
                q_ref=None if Ps[0].q_ref is None else _dev(np.stack([P.q_ref for P in Ps])))


def _call(sim, **kw):
    """sim.inverse_kinematics with the sim's own state held bit-identical across the call (asserted in every case)."""
    root0, dof0 = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
    root, dof, info = sim.inverse_kinematics(**kw)
    torch.cuda.synchronize()
    assert torch.equal(sim.tensor("ROOT_STATES").view(torch.int32), root0.view(torch.int32))
    assert torch.equal(sim.tensor("DOF_STATE").view(torch.int32), dof0.view(torch.int32))
    return dict(root=root, dof=dof, **info)


@functools.lru_cache(maxsize=None)
def _run(case, n):
    """The kernel's answer to members 0..n-1 of `case`, once per (case, n): (problems, raw tensors, numpy copies)."""
    problems = [_fresh(case, seed) for seed in range(n)]
    posture, tol = SETTINGS[case]
    raw = _call(_env(n).sim, posture=posture, damping=LAMBDA0, step_tol=tol, **_arrays(problems))
    for P, start, _ in problems:
        ik.clamp_start(P, start)                                                  # q_ref NULL: the clamped start joints
    return problems, raw, {k: _np(v) for k, v in raw.items()}


def _state(out, i):
    return out["root"][i, :3], out["root"][i, 3:7], out["dof"][i]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
@pytest.mark.parametrize("case", CASES)
def test_status_0_means_the_fp64_projected_step_is_small(case, n):
    problems, _, out = _run(case, n)
    worst, ok = 0.0, 0
    for i, (P, start, tol) in enumerate(problems):
        assert out["status"][i] in (0, 1, 2), (i, out["status"][i])
        if out["status"][i] == 0:
            ok += 1
            worst = max(worst, ik.projected_step(P, _state(out, i), LAMBDA0) / tol)
    print(case, n, "status 0: %d of %d" % (ok, n), "largest projected step / step_tol %.3f" % worst, "most iterations", out["iterations"].max())
    assert worst <= C_S, (case, n, worst)
    assert ok >= (n if not case.startswith("tradeoff") else 3 * n // 4), (case, n, out["status"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
@pytest.mark.parametrize("case", ["reach", "twice", "stance"])
def test_reaching(case, n):
    problems, _, out = _run(case, n)
    worst = 0.0
    for i, (P, start, tol) in enumerate(problems):
        assert out["status"][i] == 0, (i, out["status"][i], out["iterations"][i])
        st = _state(out, i)
        r = ik.kinematics(P, st, jac=False)[0]
        worst = max(worst, float((np.abs(r[:, :3]) / (EPS * ik.position_scales(P, st, start[0]))).max()))
    print(case, n, "largest |position residual| / (EPS scale) %.3g" % worst)
    assert worst <= C_R, (case, n, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
@pytest.mark.parametrize("case", CASES)
def test_descent_limits_and_reported_values(case, n):
    problems, raw, out = _run(case, n)
    m = _model()
    lo, hi, limited = ik.limits(m)
    live = ik.live_dofs(m)
    lim = [d for d in live if limited[d]]
    assert bool((raw["cost"][:, 1] <= raw["cost"][:, 0]).all())                    # bit-wise: fp32 against fp32
    q32 = raw["dof"].cpu().numpy()
    assert np.all(q32[:, lim] >= lo[lim].astype(np.float32)) and np.all(q32[:, lim] <= hi[lim].astype(np.float32))
    assert np.all(np.abs(np.linalg.norm(out["root"][:, 3:7], axis=1) - 1.0) <= 4 * EPS)
    worst_r = worst_c = worst_o = 0.0
    for i, (P, start, tol) in enumerate(problems):
        st, s0 = _state(out, i), ik.clamp_start(P, start)
        r = ik.kinematics(P, st, jac=False)[0]
        f1, f0 = ik.objective(P, st, r), ik.objective(P, s0)
        a1, a0 = _allowance(P, st, start[0], r), _allowance(P, s0, start[0])
        assert f1 <= f0 + a0 + a1, (i, f0, f1)
        got = out["residual"][i]
        w = ik.weights(P)
        assert np.all(got[w == 0] == 0), i                                         # skipped rows: exactly 0
        assert np.all(np.isfinite(got))
        sc = ik.position_scales(P, st, start[0])
        worst_r = max(worst_r, float((np.abs(got[:, :3] - r[:, :3]) / (EPS * sc)).max()))
        worst_o = max(worst_o, float(np.abs(got[:, 3:] - r[:, 3:]).max() / (EPS * 8.0)))
        worst_c = max(worst_c, abs(out["cost"][i, 1] - f1) / a1, abs(out["cost"][i, 0] - f0) / a0)
        # fingers: the start's bits
        assert np.array_equal(q32[i, [d for d in range(abi.NDOF) if d not in live]], np.float32(start[2])[[d for d in range(abi.NDOF) if d not in live]])
        if case == "limits":
            g, _, _ = ik.gradient_hessian(P, st)
            for d, side in _limit_joints(m):                                       # both joints on their limits, -g pointing outward
                assert q32[i, d] == np.float32(hi[d] if side > 0 else lo[d]), (i, d, q32[i, d])
                assert g[6 + live.index(d)] * side < 0, (i, d, g[6 + live.index(d)])
    print(case, n, "reported residual: position %.3f  orientation %.3f  of C_V EPS scale; cost %.3f of its allowance"
          % (worst_r / C_V, worst_o / C_V, worst_c))
    assert worst_r <= C_V and worst_o <= C_V and worst_c <= 1.0, (case, n, worst_r, worst_o, worst_c)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_nan_in_a_skipped_row_does_not_spread(n):
    first = next(seed for seed in range(NFAM) if np.isnan(_problem("stance", seed)[0].tpos).any())
    seeds = range(n) if n > 1 else [first]                                        # a member with a switched-off foot also at n = 1
    problems = [_fresh("stance", seed) for seed in seeds]
    posture, tol = SETTINGS["stance"]
    arr = _arrays(problems)
    assert bool(torch.isnan(arr["target_pos"]).any())
    raw = _call(_env(n).sim, posture=posture, damping=LAMBDA0, step_tol=tol, **arr)
    for k in ("root", "dof", "residual", "cost"):
        assert bool(torch.isfinite(raw[k]).all()), k
    assert bool((raw["status"] == 0).all())
    clean = []
    for P, start, tol_ in problems:
        Q = ik.Problem.__new__(ik.Problem); Q.__dict__.update(P.__dict__)
        Q.tpos = np.where(np.isnan(P.tpos), 0.25, P.tpos)
        clean.append((Q, start, tol_))
    assert _arrays(clean)["q_ref"] is not None
    other = _call(_env(n).sim, posture=posture, damping=LAMBDA0, step_tol=tol, **_arrays(clean))
    for k in raw:
        assert torch.equal(raw[k], other[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_targets_at_the_start_return_the_start_and_null_inits_read_the_sim(n):
    m = _model()
    env = _env(n)
    sim = env.sim
    feet, grip = ik.bodies(m)
    rbs = feet + [grip]
    starts = [_problem("reach", seed)[1] for seed in range(n)]
    tp, tq = [], []
    for s in starts:
        pos, rot = wbr.rigid_body_poses(m, s[0], ik.quat_unit(s[1]), s[2])
        tp.append(pos[rbs]); tq.append([ik.mat_to_quat(rot[r]) for r in rbs])
    root_init, dof_init = _dev(np.stack([np.r_[s[0], s[1]] for s in starts])), _dev(np.stack([s[2] for s in starts]))
    kw = dict(bodies=rbs, target_pos=_dev(np.stack(tp)), target_quat=_dev(np.array(tq)))
    a = _call(sim, root_init=root_init, dof_init=dof_init, **kw)
    assert bool((a["status"] == 0).all()) and bool((a["iterations"] == 0).all())
    assert torch.equal(a["root"].view(torch.int32), root_init.view(torch.int32)) and torch.equal(a["dof"].view(torch.int32), dof_init.view(torch.int32))
    assert torch.equal(a["cost"][:, 0], a["cost"][:, 1])
    # the same start through the sim's own state: the bits of NULL
    root0, dof0 = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
    rs, ds = root0.clone(), dof0.clone()
    rs[:, 0, :7] = root_init
    ds[..., 0] = dof_init
    sim.set_root_state(rs.contiguous()); sim.set_dof_state(ds.contiguous())
    try:
        P = [_problem("tradeoff2", seed) for seed in range(n)]
        arr = _arrays(P)
        b = _call(sim, **arr)
        arr.update(root_init=None, dof_init=None)
        c = _call(sim, **arr)
        for k in b:
            assert torch.equal(b[k], c[k]), k
        assert bool((b["iterations"] > 0).all())
    finally:
        sim.set_root_state(root0.contiguous()); sim.set_dof_state(dof0.contiguous())
        torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_translation_leaves_every_other_output_bit_identical(n):
    m = _model()
    feet, grip = ik.bodies(m)
    rbs = feet + [grip]
    grid = lambda a: np.round(np.asarray(a) * 1024.0) / 1024.0                    # noqa: E731
    problems = [_problem("tradeoff2", seed) for seed in range(n)]
    arr = _arrays(problems)
    root = _np(arr["root_init"]); root[:, :3] = grid(root[:, :3])
    tpos = grid(_np(arr["target_pos"]))
    assert np.abs(root[:, :3]).max() <= 4 and np.abs(tpos).max() <= 4
    shift = np.array([64.0, -64.0, 32.0])
    outs = []
    for s in (np.zeros(3), shift):
        r = root.copy(); r[:, :3] += s
        arr.update(root_init=_dev(r), target_pos=_dev(tpos + s))
        assert np.array_equal(_np(arr["root_init"])[:, :3], r[:, :3]) and np.array_equal(_np(arr["target_pos"]), tpos + s)   # exact in fp32
        outs.append(_call(_env(n).sim, **arr))
    a, b = outs
    assert bool((a["iterations"] > 0).all())
    for k in a:
        if k != "root":
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["root"][:, 3:], b["root"][:, 3:])
    pa, pb = _np(a["root"][:, :3]), _np(b["root"][:, :3])
    assert np.all(np.abs(pb - (pa + shift)) <= np.spacing(np.abs(pb).astype(np.float32)).astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_unreachable_target_cap_and_non_finite_input(n):
    m = _model()
    sim = _env(n).sim
    lo, hi, limited = ik.limits(m)
    lim = [d for d in ik.live_dofs(m) if limited[d]]
    # the gripper 2 m from the trunk, the feet held
    far = []
    for seed in range(n):
        P, start, tol = _fresh("tradeoff2", seed)
        d = P.tpos[4] - start[0]
        P.tpos[4] = ik.f32(start[0] + 2.0 * d / np.linalg.norm(d))
        far.append((P, start, tol))
    out = _call(sim, **_arrays(far))
    o = {k: _np(v) for k, v in out.items()}
    assert np.all(np.isin(o["status"], (1, 2))), o["status"]
    q32 = out["dof"].cpu().numpy()
    assert np.all(np.isfinite(o["root"])) and np.all(np.isfinite(o["dof"]))
    assert np.all(q32[:, lim] >= lo[lim].astype(np.float32)) and np.all(q32[:, lim] <= hi[lim].astype(np.float32))
    for i, (P, start, tol) in enumerate(far):
        s0 = ik.clamp_start(P, start)
        assert ik.objective(P, _state(o, i)) < ik.objective(P, s0), i
    print("unreachable: status", o["status"], "iterations", o["iterations"])
    # the cap
    problems = [_problem("tradeoff2", seed) for seed in range(n)]
    arr = _arrays(problems)
    full = _call(sim, **arr)
    need = full["iterations"] > 1
    assert bool(need.any())
    one = _call(sim, max_iter=1, **arr)
    assert bool((one["status"][need] == 1).all()) and bool((one["iterations"][need] == 1).all())
    # a non-finite target of one env
    # (the env: an odd one with its partner in the workgroup; at n = 64 an even one and the last as well; at n = 1 the only one)
    for bad, e in [(v, e) for v in (float("nan"), float("inf")) for e in {1: [0], 13: [5, 12], 64: [5, 6, 63]}[n]]:
        tp = arr["target_pos"].clone()
        tp[e, 4, 1] = bad
        hit = _call(sim, **{**arr, "target_pos": tp})
        assert int(hit["status"][e]) == 3 and int(hit["iterations"][e]) == 0
        assert torch.equal(hit["root"][e].view(torch.int32), arr["root_init"][e].view(torch.int32))
        assert torch.equal(hit["dof"][e].view(torch.int32), arr["dof_init"][e].view(torch.int32))
        keep = [i for i in range(n) if i != e]
        for k in full:
            assert torch.equal(hit[k][keep], full[k][keep]), k


def _facade_member(seed):
    """The family's goals for the Python layer, which keeps the feet where they are NOW: the sim holds member `seed`'s q* with the six
    arm joints moved by +-0.3 rad (clamped), so the feet stand at the family's foot targets, and the goal is the family's gripper
    target, the gripper's position at q*. q* lies anywhere inside the limits, up to 2 rad from default_dof_pos: the posture term of
    the first solve is fully at work. Returns (state now, goal)."""
    m = _model()
    P, _, star = ik.member(m, seed, "reach", 1e-2)
    rng = np.random.default_rng(400 + seed)
    q = np.array(star[2])
    for d in P.live[12:]:
        q[d] += 0.3 * rng.choice([-1.0, 1.0])
        if P.limited[d]:
            q[d] = min(max(q[d], P.lo32[d]), P.hi32[d])
    return (star[0], star[1], ik.f32(q)), P.tpos[4]


def test_facade_refinement_meets_the_family_goals_in_the_yardstick():
    """reach_configuration's scheme in the fp32 yardstick: the first solve towards default_dof_pos misses the family's targets by
    centimetres, two proximal solves (q_ref the last answer, posture 1e-5, step_tol 1e-5) bring them within 1e-6 m, every one of them
    ending with status 0."""
    m = _model()
    feet, grip = ik.bodies(m)
    from wbc_amd.config import WidowGo1RoughCfg
    qd = ik.f32(np.array(list(abi.fill_task_cfg(WidowGo1RoughCfg(), m).default_dof_pos)))
    first = last = 0.0
    for seed in range(16):
        now, goal = _facade_member(seed)
        pos, _ = wbr.rigid_body_poses(m, now[0], ik.quat_unit(now[1]), now[2])
        P = ik.Problem(m, feet + [grip], ik.f32(np.vstack([pos[feet], goal])), q_ref=qd, posture=1e-2)
        s = now
        for stage, (posture, tol) in enumerate(((1e-2, 1e-4), (1e-5, 1e-5), (1e-5, 1e-5))):
            P.posture = posture
            if stage > 0:
                P.q_ref = None
            o = ik.solve(P, s, LAMBDA0, tol, 0, np.float32)
            s = o["state"]
            r = float(np.abs(ik.kinematics(P, s, jac=False)[0][:, :3]).max())
            first = max(first, r) if stage == 0 else first
            assert stage == 0 or o["status"] == 0, (seed, stage, o["status"])
        last = max(last, r)
    print("yardstick: largest |position residual| after the first solve %.3g m, after two refinements %.3g m" % (first, last))
    assert first > 1e-2 and last <= 1e-6, (first, last)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_reach_configuration_and_goal_reachability(n):
    """The Python layer on the family's goals (_facade_member), at its defaults: ee_goal_reachable is true for them and false for a
    goal 2 m from the trunk, and leaves the state untouched; reach_configuration(apply=True) followed by refresh_rigid_body_state puts
    all four feet and the gripper where asked within the reach bound C_R 2^-24 scale, with zero velocities."""
    m = _model()
    env = _env(n)
    sim = env.sim
    feet, grip = ik.bodies(m)
    root0, dof0 = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
    members = [_facade_member(seed) for seed in range(n)]
    rs, ds = root0.clone(), dof0.clone()
    for e, (now, _) in enumerate(members):
        rs[e, 0, :7] = torch.tensor(np.r_[now[0], now[1]], dtype=torch.float32)
        ds[e, :, 0] = torch.tensor(now[2], dtype=torch.float32)
    sim.set_root_state(rs.contiguous()); sim.set_dof_state(ds.contiguous())
    try:
        goal = _dev(np.stack([g for _, g in members]))
        sim.refresh_rigid_body_state()
        torch.cuda.synchronize()
        feet_now = _np(env.rigid_body_state)[:, feet, :3]
        before = sim.tensor("ROOT_STATES").clone(), sim.tensor("DOF_STATE").clone()
        ok = env.ee_goal_reachable(goal, 1e-3)
        torch.cuda.synchronize()
        assert torch.equal(sim.tensor("ROOT_STATES"), before[0]) and torch.equal(sim.tensor("DOF_STATE"), before[1])
        assert bool(ok.all()), ok
        trunk = _dev(np.stack([now[0] for now, _ in members]))
        dirn = goal - trunk
        away = (trunk + 2.0 * dirn / dirn.norm(dim=-1, keepdim=True)).contiguous()
        assert not bool(env.ee_goal_reachable(away, 1e-3).any())
        assert torch.equal(sim.tensor("ROOT_STATES"), before[0]) and torch.equal(sim.tensor("DOF_STATE"), before[1])
        root, dof, info = env.reach_configuration(goal, apply=True)
        sim.refresh_rigid_body_state()
        torch.cuda.synchronize()
        assert bool((info["status"] == 0).all()), info["status"]
        assert torch.equal(sim.tensor("ROOT_STATES")[:, 0, :7], root) and torch.equal(sim.tensor("DOF_STATE")[..., 0], dof)
        assert bool((sim.tensor("ROOT_STATES")[:, 0, 7:] == 0).all()) and bool((sim.tensor("DOF_STATE")[..., 1] == 0).all())
        rb = _np(env.rigid_body_state)
        worst = worst_m = 0.0
        for e, (now, g) in enumerate(members):
            P = ik.Problem(m, feet + [grip], np.vstack([feet_now[e], _np(goal)[e]]))
            sc = ik.position_scales(P, (_np(root)[e, :3], _np(root)[e, 3:7], _np(dof)[e]), now[0])
            err = np.abs(rb[e][feet + [grip], :3] - P.tpos)
            worst, worst_m = max(worst, float((err / (EPS * sc)).max())), max(worst_m, float(err.max()))
        print("reach_configuration, n = %d: largest |position error| %.3g m = %.3g EPS scale, most iterations %d"
              % (n, worst_m, worst, int(info["iterations"].max())))
        assert worst <= C_R, worst
    finally:
        sim.set_root_state(root0.contiguous()); sim.set_dof_state(dof0.contiguous())
        sim.refresh_rigid_body_state()
        torch.cuda.synchronize()
