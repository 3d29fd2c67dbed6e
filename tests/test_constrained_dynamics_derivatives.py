"""Analytic derivatives of stance-constrained forward dynamics (wbc_sim_constrained_dynamics_derivatives, wbc_constraint_tangent_kernel and
wbc_constraint_derivatives_solve_kernel in csrc/wbc_arm_kernel.hip; definitions and the tangent convention in include/wbc_sim.h). The CPU
tests pin the fp64 reference of tests/constrained_derivatives_reference.py to Richardson-extrapolated central differences of
constrained_dynamics_reference.solve_with_mask, to the flow identity and to the structure of the equations, and measure the fp32
yardsticks; the GPU tests hold the kernels to the reference in residual form, column by column, to the sibling entry point and to their
own invariances.

Bounds, with the reference's residual partials evaluated at the kernel's own (nudot, lambda), D and Lam the kernel's columns:
    dynamics rows    |M_ref D + dr1_ref - Jc^T Lam|_k <= C_S 2^-24 scale_k + C_D 2^-24 mag_k(dtau_ID) + C_J 2^-24 mag_k(d(Jc^T lambda))
    constraint rows  |Jc D + damping Lam + dr2_ref|_i <= C_K 2^-24 scale_i + C_R 2^-24 mag_i(dr2)
scale from constrained_dynamics_reference.dynamics_residual_and_scale / constraint_residual_and_scale applied to the column (the
right-hand side -dr1 / -dr2 in the place of tau / a_des, so that its own size counts). C_S = 128, C_K = 32 and C_D = 32768 (q, tau) /
524288 (nu) are restated from their modules. C_J and C_R are the smallest powers of two >= 16 K_ref, K_ref the fp32 yardstick's largest
|yardstick - ref| / (2^-24 mag) over 60 members of test_constrained_dynamics._family (at the fp64 solution rounded to fp32) and the two
state families of test_centroidal._state, 64 states each (feet + gripper, their nudot, a random lambda within +-100 N), measured on the
CPU against the fp64 reference and asserted <= C / 16:

    term                    K_ref     C
    d(Jc^T lambda)/dq       655       16384
    dr2/dq, dr2/dnu         7.27      128

The large K_ref of the first is single entries, as for dtau_dq (tests/test_dynamics_derivatives.py): one component of a x (b x l) is the
difference of two products many times its size, and mag counts the component-wise size of the two summed cross products only. The two
terms are not outputs, so the kernel's own figures are those of the rows they enter. The whole fp32 chain (yardstick_f32, the first
twelve members of _family) and the kernels, as the largest residual over its allowance (n = 1, 13, 64, both families, every case of
the GPU tests):

    rows                    fp32 yardstick (CPU)    host build of the kernels' text    kernels on an MI355X
    dynamics rows           0.0231                  0.031                              0.0314  (n = 64, feet + gripper with damping)
    constraint rows         0.101                   0.17                               0.237   (n = 64, four feet)

The largest scaled Delassus condition number over the GPU cases is 96.9 (asserted <= COND_MAX = 1000; 85.1 over _family on the CPU).

The GPU tests run on the two state families of test_centroidal._state (the envs of test_dynamics_derivatives._case), the families C_D,
C_J and C_R were measured on. On the envs of test_mass_solve._case (states reached by stepping the simulator from the reset pose) the
EXISTING wbc_dynamics_derivatives_kernel exceeds its own C_D at single entries of the wrist joints' rows against each other, entries of
1e-7 N m / rad: 1.0e5 against 32768 for dtau_dq at n = 64 with tau NULL (an absolute error of 1.4e-9), 7.0e5 against 524288 for dtau_dnu
at n = 13. This call takes -dtau_ID from that kernel, so its dynamics rows then show the same entry (2.14 times the allowance at n = 64,
four feet, tau NULL; at most 0.065 in the other five cases at n = 64, 0.264 at n = 13); the two new terms measured apart on those envs:
d(Jc^T lambda)/dq 623 x 2^-24 mag, dr2 33 x 2^-24 mag, inside C_J and C_R.

The host build is the kernels' text compiled for the CPU (one thread per lane, a barrier for __syncthreads(), a stand-alone program under
AddressSanitizer and UBSan: no out-of-bounds access, and the same bits for every subset of outputs and both layouts, at n = 1, 13, 64).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import constrained_derivatives_reference as cdd
import constrained_dynamics_reference as cdr
import dynamics_derivatives_reference as ddr
import mass_solve_reference as msr
import test_centroidal as tc
import test_constrained_dynamics as tcd
import test_dynamics_derivatives as tdd

NCOL, EPS, FINGERS, LIVE, GROUPS = cdd.NCOL, cdd.EPS, cdd.FINGERS, cdd.LIVE, cdd.GROUPS
SENTINEL, MENV = 12345.0, cdd.NCOL * cdd.NCOL
ARMATURE, TRANSPOSED = 1, 2
COND_MAX = 1000.0
OUTPUTS = ("dnudot_dq", "dnudot_dnu", "dnudot_dtau", "dlambda_dq", "dlambda_dnu", "dlambda_dtau")
# restated from their modules
C_S, C_K, C_D = 128.0, 32.0, {"dq": 32768.0, "dnu": 524288.0}
assert C_S == msr.C_S == cdd.C_S and C_K == cdr.C_K == cdd.C_K and C_D == ddr.C == cdd.C_D
assert COND_MAX == tcd.COND_MAX

_model, _rotated, _richardson = tc._model, tc._rotated, tdd._richardson


@functools.lru_cache(maxsize=None)
def _armature():
    from wbc_amd import abi
    from wbc_amd.config import WidowGo1RoughCfg
    return msr.armature_vector(abi.fill_task_cfg(WidowGo1RoughCfg(), _model()))


def _solve(state, bodies, on, tau, a_des, damping, arm, dq=None, dnu=None, dtau=None):
    """solve_with_mask at the configuration moved along the tangent dq, at nu + dnu and tau + dtau."""
    pos, quat, q, nu, bp = state
    if dq is not None:
        pos, quat, q = pos + dq[0:3], _rotated(quat, dq[3:6]), q + dq[6:]
    if dnu is not None:
        nu = nu + dnu
    t = np.zeros(NCOL) if tau is None else np.asarray(tau, dtype=np.float64)
    if dtau is not None:
        t = t + dtau
    M, h, Jc, gamma = cdd.system(_model(), (pos, quat, q, nu, bp), bodies, on, arm)
    return np.concatenate(cdr.solve_with_mask(M, h, t, Jc, gamma, a_des, damping, on))


# ------------------------------------------------------------------------------------------------------------ CPU
def test_reference_against_richardson_central_differences():
    m = _model()
    worst = 0.0
    for seed in range(12):
        state, bodies, on, tau, a_des, damping, arm = tcd._family(m, seed, _armature())
        ref = cdd.constrained_dynamics_derivatives(m, state, bodies, on, tau, a_des, damping, arm)

        def diff(h):
            out = np.zeros((3, NCOL + len(on), NCOL))
            for k in range(NCOL):
                e = np.zeros(NCOL); e[k] = h
                for g, kw in enumerate(("dq", "dnu", "dtau")):
                    out[g, :, k] = (_solve(state, bodies, on, tau, a_des, damping, arm, **{kw: e})
                                    - _solve(state, bodies, on, tau, a_des, damping, arm, **{kw: -e})) / (2 * h)
            return out
        want = _richardson(diff)
        want[2][:, FINGERS] = 0.0                                 # the fingers' entries of tau are ignored: no column
        for gi, g in enumerate(GROUPS):
            for D, W in ((ref["dnudot"][g], want[gi][:NCOL]), (ref["dlambda"][g], want[gi][NCOL:])):
                if D.size == 0:
                    continue
                err = np.abs(D - W).max()
                worst = max(worst, err / max(1.0, np.abs(D).max()))
                assert err <= 1e-6 * max(1.0, np.abs(D).max()), (seed, g, err)
    print(f"reference vs Richardson differences: largest |diff| / max(1, max |D|) = {worst:.3g}")


def test_reference_flow_identity():
    """Along the motion config(t) = (p + t v, exp(t [omega]x) R, q + t qd), nu(t) = nu + t nudot(0), tau(t) = tau + t taudot at fixed
    a_des: d (nudot, lambda) / dt at 0 = D_q nu + D_nu nudot + D_tau taudot. The left side by the Richardson difference of test 1,
    whose entries agree to 1e-6 max(1, max |D|) there; this derivative is their combination with the weights nu, nudot and taudot,
    hence the allowance 1e-6 max(1, max |D_q|, max |D_nu|, max |D_tau|) (|nu|_1 + |nudot|_1 + |taudot|_1). It pins the tangent
    convention under the constraint, rotation included."""
    m = _model()
    for seed in range(12):
        state, bodies, on, tau, a_des, damping, arm = tcd._family(m, seed, _armature())
        pos, quat, q, nu, bp = state
        nu = nu.copy(); nu[FINGERS] = 0.0
        state = (pos, quat, q, nu, bp)
        taudot = msr.force_rhs(np.random.default_rng(1100 + seed), ()) * 10.0
        taudot[FINGERS] = 0.0
        ref = cdd.constrained_dynamics_derivatives(m, state, bodies, on, tau, a_des, damping, arm)
        nd = ref["nudot"]
        at = lambda t: _solve(state, bodies, on, tau, a_des, damping, arm, dq=t * nu, dnu=t * nd, dtau=t * taudot)
        got = _richardson(lambda h: (at(h) - at(-h)) / (2 * h))
        for name, rows in (("dnudot", slice(0, NCOL)), ("dlambda", slice(NCOL, None))):
            D = ref[name]
            want = D["q"] @ nu + D["nu"] @ nd + D["tau"] @ taudot
            big = max([1.0] + [np.abs(D[g]).max() for g in GROUPS if D[g].size])
            allow = 1e-6 * big * (np.abs(nu).sum() + np.abs(nd).sum() + np.abs(taudot).sum())
            assert np.abs(got[rows] - want).max() <= allow, (seed, name, np.abs(got[rows] - want).max(), allow)


def _assert_exact_structure(out, on):
    """The literal zeros of include/wbc_sim.h, as equalities; out {name: [..., rows, 26]}, on [..., m] bool."""
    for name, D in out.items():
        assert np.all(D[..., :, FINGERS] == 0), name
        if name.startswith("dnudot"):
            assert np.all(D[..., FINGERS, :] == 0), name
        else:
            assert np.all(D[~on] == 0), name
        if not name.endswith("dtau"):
            assert np.all(D[..., :, 0:3] == 0), name


def test_reference_structure():
    m = _model()
    none_seen = False
    for seed in range(15):
        state, bodies, on, tau, a_des, damping, arm = tcd._family(m, seed, _armature())
        ref = cdd.constrained_dynamics_derivatives(m, state, bodies, on, tau, a_des, damping, arm)
        out = {f"dnudot_d{g}": ref["dnudot"][g] for g in GROUPS}
        out.update({f"dlambda_d{g}": ref["dlambda"][g] for g in GROUPS})
        _assert_exact_structure(out, on)
        T = ref["dnudot"]["tau"][np.ix_(LIVE, LIVE)]
        assert np.abs(T - T.T).max() <= 1e-9 * np.abs(T).max()
        Jc, parts = ref["Jc"], ref["parts"]
        for g in GROUPS:
            res = Jc @ ref["dnudot"][g] + damping * ref["dlambda"][g] + parts["r2"][g]
            scale = np.abs(Jc) @ np.abs(ref["dnudot"][g]) + np.abs(parts["r2"][g]) + 1e-300
            assert not on.any() or np.all(np.abs(res)[on] <= 1e-9 * scale[on].max()), (seed, g)
            assert g != "tau" or np.all(parts["r2"][g] == 0)
        if not on.any():                                          # no active body: the free robot's partials
            none_seen = True
            pos, quat, q, nu, bp = state
            _, Xq, Xn, Minv, _, _ = ddr.forward_dynamics_derivatives(m, pos, quat, q, nu, tau, bp, armature=arm)
            for g, X in zip(GROUPS, (Xq, Xn, Minv)):
                assert np.abs(ref["dnudot"][g] - X).max() <= 1e-9 * max(1.0, np.abs(X).max()), (seed, g)
    assert none_seen


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """(K_ref of d(Jc^T lambda), K_ref of dr2, the fp32 chain's largest residual / allowance on the dynamics and the constraint rows,
    the largest scaled Delassus condition number over the family)."""
    m = _model()
    feet, grip = tcd._bodies(m)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    k = {"J": 0.0, "R": 0.0, "dyn": 0.0, "con": 0.0, "cond": 0.0}

    def terms(state, bodies, on, nudot, lam):
        pos, quat, q, nu, _bp = state
        r = cdd.constraint_partials(m, pos, quat, q, nu, nudot, lam, bodies, on)
        y = cdd.constraint_partials(m, pos, quat, q, nu, nudot, lam, bodies, on, dtype=np.float32)
        if on.any():
            k["R"] = max(k["R"], ddr.largest_ratio(y[0], r[0], r[1]))
            k["J"] = max(k["J"], ddr.largest_ratio(y[2], r[2], r[3]))
    for seed in range(60):
        state, bodies, on, tau, a_des, damping, arm = tcd._family(m, seed, _armature())
        M, h, Jc, gamma = cdd.system(m, state, bodies, on, arm)
        k["cond"] = max(k["cond"], cdr.delassus_condition(M, Jc, damping, on))
        nudot, lam = (f32(x) for x in cdr.solve_with_mask(M, h, tau, Jc, gamma, a_des, damping, on))
        terms(state, bodies, on, nudot, lam)
        if seed < 12:                                             # the whole chain in fp32 (slow in numpy): the first twelve members
            parts = cdd.residual_partials(m, state, bodies, on, nudot, lam)
            Ds, Ls = cdd.yardstick_f32(m, state, bodies, on, nudot, lam, M, Jc, damping)
            for g in GROUPS:
                rd, ad, rc, ac = cdd.column_bounds(M, Jc, damping, on, parts, g, Ds[g], Ls[g])
                k["dyn"] = max(k["dyn"], float((rd[ad > 0] / ad[ad > 0]).max()))
                assert np.all(rd[ad <= 0] == 0) and np.all(rc[ac <= 0] == 0)
                if (ac > 0).any():
                    k["con"] = max(k["con"], float((rc[ac > 0] / ac[ac > 0]).max()))
    for fast in (False, True):
        for seed in range(64):
            pos, quat, q, nu, bp, nudot = tc._state(seed, fast)
            lam = np.random.default_rng(1300 + seed).uniform(-100, 100, 15)
            terms((pos, quat, q, nu, bp), feet + [grip], np.ones(15, dtype=bool), f32(nudot), f32(lam))
    return k


def test_fp32_yardsticks_sit_well_inside_the_bounds():
    k = _yardsticks()
    print(f"constrained derivatives yardsticks: d(Jc^T lambda) K_ref = {k['J']:.4g} (C_J = {cdd.C_J:g}), dr2 K_ref = {k['R']:.4g} "
          f"(C_R = {cdd.C_R:g}); fp32 chain's largest residual / allowance: dynamics rows {k['dyn']:.3g}, constraint rows {k['con']:.3g}; "
          f"largest scaled Delassus condition number {k['cond']:.3g}")
    for key, Cc in (("J", cdd.C_J), ("R", cdd.C_R)):
        assert k[key] <= Cc / 16, (key, k[key])
        assert Cc == 2.0 ** np.ceil(np.log2(16 * k[key])), (key, k[key])
    assert k["dyn"] <= 1.0 and k["con"] <= 1.0                    # the yardstick meets the bounds the kernel is held to
    assert k["cond"] <= COND_MAX


def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 2)(3, 7)
    p = C.addressof(buf)
    f = L.wbc_sim_constrained_dynamics_derivatives
    assert f(None, idx, 2, None, None, None, 0.0, 0, p, None, p, p, p, p, p, p, p, None) == -1
    assert b"NULL" in L.wbc_last_error() and b"wbc_sim_constrained_dynamics_derivatives" in L.wbc_last_error()
    w = L.wbc_sim_constrained_dynamics_derivatives_workspace_floats
    assert w(10, 4) == L.wbc_sim_constrained_dynamics_workspace_floats(10, 4) + 10 * (16 + 5 * MENV + 2 * 15 * 26) + MENV
    assert w(10, 0) == 0 and w(10, 6) == 0 and w(0, 4) == 0 and w(-3, 4) == 0


def test_new_kernels_codegen():
    """The code object's metadata alone: no scratch, the launch's workgroup size, static LDS within 20 KB (8 workgroups per CU)."""
    for kernel in ("wbc_constraint_tangent_kernel", "wbc_constraint_derivatives_solve_kernel"):
        assert arm_codegen.meta(kernel, "private_segment_fixed_size") == 0, kernel
        assert arm_codegen.meta(kernel, "max_flat_workgroup_size") == 64, kernel
        assert arm_codegen.meta(kernel, "group_segment_fixed_size") <= 20480, kernel


# ------------------------------------------------------------------------------------------------------------ GPU
def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


def _launch(env, bodies, active=None, tau=None, a_des=None, damping=0.0, flags=0, which=OUTPUTS, want_lambda=True):
    """A direct C-ABI call into sentinel-framed buffers with a workspace of exactly the size asked for; returns {name: tensor} in the
    layout asked for, with "nudot" [n, 26] and "lambda" [n, K, 3]."""
    n, L, K = env.num_envs, env.sim.L, len(bodies)
    m = 3 * K
    nws = int(L.wbc_sim_constrained_dynamics_derivatives_workspace_floats(n, K))
    ws, nd, lam = _sentinel_buffer(nws), _sentinel_buffer(n * NCOL), _sentinel_buffer(n * m)
    rows = lambda k: NCOL if k.startswith("dnudot") else m
    bufs = {k: _sentinel_buffer(n * rows(k) * NCOL) for k in which}
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = L.wbc_sim_constrained_dynamics_derivatives(env.sim.h, (C.c_int32 * K)(*bodies), K, ptr(active), ptr(tau), ptr(a_des), damping, flags,
                                                    nd.data_ptr(), lam.data_ptr() if want_lambda else None,
                                                    *[ptr(bufs.get(k)) for k in OUTPUTS], ws.data_ptr(), None)
    assert rc == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    assert bool((nd[n * NCOL:] == SENTINEL).all()) and bool((ws[nws:] == SENTINEL).all())
    assert bool((lam[n * m:] == SENTINEL).all()) and (want_lambda or bool((lam == SENTINEL).all()))
    out = {"nudot": nd[:n * NCOL].view(n, NCOL).clone(), "lambda": lam[:n * m].view(n, K, 3).clone()}
    for k, b in bufs.items():
        assert bool((b[n * rows(k) * NCOL:] == SENTINEL).all()), k
        shape = (n, NCOL, rows(k)) if flags & TRANSPOSED else (n, rows(k), NCOL)
        out[k] = b[:n * rows(k) * NCOL].view(shape).clone()
    return out


CASES = ["feet", "feet_masked", "feet_gripper_ades_damping", "gripper", "armature", "tau_null"]
_WORST = {"dyn": 0.0, "con": 0.0, "cond": 0.0}


@functools.lru_cache(maxsize=None)
def _case(n, fast):
    """test_dynamics_derivatives._case(n, fast): an env whose robots hold members 0..n-1 of a state family of test_centroidal._state, the
    families C_D, C_J and C_R were measured on (every member has nu != 0); plus each env's downloaded fp32 state in fp64 and M_ref.
    Computed once and left unchanged."""
    env, _, _, _, (r64, d64, b64, _) = tdd._case(n, fast)
    states = [(r64[e, :3], r64[e, 3:7], d64[e, :, 0], np.r_[r64[e, 7:13], d64[e, :, 1]], b64[e]) for e in range(n)]
    M = [msr.mass_matrix(env.robot_model, st[0], st[1], st[2], st[4]) for st in states]
    return env, states, M


def _problem(n, case, fast=True):
    env = _case(n, fast)[0]
    feet, grip = tcd._bodies(env.robot_model)
    rng = np.random.default_rng(197)
    tau = torch.tensor(msr.force_rhs(rng, (n,)), dtype=torch.float32, device="cuda")
    p = dict(bodies=feet, active=None, tau=tau, a_des=None, damping=0.0, armature=False)
    if case == "feet_masked":
        p["active"] = tcd._masks(n, 4)
    elif case == "feet_gripper_ades_damping":
        p.update(bodies=feet + [grip], damping=1e-3, a_des=torch.tensor(rng.uniform(-5, 5, (n, 5, 3)), dtype=torch.float32, device="cuda"))
    elif case == "gripper":
        p["bodies"] = [grip]
    elif case == "armature":
        p["armature"] = True
    elif case == "tau_null":
        p["tau"] = None
    return env, p


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fast", [False, True], ids=["slow", "fast"])
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_row_and_column(n, fast, case):
    env, states, M0 = _case(n, fast)
    _, p = _problem(n, case, fast)
    bodies, active, damping = p["bodies"], p["active"], p["damping"]
    K, m = len(bodies), env.robot_model
    flags = ARMATURE if p["armature"] else 0
    got = _launch(env, bodies, active, p["tau"], p["a_des"], damping, flags)
    # the sibling's bits
    nd2, lam2 = env.sim.constrained_dynamics(bodies, tau=p["tau"], active=active, acc_des=p["a_des"], damping=damping, armature=p["armature"])
    assert torch.equal(got["nudot"], nd2) and torch.equal(got["lambda"], lam2)
    g = [float(x) for x in env.tcfg.gravity]
    A = msr.armature_vector(env.tcfg) if p["armature"] else None
    act = np.ones((n, K), dtype=bool) if active is None else active.cpu().numpy().astype(bool)
    out = {k: got[k].cpu().numpy().astype(np.float64) for k in OUTPUTS}
    assert all(np.isfinite(x).all() for x in out.values())
    assert all(np.all(st[3][3:6] != 0) and np.all(st[3][6:24] != 0) for st in states)   # nu is live
    _assert_exact_structure(out, np.repeat(act, 3, axis=1))
    nd64, lm64 = got["nudot"].cpu().numpy().astype(np.float64), got["lambda"].cpu().numpy().astype(np.float64).reshape(n, 3 * K)
    wd = wc = 0.0
    for e in range(n):
        on = np.repeat(act[e], 3)
        state = states[e]
        Me = M0[e] if A is None else M0[e] + np.diag(A)
        Jc = cdr.constraint_rows(m, state[0], state[1], state[2], state[3], bodies, act[e])[0]
        cond = cdr.delassus_condition(Me, Jc, damping, on)
        assert cond <= COND_MAX, (e, cond)
        _WORST["cond"] = max(_WORST["cond"], cond)
        parts = cdd.residual_partials(m, state, bodies, on, nd64[e], lm64[e], g)
        for grp in GROUPS:
            D, Lam = out[f"dnudot_d{grp}"][e], out[f"dlambda_d{grp}"][e]
            rd, ad, rc, ac = cdd.column_bounds(Me, Jc, damping, on, parts, grp, D, Lam)
            cols = slice(0, NCOL) if grp == "tau" else slice(3, NCOL)
            live = np.zeros((NCOL, NCOL), dtype=bool)
            live[np.ix_(LIVE, LIVE)] = True
            live[:, :cols.start] = False
            assert np.all(ad[live] > 0) and np.all(rd[~live] == 0)
            assert np.all(rd[live] <= ad[live]), ("dynamics", grp, e, float((rd[live] / ad[live]).max()))
            wd = max(wd, float((rd[live] / ad[live]).max()))
            if on.any():
                lc = np.zeros_like(ac, dtype=bool)
                lc[np.ix_(np.nonzero(on)[0], [c for c in LIVE if c >= cols.start])] = True
                assert np.all(ac[lc] > 0) and np.all(rc[~lc] == 0)
                assert np.all(rc[lc] <= ac[lc]), ("constraint", grp, e, float((rc[lc] / ac[lc]).max()))
                wc = max(wc, float((rc[lc] / ac[lc]).max()))
        if not on.any():
            assert all(np.all(out[f"dlambda_d{grp}"][e] == 0) for grp in GROUPS)
    _WORST["dyn"], _WORST["con"] = max(_WORST["dyn"], wd), max(_WORST["con"], wc)
    print(f"constrained derivatives n={n} {'fast' if fast else 'slow'} {case}: largest residual / allowance: dynamics rows {wd:.3g}, constraint rows {wc:.3g}; "
          f"running maxima {_WORST}")
    if case == "feet_masked":
        assert not act[0].any()                                                   # an env with no active body


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_layouts_subsets_and_python_entry_points(n):
    env, p = _problem(n, "feet_gripper_ades_damping")
    bodies = p["bodies"]
    active = tcd._masks(n, 5) if n > 1 else torch.ones(1, 5, dtype=torch.uint8, device="cuda")   # env 0 of the masks has no active body
    kw = dict(active=active, tau=p["tau"], a_des=p["a_des"], damping=1e-3)
    full = _launch(env, bodies, flags=ARMATURE, **kw)
    tr = _launch(env, bodies, flags=ARMATURE | TRANSPOSED, **kw)
    for k in ("nudot", "lambda"):
        assert torch.equal(tr[k], full[k])
    for k in OUTPUTS:
        assert bool(full[k].abs().sum() > 0) and torch.equal(tr[k], full[k].transpose(1, 2)), k
        for flags in (ARMATURE, ARMATURE | TRANSPOSED):
            one = _launch(env, bodies, flags=flags, which=(k,), want_lambda=False, **kw)
            assert torch.equal(one[k], (tr if flags & TRANSPOSED else full)[k]) and torch.equal(one["nudot"], full["nudot"]), (k, flags)
    # the Python entry points are the same call
    r = env.sim.constrained_dynamics_derivatives(bodies, tau=p["tau"], active=active.bool(), acc_des=p["a_des"], damping=1e-3, armature=True)
    assert all(torch.equal(r[k], full[k]) for k in OUTPUTS + ("nudot", "lambda"))
    own = torch.zeros_like(full["dlambda_dnu"].transpose(1, 2).contiguous())
    r = env.sim.constrained_dynamics_derivatives(bodies, tau=p["tau"], active=active, acc_des=p["a_des"], damping=1e-3, armature=True,
                                                 transposed=True, want=("dlambda_dnu",), out={"dlambda_dnu": own})
    assert r["dlambda_dnu"] is own and torch.equal(own, tr["dlambda_dnu"]) and set(r) == {"nudot", "lambda", "dlambda_dnu"}
    feet = bodies[:4]
    outs = env.stance_forward_dynamics_derivatives(p["tau"], stance=active[:, :4].bool())
    want = _launch(env, feet, active=active[:, :4].contiguous(), tau=p["tau"])
    assert len(outs) == 8 and all(torch.equal(a, want[k]) for a, k in zip(outs, ("nudot", "lambda") + OUTPUTS))
    # tau NULL is a zeros tensor; the fingers' entries of tau are ignored
    z0 = _launch(env, feet, tau=None)
    t2 = torch.zeros_like(p["tau"]); t2[:, FINGERS] = 7.0
    z1 = _launch(env, feet, tau=t2)
    assert all(torch.equal(z0[k], z1[k]) for k in z0)


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    feet, grip = tcd._bodies(robot["model"])
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(171), (n,)), dtype=torch.float32, device="cuda")
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        r = env.sim.constrained_dynamics_derivatives(feet + [grip], tau=tau, damping=1e-3, armature=True)
        torch.cuda.synchronize()
        outs.append([r[k].clone() for k in OUTPUTS + ("nudot", "lambda")])
    for x, y in zip(*outs):
        assert bool(x.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
def test_flow_against_the_central_difference_of_two_sibling_calls():
    """D_q nu + D_nu nudot + D_tau 0 against (cd(+s) - cd(-s)) / (2 s) of wbc_sim_constrained_dynamics along the flow, the states set
    through set_root_state / set_dof_state on a scratch env, s = 2^-9. The allowance is the fp32 difference's own noise, none of it
    taken from the kernel under test:
      T          the difference's truncation and the rounding of the perturbed states to fp32 are removed exactly: T = the fp64 difference of
                 the fp64 solves at the states the sim actually holds (downloaded) minus the fp64 analytic flow with the same weights,
                 subtracted from the kernel's difference;
      N / s      each differenced output carries the sibling's rounding; N = 16 x the error of its fp32 yardstick
                 (constrained_dynamics_reference.yardstick_f32 against the fp64 solve at the same state), per output block, two of
                 them over 2 s;
      rel (|D_q| |nu| + |D_nu| |nudot|)   the derivative's own rounding, rel = N / max |x| the yardstick's relative error: the
                 columns pass through the same two factorisations as the solution."""
    import test_inverse_dynamics as tid
    n, s = 13, 2.0 ** -9
    env = tid._env(n, seed=5, steps=0)
    m = env.robot_model
    feet, _ = tcd._bodies(m)
    on = np.ones(12, dtype=bool)
    g = [float(x) for x in env.tcfg.gravity]
    states = [tc._state(seed, False) for seed in range(n)]
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(173), (n,)), dtype=torch.float32, device="cuda")
    t64 = tau.double().cpu().numpy()
    t64[:, FINGERS] = 0.0
    env.sim.tensor("BODY_PARAMS").copy_(torch.tensor(np.array([st[4] for st in states]), dtype=torch.float32))
    b64 = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)

    def put(t, nd64):
        """Sets the states moved by t along the flow; returns the fp64 copy of what the sim then holds."""
        root, dof = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
        for e, (pos, quat, q, nu, _bp, _nd) in enumerate(states):
            nu_t = nu + t * nd64[e] if nd64 is not None else nu
            root[e, 0] = torch.tensor(np.concatenate([pos + t * nu[0:3], _rotated(quat, t * nu[3:6]), nu_t[0:6]]), dtype=torch.float32)
            dof[e] = torch.tensor(np.stack([q + t * nu[6:], nu_t[6:]], -1), dtype=torch.float32)
        env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
        torch.cuda.synchronize()
        r64 = env.sim.tensor("ROOT_STATES")[:, 0].cpu().numpy().astype(np.float64)
        d64 = env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64)
        return [(r64[e, :3], r64[e, 3:7], d64[e, :, 0], np.r_[r64[e, 7:13], d64[e, :, 1]], b64[e]) for e in range(n)]

    def solve64(st, e):
        M, h, Jc, gamma = cdd.system(m, st, feet, on, None, g)
        return np.concatenate(cdr.solve_with_mask(M, h, t64[e], Jc, gamma, np.zeros(12), 0.0, on))
    held0 = put(0.0, None)
    r = env.sim.constrained_dynamics_derivatives(feet, tau=tau)
    torch.cuda.synchronize()
    R = {k: v.double().cpu().numpy() for k, v in r.items()}
    nd64 = R["nudot"]
    side, held = [], []
    for sgn in (1.0, -1.0):
        held.append(put(sgn * s, nd64))
        a, b = env.sim.constrained_dynamics(feet, tau=tau)
        torch.cuda.synchronize()
        side.append(np.concatenate([a.double().cpu().numpy(), b.double().cpu().numpy().reshape(n, 12)], 1))
    fd = (side[0] - side[1]) / (2 * s)
    worst = 0.0
    for e in range(n):
        st = held0[e]
        nu = st[3].copy(); nu[FINGERS] = 0.0
        ref = cdd.constrained_dynamics_derivatives(m, st, feet, on, t64[e], np.zeros(12), 0.0, None, g)
        M, h, Jc, gamma = cdd.system(m, st, feet, on, None, g)
        y32 = np.concatenate(cdr.yardstick_f32(M, h, t64[e], Jc, gamma, np.zeros(12), 0.0, on))
        x64 = np.concatenate([ref["nudot"], ref["lambda"]])
        fd64 = (solve64(held[0][e], e) - solve64(held[1][e], e)) / (2 * s)
        for name, cols in (("dnudot", slice(0, NCOL)), ("dlambda", slice(NCOL, None))):
            Dq, Dn = ref[name]["q"], ref[name]["nu"]
            N = 16.0 * np.abs(y32 - x64)[cols].max()
            T = fd64[cols] - (Dq @ nu + Dn @ nd64[e])
            allow = N / s + N / np.abs(x64[cols]).max() * (np.abs(Dq) @ np.abs(nu) + np.abs(Dn) @ np.abs(nd64[e]))
            got = R[f"{name}_dq"][e] @ nu + R[f"{name}_dnu"][e] @ nd64[e]
            err = np.abs(fd[e, cols] - got - T)
            worst = max(worst, float((err / allow).max()))
            assert np.all(err <= allow), (name, e, float((err / allow).max()))
    print(f"flow vs the central difference of the sibling (n = 13, s = 2^-9): largest error / allowance = {worst:.3g}")


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env, p = _problem(n, "feet_gripper_ades_damping")
    active = tcd._masks(n, 5)
    kw = dict(tau=p["tau"], active=active, acc_des=p["a_des"], damping=1e-3, armature=True)
    want = env.sim.constrained_dynamics_derivatives(p["bodies"], **kw)
    outs = {k: torch.zeros_like(v) for k, v in want.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream (the workspace exists already)
        env.sim.constrained_dynamics_derivatives(p["bodies"], out=outs, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in outs.values():
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.constrained_dynamics_derivatives(p["bodies"], out=outs, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k], want[k]) for k in want)


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env = _case(n, True)[0]
    m = env.robot_model
    feet, grip = tcd._bodies(m)
    L, h = env.sim.L, env.sim.h
    K = 4
    nd, lam = _sentinel_buffer(n * NCOL), _sentinel_buffer(n * 15)
    ws = _sentinel_buffer(int(L.wbc_sim_constrained_dynamics_derivatives_workspace_floats(n, 5)))
    bufs = {k: _sentinel_buffer(n * MENV) for k in OUTPUTS}
    tau = torch.ones(n, NCOL, device="cuda")
    idx = (C.c_int32 * 5)(*(feet + [grip]))
    same_body = next(r for r in range(27) if r != feet[0] and m.rb_body[r] == m.rb_body[feet[0]])
    base = [("sim", h), ("rb", idx), ("k", K), ("active", None), ("tau", tau.data_ptr()), ("a_des", None), ("damping", 0.0), ("flags", 0),
            ("nudot", nd.data_ptr()), ("lam", lam.data_ptr())] + [(k, bufs[k].data_ptr()) for k in OUTPUTS] + [("ws", ws.data_ptr()), ("stream", None)]
    call = lambda **kw: L.wbc_sim_constrained_dynamics_derivatives(*[kw.get(k, d) for k, d in base])
    refusals = [
        (dict(sim=None), b"NULL"), (dict(rb=None), b"NULL"), (dict(nudot=None), b"NULL"), (dict(ws=None), b"NULL"),
        ({k: None for k in OUTPUTS}, b"NULL"),
        (dict(k=0), b"nbodies"), (dict(k=6), b"nbodies"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], 27, feet[3])), b"index"), (dict(rb=(C.c_int32 * 4)(feet[0], -1, feet[2], feet[3])), b"index"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], same_body, feet[3])), b"same moving body"),
        (dict(damping=-1e-3), b"damping"), (dict(damping=float("inf")), b"damping"), (dict(damping=float("nan")), b"damping"),
        (dict(flags=4), b"flag"), (dict(flags=ARMATURE | TRANSPOSED | 8), b"flag"),
        (dict(tau=tau.data_ptr() + 2), b"aligned"), (dict(a_des=tau.data_ptr() + 1), b"aligned"), (dict(nudot=nd.data_ptr() + 2), b"aligned"),
        (dict(lam=lam.data_ptr() + 3), b"aligned"), (dict(ws=ws.data_ptr() + 2), b"aligned"),
    ]
    refusals += [({k: bufs[k].data_ptr() + off}, b"aligned") for k in OUTPUTS for off in (1, 2, 3)]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for t in [nd, lam, ws] + list(bufs.values()):
        assert bool((t == SENTINEL).all())
    # 4-byte alignment is all that is needed: every output one float into its buffer
    want = _launch(env, feet, tau=tau)
    assert call(nudot=nd.data_ptr() + 4, lam=lam.data_ptr() + 4, ws=ws.data_ptr() + 4, **{k: bufs[k].data_ptr() + 4 for k in OUTPUTS}) == 0
    torch.cuda.synchronize()
    assert torch.equal(nd[1:1 + n * NCOL].view(n, NCOL), want["nudot"]) and float(nd[0]) == SENTINEL and float(ws[0]) == SENTINEL
    assert torch.equal(lam[1:1 + n * 12].view(n, 4, 3), want["lambda"]) and float(lam[0]) == SENTINEL
    for k in OUTPUTS:
        b, numel = bufs[k], want[k].numel()
        assert torch.equal(b[1:1 + numel].view(want[k].shape), want[k]) and float(b[0]) == SENTINEL and bool((b[1 + numel:] == SENTINEL).all()), k


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_call():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        feet, grip = tcd._bodies(env.robot_model)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        b = torch.ones(n, 26, device="cuda")
        for _ in range(5):
            if use:
                env.stance_forward_dynamics_derivatives(b, stance=env.get_foot_contacts())
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.sim.constrained_dynamics_derivatives(feet + [grip], armature=True, damping=1e-3, transposed=True)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
