"""Analytic derivatives of inverse and forward dynamics (wbc_sim_inverse_dynamics_derivatives, wbc_sim_forward_dynamics_derivatives,
wbc_dynamics_derivatives_kernel in csrc/wbc_arm_kernel.hip; definitions and the tangent convention in include/wbc_sim.h). The CPU tests pin
the fp64 reference of tests/dynamics_derivatives_reference.py to Richardson-extrapolated central differences of the inverse-dynamics
restatement, to the flow identity d tau / dt = D_q nu + D_nu nudot + M d(nudot)/dt and to the structure of the equations, and measure the
fp32 yardstick; the GPU tests hold the kernel to the reference entry by entry, the forward-dynamics derivatives in residual form
against M_ref, and both calls to their own invariances.

Bound: every entry satisfies |kernel - ref| <= C 2^-24 mag, mag = sum |J|^T |dF| + |J|^T |dT| + |dJ|^T |F| + |dJ|^T |T| of the reference.
K_ref is the fp32 yardstick's largest ratio over the two state families of tests/test_centroidal.py (_state), 64 states each, with nudot
given and NULL (asserted <= C / 16 on the CPU), C the smallest power of two >= 16 K_ref, and the last column the kernel's largest ratio on
an MI355X over n = 1, 13, 64, both families, nudot given and NULL:

    output       K_ref      C          kernel's largest ratio
    dtau_dq      1.32e3     32768      6.18e3  (n = 64, nudot given; 1.55e3 with nudot NULL)
    dtau_dnu     1.97e4     524288     7.25e3  (n = 64; 5.29e3 at n = 13)

The large figures are single entries: a root-force row against a wrist joint's column, where one component of a cross product such as
alpha x d(r_c) is the difference of two products a thousand times its size, so that mag (the size of the SUM's terms, 4e-7 N s for the
entry behind 1.97e4) says nothing of the operands' sizes; which entry is worst, and by how much, changes with every reordering of the
arithmetic. The kernel's text compiled for the host (one thread per lane, a barrier for __syncthreads(), a stand-alone program under
AddressSanitizer and UBSan: no out-of-bounds access at n = 1, 13, 64) had predicted, with fused multiply-adds as the GPU compiler
contracts them, 175 and 3.80e4 at n = 13 and 4.33e3 and 3.80e4 at n = 64 (1.55e3 for dtau_dq with nudot NULL, the GPU's figure to four
digits); without contraction 187 / 2.41e4 and 846 / 2.41e4. The forward-dynamics derivatives' largest residual over its allowance on an
MI355X: 0.0068 (dnudot_dq), 0.0059 (dnudot_dnu), 0.027 (minv), all at n = 64 or 13 with the armature.

A first version of the kernel carried spatial velocities and accelerations about the base origin, as wbc_inverse_dynamics_kernel does; its
dtau_dnu reached 9.3e5 on the GPU (1.39e5 in the host build) at the 4e-7 entry above and missed the bound: v x (S qd) terms the size of
|p| |omega| cancel there down to |r_c| |omega|. The kernel now walks angular velocity, angular acceleration and the CLASSICAL acceleration
of each body's own origin, so that every lever is a link or centre-of-mass offset.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dynamics_derivatives_reference as ddr
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import test_centroidal as tc
import arm_codegen
import whole_body_reference as wb

EPS, NCOL = ddr.EPS, ddr.NCOL
FINGERS, LIVE = ddr.FINGERS, ddr.LIVE
SENTINEL = 12345.0
MENV = NCOL * NCOL
TRANSPOSED, ARMATURE = 2, 1
# The mass solve's allowance, restated from tests/mass_solve_reference.py (where its derivation stands):
# |M_ref x - b|_k <= C_S 2^-24 (d_k sum_j d_j |x_j| + |b_k|), d = sqrt(diag M).
C_S = 128.0
assert C_S == msr.C_S

_model, _state, _rotated = tc._model, tc._state, tc._rotated


def _chain_root(m, b):
    while m.parent[b] > 0:
        b = m.parent[b]
    return b


@functools.lru_cache(maxsize=None)
def _cross_chain():
    """Boolean [26, 26]: joint row x joint column whose joints lie on different chains (different legs, or a leg and the arm)."""
    m = _model()
    body = wb.dof_body(m)
    mask = np.zeros((NCOL, NCOL), dtype=bool)
    for i in range(20):
        for j in range(20):
            if body[i] > 0 and body[j] > 0 and _chain_root(m, body[i]) != _chain_root(m, body[j]):
                mask[6 + i, 6 + j] = True
    assert mask.sum() == 18 * 18 - 4 * 9 - 36
    return mask


def _assert_exact_structure(Dq, Dnu):
    """The literal zeros of include/wbc_sim.h, as equalities; Dq, Dnu [..., 26, 26] indexed [i, j]."""
    assert np.all(Dq[..., :, 0:3] == 0) and np.all(Dnu[..., :, 0:3] == 0)
    for D in (Dq, Dnu):
        assert np.all(D[..., FINGERS, :] == 0) and np.all(D[..., :, FINGERS] == 0)
        assert np.all(D[..., _cross_chain()] == 0)


# ------------------------------------------------------------------------------------------------------------ CPU
def _tau(m, pos, quat, q, nu, nudot, bp, dq=None, dnu=None):
    """tau of the restatement at the configuration moved along the tangent dq (root translated, rotated by the world rotation vector,
    joints incremented) and at nu + dnu."""
    if dq is not None:
        pos, quat, q = pos + dq[0:3], _rotated(quat, dq[3:6]), q + dq[6:]
    return idr.inverse_dynamics(m, pos, quat, q, nu if dnu is None else nu + dnu, nudot, bp)[0]


def _richardson(f):
    """(4 D_1 - D_2) / 3 of the central differences with steps 1e-4 and 2e-4: f(step) -> f(+step) - f(-step) over 2 step."""
    return (4.0 * f(1e-4) - f(2e-4)) / 3.0


def test_reference_against_richardson_central_differences():
    m = _model()
    worst = 0.0
    for seed in range(20):
        pos, quat, q, nu, bp, nudot = _state(seed, fast=seed % 2 == 1)
        Dq, Dnu, _, _ = ddr.inverse_dynamics_derivatives(m, pos, quat, q, nu, nudot, bp)

        def diff(h):
            out = np.zeros((2, NCOL, NCOL))
            for k in range(NCOL):
                e = np.zeros(NCOL); e[k] = h
                out[0, :, k] = (_tau(m, pos, quat, q, nu, nudot, bp, dq=e) - _tau(m, pos, quat, q, nu, nudot, bp, dq=-e)) / (2 * h)
                out[1, :, k] = (_tau(m, pos, quat, q, nu, nudot, bp, dnu=e) - _tau(m, pos, quat, q, nu, nudot, bp, dnu=-e)) / (2 * h)
            return out
        want = _richardson(diff)
        for D, W in ((Dq, want[0]), (Dnu, want[1])):
            err = np.abs(D - W).max()
            worst = max(worst, err / max(1.0, np.abs(D).max()))
            assert err <= 1e-8 * max(1.0, np.abs(D).max()), (seed, err)
    print(f"reference vs Richardson differences: largest |diff| / max(1, max |D|) = {worst:.3g}")


def test_reference_flow_identity():
    """Along the motion config(t) = (p + t v, exp(t [omega]x) R, q + t qd), nu(t) = nu + t nudot, nudot(t) = nudot + t jerk:
    d tau / dt at 0 = D_q nu + D_nu nudot + M jerk. The left side by the Richardson difference of test 1, whose entries agree to
    1e-8 max(1, max |D|) there; this derivative is their combination with the weights nu, nudot and jerk, hence the allowance
    1e-8 max(1, max |D_q|, max |D_nu|, max |M|) (|nu|_1 + |nudot|_1 + |jerk|_1). It pins the tangent convention, rotation included."""
    m = _model()
    for seed in range(12):
        pos, quat, q, nu, bp, nudot = _state(seed, fast=seed % 2 == 1)
        nudot[FINGERS] = 0.0
        nu[FINGERS] = 0.0
        rng = np.random.default_rng(900 + seed)
        jerk = np.r_[rng.uniform(-100, 100, 6), rng.uniform(-500, 500, 20)]
        jerk[FINGERS] = 0.0
        Dq, Dnu, _, _ = ddr.inverse_dynamics_derivatives(m, pos, quat, q, nu, nudot, bp)
        M = wb.mass_matrix(m, pos, quat, q, bp)
        at = lambda t: _tau(m, pos, quat, q, nu + t * nudot, nudot + t * jerk, bp, dq=t * nu)
        got = _richardson(lambda h: (at(h) - at(-h)) / (2 * h))
        want = Dq @ nu + Dnu @ nudot + M @ jerk
        allow = 1e-8 * max(1.0, np.abs(Dq).max(), np.abs(Dnu).max(), np.abs(M).max()) * (np.abs(nu).sum() + np.abs(nudot).sum() + np.abs(jerk).sum())
        assert np.abs(got - want).max() <= allow, (seed, np.abs(got - want).max(), allow)


def test_reference_structure():
    """The gravity-only derivative's joint block is symmetric (the Hessian of potential_energy, checked against its second difference
    on a few entries); tau(nudot + e_k) - tau(nudot) is column k of M; the exact zeros, in value and in magnitude."""
    m = _model()
    for seed in range(8):
        pos, quat, q, nu, bp, nudot = _state(seed, fast=seed % 2 == 1)
        G, Gnu, _, _ = ddr.inverse_dynamics_derivatives(m, pos, quat, q, np.zeros(NCOL), None, bp)
        J = G[6:, 6:]
        assert np.abs(J - J.T).max() <= 1e-12 * np.abs(J).max() and np.abs(J).max() > 1
        assert np.all(Gnu == 0)                                  # every velocity term is at least bilinear in nu
        h = 1e-4
        for i, j in ((0, 1), (13, 14), (4, 4)):
            ei, ej = np.eye(20)[i] * h, np.eye(20)[j] * h
            U = lambda d: idr.potential_energy(m, pos, quat, q + d, bp)
            second = (U(ei + ej) - U(ei - ej) - U(ej - ei) + U(-ei - ej)) / (4 * h * h)
            assert abs(second - J[i, j]) <= 1e-5 * np.abs(J).max(), (seed, i, j)
        M = wb.mass_matrix(m, pos, quat, q, bp)
        tau, mag = idr.inverse_dynamics(m, pos, quat, q, nu, nudot, bp)
        for k in (0, 4, 7, 20, 23):
            col = idr.inverse_dynamics(m, pos, quat, q, nu, nudot + np.eye(NCOL)[k], bp)[0] - tau
            assert np.abs(col - M[:, k]).max() <= 1e-12 * mag.max(), (seed, k)
        Dq, Dnu, mq, mn = ddr.inverse_dynamics_derivatives(m, pos, quat, q, nu, nudot, bp)
        _assert_exact_structure(Dq, Dnu)
        _assert_exact_structure(mq, mn)
        live = ~_cross_chain()
        live[FINGERS, :] = False; live[:, FINGERS] = False; live[:, 0:3] = False
        assert np.all(mq[live] > 0)                               # every other entry is exercised


def test_reference_forward_dynamics_derivatives_against_central_differences(robot):
    """-M^-1 D and M^-1 against Richardson differences of the fp64 nudot = (M + A)^-1 (tau - h), with and without the armature. The
    differenced solve loses cond(M) 2^-52 |nudot| / step to rounding on top of test 1's 1e-8 (cond M reaches 3e5,
    mass_solve_reference.py): allowance 1e-8 max(1, max |X|) + 8 cond 2^-52 max |nudot| / 1e-4 per output."""
    m = robot["model"]
    A = msr.armature_vector(robot["tcfg"])
    for seed in range(4):
        pos, quat, q, nu, bp, _ = _state(seed, fast=seed % 2 == 1)
        tau = msr.force_rhs(np.random.default_rng(950 + seed), ())
        arm = A if seed % 2 == 0 else None
        nd, Xq, Xn, Minv, M, _ = ddr.forward_dynamics_derivatives(m, pos, quat, q, nu, tau, bp, armature=arm)
        assert np.all(Xq[:, 0:3] == 0) and np.all(Xn[:, 0:3] == 0)
        for X in (Xq, Xn, Minv):
            assert np.all(X[FINGERS, :] == 0) and np.all(X[:, FINGERS] == 0)
        fd = lambda dq=None, dnu=None, dtau=None: msr.forward_dynamics(
            m, *((pos, quat, q) if dq is None else (pos + dq[0:3], _rotated(quat, dq[3:6]), q + dq[6:])), nu if dnu is None else nu + dnu,
            tau if dtau is None else tau + dtau, bp, armature=arm)[0]

        def diff(h):
            out = np.zeros((3, NCOL, NCOL))
            for k in range(NCOL):
                e = np.zeros(NCOL); e[k] = h
                out[0, :, k] = (fd(dq=e) - fd(dq=-e)) / (2 * h)
                out[1, :, k] = (fd(dnu=e) - fd(dnu=-e)) / (2 * h)
                out[2, :, k] = (fd(dtau=e) - fd(dtau=-e)) / (2 * h)
            return out
        want = _richardson(diff)
        want[2][:, FINGERS] = 0.0                                 # the fingers' entries of tau are ignored: no column
        noise = 8 * np.linalg.cond(M[np.ix_(LIVE, LIVE)]) * 2.0 ** -52 * np.abs(nd).max() / 1e-4
        for X, W in zip((Xq, Xn, Minv), want):
            err = np.abs(X - W).max()
            assert err <= 1e-8 * max(1.0, np.abs(X).max()) + noise, (seed, err, np.abs(X).max(), noise)


@functools.lru_cache(maxsize=None)
def _reference(seed, fast):
    """(reference with nudot, reference without) of one family member in fp64; computed once and left unchanged."""
    pos, quat, q, nu, bp, nudot = _state(seed, fast)
    return (ddr.inverse_dynamics_derivatives(_model(), pos, quat, q, nu, nudot, bp),
            ddr.inverse_dynamics_derivatives(_model(), pos, quat, q, nu, None, bp))


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output: the fp32 yardstick's largest ratio over 64 members of each state family, nudot given and NULL."""
    m = _model()
    k = {"dq": 0.0, "dnu": 0.0}
    for fast in (False, True):
        for seed in range(64):
            pos, quat, q, nu, bp, nudot = _state(seed, fast)
            for nd, ref in zip((nudot, None), _reference(seed, fast)):
                y = ddr.inverse_dynamics_derivatives(m, pos, quat, q, nu, nd, bp, dtype=np.float32)
                k["dq"] = max(k["dq"], ddr.largest_ratio(y[0], ref[0], ref[2]))
                k["dnu"] = max(k["dnu"], ddr.largest_ratio(y[1], ref[1], ref[3]))
    return k


def test_fp32_yardsticks_sit_well_inside_the_bounds():
    k = _yardsticks()
    print("dynamics derivatives yardsticks: " + ", ".join(f"{f} K_ref = {k[f]:.4g} (C = {ddr.C[f]:g})" for f in k))
    for f in k:
        assert k[f] <= ddr.C[f] / 16, (f, k[f])
        assert ddr.C[f] == 2.0 ** np.ceil(np.log2(16 * k[f])), (f, k[f])


def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.wbc_sim_inverse_dynamics_derivatives(None, None, p, p, 0, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_inverse_dynamics_derivatives(None, None, None, None, 0, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_forward_dynamics_derivatives(None, None, p, p, p, p, 0, p, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_forward_dynamics_derivatives(None, None, p, None, None, None, 0, p, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_forward_dynamics_derivatives_workspace_floats(0) == 0 and L.wbc_sim_forward_dynamics_derivatives_workspace_floats(-3) == 0
    assert L.wbc_sim_forward_dynamics_derivatives_workspace_floats(13) == 13 * MENV * 5 + MENV


def test_dynamics_derivatives_kernel_codegen():
    """The code object's metadata alone: no scratch, the launch's workgroup size, static LDS within 20 KB (8 workgroups per CU)."""
    assert arm_codegen.meta("wbc_dynamics_derivatives_kernel", "private_segment_fixed_size") == 0
    assert arm_codegen.meta("wbc_dynamics_derivatives_kernel", "max_flat_workgroup_size") == 64
    assert arm_codegen.meta("wbc_dynamics_derivatives_kernel", "group_segment_fixed_size") <= 20480


# ------------------------------------------------------------------------------------------------------------ GPU
def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(n, fast):
    """An env whose n robots hold members 0..n-1 of a family (state, body params), the nudot tensor, the downloaded fp32 state in fp64
    and the fp64 reference of every env at that state, with nudot and without. Computed once and left unchanged."""
    import test_inverse_dynamics as tid
    env = tid._env(n, seed=5, steps=0)
    states = [_state(seed, fast) for seed in range(n)]
    root, dof = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    for e, (pos, quat, q, nu, _bp, _nd) in enumerate(states):
        root[e, 0] = torch.tensor(np.concatenate([pos, quat, nu[0:6]]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q, nu[6:]], -1), dtype=torch.float32)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    env.sim.tensor("BODY_PARAMS").copy_(torch.tensor(np.array([s[4] for s in states]), dtype=torch.float32))
    nudot = torch.tensor(np.array([s[5] for s in states]), dtype=torch.float32, device="cuda").contiguous()
    torch.cuda.synchronize()
    r64 = env.sim.tensor("ROOT_STATES")[:, 0].cpu().numpy().astype(np.float64)
    d64 = env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64)
    b64 = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    n64 = nudot.cpu().numpy().astype(np.float64)
    refs = [[_ref_at(env, (r64, d64, b64), e, nd) for e in range(n)] for nd in (n64, None)]
    return env, nudot, refs[0], refs[1], (r64, d64, b64, n64)


def _ref_at(env, state, e, nudot):
    r64, d64, b64 = state
    g = [float(x) for x in env.tcfg.gravity]
    return ddr.inverse_dynamics_derivatives(env.robot_model, r64[e, :3], r64[e, 3:7], d64[e, :, 0], np.r_[r64[e, 7:13], d64[e, :, 1]],
                                            None if nudot is None else nudot[e], b64[e], g)


def _launch(env, nudot, which=("dq", "dnu"), flags=0):
    """A direct C-ABI call into sentinel-framed buffers; returns {name: [n, 26, 26] tensor} of the outputs asked for."""
    n = env.num_envs
    bufs = {k: _sentinel_buffer(n * MENV) for k in which}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None
    rc = env.sim.L.wbc_sim_inverse_dynamics_derivatives(env.sim.h, nudot.data_ptr() if nudot is not None else None, ptr("dq"), ptr("dnu"),
                                                        flags, None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[n * MENV:] == SENTINEL).all()), k
    return {k: b[:n * MENV].view(n, NCOL, NCOL).clone() for k, b in bufs.items()}


def _ratios(got, refs):
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    return {"dq": max(ddr.largest_ratio(g["dq"][e], r[0], r[2]) for e, r in enumerate(refs)),
            "dnu": max(ddr.largest_ratio(g["dnu"][e], r[1], r[3]) for e, r in enumerate(refs))}


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["slow", "fast"])
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_and_entry_of_both_outputs(n, fast):
    env, nudot, with_nd, without, _ = _case(n, fast)
    got, got0 = _launch(env, nudot), _launch(env, None)
    for tag, g, refs in (("nudot", got, with_nd), ("NULL", got0, without)):
        worst = _ratios(g, refs)
        print(f"dynamics derivatives n={n} {'fast' if fast else 'slow'} {tag}: largest |kernel - ref| / (2^-24 mag): {worst}")
        for f, w in worst.items():
            assert w <= ddr.C[f], (tag, f, w)
        # the literal zeros, as equalities
        _assert_exact_structure(g["dq"].cpu().numpy(), g["dnu"].cpu().numpy())
        assert bool(g["dq"].abs().sum() > 0) and bool(g["dnu"].abs().sum() > 0)
    # single-output calls give the bits of the two-output call; the transposed layout is the exact transpose
    for nd, full in ((nudot, got), (None, got0)):
        for k in ("dq", "dnu"):
            assert torch.equal(_launch(env, nd, which=(k,))[k], full[k]), k
            assert torch.equal(_launch(env, nd, which=(k,), flags=TRANSPOSED)[k], full[k].transpose(1, 2)), k
        both = _launch(env, nd, flags=TRANSPOSED)
        assert torch.equal(both["dq"], full["dq"].transpose(1, 2)) and torch.equal(both["dnu"], full["dnu"].transpose(1, 2))
    # nudot NULL is a zeros tensor; the fingers' entries of nudot are ignored
    zeros = _launch(env, torch.zeros_like(nudot))
    assert torch.equal(zeros["dq"], got0["dq"]) and torch.equal(zeros["dnu"], got0["dnu"])
    nd2 = nudot.clone(); nd2[:, FINGERS] = 7.0
    again = _launch(env, nd2)
    assert torch.equal(again["dq"], got["dq"]) and torch.equal(again["dnu"], got["dnu"])
    # the Python entry points are the same call
    dq, dnu = env.sim.inverse_dynamics_derivatives(nudot)
    assert dq.shape == (n, NCOL, NCOL) and torch.equal(dq, got["dq"]) and torch.equal(dnu, got["dnu"])
    dqt, dnut = env.sim.inverse_dynamics_derivatives(nudot, transposed=True)
    assert torch.equal(dqt, dq.transpose(1, 2)) and torch.equal(dnut, dnu.transpose(1, 2))
    own = torch.zeros_like(dq)
    assert env.sim.inverse_dynamics_derivatives(None, dq=own)[0] is own and torch.equal(own, got0["dq"])
    e0, e1 = env.inverse_dynamics_derivatives()
    assert torch.equal(e0, got0["dq"]) and torch.equal(e1, got0["dnu"])
    e0, e1 = env.inverse_dynamics_derivatives(nudot)
    assert torch.equal(e0, got["dq"]) and torch.equal(e1, got["dnu"])


def _fdd_launch(env, tau, which=("dq", "dnu", "minv"), flags=0):
    """A direct C-ABI call of the forward-dynamics derivatives into sentinel-framed buffers with a workspace of exactly the size asked for."""
    n, L = env.num_envs, env.sim.L
    ws = _sentinel_buffer(int(L.wbc_sim_forward_dynamics_derivatives_workspace_floats(n)))
    nd = _sentinel_buffer(n * NCOL)
    bufs = {k: _sentinel_buffer(n * MENV) for k in which}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None
    rc = L.wbc_sim_forward_dynamics_derivatives(env.sim.h, tau.data_ptr() if tau is not None else None, nd.data_ptr(), ptr("dq"), ptr("dnu"),
                                                ptr("minv"), flags, ws.data_ptr(), None)
    assert rc == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    assert bool((nd[n * NCOL:] == SENTINEL).all()) and bool((ws[-8:] == SENTINEL).all())
    for k, b in bufs.items():
        assert bool((b[n * MENV:] == SENTINEL).all()), k
    out = {k: b[:n * MENV].view(n, NCOL, NCOL).clone() for k, b in bufs.items()}
    out["nudot"] = nd[:n * NCOL].view(n, NCOL).clone()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("armature", [False, True])
@pytest.mark.parametrize("n", [1, 13, 64])
def test_forward_dynamics_derivatives_in_residual_form(n, armature):
    """Every column of M_ref X_kernel + D_ref(nudot_kernel) within the solve's allowance for that right-hand side plus C 2^-24 mag;
    M_ref minv against the identity likewise; nudot is forward_dynamics(tau) bit for bit."""
    env, _, _, _, state = _case(n, True)
    r64, d64, b64, _ = state
    m = env.robot_model
    flags = ARMATURE if armature else 0
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(61 + n), (n,)), dtype=torch.float32, device="cuda").contiguous()
    got = _fdd_launch(env, tau, flags=flags)
    assert torch.equal(got["nudot"], env.forward_dynamics(tau, armature=armature))
    A = msr.armature_vector(env.tcfg) if armature else None
    nd64 = got["nudot"].cpu().numpy().astype(np.float64)
    X = {k: got[k].cpu().numpy().astype(np.float64) for k in ("dq", "dnu", "minv")}
    assert all(np.isfinite(x).all() for x in X.values())
    assert np.all(X["dq"][:, :, 0:3] == 0) and np.all(X["dnu"][:, :, 0:3] == 0)
    for x in X.values():
        assert np.all(x[:, FINGERS, :] == 0) and np.all(x[:, :, FINGERS] == 0)
    worst = {"dq": 0.0, "dnu": 0.0, "minv": 0.0}
    for e in range(n):
        M = msr.mass_matrix(m, r64[e, :3], r64[e, 3:7], d64[e, :, 0], b64[e], A)
        Dq, Dnu, mq, mn = _ref_at(env, (r64, d64, b64), e, nd64)
        eye = np.eye(NCOL); eye[FINGERS, FINGERS] = 0.0
        for k, D, mag in (("dq", Dq, mq), ("dnu", Dnu, mn), ("minv", -eye, np.zeros((NCOL, NCOL)))):
            x, b = X[k][e].T, -D.T                                  # row j: direction j's solution and right-hand side
            res = msr.residual(M, x, b)
            allow = C_S * EPS * msr.row_scale(M, x, b) + ddr.C["dnu" if k == "dnu" else "dq"] * EPS * mag.T
            ok = res <= allow
            assert np.all(ok), (k, e, np.argwhere(~ok)[:4].tolist(), float((res[~ok] / allow[~ok]).max()))
            live = allow > 0
            worst[k] = max(worst[k], float((res[live] / allow[live]).max()))
    print(f"forward-dynamics derivatives n={n} armature={armature}: largest residual / allowance: {worst}")
    # the layouts and the partial calls are the same numbers
    tr = _fdd_launch(env, tau, flags=flags | TRANSPOSED)
    assert torch.equal(tr["nudot"], got["nudot"])
    for k in ("dq", "dnu", "minv"):
        assert torch.equal(tr[k], got[k].transpose(1, 2)), k
        one = _fdd_launch(env, tau, which=(k,), flags=flags)
        assert torch.equal(one[k], got[k]) and torch.equal(one["nudot"], got["nudot"]), k
    # tau NULL is a zeros tensor; the Python entry points are the same call
    z0, z1 = _fdd_launch(env, None, flags=flags), _fdd_launch(env, torch.zeros_like(tau), flags=flags)
    assert all(torch.equal(z0[k], z1[k]) for k in z0)
    outs = env.forward_dynamics_derivatives(tau, armature=armature)
    assert all(torch.equal(a, got[k]) for a, k in zip(outs, ("nudot", "dq", "dnu", "minv")))
    outs = env.sim.forward_dynamics_derivatives(tau, armature=armature, transposed=True)
    assert all(torch.equal(a, tr[k]) for a, k in zip(outs, ("nudot", "dq", "dnu", "minv")))


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    nudot = tid._random_nudot(n, 89)
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(71), (n,)), dtype=torch.float32, device="cuda")
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        outs.append([t.clone() for t in env.sim.inverse_dynamics_derivatives(nudot) + env.sim.forward_dynamics_derivatives(tau, armature=True)])
        torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert bool(x.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env, nudot, _, _, _ = _case(n, True)
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(77), (n,)), dtype=torch.float32, device="cuda").contiguous()
    want = env.sim.inverse_dynamics_derivatives(nudot)
    want_fd = env.sim.forward_dynamics_derivatives(tau)
    outs = [torch.zeros_like(t) for t in want]
    outs_fd = [torch.zeros_like(t) for t in want_fd]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream
        env.sim.inverse_dynamics_derivatives(nudot, *outs)
        env.sim.forward_dynamics_derivatives(tau, *outs_fd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in outs + outs_fd:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.inverse_dynamics_derivatives(nudot, *outs)
        env.sim.forward_dynamics_derivatives(tau, *outs_fd)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want)) and all(torch.equal(a, b) for a, b in zip(outs_fd, want_fd))


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env, nudot, _, _, _ = _case(n, False)
    L, h = env.sim.L, env.sim.h
    bufs = {k: _sentinel_buffer(n * MENV) for k in ("dq", "dnu", "minv")}
    nd_out = _sentinel_buffer(n * NCOL)
    ws = _sentinel_buffer(int(L.wbc_sim_forward_dynamics_derivatives_workspace_floats(n)))
    # wbc_sim_inverse_dynamics_derivatives
    id_names = ("sim", "nudot", "dq", "dnu", "flags", "stream")
    base = dict(sim=h, nudot=nudot.data_ptr(), dq=bufs["dq"].data_ptr(), dnu=bufs["dnu"].data_ptr(), flags=0, stream=None)
    call = lambda **kw: L.wbc_sim_inverse_dynamics_derivatives(*[kw.get(k, base[k]) for k in id_names])
    refusals = [(dict(sim=None), b"NULL"), (dict(dq=None, dnu=None), b"NULL"), (dict(flags=ARMATURE), b"flag"), (dict(flags=4), b"flag"),
                (dict(flags=TRANSPOSED | 8), b"flag")]
    refusals += [({k: base[k] + off}, b"aligned") for k in ("nudot", "dq", "dnu") for off in (1, 2, 3)]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    # wbc_sim_forward_dynamics_derivatives
    fd_names = ("sim", "tau", "nudot", "dq", "dnu", "minv", "flags", "ws", "stream")
    fd_base = dict(sim=h, tau=nudot.data_ptr(), nudot=nd_out.data_ptr(), dq=bufs["dq"].data_ptr(), dnu=bufs["dnu"].data_ptr(),
                   minv=bufs["minv"].data_ptr(), flags=0, ws=ws.data_ptr(), stream=None)
    call_fd = lambda **kw: L.wbc_sim_forward_dynamics_derivatives(*[kw.get(k, fd_base[k]) for k in fd_names])
    refusals = [(dict(sim=None), b"NULL"), (dict(nudot=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(dq=None, dnu=None, minv=None), b"NULL"),
                (dict(flags=4), b"flag"), (dict(flags=ARMATURE | TRANSPOSED | 16), b"flag")]
    refusals += [({k: fd_base[k] + off}, b"aligned") for k in ("tau", "nudot", "dq", "dnu", "minv", "ws") for off in (1, 2, 3)]
    for kw, word in refusals:
        assert call_fd(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for b in list(bufs.values()) + [nd_out, ws]:
        assert bool((b == SENTINEL).all())
    # 4-byte alignment is all that is needed: every output one float into its buffer
    want = _launch(env, nudot)
    assert call(dq=bufs["dq"].data_ptr() + 4, dnu=bufs["dnu"].data_ptr() + 4) == 0
    torch.cuda.synchronize()
    for k in ("dq", "dnu"):
        b = bufs[k]
        assert torch.equal(b[1:1 + n * MENV].view(n, NCOL, NCOL), want[k]) and float(b[0]) == SENTINEL and bool((b[1 + n * MENV:] == SENTINEL).all()), k


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_calls():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        b = torch.ones(n, 26, device="cuda")
        for _ in range(5):
            if use:
                env.inverse_dynamics_derivatives(b); env.forward_dynamics_derivatives(b, armature=True)
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.inverse_dynamics_derivatives(); env.sim.forward_dynamics_derivatives(transposed=True)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
