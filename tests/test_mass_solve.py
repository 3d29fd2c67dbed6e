"""Mass-matrix solves out = M^-1 rhs and forward dynamics nudot = M^-1 (tau - h) (wbc_sim_mass_solve, wbc_sim_forward_dynamics,
csrc/wbc_arm_kernel.hip; definitions in include/wbc_sim.h). The CPU tests pin the fp64 references of tests/mass_solve_reference.py
to themselves, to the inverse-dynamics restatement and to the C oracle's articulated-body algorithm, and measure the fp32 yardstick;
the GPU tests hold the kernel to M_ref row by row, to the mass-matrix kernel, to the oracle and to its own invariances.

The bound is derived, not measured (mass_solve_reference.py): |M_ref x - b|_k <= C_S 2^-24 (d_k sum_j d_j |x_j| + |b_k|), d = sqrt(diag M),
C_S = 128. K_ref is the largest ratio of the fp32 row-order L D L^T yardstick against that scale on the tests' right-hand-side families
(asserted <= C_S / 4 on the CPU); the kernel's largest ratios on an MI355X stand next to it:

    family                                                              K_ref    C_S    kernel's largest ratio
    solve, rigid      (n = 1, 13, 64, 1000; nrhs 1, 7, 32)               3.24     128    6.14  (n = 1000, nrhs = 7)
    solve, armature   (the same cases)                                   2.00     128    3.74  (n = 1000, nrhs = 7)
    forward dynamics  (n = 1, 13, 1000; C_ID 2^-24 mag of its h on top)  --       128    2.80  (n = 1000, rigid; 0.77 with armature)

Further figures of that run, each as a fraction of its own bound: inverse operational-space inertia 0.036 (gripper) and 0.024 (foot),
round trip ID(FD(tau)) 0.042, against the oracle's ABA 0.0043 (armature) and 0.0085 (rigid), against the mass-matrix kernel 0.13.
"""
import copy
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import arm_codegen
import whole_body_reference as wb
from wbc_amd import abi

FINGERS, LIVE, EPS, C_S = msr.FINGERS, msr.LIVE, msr.EPS, msr.C_S
# The allowances of the two sibling kernels, restated from tests/test_inverse_dynamics.py (where their derivation stands):
# |h_kernel - h_ref|_k <= C_ID 2^-24 mag_k, and the mass-matrix kernel's share C_MM 2^-24 (|mm| |x|)_k of a product mm @ x.
C_ID = 4096.0
C_MM = 512.0


def _random_state(rng):
    quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
    pos = rng.normal(size=3)
    q = rng.uniform(-1, 1, 20); q[18:] = rng.uniform(-0.03, 0.03, 2)
    nu = np.r_[rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3), rng.uniform(-3, 3, 20)]
    return pos, quat, q, nu


def _random_body_params(m, rng):
    return abi.body_params_from_randomisation(m, rng.uniform(-0.5, 2.5, 1), rng.uniform(-0.1, 0.1, (1, 3)),
                                              rng.uniform(0, 0.1, 1)).astype(np.float64)[0]


def _gripper_and_foot(model):
    """Rigid-body indices of the gripper (the end-effector link) and of the first foot."""
    return model.rb_names.index("wx250s/ee_gripper_link"), next(i for i, name in enumerate(model.rb_names) if "foot" in name)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    assert L.wbc_sim_mass_solve(None, C.addressof(buf), 26, 1, C.addressof(buf) + 128, 0, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_forward_dynamics(None, None, C.addressof(buf), 0, None) == -1
    assert b"NULL" in L.wbc_last_error()


def test_mass_solve_kernel_codegen():
    """No scratch, no flat memory instructions, the launch's workgroup size, static LDS small enough for 16 workgroups per CU."""
    assert arm_codegen.meta("wbc_mass_solve_kernel", "private_segment_fixed_size") == 0
    assert arm_codegen.meta("wbc_mass_solve_kernel", "max_flat_workgroup_size") == 64
    assert arm_codegen.meta("wbc_mass_solve_kernel", "group_segment_fixed_size") <= 160 * 1024 // 16
    body = arm_codegen.body("wbc_mass_solve_kernel")
    assert "s_endpgm" in body
    assert not re.search(r"\bflat_", body) and "scratch_" not in body


def test_reference_solve_and_round_trip(robot):
    """M_ref x = b in fp64: residual <= 1e-12 relative; forward(inverse(nudot)) == nudot, with and without the armature."""
    m = robot["model"]
    A = msr.armature_vector(robot["tcfg"])
    assert A[6:24].min() > 0 and np.all(A[:6] == 0) and np.all(A[FINGERS] == 0)
    for seed in range(20):
        rng = np.random.default_rng(seed)
        pos, quat, q, nu = _random_state(rng)
        bp = _random_body_params(m, rng)
        for arm in (None, A):
            M = msr.mass_matrix(m, pos, quat, q, bp, arm)
            b = msr.force_rhs(rng, (5,))
            x = msr.solve(M, b)
            assert np.all(x[:, FINGERS] == 0)
            assert msr.residual(M, x, b).max() <= 1e-12 * np.abs(b).max()
            nudot = np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]
            nudot[FINGERS] = 0.0
            tau, _ = idr.inverse_dynamics(m, pos, quat, q, nu, nudot, bp)
            if arm is not None:
                tau = tau + arm * nudot
            back, _, _, _ = msr.forward_dynamics(m, pos, quat, q, nu, tau, bp, armature=arm)
            assert np.abs(back - nudot).max() <= 1e-9 * np.abs(nudot).max(), seed


@functools.lru_cache(maxsize=None)
def _yardstick(armature):
    """K_ref: the fp32 row-order L D L^T's largest ratio against the row scale, on the right-hand-side families of the GPU tests
    (random generalised forces; the Jacobian rows of the gripper body and of a foot plus one force). A bound check, not a
    statistic: 20 random states x 13 right-hand sides (the figure 3.3 quoted with the bound's derivation came from 60 states), and
    the Jacobian rows are the fp64 reference's rounded to fp32, not the kernel's own, so the last digits of K_ref in the module
    docstring's table are those of this sample."""
    from wbc_amd.config import WidowGo1RoughCfg
    m = abi.load_default_model()
    A = msr.armature_vector(abi.fill_task_cfg(WidowGo1RoughCfg(), m)) if armature else None
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(100 + seed)
        pos, quat, q, _nu = _random_state(rng)
        M = msr.mass_matrix(m, pos, quat, q, _random_body_params(m, rng), A)
        b = np.concatenate([msr.force_rhs(rng, (1,))] + [msr.jacobian_rows(m, pos, quat, q, r) for r in _gripper_and_foot(m)])
        b = b.astype(np.float32).astype(np.float64)
        worst = max(worst, msr.largest_ratio(M, msr.ldlt_solve_f32(M, b), b))
    return worst


@pytest.mark.parametrize("armature", [False, True])
def test_fp32_yardstick_sits_well_inside_the_bound(armature):
    k_ref = _yardstick(armature)
    print(f"mass solve yardstick (armature={armature}): K_ref = {k_ref:.3g}, C_S = {C_S}")
    assert k_ref <= C_S / 4


def _oracle(robot, armature):
    from oracle import OracleSim
    tc = copy.copy(robot["tcfg"])
    if not armature:
        for j in range(18):
            tc.joint_armature[j] = 0.0
    return OracleSim(robot["wmodel"], tc, 1)


@pytest.mark.parametrize("armature", [True, False])
def test_reference_agrees_with_the_oracle_forward_dynamics(robot, armature):
    """(M_ref + A)^-1 (tau - h_ref) against the C oracle's articulated-body algorithm on the 40 airborne states of
    tests/test_inverse_dynamics.py, in torque space, to that test's allowance 1e-4 max(1, |tau|) (the oracle reads fp32 model tables);
    with the oracle's armature zeroed it is the rigid solve."""
    import test_inverse_dynamics as tid
    model = robot["model"]
    o = _oracle(robot, armature)
    A = msr.armature_vector(robot["tcfg"]) if armature else None
    worst = 0.0
    for seed in range(40):
        pos, quat, q, qd, v, w, tau = tid._airborne_state(model, seed)
        a0, qdd = tid._oracle_accelerations(o, np.concatenate([pos, quat, v, w]), q, qd, tau)
        ref, M, _, _ = msr.forward_dynamics(model, pos, quat, q, np.r_[v, w, qd], np.r_[np.zeros(6), tau], o.get("BODY_PARAMS")[0], armature=A)
        err = np.abs(M @ (ref - np.r_[a0, qdd]))[LIVE].max()
        worst = max(worst, err)
        assert err < 1e-4 * max(1.0, np.abs(tau).max()), (seed, err)
    print(f"reference vs oracle ABA (armature={armature}): worst torque-space difference {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(n):
    """(env, M_ref [n, 26, 26], h_ref [n, 26], mag [n, 26], state) of the env the residual tests share; computed once."""
    import test_inverse_dynamics as tid
    env = tid._env(n, gravity=(0.7, -1.3, -9.5) if n == 64 else None) if n > 1 else tid._env(1, seed=9, steps=5)
    torch.cuda.synchronize()
    m = env.robot_model
    root = env.root_states.cpu().numpy().astype(np.float64)
    q, qd = env.dof_pos.cpu().numpy().astype(np.float64), env.dof_vel.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    g = [float(x) for x in env.tcfg.gravity]
    M = np.array([wb.mass_matrix(m, root[e, :3], root[e, 3:7], q[e], bp[e]) for e in range(n)])
    hm = [idr.bias_forces(m, root[e, :3], root[e, 3:7], q[e], np.r_[root[e, 7:13], qd[e]], bp[e], g) for e in range(n)]
    return env, M, np.array([h for h, _ in hm]), np.array([mg for _, mg in hm]), (root, q, qd, bp)


def _row_check(M, x, b, extra=None):
    """Asserts the row bound for every env, right-hand side and row; returns the largest ratio against the row scale alone.
    M [n, 26, 26], x, b [n, K, 26], extra [n, K, 26] or None: an allowance on top of C_S 2^-24 scale."""
    assert np.isfinite(x).all()
    assert np.all(x[..., FINGERS] == 0)
    res = np.abs(np.einsum("nij,nkj->nki", M, x) - b)
    d = np.sqrt(np.einsum("nii->ni", M)[:, LIVE])
    scale = d[:, None, :] * np.einsum("nkj,nj->nk", np.abs(x[..., LIVE]), d)[..., None] + np.abs(b[..., LIVE])
    assert np.all(scale.reshape(-1, len(LIVE)).max(axis=0) > 0)                   # every live row is exercised
    assert np.all(scale > 0)
    bound = C_S * EPS * scale + (0.0 if extra is None else extra[..., LIVE])
    r = res[..., LIVE]
    worst = float((r / (EPS * scale)).max())
    assert np.all(r <= bound), (worst, np.unravel_index(np.argmax(r / bound), r.shape))
    return worst


def _rhs(env, n, nrhs, seed):
    """nrhs random generalised forces; for nrhs == 7 the six Jacobian rows of the gripper body (as the kernel computed them) and one
    such force."""
    rng = np.random.default_rng(seed)
    b = torch.tensor(msr.force_rhs(rng, (n, nrhs)), dtype=torch.float32, device="cuda")
    if nrhs == 7:
        env.refresh_jacobian_tensors()
        b[:, :6] = env.jacobian_whole[:, _gripper_and_foot(env.robot_model)[0]]
    return b.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("armature", [False, True])
@pytest.mark.parametrize("nrhs", [1, 7, 32])
@pytest.mark.parametrize("n", [1, 13, 64, 1000])
def test_solve_residual_every_env_and_row(n, nrhs, armature):
    env, M, _, _, _ = _case(n)
    if armature:
        M = M + np.diag(msr.armature_vector(env.tcfg))
    b = _rhs(env, n, nrhs, 41 + nrhs)
    x = env.mass_matrix_solve(b, armature=armature)
    assert x.shape == (n, nrhs, 26)
    torch.cuda.synchronize()
    worst = _row_check(M, x.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
    print(f"mass solve n={n} nrhs={nrhs} armature={armature}: largest |M_ref x - b| / (2^-24 scale) = {worst:.3g}")
    if nrhs == 1:                                                                 # the [N, 26] form is the same solve
        assert torch.equal(env.mass_matrix_solve(b[:, 0], armature=armature), x[:, 0])


@pytest.mark.gpu
def test_strided_jacobian_rhs_and_operational_space_inertia():
    n = 1000
    env, M, _, _, (root, q, _, _) = _case(n)
    m = env.robot_model
    for r in _gripper_and_foot(m):
        env.refresh_jacobian_tensors()
        view = env.jacobian_whole[:, r]
        assert not view.is_contiguous() and view.stride(0) == 27 * 156
        a, b = env.mass_matrix_solve(view), env.mass_matrix_solve(view.contiguous())
        assert bool(a.abs().sum() > 0) and torch.equal(a, b)
        lam = env.operational_space_inverse_inertia(r)
        assert lam.shape == (n, 6, 6)
        lam = lam.cpu().numpy().astype(np.float64)
        dg = np.einsum("nii->ni", lam)
        assert np.all(dg > 0)
        assert np.all(np.abs(lam - lam.transpose(0, 2, 1)) <= 2.0 ** -20 * np.sqrt(dg[:, :, None] * dg[:, None, :]))
        worst = 0.0
        for e in range(n):
            ref, bound = msr.lambda_inverse(M[e], msr.jacobian_rows(m, root[e, :3], root[e, 3:7], q[e], r))
            err = np.abs(lam[e] - ref)
            assert np.all(err <= bound), (r, e, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
        print(f"inverse operational-space inertia, rigid body {r}: largest error / bound = {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("armature", [False, True])
@pytest.mark.parametrize("n", [1, 13, 1000])
def test_forward_dynamics_residual_and_round_trip(n, armature):
    env, M, h, mag, (root, q, qd, bp) = _case(n)
    if armature:
        M = M + np.diag(msr.armature_vector(env.tcfg))
    tau = _rhs(env, n, 1, 59)[:, 0].contiguous()
    nd = env.forward_dynamics(tau, armature=armature)
    assert nd.shape == (n, 26)
    torch.cuda.synchronize()
    t64 = tau.cpu().numpy().astype(np.float64)
    t64[:, FINGERS] = 0.0                                                         # the fingers' entries of tau are ignored
    b = t64 - h
    worst = _row_check(M, nd.cpu().numpy().astype(np.float64)[:, None], b[:, None], extra=(C_ID * EPS * mag)[:, None])
    print(f"forward dynamics n={n} armature={armature}: largest |(M_ref + A) nudot + h_ref - tau| / (2^-24 scale) = {worst:.3g}")
    # tau = None is an explicit zero tensor
    assert torch.equal(env.forward_dynamics(None, armature=armature), env.forward_dynamics(torch.zeros_like(tau), armature=armature))
    if not armature:                                                              # inverse_dynamics is rigid-body dynamics
        back = env.inverse_dynamics(nd).cpu().numpy().astype(np.float64)
        m = env.robot_model
        g = [float(x) for x in env.tcfg.gravity]
        nd64 = nd.cpu().numpy().astype(np.float64)
        mag1 = np.array([idr.inverse_dynamics(m, root[e, :3], root[e, 3:7], q[e], np.r_[root[e, 7:13], qd[e]], nd64[e], bp[e], g)[1]
                         for e in range(n)])
        d = np.sqrt(np.einsum("nii->ni", M))
        scale = d * np.einsum("nj,nj->n", np.abs(nd64), d)[:, None] + np.abs(b)
        allow = C_ID * EPS * mag1 + C_S * EPS * scale + C_ID * EPS * mag
        err = np.abs(back - t64)
        assert np.all(err[:, LIVE] <= allow[:, LIVE]), float((err[:, LIVE] / allow[:, LIVE]).max())
        print(f"round trip n={n}: largest |ID(FD(tau)) - tau| / allowance = {(err[:, LIVE] / allow[:, LIVE]).max():.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("armature", [True, False])
def test_forward_dynamics_against_the_oracle(robot, armature):
    """(M_ref + A) (nudot_kernel - nudot_oracle) within the row bound plus the oracle's 1e-4 max(1, |tau|) torque allowance."""
    import test_inverse_dynamics as tid
    n = 64
    env, states = tid._airborne_env(robot, n)
    m = env.robot_model
    root = env.root_states.cpu().numpy().astype(np.float64)
    q, qd = env.dof_pos.cpu().numpy().astype(np.float64), env.dof_vel.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    o = _oracle(robot, armature)
    A = msr.armature_vector(env.tcfg) if armature else None
    tau = np.zeros((n, 26))
    for e in range(n):
        tau[e, 6:] = states[e][6]
    nd = env.forward_dynamics(torch.tensor(tau, dtype=torch.float32, device="cuda"), armature=armature)
    torch.cuda.synchronize()
    nd = nd.cpu().numpy().astype(np.float64)
    assert np.isfinite(nd).all() and np.all(nd[:, FINGERS] == 0)
    tau = tau.astype(np.float32).astype(np.float64)
    worst = 0.0
    for e in range(n):
        o.set("BODY_PARAMS", bp[e][None])
        a0, qdd = tid._oracle_accelerations(o, root[e], q[e], qd[e], states[e][6])
        M = msr.mass_matrix(m, root[e, :3], root[e, 3:7], q[e], bp[e], A)
        h, _ = idr.bias_forces(m, root[e, :3], root[e, 3:7], q[e], np.r_[root[e, 7:13], qd[e]], bp[e])
        diff = np.abs(M @ (nd[e] - np.r_[a0, qdd]))
        bound = C_S * EPS * msr.row_scale(M, nd[e], tau[e] - h) + 1e-4 * max(1.0, np.abs(tau[e]).max())
        assert np.all(diff[LIVE] <= bound[LIVE]), (e, float((diff[LIVE] / bound[LIVE]).max()))
        worst = max(worst, float((diff[LIVE] / bound[LIVE]).max()))
    print(f"forward dynamics vs oracle ABA (armature={armature}): largest difference / bound = {worst:.3g}")


@pytest.mark.gpu
def test_consistent_with_the_mass_matrix_kernel():
    """mm_whole @ x - b at 4096 envs, every 37th env plus the last: the row bound plus the mass-matrix kernel's C_MM 2^-24 |mm| |x|."""
    import test_inverse_dynamics as tid
    n, nrhs = 4096, 7
    env = tid._env(n, seed=3, steps=10)
    b = torch.tensor(msr.force_rhs(np.random.default_rng(67), (n, nrhs)), dtype=torch.float32, device="cuda")
    x = env.mass_matrix_solve(b)
    env.refresh_mass_matrix_tensors()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and bool((x[..., FINGERS] == 0).all())
    envs = sorted(set(range(0, n, 37)) | {n - 1})
    mm = env.mm_whole[envs].double().cpu().numpy()
    xs, bs = x[envs].double().cpu().numpy(), b[envs].double().cpu().numpy()
    m = env.robot_model
    root = env.root_states[envs].cpu().numpy().astype(np.float64)
    q = env.dof_pos[envs].cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS")[envs].cpu().numpy().astype(np.float64)
    worst = 0.0
    for i in range(len(envs)):
        M = wb.mass_matrix(m, root[i, :3], root[i, 3:7], q[i], bp[i])
        res = np.abs(xs[i] @ mm[i].T - bs[i])
        bound = C_S * EPS * msr.row_scale(M, xs[i], bs[i]) + C_MM * EPS * (np.abs(xs[i]) @ np.abs(mm[i]).T)
        assert np.all(res[:, LIVE] <= bound[:, LIVE]), (envs[i], float((res[:, LIVE] / bound[:, LIVE]).max()))
        worst = max(worst, float((res[:, LIVE] / bound[:, LIVE]).max()))
    print(f"mass-matrix kernel consistency: largest |mm x - b| / bound = {worst:.3g}")


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    b = torch.tensor(msr.force_rhs(np.random.default_rng(71), (n, 32)), dtype=torch.float32, device="cuda")
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        x, nd = env.mass_matrix_solve(b, armature=True), env.forward_dynamics(b[:, 0].contiguous())
        torch.cuda.synchronize()
        outs.append((x.clone(), nd.clone()))
    assert bool(outs[0][0].abs().sum() > 0) and bool(outs[0][1].abs().sum() > 0)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_argument_errors_leave_the_outputs_untouched():
    import test_inverse_dynamics as tid
    n = 13
    env = tid._env(n, seed=4, steps=3)
    L, h = env.sim.L, env.sim.h
    b = torch.tensor(msr.force_rhs(np.random.default_rng(73), (n, 2)), dtype=torch.float32, device="cuda")
    out = torch.full((n, 2, 26), 12345.0, device="cuda")
    nd = torch.full((n, 26), 12345.0, device="cuda")
    bad = [L.wbc_sim_mass_solve(None, b.data_ptr(), 52, 2, out.data_ptr(), 0, None),
           L.wbc_sim_mass_solve(h, None, 52, 2, out.data_ptr(), 0, None),
           L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 2, None, 0, None),
           L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 0, out.data_ptr(), 0, None),
           L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 33, out.data_ptr(), 0, None),
           L.wbc_sim_mass_solve(h, b.data_ptr(), 51, 2, out.data_ptr(), 0, None),
           L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 2, out.data_ptr(), 2, None),
           L.wbc_sim_mass_solve(h, b.data_ptr() + 2, 52, 1, out.data_ptr(), 0, None),
           L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 2, out.data_ptr() + 1, 0, None),
           L.wbc_sim_forward_dynamics(None, b.data_ptr(), nd.data_ptr(), 0, None),
           L.wbc_sim_forward_dynamics(h, b.data_ptr(), None, 0, None),
           L.wbc_sim_forward_dynamics(h, b.data_ptr(), nd.data_ptr(), 4, None),
           L.wbc_sim_forward_dynamics(h, b.data_ptr() + 2, nd.data_ptr(), 0, None),
           L.wbc_sim_forward_dynamics(h, None, nd.data_ptr() + 3, 0, None)]
    assert bad == [-1] * len(bad), bad
    assert L.wbc_sim_mass_solve(h, None, 52, 2, out.data_ptr(), 0, None) == -1 and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 2, out.data_ptr() + 2, 0, None) == -1 and b"aligned" in L.wbc_last_error()
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all()) and bool((nd == 12345.0).all())
    # 4-byte alignment is all that is needed: an output one float into a buffer
    want = env.mass_matrix_solve(b)
    big = torch.full((n * 52 + 1,), 12345.0, device="cuda")
    assert L.wbc_sim_mass_solve(h, b.data_ptr(), 52, 2, big.data_ptr() + 4, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[1:].view(n, 2, 26), want) and float(big[0]) == 12345.0
    # the fingers' entries of the right-hand side are ignored
    b2 = b.clone(); b2[..., FINGERS] = 7.0
    assert torch.equal(env.mass_matrix_solve(b2), want)


@pytest.mark.gpu
def test_step_is_untouched_by_solves():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for solve in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        b = torch.ones(n, 3, 26, device="cuda")
        for _ in range(5):
            if solve:
                env.mass_matrix_solve(b, armature=True); env.forward_dynamics()
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if solve:
                env.forward_dynamics(b[:, 0].contiguous(), armature=True); env.operational_space_inverse_inertia(0)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
