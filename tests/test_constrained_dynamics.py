"""Rigid-body accelerations acc = J nudot + Jdot nu (wbc_sim_body_accelerations) and forward dynamics with contacts held
(wbc_sim_constrained_dynamics; csrc/wbc_arm_kernel.hip, definitions in include/wbc_sim.h). The CPU tests pin the fp64 references of
tests/constrained_dynamics_reference.py to a central difference of the Jacobian, to the Jacobian itself, to their own residuals and to
forward dynamics, and measure the fp32 yardsticks; the GPU tests hold the kernels to the references row by row, to the sibling entry
points and to their own invariances.

Bounds (constrained_dynamics_reference.py): accelerations |acc - ref| <= C_A 2^-24 mag; dynamics rows C_S 2^-24 scale + C_ID 2^-24 mag(h);
constraint rows C_K 2^-24 scale + C_A 2^-24 mag(gamma). K_ref is the fp32 yardstick's largest ratio against the scale over the families
below (60 random states; asserted <= C / 16 on the CPU), C the smallest power of two >= 16 K_ref (C_K >= 32), and the last column the
kernel's largest ratio on an MI355X (n = 1, 13, 64 and every case of the GPU tests):

    rows                                          K_ref     C       kernel's largest ratio
    accelerations (Jdot nu and a random nudot)    3.49      64      not measured
    constraint rows                               0.457     32      not measured
    dynamics rows (C_S, C_ID restated)            2.02      128     not measured

"not measured" stands for the kernels as they are. A first form of the acceleration walk (spatial vectors about the base origin) was
measured on an MI355X: Jdot nu at n = 13 reached 77.8 against C_A = 64, the cancellation of |w|^2 |x| terms at far bodies; the walk
now carries classical accelerations at each body's own origin (fp32 emulation on the CPU: 5.1 where the first form gives 780).

The largest condition number of the diagonally scaled Delassus matrix over the GPU cases' active rows is not measured on the GPU (85.1 over the CPU families; asserted <= 1000 on both).
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
import arm_codegen
import whole_body_reference as wb
from wbc_amd import abi

FINGERS, LIVE, EPS = cdr.FINGERS, cdr.LIVE, cdr.EPS
C_S, C_ID, C_A, C_K = cdr.C_S, cdr.C_ID, cdr.C_A, cdr.C_K
COND_MAX = 1000.0
SENTINEL = 12345.0


def _random_state(rng):
    import test_mass_solve as tms
    return tms._random_state(rng)


def _random_body_params(m, rng):
    import test_mass_solve as tms
    return tms._random_body_params(m, rng)


def _bodies(model):
    """(feet [4], gripper) rigid-body indices."""
    feet = [i for i, name in enumerate(model.rb_names) if "foot" in name]
    assert len(feet) == 4
    return feet, model.rb_names.index("wx250s/ee_gripper_link")


def _rotated(quat, w):
    """exp(w^) applied to the orientation quat (xyzw): the quaternion of the rotation vector w times quat."""
    import test_inverse_dynamics as tid
    th = np.linalg.norm(w)
    dq = np.r_[np.sin(th / 2) * w / th, np.cos(th / 2)] if th > 0 else np.array([0.0, 0.0, 0.0, 1.0])
    return tid._quat_mul(dq, quat)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 2)(3, 7)
    p = C.addressof(buf)
    assert L.wbc_sim_body_accelerations(None, None, p, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_constrained_dynamics(None, idx, 2, None, None, None, 0.0, 0, p, None, p, None) == -1
    assert b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_constrained_dynamics_workspace_floats(10, 4) == 10 * (2 * 13 * 26 + 16)
    assert L.wbc_sim_constrained_dynamics_workspace_floats(10, 0) == 0 and L.wbc_sim_constrained_dynamics_workspace_floats(10, 6) == 0


def test_new_kernels_codegen():
    """No scratch, no flat memory instructions, the launch's workgroup size, static LDS small enough for 16 workgroups per CU."""
    for kernel in ("wbc_body_accel_kernel", "wbc_constraint_rhs_kernel", "wbc_constraint_solve_kernel"):
        assert arm_codegen.meta(kernel, "private_segment_fixed_size") == 0, kernel
        assert arm_codegen.meta(kernel, "max_flat_workgroup_size") == 64, kernel
        assert arm_codegen.meta(kernel, "group_segment_fixed_size") <= 160 * 1024 // 16, kernel
        body = arm_codegen.body(kernel)
        assert "s_endpgm" in body and re.search(r"\bglobal_store_dword", body), kernel
        assert not re.search(r"\bflat_", body) and "scratch_" not in body, kernel


def test_reference_bias_acceleration_is_the_jacobian_derivative_along_the_flow(robot):
    """Jdot nu against (J(t + eps) - J(t - eps)) / (2 eps) nu with q +- eps qd, the root rotated by exp(+-eps omega^) and translated by
    +-eps v: fp64, error O(eps^2)."""
    m = robot["model"]
    eps = 1e-5
    for seed in range(12):
        rng = np.random.default_rng(300 + seed)
        pos, quat, q, nu = _random_state(rng)
        Js = [wb.jacobian(m, pos + sgn * eps * nu[0:3], _rotated(quat, sgn * eps * nu[3:6]), q + sgn * eps * nu[6:]) for sgn in (1.0, -1.0)]
        want = ((Js[0] - Js[1]) / (2 * eps)) @ nu
        got, mag = cdr.body_accelerations(m, pos, quat, q, nu)
        assert np.all(got[mag == 0] == 0) and np.mean(mag > 0) > 0.9
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), (seed, np.abs(got - want).max())


def test_reference_acceleration_is_linear_in_nudot_through_the_jacobian(robot):
    m = robot["model"]
    for seed in range(12):
        rng = np.random.default_rng(320 + seed)
        pos, quat, q, nu = _random_state(rng)
        nudot = np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]
        nudot[FINGERS] = 0.0
        a1, _ = cdr.body_accelerations(m, pos, quat, q, nu, nudot)
        a0, _ = cdr.body_accelerations(m, pos, quat, q, nu)
        want = wb.jacobian(m, pos, quat, q) @ nudot
        assert np.abs(a1 - a0 - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        far, _ = cdr.body_accelerations(m, pos + np.array([3.0, 110.0, 0.0]), quat, q, nu, nudot)
        assert np.abs(far - a1).max() <= 1e-9


def _acc_ratio(got, ref, mag):
    """Largest |got - ref| / (2^-24 mag); where the magnitude is 0 (a body fixed to a root that does not accelerate) both are exactly 0."""
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    return float((np.abs(got - ref)[~zero] / (EPS * mag[~zero])).max())


def _family(m, seed, arm_vec):
    """One member of the families the GPU tests use: (state, bodies, on [3K], tau, a_des [3K], damping, armature vector or None)."""
    rng = np.random.default_rng(500 + seed)
    pos, quat, q, nu = _random_state(rng)
    bp = _random_body_params(m, rng)
    feet, grip = _bodies(m)
    bodies = [feet, feet + [grip], [grip]][seed % 3]
    active = np.ones(len(bodies), dtype=bool)
    if seed % 3 == 0:                                                              # 0..4 active feet, every count
        active[:] = False
        active[rng.permutation(4)[:(seed // 3) % 5]] = True
    a_des = rng.uniform(-5, 5, 3 * len(bodies))
    tau = None if seed % 7 == 6 else msr.force_rhs(rng, ())
    damping = 1e-3 if seed % 4 == 3 else 0.0
    return (pos, quat, q, nu, bp), bodies, np.repeat(active, 3), tau, a_des, damping, (arm_vec if seed % 2 else None)


def _system(m, state, bodies, on, armature):
    pos, quat, q, nu, bp = state
    M = msr.mass_matrix(m, pos, quat, q, bp, armature)
    h, magh = idr.bias_forces(m, pos, quat, q, nu, bp)
    Jc, gamma, magg = cdr.constraint_rows(m, pos, quat, q, nu, bodies, on[::3])
    return M, h, magh, Jc, gamma, magg


def test_kkt_reference_satisfies_both_residuals_and_reduces_to_forward_dynamics(robot):
    m = robot["model"]
    A = msr.armature_vector(robot["tcfg"])
    for seed in range(15):
        state, bodies, on, tau, a_des, damping, arm = _family(m, seed, A)
        M, h, _, Jc, gamma, _ = _system(m, state, bodies, on, arm)
        a_on = np.where(on, a_des, 0.0)
        nudot, lam = cdr.solve_with_mask(M, h, tau, Jc, gamma, a_des, damping, on)
        assert np.all(nudot[FINGERS] == 0) and np.all(lam[~on] == 0)
        r, s = cdr.dynamics_residual_and_scale(M, h, tau, Jc, nudot, lam)
        assert np.all(r[LIVE] <= 1e-10 * s[LIVE])
        r, s = cdr.constraint_residual_and_scale(M, Jc, gamma, a_on, damping, nudot, lam)
        assert np.all(r[on] <= 1e-10 * s[on]) and np.all(r[~on] == 0)
        pos, quat, q, nu, bp = state
        free, _ = cdr.solve_with_mask(M, h, tau, Jc, gamma, a_des, damping, np.zeros_like(on))
        want, _, _, _ = msr.forward_dynamics(m, pos, quat, q, nu, tau, bp, armature=arm)
        assert np.abs(free - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref of the three row kinds and the largest scaled condition number, over 60 members of _family and, for the accelerations,
    the same states with nudot = 0 and with a random nudot (the range of test_inverse_dynamics._random_nudot)."""
    from wbc_amd.config import WidowGo1RoughCfg
    m = abi.load_default_model()
    A = msr.armature_vector(abi.fill_task_cfg(WidowGo1RoughCfg(), m))
    k_acc = k_dyn = k_con = cond = 0.0
    counts = set()
    for seed in range(60):
        state, bodies, on, tau, a_des, damping, arm = _family(m, seed, A)
        pos, quat, q, nu, _bp = state
        rng = np.random.default_rng(900 + seed)
        for nudot in (None, np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]):
            ref, mag = cdr.body_accelerations(m, pos, quat, q, nu, nudot)
            y32, _ = cdr.body_accelerations(m, pos, quat, q, nu, nudot, dtype=np.float32)
            k_acc = max(k_acc, _acc_ratio(y32, ref, mag))
        M, h, magh, Jc, gamma, magg = _system(m, state, bodies, on, arm)
        cond = max(cond, cdr.delassus_condition(M, Jc, damping, on))
        counts.add((len(bodies), int(on.sum()) // 3))
        a_on = np.where(on, a_des, 0.0)
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        t32 = None if tau is None else f32(tau)
        nudot, lam = cdr.yardstick_f32(M, h, t32, Jc, gamma, f32(a_on), damping, on)
        r, s = cdr.dynamics_residual_and_scale(M, h, t32, Jc, nudot, lam)
        k_dyn = max(k_dyn, float((r[LIVE] / (EPS * s[LIVE])).max()))
        if on.any():
            r, s = cdr.constraint_residual_and_scale(M, Jc, gamma, f32(a_on), damping, nudot, lam)
            k_con = max(k_con, float((r[on] / (EPS * s[on])).max()))
    assert {(4, k) for k in range(5)} <= counts and (5, 5) in counts and (1, 1) in counts
    return k_acc, k_dyn, k_con, cond


def test_fp32_yardsticks_sit_well_inside_the_bounds():
    k_acc, k_dyn, k_con, cond = _yardsticks()
    print(f"yardsticks: accelerations K_ref = {k_acc:.3g} (C_A = {C_A}), dynamics rows {k_dyn:.3g} (C_S = {C_S}), "
          f"constraint rows {k_con:.3g} (C_K = {C_K}); largest scaled Delassus condition number {cond:.3g}")
    assert k_acc <= C_A / 16 and k_con <= C_K / 16 and k_dyn <= C_S / 16
    assert C_A <= 1024 and C_K >= 32
    assert C_A == 2.0 ** np.ceil(np.log2(16 * k_acc)) and C_K == max(32.0, 2.0 ** np.ceil(np.log2(16 * k_con)))


def test_delassus_conditioning_of_the_families():
    assert _yardsticks()[3] <= COND_MAX


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(n):
    """test_mass_solve._case(n) (env, M_ref, h_ref, mag(h), state) plus the fp64 kinematics of every env: J [n, 27, 6, 26],
    Jdot nu [n, 27, 6] and its magnitude. Computed once and left unchanged."""
    import test_mass_solve as tms
    env, M, h, magh, (root, q, qd, bp) = tms._case(n)
    m = env.robot_model
    J = np.array([wb.jacobian(m, root[e, :3], root[e, 3:7], q[e]) for e in range(n)])
    am = [cdr.body_accelerations(m, root[e, :3], root[e, 3:7], q[e], np.r_[root[e, 7:13], qd[e]]) for e in range(n)]
    return env, M, h, magh, (root, q, qd, bp), J, np.array([a for a, _ in am]), np.array([g for _, g in am])


def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_accelerations_every_env_body_and_row(n):
    import test_inverse_dynamics as tid
    env, _, _, _, (root, q, qd, _), J, g_ref, g_mag = _case(n)
    m = env.robot_model
    nudot = tid._random_nudot(n, 83)
    buf = _sentinel_buffer(n * 27 * 6)
    L = env.sim.L
    assert L.wbc_sim_body_accelerations(env.sim.h, None, buf.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((buf[n * 162:] == SENTINEL).all())
    jd = buf[:n * 162].view(n, 27, 6).clone()
    assert torch.equal(env.rigid_body_accelerations(), jd)
    acc = env.rigid_body_accelerations(nudot)
    assert acc.shape == (n, 27, 6)
    torch.cuda.synchronize()
    nd64 = nudot.cpu().numpy().astype(np.float64)
    am = [cdr.body_accelerations(m, root[e, :3], root[e, 3:7], q[e], np.r_[root[e, 7:13], qd[e]], nd64[e]) for e in range(n)]
    a_ref, a_mag = np.array([a for a, _ in am]), np.array([g for _, g in am])
    worst = {}
    for name, got, ref, mag in (("Jdot nu", jd, g_ref, g_mag), ("acc", acc, a_ref, a_mag)):
        worst[name] = _acc_ratio(got.cpu().numpy().astype(np.float64), ref, mag)
        assert worst[name] <= C_A, (name, worst[name])
    print(f"body accelerations n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")
    # the fingers' entries of nudot are ignored
    nd2 = nudot.clone(); nd2[:, FINGERS] = 7.0
    assert torch.equal(env.rigid_body_accelerations(nd2), acc)
    # acc(nudot) - acc(0) against the Jacobian kernel's own J @ nudot: that kernel's entry allowance 5e-6 + 1e-4 |J| (tests/
    # test_whole_body_dynamics.py) through |nudot|, plus this kernel's two evaluations
    env.refresh_jacobian_tensors()
    torch.cuda.synchronize()
    Jk = env.jacobian_whole.double().cpu().numpy()
    diff = np.abs(acc.double().cpu().numpy() - jd.double().cpu().numpy() - np.einsum("nrkc,nc->nrk", Jk, nd64))
    allow = np.einsum("nrkc,nc->nrk", 5e-6 + 1e-4 * np.abs(J), np.abs(nd64)) + C_A * EPS * (a_mag + g_mag)
    assert np.all(allow > 0) and np.all(diff <= allow), float((diff / allow).max())
    print(f"body accelerations n={n}: largest |acc(nudot) - acc(0) - jacobian_whole @ nudot| / allowance = {(diff / allow).max():.3g}")


@pytest.mark.gpu
def test_accelerations_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    nudot = tid._random_nudot(n, 89)
    feet, grip = _bodies(robot["model"])
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        a, (nd, lam) = env.rigid_body_accelerations(nudot), env.sim.constrained_dynamics(feet + [grip], tau=nudot, damping=1e-3)
        torch.cuda.synchronize()
        outs.append((a.clone(), nd.clone(), lam.clone()))
    for x, y in zip(*outs):
        assert bool(x.abs().sum() > 0) and torch.equal(x, y)


_WORST = {"dyn": 0.0, "con": 0.0, "cond": 0.0}


def _check(n, bodies, active, tau, a_des, damping, armature, nudot, lam):
    """Both bounds for every env and row, from the kernel's own (nudot, lam) against the fp64 system; the conditioning condition."""
    env, M, h, magh, _, J, g_ref, g_mag = _case(n)
    if armature:
        M = M + np.diag(msr.armature_vector(env.tcfg))
    K = len(bodies)
    nd, lm = nudot.cpu().numpy().astype(np.float64), lam.cpu().numpy().astype(np.float64).reshape(n, 3 * K)
    assert np.isfinite(nd).all() and np.isfinite(lm).all()
    assert np.all(nd[:, FINGERS] == 0)
    act = np.ones((n, K), dtype=bool) if active is None else active.cpu().numpy().astype(bool)
    t64 = None if tau is None else tau.cpu().numpy().astype(np.float64)
    a64 = np.zeros((n, 3 * K)) if a_des is None else a_des.cpu().numpy().astype(np.float64).reshape(n, 3 * K)
    wd = wc = 0.0
    for e in range(n):
        on = np.repeat(act[e], 3)
        assert np.all(lm[e][~on] == 0)
        Jc = np.concatenate([J[e, r, 0:3] for r in bodies]) * on[:, None]
        gamma = np.concatenate([g_ref[e, r, 0:3] for r in bodies]) * on
        magg = np.concatenate([g_mag[e, r, 0:3] for r in bodies]) * on
        a_on = np.where(on, a64[e], 0.0)
        cond = cdr.delassus_condition(M[e], Jc, damping, on)
        assert cond <= COND_MAX, (e, cond)
        _WORST["cond"] = max(_WORST["cond"], cond)
        te = None if t64 is None else np.where(np.isin(np.arange(26), FINGERS), 0.0, t64[e])
        r, s = cdr.dynamics_residual_and_scale(M[e], h[e], te, Jc, nd[e], lm[e])
        assert np.all(s[LIVE] > 0)
        bound = C_S * EPS * s + C_ID * EPS * magh[e]
        assert np.all(r[LIVE] <= bound[LIVE]), ("dynamics", e, float((r[LIVE] / bound[LIVE]).max()))
        wd = max(wd, float((r[LIVE] / (EPS * s[LIVE])).max()))
        if on.any():
            r, s = cdr.constraint_residual_and_scale(M[e], Jc, gamma, a_on, damping, nd[e], lm[e])
            bound = C_K * EPS * s + C_A * EPS * magg
            assert np.all(s[on] > 0)
            assert np.all(r[on] <= bound[on]), ("constraint", e, float((r[on] / bound[on]).max()))
            wc = max(wc, float((r[on] / (EPS * s[on])).max()))
    _WORST["dyn"], _WORST["con"] = max(_WORST["dyn"], wd), max(_WORST["con"], wc)
    return wd, wc


def _masks(n, K):
    """Stance masks [n, K] u8: env e has the feet of the bits of e % 16 active (all 16 patterns at n = 64, none active at env 0 of every
    n), a fifth body active on odd envs."""
    e = torch.arange(n, device="cuda")
    return torch.stack([((e >> k) & 1) if k < 4 else (e & 1) for k in range(K)], 1).to(torch.uint8).contiguous()


CASES = ["feet", "feet_masked", "feet_gripper_ades", "gripper", "armature", "damping", "tau_null", "lambda_null"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [1, 13, 64])
def test_constrained_dynamics_every_env_and_row(n, case):
    env = _case(n)[0]
    feet, grip = _bodies(env.robot_model)
    rng = np.random.default_rng(97)
    tau = torch.tensor(msr.force_rhs(rng, (n,)), dtype=torch.float32, device="cuda")
    bodies, active, a_des, damping, armature = feet, None, None, 0.0, False
    if case == "feet_masked":
        active = _masks(n, 4)
    elif case == "feet_gripper_ades":
        bodies = feet + [grip]
        a_des = torch.tensor(rng.uniform(-5, 5, (n, 5, 3)), dtype=torch.float32, device="cuda")
    elif case == "gripper":
        bodies = [grip]
    elif case == "armature":
        armature = True
    elif case == "damping":
        damping = 1e-3
    elif case == "tau_null":
        tau = None
    K = len(bodies)
    L, sim = env.sim.L, env.sim
    nws = int(L.wbc_sim_constrained_dynamics_workspace_floats(n, K))
    assert nws == n * (2 * (3 * K + 1) * 26 + 16)
    ndb, lmb, ws = _sentinel_buffer(n * 26), _sentinel_buffer(n * 3 * K), _sentinel_buffer(nws)
    idx = (C.c_int32 * K)(*bodies)
    a_in = a_des
    if case == "feet_masked":                                                      # NaN where inactive: never read
        a_in = torch.tensor(rng.uniform(-5, 5, (n, 4, 3)), dtype=torch.float32, device="cuda")
        a_in[active == 0] = float("nan")
    rc = L.wbc_sim_constrained_dynamics(sim.h, idx, K, active.data_ptr() if active is not None else None,
                                        tau.data_ptr() if tau is not None else None, a_in.data_ptr() if a_in is not None else None,
                                        damping, 1 if armature else 0, ndb.data_ptr(),
                                        None if case == "lambda_null" else lmb.data_ptr(), ws.data_ptr(), None)
    assert rc == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    assert bool((ndb[n * 26:] == SENTINEL).all()) and bool((lmb[n * 3 * K:] == SENTINEL).all()) and bool((ws[nws:] == SENTINEL).all())
    nudot = ndb[:n * 26].view(n, 26)
    # the Python entry point is the same call
    nd2, lam2 = sim.constrained_dynamics(bodies, tau=tau, active=None if active is None else active.bool(), acc_des=a_in,
                                         damping=damping, armature=armature)
    assert torch.equal(nd2, nudot) and lam2.shape == (n, K, 3)
    if case == "lambda_null":
        assert bool((lmb == SENTINEL).all())
        lam = lam2
    else:
        lam = lmb[:n * 3 * K].view(n, K, 3)
        assert torch.equal(lam, lam2)
    if case == "feet":
        nd3, lam3 = env.stance_forward_dynamics(tau)
        assert torch.equal(nd3, nudot) and torch.equal(lam3, lam)
    a_chk = a_in
    if case == "feet_masked":
        a_chk = torch.nan_to_num(a_in, nan=0.0)
        nd3, lam3 = env.stance_forward_dynamics(tau, stance=active.bool())        # a_des = 0 there: another problem, the same masks
        _check(n, bodies, active, tau, None, damping, armature, nd3, lam3)
    wd, wc = _check(n, bodies, active, tau, a_chk, damping, armature, nudot, lam)
    print(f"constrained dynamics n={n} {case}: largest dynamics-row residual / (2^-24 scale) = {wd:.3g}, constraint-row = {wc:.3g}; "
          f"running maxima {_WORST}")
    if case == "feet_masked":
        # an env with no active body is forward dynamics, within that entry point's row bound on either side
        _, M, h, magh, _, _, _, _ = _case(n)
        none = (active.sum(1) == 0).cpu().numpy()
        assert none[0]
        fd = env.forward_dynamics(tau).cpu().numpy().astype(np.float64)
        nd = nudot.cpu().numpy().astype(np.float64)
        t64 = tau.cpu().numpy().astype(np.float64)
        for e in np.nonzero(none)[0]:
            diff = np.abs(M[e] @ (nd[e] - fd[e]))
            bound = (C_S * EPS * msr.row_scale(M[e], nd[e], t64[e] - h[e]) + C_S * EPS * msr.row_scale(M[e], fd[e], t64[e] - h[e])
                     + 2 * C_ID * EPS * magh[e])
            assert np.all(diff[LIVE] <= bound[LIVE]), (e, float((diff[LIVE] / bound[LIVE]).max()))


@pytest.mark.gpu
def test_gripper_force_agrees_with_the_operational_space_route():
    """Gripper alone, a_des = 0: (J M^-1 J^T) lam = -(J a_free + gamma) with the 3 x 3 block of operational_space_inverse_inertia,
    a_free of forward_dynamics, gamma of rigid_body_accelerations and the Jacobian kernel's J. Allowance: lambda_inverse's entry
    bound through |lam| for the block, and the constraint-row bound twice (once for this call, once for a_free and gamma of the
    other route, which meet the same rows)."""
    n = 64
    env, M, h, _, (root, q, _, _), J, g_ref, g_mag = _case(n)
    m = env.robot_model
    _, grip = _bodies(m)
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(101), (n,)), dtype=torch.float32, device="cuda")
    nudot, lam = env.sim.constrained_dynamics([grip], tau=tau)
    blk = env.operational_space_inverse_inertia(grip)[:, :3, :3].double().cpu().numpy()
    a_free = env.forward_dynamics(tau).double().cpu().numpy()
    gamma = env.rigid_body_accelerations()[:, grip, :3].double().cpu().numpy()
    Jk = env.jacobian_whole[:, grip, :3].double().cpu().numpy()
    torch.cuda.synchronize()
    lm, nd = lam.double().cpu().numpy()[:, 0], nudot.double().cpu().numpy()
    worst = 0.0
    for e in range(n):
        _, lbound = msr.lambda_inverse(M[e], J[e, grip])
        res = np.abs(blk[e] @ lm[e] + Jk[e] @ a_free[e] + gamma[e])
        _, s1 = cdr.constraint_residual_and_scale(M[e], J[e, grip, :3], g_ref[e, grip, :3], np.zeros(3), 0.0, nd[e], lm[e])
        _, s2 = cdr.constraint_residual_and_scale(M[e], J[e, grip, :3], g_ref[e, grip, :3], np.zeros(3), 0.0, a_free[e], 0 * lm[e])
        allow = lbound[:3, :3] @ np.abs(lm[e]) + C_K * EPS * (s1 + s2) + 2 * C_A * EPS * g_mag[e, grip, :3]
        assert np.all(res <= allow), (e, float((res / allow).max()))
        worst = max(worst, float((res / allow).max()))
    print(f"gripper alone vs operational-space route: largest residual / allowance = {worst:.3g}")


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env = _case(n)[0]
    feet, grip = _bodies(env.robot_model)
    bodies = feet + [grip]
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(103), (n,)), dtype=torch.float32, device="cuda")
    active = _masks(n, 5)
    want_nd, want_lam = env.sim.constrained_dynamics(bodies, tau=tau, active=active, damping=1e-3)
    want_acc = env.rigid_body_accelerations(tau)
    nd, lam, acc = torch.zeros_like(want_nd), torch.zeros_like(want_lam), torch.zeros_like(want_acc)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream (the workspace exists already)
        env.sim.constrained_dynamics(bodies, tau=tau, active=active, damping=1e-3, out=(nd, lam))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    nd.zero_(); lam.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.constrained_dynamics(bodies, tau=tau, active=active, damping=1e-3, out=(nd, lam))
        env.sim.body_accelerations(tau, out=acc)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(nd, want_nd) and torch.equal(lam, want_lam) and torch.equal(acc, want_acc)


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env = _case(n)[0]
    m = env.robot_model
    feet, grip = _bodies(m)
    L, h = env.sim.L, env.sim.h
    K = 4
    nd, lam = _sentinel_buffer(n * 26), _sentinel_buffer(n * 3 * 5)
    ws = _sentinel_buffer(int(L.wbc_sim_constrained_dynamics_workspace_floats(n, 5)))
    acc = _sentinel_buffer(n * 162)
    tau = torch.ones(n, 26, device="cuda")
    idx = (C.c_int32 * 5)(*(feet + [grip]))
    same_body = next(r for r in range(27) if r != feet[0] and m.rb_body[r] == m.rb_body[feet[0]])   # e.g. the calf the foot is fixed to
    call = lambda **kw: L.wbc_sim_constrained_dynamics(*[kw.get(k, d) for k, d in (
        ("sim", h), ("rb", idx), ("k", K), ("active", None), ("tau", tau.data_ptr()), ("a_des", None), ("damping", 0.0), ("flags", 0),
        ("nudot", nd.data_ptr()), ("lam", lam.data_ptr()), ("ws", ws.data_ptr()), ("stream", None))])
    refusals = [
        (dict(sim=None), b"NULL"), (dict(rb=None), b"NULL"), (dict(nudot=None), b"NULL"), (dict(ws=None), b"NULL"),
        (dict(k=0), b"nbodies"), (dict(k=6), b"nbodies"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], 27, feet[3])), b"index"), (dict(rb=(C.c_int32 * 4)(feet[0], -1, feet[2], feet[3])), b"index"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], same_body, feet[3])), b"same moving body"),
        (dict(damping=-1e-3), b"damping"), (dict(damping=float("inf")), b"damping"), (dict(damping=float("nan")), b"damping"),
        (dict(flags=2), b"flag"),
        (dict(tau=tau.data_ptr() + 2), b"aligned"), (dict(a_des=tau.data_ptr() + 1), b"aligned"), (dict(nudot=nd.data_ptr() + 2), b"aligned"),
        (dict(lam=lam.data_ptr() + 3), b"aligned"), (dict(ws=ws.data_ptr() + 2), b"aligned"),
    ]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert L.wbc_sim_body_accelerations(None, None, acc.data_ptr(), None) == -1
    assert L.wbc_sim_body_accelerations(h, None, None, None) == -1 and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_body_accelerations(h, None, acc.data_ptr() + 2, None) == -1 and b"aligned" in L.wbc_last_error()
    assert L.wbc_sim_body_accelerations(h, tau.data_ptr() + 1, acc.data_ptr(), None) == -1
    torch.cuda.synchronize()
    for t in (nd, lam, ws, acc):
        assert bool((t == SENTINEL).all())
    # 4-byte alignment is all that is needed: outputs one float into their buffers
    want_nd, want_lam = env.sim.constrained_dynamics(feet, tau=tau)
    want_acc = env.rigid_body_accelerations()
    assert call(nudot=nd.data_ptr() + 4, lam=lam.data_ptr() + 4, ws=ws.data_ptr() + 4) == 0
    assert L.wbc_sim_body_accelerations(h, None, acc.data_ptr() + 4, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(nd[1:1 + n * 26].view(n, 26), want_nd) and float(nd[0]) == SENTINEL
    assert torch.equal(lam[1:1 + n * 12].view(n, 4, 3), want_lam) and float(lam[0]) == SENTINEL
    assert torch.equal(acc[1:1 + n * 162].view(n, 27, 6), want_acc) and float(acc[0]) == SENTINEL and float(ws[0]) == SENTINEL


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_calls():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        feet, grip = _bodies(env.robot_model)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        b = torch.ones(n, 26, device="cuda")
        for _ in range(5):
            if use:
                env.stance_forward_dynamics(b, stance=env.get_foot_contacts()); env.rigid_body_accelerations()
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.sim.constrained_dynamics(feet + [grip], armature=True, damping=1e-3); env.rigid_body_accelerations(b)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
