"""Whole-body inverse dynamics tau = M nudot + C nu + g [N, 26] (wbc_sim_inverse_dynamics, csrc/wbc_arm_kernel.hip; definition in
include/wbc_sim.h). The CPU tests pin the fp64 restatement tests/inverse_dynamics_reference.py to the C oracle's forward dynamics,
to the mass-matrix restatement, to the power identity and to the potential energy; the GPU tests hold the kernel to that
restatement element-wise, to the existing mass-matrix kernel, to the oracle's forward dynamics and to its own invariances.

Element-wise bound of the GPU tests: |kernel - ref|_k <= C_ID * 2^-24 * mag_k, mag the restatement's magnitude vector (the sum of
the absolute values of the terms that make up row k). C_ID and C_MM follow the largest ratios measured on an MI355X (4x, rounded up
to a power of two) and may not exceed 4096; the measured ratios stand next to the constants."""
import copy
import ctypes as C
import re

import numpy as np
import pytest
import torch

import inverse_dynamics_reference as idr
import arm_codegen
import whole_body_reference as wb
from wbc_amd import abi

FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(wb.NCOL) if c not in FINGERS]
EPS = 2.0 ** -24
# Largest |kernel - ref| / (2^-24 mag) over every case, env and row of test_kernel_matches_reference_elementwise, measured on an
# MI355X: n = 1: 18.4, n = 64 (tilted gravity): 52.3, n = 1000: h 158, tau 91, grav 1259. The 1259 is ONE of the 18 000 joint rows
# of the grav case (the next is 172): a calf whose weight lever stands within 0.02 degrees of the vertical, so that mag is
# 1.0e-4 N m where m g |axis x lever| is 0.28 N m; the kernel's error there is 7.7e-9 N m = 0.46 * 2^-24 * 0.28, below half an ulp
# of the terms that cancel, which no fp32 evaluation undercuts. 4 x 1259 rounds up to 8192, above the cap of 4096 that the bound
# may not exceed: C_ID stands at the cap (3.25 x the measured maximum instead of 4 x).
C_ID = 4096.0
# Largest |ID(nudot) - h - mm @ nudot| / (2^-24 |mm| @ |nudot|) over the sampled envs of test_consistent_with_the_mass_matrix_kernel
# (the whole difference charged to the mass-matrix kernel), measured: 78.6; the same difference over the new kernel's own
# allowance 2^-24 (mag(nudot) + mag(0)): 156. 4 x 78.6 rounded up to a power of two.
C_MM = 512.0
assert C_ID <= 4096 and C_MM <= 4096


def _quat_mul(a, b):             # xyzw
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _airborne_state(model, seed):
    """The states of test_oracle_physics.test_aba_satisfies_kanes_equations: joints 0.05 rad inside their limits, |qd| <= 3,
    |tau| <= 10, 5 m above the ground. Returns pos, quat, q, qd, v, w, tau."""
    rng = np.random.default_rng(seed)
    lo = np.where(model.dof_lower < model.dof_upper, model.dof_lower, -2.0)
    hi = np.where(model.dof_lower < model.dof_upper, model.dof_upper, 2.0)
    locked = np.array(model.dof_locked)
    lo, hi = np.where(locked, -1.0, lo), np.where(locked, 1.0, hi)
    q = rng.uniform(lo + 0.05, hi - 0.05)
    qd = rng.uniform(-3, 3, size=20)
    q[locked], qd[locked] = 0.0, 0.0
    tau = rng.uniform(-10, 10, size=20)
    tau[locked] = 0
    quat = rng.normal(size=4)
    quat /= np.linalg.norm(quat)
    pos = np.array([3.0, -2.0, 5.0])
    v, w = rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3)
    return pos, quat, q, qd, v, w, tau


def _rigid_oracle(robot, n=1):
    from oracle import OracleSim
    tc = copy.copy(robot["tcfg"])
    for j in range(18):
        tc.joint_armature[j] = 0.0      # the implicit-PD armature is a modelling term, not rigid-body dynamics
    return OracleSim(robot["wmodel"], tc, n)


def _oracle_accelerations(o, root_row, q, qd, tau):
    """(a0 [6], qdd [20]) of the oracle's articulated-body algorithm for one airborne state, the box parked."""
    root = np.zeros((1, 2, 13))
    root[0, 0] = root_row
    root[0, 1, 6] = 1
    o.set("ROOT_STATES", root)
    o.set("DOF_STATE", np.stack([q, qd], -1)[None])
    o.set("TORQUES", tau[None])
    qdd, a0 = o.debug_aba(0)
    return a0, qdd


def _random_state(rng, far=False):
    quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
    pos = rng.normal(size=3) + (np.array([3.0, 110.0, 0.0]) if far else 0.0)
    q = rng.uniform(-1, 1, 20); q[18:] = rng.uniform(-0.03, 0.03, 2)
    nu = np.r_[rng.uniform(-1, 1, 3), rng.uniform(-2, 2, 3), rng.uniform(-3, 3, 20)]
    return pos, quat, q, nu


def _random_body_params(m, rng):
    return abi.body_params_from_randomisation(m, rng.uniform(-0.5, 2.5, 1), rng.uniform(-0.1, 0.1, (1, 3)),
                                              rng.uniform(0, 0.1, 1)).astype(np.float64)[0]


# ------------------------------------------------------------------------------------------------------------ CPU: restatement
def test_forward_then_inverse_dynamics_is_the_identity(robot):
    """ID(q, nu, ABA(q, nu, tau)) == (0_6, tau): worst 1.3e-5 N m over these 40 seeds (the oracle reads float32 model tables)."""
    model = robot["model"]
    o = _rigid_oracle(robot)
    locked = np.array(model.dof_locked)
    live = ~np.concatenate([np.zeros(6, bool), locked])
    worst = 0.0
    for seed in range(40):
        pos, quat, q, qd, v, w, tau = _airborne_state(model, seed)
        a0, qdd = _oracle_accelerations(o, np.concatenate([pos, quat, v, w]), q, qd, tau)
        got, _ = idr.inverse_dynamics(model, pos, quat, q, np.r_[v, w, qd], np.r_[a0, qdd], o.get("BODY_PARAMS")[0])
        err = np.abs(got - np.r_[np.zeros(6), tau])[live].max()
        worst = max(worst, err)
        assert err < 1e-4 * max(1.0, np.abs(tau).max()), (seed, err)
    print(f"forward-then-inverse worst residual {worst:.3g}")


def test_reference_is_consistent_with_the_mass_matrix():
    m = abi.load_default_model()
    for seed in range(40):
        rng = np.random.default_rng(seed)
        pos, quat, q, nu = _random_state(rng, far=seed % 2 == 1)
        bp = _random_body_params(m, rng)
        nudot = np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]
        t1, _ = idr.inverse_dynamics(m, pos, quat, q, nu, nudot, bp)
        t0, _ = idr.bias_forces(m, pos, quat, q, nu, bp)
        Ma = wb.mass_matrix(m, pos, quat, q, bp) @ nudot
        assert np.abs(t1 - t0 - Ma).max() <= 1e-12 * np.abs(Ma).max(), seed
        assert np.all(t1[FINGERS] == 0) and np.all(t0[FINGERS] == 0)


def test_reference_power_identity():
    """Without gravity nu . h == 1/2 nu^T Mdot nu (the velocity-product term does the work that changes the kinetic energy)."""
    m = abi.load_default_model()
    h = 1e-6
    for seed in range(40):
        rng = np.random.default_rng(seed)
        pos, quat, q, nu = _random_state(rng)
        bp = _random_body_params(m, rng)

        def M_at(t):                  # the mass matrix along the flow of nu
            w = nu[3:6]; ang = np.linalg.norm(w) * t
            dq = np.r_[np.sin(ang / 2) * w / np.linalg.norm(w), np.cos(ang / 2)]
            return wb.mass_matrix(m, pos + t * nu[0:3], _quat_mul(dq, quat), q + t * nu[6:], bp)
        Mdot = (M_at(h) - M_at(-h)) / (2 * h)
        tau, _ = idr.bias_forces(m, pos, quat, q, nu, bp, gravity=(0.0, 0.0, 0.0))
        assert nu @ tau == pytest.approx(0.5 * nu @ Mdot @ nu, rel=1e-6), seed


def test_reference_gravity_term():
    m = abi.load_default_model()
    rng = np.random.default_rng(7)
    g = np.array([1.0, -2.0, -9.0])
    h = 1e-6
    for _ in range(10):
        pos, quat, q, _nu = _random_state(rng)
        bp = _random_body_params(m, rng)
        gq, _ = idr.gravity_forces(m, pos, quat, q, bp, g)
        m_total = sum(mass for mass, _, _ in wb.body_inertias(m, bp))
        assert np.abs(gq[0:3] + m_total * g).max() <= 1e-12 * np.abs(m_total * g).max()
        for d in range(20):
            e = np.zeros(20); e[d] = h
            dV = (idr.potential_energy(m, pos, quat, q + e, bp, g) - idr.potential_energy(m, pos, quat, q - e, bp, g)) / (2 * h)
            assert abs(gq[6 + d] - dV) <= 1e-6, (d, gq[6 + d], dV)


def test_reference_translation():
    m = abi.load_default_model()
    rng = np.random.default_rng(7)
    for _ in range(10):
        pos, quat, q, nu = _random_state(rng)
        bp = _random_body_params(m, rng)
        nudot = np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]
        a, _ = idr.inverse_dynamics(m, pos, quat, q, nu, nudot, bp)
        b, _ = idr.inverse_dynamics(m, pos + np.array([3.0, 110.0, 0.0]), quat, q, nu, nudot, bp)
        assert np.abs(a - b).max() <= 1e-9


def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 32)()
    assert L.wbc_sim_inverse_dynamics(None, None, C.addressof(buf), C.addressof(buf), None) == -1
    assert b"NULL" in L.wbc_last_error()


def test_inverse_dynamics_kernel_codegen():
    """No scratch, no flat memory instructions, and static LDS small enough for 16 workgroups (of 64 lanes: 32 envs) per CU."""
    assert arm_codegen.meta("wbc_inverse_dynamics_kernel", "private_segment_fixed_size") == 0
    assert arm_codegen.meta("wbc_inverse_dynamics_kernel", "max_flat_workgroup_size") == 64
    assert arm_codegen.meta("wbc_inverse_dynamics_kernel", "group_segment_fixed_size") <= 160 * 1024 // 16
    body = arm_codegen.body("wbc_inverse_dynamics_kernel")
    assert "s_endpgm" in body and re.search(r"\bglobal_store_dword\b", body)
    assert not re.search(r"\bflat_", body) and "scratch_" not in body


# ------------------------------------------------------------------------------------------------------------ GPU: the kernel
def _env(n, seed=5, steps=15, gravity=None, randomise=True):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    cfg.domain_rand.randomize_base_mass = randomise
    cfg.domain_rand.randomize_base_com = randomise
    cfg.domain_rand.randomize_gripper_mass = randomise
    if gravity is not None:
        cfg.sim.gravity = list(gravity)
    env = WidowGo1(cfg, sim_device="cuda:0", seed=seed)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    for _ in range(steps):                                                    # leave the reset pose
        env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
    return env


def _random_nudot(n, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    nd = (torch.rand(n, 26, device="cuda", generator=g) * 2 - 1)
    nd[:, :6] *= 10.0
    nd[:, 6:] *= 50.0
    return nd.contiguous()


def _reference(env, envs, nudot=None, still=False):
    """(tau [len(envs), 26], mag) of the restatement at the sim's downloaded fp32 state; still: nu = 0 (the gravity term)."""
    m = env.robot_model
    root = env.root_states.cpu().numpy().astype(np.float64)
    q, qd = env.dof_pos.cpu().numpy().astype(np.float64), env.dof_vel.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    nd = None if nudot is None else nudot.cpu().numpy().astype(np.float64)
    g = [float(x) for x in env.tcfg.gravity]
    out = [idr.inverse_dynamics(m, root[e, :3], root[e, 3:7], q[e], np.zeros(26) if still else np.r_[root[e, 7:13], qd[e]],
                                None if nd is None else nd[e], bp[e], g) for e in envs]
    return np.array([t for t, _ in out]), np.array([mg for _, mg in out])


def _ratio(got, ref, mag):
    """Largest |got - ref| / (2^-24 mag); rows whose magnitude is 0 (the locked fingers) must be exactly 0."""
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    return float((np.abs(got - ref)[~zero] / (EPS * mag[~zero])).max())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 1000])
def test_kernel_matches_reference_elementwise(n):
    """h, tau for a random nudot and g(q), every env and every row; the measured ratios stand next to C_ID."""
    env = _env(n, gravity=(0.7, -1.3, -9.5) if n == 64 else None) if n > 1 else _env(1, seed=9, steps=5)
    if n > 1:
        bp = env.sim.tensor("BODY_PARAMS").cpu().numpy()
        assert np.ptp(bp[:, 0]) > 0 and np.ptp(bp[:, 1:4], axis=0).max() > 0 and np.ptp(bp[:, 10]) > 0    # randomised per env
    nudot = _random_nudot(n, 17)
    h, tau, grav = env.inverse_dynamics(), env.inverse_dynamics(nudot), env.gravity_forces()
    torch.cuda.synchronize()
    ratios = {}
    for name, got, kw in (("h", h, {}), ("tau", tau, dict(nudot=nudot)), ("grav", grav, dict(still=True))):
        got = got.cpu().numpy().astype(np.float64)
        ref, mag = _reference(env, range(n), **kw)
        assert np.all(got[:, FINGERS] == 0)
        assert name == "grav" or np.all(mag[:, LIVE].max(axis=0) > 0)                # every live row is exercised
        ratios[name] = _ratio(got, ref, mag)
    print(f"inverse dynamics n={n}: largest |kernel - ref| / (2^-24 mag): {ratios}")
    assert max(ratios.values()) <= C_ID, ratios


@pytest.mark.gpu
def test_consistent_with_the_mass_matrix_kernel():
    """inverse_dynamics(nudot) - bias_forces == mm_whole @ nudot at 4096 envs, in fp64 from the three fp32 tensors; the measured ratios stand next to C_MM."""
    n = 4096
    env = _env(n, seed=3, steps=10)
    nudot = _random_nudot(n, 23)
    env.refresh_mass_matrix_tensors(); env.refresh_bias_force_tensors()
    tau = env.inverse_dynamics(nudot)
    torch.cuda.synchronize()
    diff = (tau.double() - env.bias_forces.double() - torch.einsum("nij,nj->ni", env.mm_whole.double(), nudot.double())).abs()
    share = torch.einsum("nij,nj->ni", env.mm_whole.double().abs(), nudot.double().abs())
    assert bool(torch.isfinite(tau).all()) and bool(torch.isfinite(env.bias_forces).all()) and bool(torch.isfinite(diff).all())
    assert bool((tau[:, FINGERS] == 0).all()) and bool((env.bias_forces[:, FINGERS] == 0).all())
    envs = sorted(set(range(0, n, 37)) | {n - 1})
    _, mag1 = _reference(env, envs, nudot=nudot)
    _, mag0 = _reference(env, envs)
    d, s = diff[envs].cpu().numpy(), share[envs].cpu().numpy()
    zero = s == 0
    assert np.all(d[zero] == 0)
    print(f"mass-matrix consistency: largest diff / (2^-24 |mm| @ |nudot|) = {(d[~zero] / (EPS * s[~zero])).max():.4g}, "
          f"largest diff / (2^-24 (mag(nudot) + mag(0))) = {(d[~zero] / (EPS * (mag1 + mag0)[~zero])).max():.4g}")
    assert np.all(d <= EPS * (C_ID * (mag1 + mag0) + C_MM * s)), float((d / np.maximum(EPS * (C_ID * (mag1 + mag0) + C_MM * s), 1e-300)).max())


def _airborne_env(robot, n=64, shift=(0.0, 0.0, 0.0)):
    """n envs with default body parameters holding the airborne states of the CPU test (seeds 0..n-1), moved by `shift`."""
    env = _env(n, seed=2, steps=2, randomise=False)
    m = env.robot_model
    states = [_airborne_state(m, seed) for seed in range(n)]
    root = env.sim.tensor("ROOT_STATES").clone()
    dof = env.sim.tensor("DOF_STATE").clone()
    for e, (pos, quat, q, qd, v, w, _tau) in enumerate(states):
        root[e, 0] = torch.tensor(np.concatenate([pos + np.asarray(shift), quat, v, w]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q, qd], -1), dtype=torch.float32)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    torch.cuda.synchronize()
    return env, states


@pytest.mark.gpu
def test_inverse_of_the_oracle_forward_dynamics(robot):
    n = 64
    env, states = _airborne_env(robot, n)
    root = env.root_states.cpu().numpy().astype(np.float64)
    q, qd = env.dof_pos.cpu().numpy().astype(np.float64), env.dof_vel.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    o = _rigid_oracle(robot)
    np.testing.assert_allclose(bp, np.broadcast_to(o.get("BODY_PARAMS"), bp.shape), rtol=1e-6, atol=1e-9)   # default body parameters
    nudot = np.zeros((n, 26))
    for e in range(n):
        o.set("BODY_PARAMS", bp[e][None])
        a0, qdd = _oracle_accelerations(o, root[e], q[e], qd[e], states[e][6])
        nudot[e] = np.r_[a0, qdd]
    nd = torch.tensor(nudot, dtype=torch.float32, device="cuda")
    tau = env.inverse_dynamics(nd).cpu().numpy().astype(np.float64)
    _, mag = _reference(env, range(n), nudot=nd)
    assert np.isfinite(tau).all() and np.all(tau[:, FINGERS] == 0)
    for e in range(n):
        want = np.r_[np.zeros(6), states[e][6]]
        bound = C_ID * EPS * mag[e] + 1e-4 * max(1.0, np.abs(want).max())
        assert np.all(np.abs(tau[e] - want)[LIVE] <= bound[LIVE]), (e, np.abs(tau[e] - want).max())


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    n = 64
    nudot = _random_nudot(n, 29)
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = _airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        tau, grav = env.inverse_dynamics(nudot), env.gravity_forces()
        torch.cuda.synchronize()
        outs.append((tau.clone(), grav.clone()))
    assert bool(outs[0][0].abs().sum() > 0) and bool(outs[0][1].abs().sum() > 0)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.gpu
def test_persistent_tensor_partial_outputs_and_argument_errors():
    n = 1000
    env = _env(n, seed=4, steps=3)
    hb = env.bias_forces
    assert env.bias_forces is hb and hb.shape == (n, 26)
    arm_view = hb[:, -8:-2]                                                   # a view taken before the refresh
    env.refresh_bias_force_tensors()
    h0 = arm_view.clone()
    env.step(torch.randn(n, 18, device="cuda"))
    env.refresh_bias_force_tensors()
    assert not torch.equal(arm_view, h0) and torch.equal(arm_view, env.bias_forces[:, -8:-2])
    assert torch.equal(env.inverse_dynamics(), hb)
    # one output at a time: the other buffer keeps its sentinel; both at once give the same values
    T = torch.full_like(hb, 12345.0); G = torch.full_like(hb, 12345.0)
    env.sim.inverse_dynamics(tau=T)
    torch.cuda.synchronize()
    assert torch.equal(T, hb) and bool((G == 12345.0).all())
    T.fill_(12345.0)
    env.sim.inverse_dynamics(grav=G)
    torch.cuda.synchronize()
    assert torch.equal(G, env.gravity_forces()) and bool((T == 12345.0).all())
    T2, G2 = torch.empty_like(hb), torch.empty_like(hb)
    env.sim.inverse_dynamics(tau=T2, grav=G2)
    assert torch.equal(T2, hb) and torch.equal(G2, G)
    # zeros for nudot are the same as no nudot; the fingers' entries of nudot are ignored
    nd = torch.zeros_like(hb); nd[:, FINGERS] = 7.0
    assert torch.equal(env.inverse_dynamics(nd), hb)
    # argument errors
    L = env.sim.L
    T.fill_(12345.0); G.fill_(12345.0)
    assert L.wbc_sim_inverse_dynamics(env.sim.h, None, None, None, None) == -1 and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_inverse_dynamics(None, None, T.data_ptr(), G.data_ptr(), None) == -1
    assert L.wbc_sim_inverse_dynamics(env.sim.h, None, T.data_ptr() + 2, None, None) == -1 and b"aligned" in L.wbc_last_error()
    assert L.wbc_sim_inverse_dynamics(env.sim.h, nd.data_ptr() + 1, T.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert bool((T == 12345.0).all()) and bool((G == 12345.0).all())
    # 4-byte alignment is all that is needed: an output one float into a buffer
    big = torch.full((n * 26 + 1,), 12345.0, device="cuda")
    assert L.wbc_sim_inverse_dynamics(env.sim.h, None, big.data_ptr() + 4, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(big[1:].view(n, 26), hb) and float(big[0]) == 12345.0


@pytest.mark.gpu
def test_step_is_untouched_by_refreshes():
    n = 64
    finals = []
    for refresh in (False, True):
        env = _env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        for _ in range(5):
            if refresh:
                env.refresh_bias_force_tensors()
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if refresh:
                env.refresh_bias_force_tensors(); env.gravity_forces()
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
