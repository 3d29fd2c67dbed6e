"""Whole-body Jacobian [N, 27, 6, 26] and mass matrix [N, 26, 26] (wbc_sim_body_dynamics, csrc/wbc_arm_kernel.hip; definition in
include/wbc_sim.h). The CPU tests pin the fp64 restatement tests/whole_body_reference.py to finite differences, to the C oracle's
rigid-body velocities and to the arm restatement oracle/arm_osc_oracle.py; the GPU tests hold the kernel to that restatement, to
the step kernel's rigid-body state and to wbc_sim_arm_dynamics, through the reference's own slicing expressions."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import arm_codegen
import arm_osc_oracle as ao
import whole_body_reference as wb
from wbc_amd import abi

FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(wb.NCOL) if c not in FINGERS]


def _random_pose(rng, far=False):
    quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
    pos = rng.normal(size=3) + (np.array([3.0, 110.0, 0.0]) if far else 0.0)
    q = rng.uniform(-1, 1, 20); q[18:] = rng.uniform(-0.03, 0.03, 2)
    return pos, quat, q


def _quat_mul(a, b):             # xyzw
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _structure(m):
    """Masks of the entries that are zero by construction: J [27, 6, 26], M [26, 26]."""
    dof_body = wb.dof_body(m)
    J = np.zeros((m.num_rigid_bodies, 6, wb.NCOL), dtype=bool)
    for r, b in enumerate(m.rb_body):
        anc = wb.ancestors(m, b)
        J[r, 3:6, 0:3] = True                                          # v_root moves no body's orientation
        for k in range(3):
            J[r, k, [c for c in range(3) if c != k]] = True            # ... and the origin along the identity only
            J[r, k, 3 + k] = True                                      # (e_k x d)_k
            J[r, 3 + k, [3 + c for c in range(3) if c != k]] = True
        for dof, bj in enumerate(dof_body):
            if bj < 0 or bj not in anc:
                J[r, :, 6 + dof] = True
    M = np.zeros((wb.NCOL, wb.NCOL), dtype=bool)
    M[FINGERS, :] = True; M[:, FINGERS] = True
    for i, bi in enumerate(dof_body):
        for j, bj in enumerate(dof_body):
            if bi >= 0 and bj >= 0 and bi not in wb.ancestors(m, bj) and bj not in wb.ancestors(m, bi):
                M[6 + i, 6 + j] = True
    return J, M


# ------------------------------------------------------------------------------------------------------------ CPU: restatement
def test_reference_jacobian_matches_finite_differences():
    m = abi.load_default_model()
    rng = np.random.default_rng(0)
    h = 1e-6
    for trial in range(4):
        pos, quat, q = _random_pose(rng, far=trial % 2 == 1)
        J = wb.jacobian(m, pos, quat, q)

        def poses(dp=np.zeros(3), dquat=None, dq=np.zeros(20)):
            qu = quat if dquat is None else _quat_mul(dquat, quat)
            return wb.rigid_body_poses(m, pos + dp, qu, q + dq)
        for c in range(wb.NCOL):
            if c < 3:
                e = np.eye(3)[c] * h
                (p1, R1), (p0, R0) = poses(dp=e), poses(dp=-e)
            elif c < 6:                                                # a world-frame rotation of the root by +-h about axis c-3
                ax = np.eye(3)[c - 3]
                (p1, R1) = poses(dquat=np.r_[np.sin(h / 2) * ax, np.cos(h / 2)])
                (p0, R0) = poses(dquat=np.r_[-np.sin(h / 2) * ax, np.cos(h / 2)])
            else:
                e = np.zeros(20); e[c - 6] = h
                (p1, R1), (p0, R0) = poses(dq=e), poses(dq=-e)
            np.testing.assert_allclose((p1 - p0) / (2 * h), J[:, 0:3, c], atol=2e-6)
            W = np.einsum("rij,rkj->rik", (R1 - R0) / (2 * h), 0.5 * (R0 + R1))         # [omega]x per rigid body
            np.testing.assert_allclose(np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], 1), J[:, 3:6, c], atol=2e-6)
        Js, _ = _structure(m)
        assert np.all(J[Js] == 0) and np.all(J[:, :, FINGERS] == 0)


def test_reference_velocities_match_the_oracle_rigid_body_state(robot):
    from oracle import OracleSim
    m, n = robot["model"], 6
    rng = np.random.default_rng(1)
    o = OracleSim(robot["wmodel"], robot["tcfg"], n, seed=1)
    root, dof = o.get("ROOT_STATES"), o.get("DOF_STATE")
    poses = [_random_pose(rng, far=e % 2 == 0) for e in range(n)]
    for e, (pos, quat, q) in enumerate(poses):
        root[e, 0, 0:3], root[e, 0, 3:7], root[e, 0, 7:13] = pos, quat, rng.normal(size=6)
        dof[e, :, 0], dof[e, :, 1] = q, rng.normal(size=20) * 3
    o.set("ROOT_STATES", root); o.set("DOF_STATE", dof)
    o.refresh_rigid_body_state()
    rbs = o.get("RIGID_BODY_STATE")[:, :m.num_rigid_bodies]
    # the oracle reads the float32 tables of wbc_model, the restatement the float64 RobotModel: ~1e-8 relative on every offset
    for e, (pos, quat, q) in enumerate(poses):
        p, R = wb.rigid_body_poses(m, pos, quat, q)
        np.testing.assert_allclose(rbs[e, :, 0:3], p, atol=5e-8)
        np.testing.assert_allclose(np.array([ao.quat_to_mat(x) for x in rbs[e, :, 3:7]]), R, atol=1e-9)
        nu = np.r_[root[e, 0, 7:13], dof[e, :, 1]]
        np.testing.assert_allclose(wb.jacobian(m, pos, quat, q) @ nu, rbs[e, :, 7:13], atol=1e-6)


def test_reference_mass_matrix_properties_and_arm_block():
    m = abi.load_default_model()
    rng = np.random.default_rng(2)
    n = 4
    bp = abi.body_params_from_randomisation(m, rng.uniform(-0.5, 2.5, n), rng.uniform(-0.1, 0.1, (n, 3)),
                                            rng.uniform(0, 0.1, n)).astype(np.float64)
    _, Ms = _structure(m)
    gripper_rb = m.rb_names.index("wx250s/ee_gripper_link")
    link_rb = list(range(m.num_rigid_bodies - 9, m.num_rigid_bodies))
    for e in range(n):
        pos, quat, q = _random_pose(rng, far=e % 2 == 1)
        M = wb.mass_matrix(m, pos, quat, q, bp[e])
        np.testing.assert_allclose(M, M.T, atol=1e-12)
        assert np.all(M[Ms] == 0)
        assert np.all(np.linalg.eigvalsh(M[np.ix_(LIVE, LIVE)]) > 1e-6)
        for _ in range(3):
            v, w, qd = rng.normal(size=3), rng.normal(size=3), rng.normal(size=20) * 2
            nu = np.r_[v, w, qd]
            ke = wb.kinetic_energy(m, pos, quat, q, v, w, qd, bp[e])
            assert 0.5 * nu @ M @ nu == pytest.approx(ke, rel=1e-12)
        Ma, Ja, _ = ao.arm_quantities(m, pos, quat, q, gripper_rb, link_rb, m.rb_mass[-9:],
                                      gripper_params=(bp[e, 10], bp[e, 11:14], bp[e, 14:20]))
        np.testing.assert_allclose(M[-8:-2, -8:-2], Ma, atol=1e-12)
        np.testing.assert_allclose(wb.jacobian(m, pos, quat, q)[gripper_rb, :, -8:-2], Ja, atol=1e-12)


def test_body_dynamics_kernel_codegen():
    """No scratch, no flat memory instructions, and every global store is a 16-byte-per-lane store (the sweeps' coalesced rows)."""
    assert arm_codegen.meta("wbc_body_dynamics_kernel", "private_segment_fixed_size") == 0
    # static LDS (+ 5.6 KB dynamic for the J chunk when J is written): 15 envs per CU either way
    assert arm_codegen.meta("wbc_body_dynamics_kernel", "group_segment_fixed_size") + 9 * 156 * 4 <= 160 * 1024 // 15
    body = arm_codegen.body("wbc_body_dynamics_kernel", end="s_endpgm")
    assert not re.search(r"\bflat_(load|store)", body) and "scratch_" not in body
    stores = re.findall(r"\bglobal_store_\w+", body)
    assert stores and set(stores) == {"global_store_dwordx4"}


def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 8)()
    assert L.wbc_sim_body_dynamics(None, C.addressof(buf), C.addressof(buf), None) == -1
    assert b"NULL" in L.wbc_last_error()


# ------------------------------------------------------------------------------------------------------------ GPU: the kernel
def _env(n, seed=5, steps=15):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    cfg.domain_rand.randomize_base_mass = True
    cfg.domain_rand.randomize_base_com = True
    cfg.domain_rand.randomize_gripper_mass = True
    env = WidowGo1(cfg, sim_device="cuda:0", seed=seed)
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    for _ in range(steps):                                                    # leave the reset pose
        env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
    return env


def _check_against_reference(env, envs):
    m = env.robot_model
    env.refresh_jacobian_tensors(); env.refresh_mass_matrix_tensors()
    torch.cuda.synchronize()
    J, M = env.jacobian_whole.cpu().numpy(), env.mm_whole.cpu().numpy()
    root, dof = env.root_states.cpu().numpy().astype(np.float64), env.dof_pos.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    assert np.isfinite(J).all() and np.isfinite(M).all()
    Js, Ms = _structure(m)
    for e in envs:
        Jr = wb.jacobian(m, root[e, :3], root[e, 3:7], dof[e])
        Mr = wb.mass_matrix(m, root[e, :3], root[e, 3:7], dof[e], bp[e])
        assert np.all(np.abs(J[e] - Jr) <= 5e-6 + 1e-4 * np.abs(Jr)), (e, np.abs(J[e] - Jr).max())
        assert np.abs(M[e] - Mr).max() <= 1e-5 * np.abs(Mr).max(), (e, np.abs(M[e] - Mr).max())
        assert np.all(J[e][Js] == 0) and np.all(M[e][Ms] == 0)
    assert np.all(J[:, :, :, FINGERS] == 0) and np.all(M[:, FINGERS, :] == 0) and np.all(M[:, :, FINGERS] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1000])
def test_kernel_matches_reference(n):
    env = _env(n)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy()
    assert np.ptp(bp[:, 0]) > 0 and np.ptp(bp[:, 1:4], axis=0).max() > 0 and np.ptp(bp[:, 10]) > 0    # randomised per env
    _check_against_reference(env, range(n) if n <= 64 else sorted(set(range(0, n, 37)) | {n - 1}))


@pytest.mark.gpu
def test_single_env():
    _check_against_reference(_env(1, seed=9, steps=5), [0])


@pytest.mark.gpu
def test_jacobian_reproduces_rigid_body_velocities_at_4096_envs():
    n = 4096
    env = _env(n, seed=3, steps=10)
    env.sim.refresh_rigid_body_state()
    env.refresh_jacobian_tensors()
    nu = torch.cat([env.root_states[:, 7:13], env.dof_vel], 1)
    v = torch.einsum("nrkc,nc->nrk", env.jacobian_whole.double(), nu.double())
    rbv = env.rigid_body_state[:, :27, 7:13].double()
    scale = rbv.abs().flatten(1).max(1).values
    err = (v - rbv).abs().flatten(1).max(1).values
    assert bool(torch.isfinite(v).all()) and float(scale.min()) > 0
    assert bool((err <= 1e-4 * scale).all()), float((err / scale).max())


@pytest.mark.gpu
def test_reference_expressions_reproduce_the_arm_entry_point():
    env = _env(256, seed=11)
    m = env.robot_model
    env.refresh_jacobian_tensors(); env.refresh_mass_matrix_tensors()
    mm_ref = env.mm_whole[:, -8:-2, -8:-2]                                           # WG:558
    ee_ref = env.jacobian_whole[:, env.gripper_idx, :6, -8:-2]                       # WG:557
    link_mass = torch.tensor(np.asarray(m.rb_mass[-9:], dtype=np.float64), dtype=torch.float, device="cuda")
    link_mass[env._arm_link_rb.index(env.gripper_idx)] += env.mass_params_tensor[0, 4]   # env 0's properties (WG:664-670)
    g = torch.zeros(env.num_envs, 9, 6, 1, device="cuda"); g[:, :, 2, :] = 9.81
    g_force = link_mass.view(1, 9, 1, 1) * g
    g_torque = (torch.transpose(env.jacobian_whole[:, -9:, :, -8:], 2, 3) @ g_force).squeeze(-1)     # WG:1204-1205
    g_torque = torch.sum(g_torque, dim=1)[:, :6]
    mm, ee, gt = env.get_arm_mm(), env.get_ee_jac(), env.get_g_torques()
    torch.testing.assert_close(mm_ref, mm, rtol=2e-4, atol=2e-6)
    torch.testing.assert_close(ee_ref, ee, rtol=1e-4, atol=2e-6)
    torch.testing.assert_close(g_torque, gt, rtol=2e-4, atol=2e-5)


@pytest.mark.gpu
def test_persistent_tensors_partial_outputs_and_null_arguments():
    n = 1000
    env = _env(n, seed=4, steps=3)
    jw, mw = env.jacobian_whole, env.mm_whole
    assert env.jacobian_whole is jw and env.mm_whole is mw
    assert jw.shape == (n, 27, 6, 26) and mw.shape == (n, 26, 26)
    ee_view, mm_view = jw[:, env.gripper_idx, :6, -8:-2], mw[:, -8:-2, -8:-2]       # views taken before the refresh
    env.refresh_jacobian_tensors(); env.refresh_mass_matrix_tensors()
    ee0, mm0 = ee_view.clone(), mm_view.clone()
    env.step(torch.randn(n, 18, device="cuda"))
    env.refresh_jacobian_tensors(); env.refresh_mass_matrix_tensors()
    assert not torch.equal(ee_view, ee0) and not torch.equal(mm_view, mm0)
    assert torch.equal(ee_view, env.jacobian_whole[:, env.gripper_idx, :6, -8:-2]) and torch.equal(mm_view, env.mm_whole[:, -8:-2, -8:-2])
    # one output at a time: the other buffer keeps its sentinel
    J = torch.full_like(jw, 12345.0); M = torch.full_like(mw, 12345.0)
    env.sim.body_dynamics(jac=J)
    torch.cuda.synchronize()
    assert torch.equal(J, jw) and bool((M == 12345.0).all())
    J.fill_(12345.0)
    env.sim.body_dynamics(mm=M)
    torch.cuda.synchronize()
    assert torch.equal(M, mw) and bool((J == 12345.0).all())
    # NULL arguments
    L = env.sim.L
    assert L.wbc_sim_body_dynamics(env.sim.h, None, None, None) == -1 and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_body_dynamics(None, J.data_ptr(), M.data_ptr(), None) == -1
    assert L.wbc_sim_body_dynamics(env.sim.h, J.data_ptr() + 4, None, None) == -1
    torch.cuda.synchronize()
    assert bool((J == 12345.0).all())
