"""Whole-body Jacobian [N, 27, 6, 26] and mass matrix [N, 26, 26] (wbc_sim_body_dynamics, csrc/wbc_arm_kernel.hip; definition in
include/wbc_sim.h). The CPU tests pin the fp64 restatement tests/whole_body_reference.py to finite differences, to the C oracle's
rigid-body velocities and to the arm restatement oracle/arm_osc_oracle.py; the GPU tests hold the kernel to that restatement, to
the step kernel's rigid-body state and to wbc_sim_arm_dynamics, through the reference's own slicing expressions.

Per-entry bound (the siblings' convention): every entry of J and M satisfies |kernel - ref| <= C 2^-24 mag, mag the rotation-invariant
magnitude of tests/body_dynamics_reference.py (tree path lengths for J, norms of the per-body blocks about the root origin for M); where
mag is 0 the entry is structure and kernel and reference are EQUAL. C = 4 K_ref rounded up to a power of two (at least 8, at most 4096),
K_ref the fp32 yardstick's largest ratio over 64 near, 64 far and the 8 edge states in the larger of its two formulations (world-axes
per-body sum, base-frame composites), measured on the CPU and asserted there. C never follows the kernel; the kernel's column is what an
MI355X gave, printed by the GPU tests:

    output   K_ref    C     kernel's largest ratio (n, env, entry)
    J        10.3     64    23.5  (n = 64, env 50, J[23, 0, 22])
    M        3.07     16    3.36  (n = 64, env 25, M[2, 2])

(n = 1: J 7.49, M 1.30; n = 13: J 12.0, M 2.55.) No entry needed a cancellation argument, and the kernel is unchanged.

The old allowances on the same states: M 1e-5 max|M_ref|, about 1.5e-4 on every entry, where the new one, 16 2^-24 mag, is at most 2.7e-5
(the root's linear block) and 2.7e-7 on the wrist diagonals of 0.003 kg m^2: 6.05 x to 24 500 x below the old one, entry by entry. J
5e-6 + 1e-4 |J_ref|, where the new one is 3.8e-6 on the angular rows and at most 3.3e-6 (64 2^-24 x the 0.86 m from the root to a foot)
on the linear ones: 1.31 x to 46 x below it. test_new_allowances_lie_below_the_old_ones_on_every_entry asserts that on every entry with
a magnitude; the old checks stay as they are.

State families: member `seed` of near / far is test_inverse_dynamics._random_state (arbitrary attitudes; far: the root near (3, 110, 0))
with random body params; the edge family is q = 0 under the identity and the three 180 degree turns, every joint on its lower and on its
upper limit, and a state with its copy under the negated root quaternion. In the GPU cases env e holds member e of the near (e even) or
far (e odd) family; from n = 9 on the last 8 envs hold the edge family instead.
"""
import copy
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import arm_codegen
import arm_osc_oracle as ao
import body_dynamics_reference as bd
import whole_body_reference as wb
from wbc_amd import abi

FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(wb.NCOL) if c not in FINGERS]
EPS = bd.EPS
SENTINEL = 12345.0
FRAME = 8                                        # sentinel floats on either side of an output (32 bytes: the 16-byte alignment holds)
# K_ref per output of both kernels (the docstring's tables here and in tests/test_arm_osc.py) and the constants they give
K_REF = {"J": 10.3, "M": 3.07, "mm": 1.69, "ee": 5.70, "g": 7.10}
CONST = {"J": 64.0, "M": 16.0, "mm": 8.0, "ee": 32.0, "g": 32.0}
assert all(CONST[f] == max(8.0, 2.0 ** np.ceil(np.log2(4 * K_REF[f]))) and CONST[f] <= 4096 for f in bd.OUTPUTS)
# the allowances of _check_against_reference below, restated
OLD_M_REL, OLD_J_ABS, OLD_J_REL = 1e-5, 5e-6, 1e-4


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


# ------------------------------------------------------------------------------------------------------------ CPU: the per-entry bound
@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _member(seed, far):
    """(pos, quat, q, nu, body_params) of member `seed` of the near or the far family."""
    import test_inverse_dynamics as tid
    rng = np.random.default_rng(7300 + 1000 * int(far) + seed)
    pos, quat, q, nu = tid._random_state(rng, far=far)
    return pos, quat, q, nu, tid._random_body_params(_model(), rng)


@functools.lru_cache(maxsize=None)
def _edge_states():
    """The 8 members of the edge family; the last two differ in the sign of the root quaternion alone."""
    import test_inverse_dynamics as tid
    m = _model()
    rng = np.random.default_rng(7299)
    zero = np.zeros(26)
    out = []
    for quat in ([0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]):                 # identity, 180 degrees about x, y, z
        out.append((np.array([0.3, -0.2, 0.5]), np.array(quat, dtype=np.float64), np.zeros(20), zero, tid._random_body_params(m, rng)))
    for limit, far in ((m.dof_lower, False), (m.dof_upper, True)):
        pos, quat, _, _ = tid._random_state(rng, far=far)
        out.append((pos, quat, np.array(limit, dtype=np.float64), zero, tid._random_body_params(m, rng)))
    pos, quat, q, _ = tid._random_state(rng)
    bp = tid._random_body_params(m, rng)
    out += [(pos, quat, q, zero, bp), (pos, -quat, q, zero, bp)]
    return tuple(out)


def _states(n):
    """The states of the n envs of a GPU case."""
    states = [_member(e, far=e % 2 == 1) for e in range(n)]
    if n > len(_edge_states()):
        states[n - len(_edge_states()):] = _edge_states()
    return states


def _yardstick_states():
    return [_member(s, far) for far in (False, True) for s in range(64)] + list(_edge_states())


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """{output: (K_ref of the world-axes sum, K_ref of the base-frame composites)} over the 64 + 64 + 8 states."""
    m = _model()
    k = {f: [0.0, 0.0] for f in bd.OUTPUTS}
    for pos, quat, q, _, bp in _yardstick_states():
        out, mag = bd.reference(m, pos, quat, q, bp)
        for i, y in enumerate((bd.yardstick_world(m, quat, q, bp), bd.yardstick_base(m, quat, q, bp))):
            for f in bd.OUTPUTS:
                k[f][i] = max(k[f][i], bd.ratio(y[f], out[f], mag[f])[0])
    return {f: tuple(v) for f, v in k.items()}


def _assert_yardsticks(outputs):
    k = _yardsticks()
    print("body dynamics yardsticks: " + ", ".join(f"{f} K_ref = max(world {k[f][0]:.3g}, base {k[f][1]:.3g}) (C = {CONST[f]:g})" for f in outputs))
    for f in outputs:
        assert abs(max(k[f]) - K_REF[f]) <= 0.25 * K_REF[f], (f, k[f])      # a largest ratio moves with the summation order of the BLAS at hand
        assert 4 * max(k[f]) <= CONST[f] <= 4096


def test_fp32_yardsticks_are_the_ones_the_constants_were_taken_from():
    _assert_yardsticks(("J", "M"))


def test_magnitudes_cover_the_structure_and_do_not_turn_with_the_root():
    """mag == 0 exactly on the masks of _structure, the finger columns, the identity parts of the root columns and a joint's lever to a
    rigid body at its own origin, and the reference is EQUAL to its structural value there; mag_M does not move when the whole robot
    is turned; both yardstick formulations, evaluated in fp64, are the reference."""
    m = _model()
    Js, Ms = _structure(m)
    magJ = bd.jacobian_magnitude(m)
    ident = np.zeros_like(Js)
    ident[:, 0:3, 0:3] = ident[:, 3:6, 3:6] = True
    own = np.zeros_like(Js)                                          # rigid bodies at the origin of their own moving body: no lever
    for r, b in enumerate(m.rb_body):
        if b > 0 and not np.any(m.rb_offset[r]):
            own[r, 0:3, 6 + m.body_dof[b]] = True
    assert own.sum() == 3 * 18                                       # 12 leg links and 6 arm links
    no_lever = (bd.lever_paths(m)[:, None, :] == 0) & (np.arange(6) < 3)[None, :, None]      # own, and the root columns of base and trunk
    assert np.all(no_lever[own]) and np.array_equal(magJ == 0, Js | ident | no_lever)
    assert magJ[:, 3:6].max() == 1.0 and 0.8 < magJ[:, 0:3].max() < 0.9          # the longest path: root origin to a foot, metres
    rng = np.random.default_rng(12)
    for pos, quat, q, _, bp in [_member(0, False), _member(1, True)] + list(_edge_states()):
        out, mag = bd.reference(m, pos, quat, q, bp)
        assert np.array_equal(mag["M"] == 0, Ms) and np.array_equal(mag["M"], mag["M"].T)
        assert np.all(out["M"][Ms] == 0) and np.all(out["J"][Js | own] == 0) and np.all(out["J"][:, :, FINGERS] == 0)
        assert np.all(out["J"][:, 0:3, 0:3] == np.eye(3)) and np.all(out["J"][:, 3:6, 3:6] == np.eye(3))
        turn = rng.normal(size=4); turn /= np.linalg.norm(turn)
        _, mag2 = bd.reference(m, pos + 7.0, _quat_mul(turn, quat), q, bp)
        assert np.abs(mag2["M"] - mag["M"]).max() <= 1e-13 * mag["M"].max()
        assert np.array_equal(mag2["J"], mag["J"]) and np.abs(mag2["g"] - mag["g"]).max() == 0
        for y in (bd.yardstick_world(m, quat, q, bp, dtype=np.float64), bd.yardstick_base(m, quat, q, bp, dtype=np.float64)):
            for f in bd.OUTPUTS:
                # the reference forms its levers from world coordinates, |y| = 110 m in the far family: 2^-53 x 110 m per operation
                # against levers of centimetres. 2^-15 of the unit the bounds are counted in.
                assert bd.ratio(y[f], out[f], mag[f])[0] <= 2.0 ** -15, f


def test_new_allowances_lie_below_the_old_ones_on_every_entry():
    """C 2^-24 mag against 1e-5 max|M_ref| and 5e-6 + 1e-4 |J_ref| on every entry of every state of the families: the old checks are kept,
    and nothing they constrained is constrained less."""
    m = _model()
    least = {"J": np.inf, "M": np.inf}
    most = {"J": 0.0, "M": 0.0}
    for pos, quat, q, _, bp in _yardstick_states()[::4] + list(_edge_states()):
        out, mag = bd.reference(m, pos, quat, q, bp)
        old = {"M": np.full((26, 26), OLD_M_REL * np.abs(out["M"]).max()), "J": OLD_J_ABS + OLD_J_REL * np.abs(out["J"])}
        for f in ("J", "M"):
            live = mag[f] > 0
            r = old[f][live] / (CONST[f] * EPS * mag[f][live])
            least[f], most[f] = min(least[f], float(r.min())), max(most[f], float(r.max()))
    print(f"old allowance / new allowance per entry: J {least['J']:.3g} .. {most['J']:.3g}, M {least['M']:.3g} .. {most['M']:.3g}")
    assert least["J"] > 1 and least["M"] > 1


def _wrong_models():
    """The five model errors of the checker's self-test: (name, model)."""
    def changed(field, edit):
        a = copy.deepcopy(_model())
        x = np.array(getattr(a, field), dtype=np.float64)
        edit(x)
        setattr(a, field, x)
        return a

    def scale(x): x[16:19] *= 1.04
    def permute(x): x[16:19, 0:3] = np.roll(x[16:19, 0:3], 1, axis=1)
    def arm_products(x): x[13:19, 3:6] = 0.0
    def com(x): x[16:19, 0] += 1e-3
    def leg_products(x): x[1:13, 3:6] = 0.0
    return [("last 3 arm bodies' rotational inertia x 1.04", changed("inertia", scale)),
            ("their Ixx / Iyy / Izz permuted", changed("inertia", permute)),
            ("arm products of inertia dropped", changed("inertia", arm_products)),
            ("last 3 bodies' centre of mass moved 1 mm", changed("com", com)),
            ("leg products of inertia dropped", changed("inertia", leg_products))]


def test_the_checker_rejects_wrong_models():
    """A wrong model's fp64 M (and J) goes through bd.ratio in the kernel's place, on 8 near states with the model's own body parameters.
    Every error is rejected by at least 100 C. Smallest new ratio over the states (units of 2^-24 mag; C_M = 16), and what the old
    bound max|M - M_ref| <= 1e-5 max|M_ref| made of it (largest excess over the states; <= 1 passes):

        last 3 arm bodies' rotational inertia x 1.04      9 500      0.95 (passed)
        their Ixx / Iyy / Izz permuted                     6 500      1.5
        arm products of inertia dropped                   10 400      3.1
        last 3 bodies' centre of mass moved 1 mm          11 900      3.4
        leg products of inertia dropped                   25 800      4.9

    J: the rigid-body offset of the end effector moved along its x. By 40 um the new bound is exceeded 3 100 x 2^-24 mag (C_J = 64: 49
    allowances); the old one 5e-6 + 1e-4 |J_ref| is exceeded too, but by 3.5 allowances at the worst entry. By 4 um every entry passes
    the old bound (a change of at most 4e-6 against 5e-6: 0.35 allowances) and the new one rejects it by 310 x 2^-24 mag, 4.9 allowances."""
    m = _model()
    states = [_member(s, False)[0:3] for s in range(8)]
    refs = [bd.reference(m, *s) for s in states]
    for name, wrong in _wrong_models():
        new = min(bd.ratio(wb.mass_matrix(wrong, *s), out["M"], mag["M"])[0] for s, (out, mag) in zip(states, refs))
        old = max(np.abs(wb.mass_matrix(wrong, *s) - out["M"]).max() / (OLD_M_REL * np.abs(out["M"]).max()) for s, (out, _) in zip(states, refs))
        print(f"{name}: smallest ratio {new:.4g} x 2^-24 mag, old bound's largest excess {old:.3g}")
        assert new >= 100 * CONST["M"], name
    ee = m.rb_names.index(bd.EE_NAME)
    for shift, old_passes in ((40e-6, False), (4e-6, True)):
        wrong = copy.deepcopy(m)
        wrong.rb_offset = np.array(m.rb_offset, dtype=np.float64)
        wrong.rb_offset[ee, 0] += shift
        new, old = np.inf, 0.0
        for s, (out, mag) in zip(states, refs):
            Jw = wb.jacobian(wrong, *s)
            new = min(new, bd.ratio(Jw, out["J"], mag["J"])[0])
            old = max(old, float((np.abs(Jw - out["J"]) / (OLD_J_ABS + OLD_J_REL * np.abs(out["J"]))).max()))
        print(f"end-effector offset moved {shift * 1e6:g} um: smallest ratio {new:.4g} x 2^-24 mag, old bound's largest excess {old:.3g}")
        assert new > CONST["J"] and (old <= 1) == old_passes


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


# ------------------------------------------------------------------------------------------------------------ GPU: the per-entry bound
def _framed(numel):
    return torch.full((FRAME + numel + FRAME,), SENTINEL, dtype=torch.float32, device="cuda")


def _unframed(buf, shape, name):
    numel = int(np.prod(shape))
    assert bool((buf[:FRAME] == SENTINEL).all()) and bool((buf[FRAME + numel:] == SENTINEL).all()), f"{name}: written outside its {shape}"
    return buf[FRAME:FRAME + numel].view(shape).clone()


@functools.lru_cache(maxsize=None)
def _case(n):
    """An env whose robots hold _states(n), the fp64 reference and magnitudes of every env at the sim's DOWNLOADED fp32 state, and the link
    masses g_torque weighs with (env 0's randomised gripper mass on every env, WG:664-670). Computed once and left unchanged."""
    import test_coriolis as tc
    import test_inverse_dynamics as tid
    env = tid._env(n, seed=5, steps=0)
    tc._set_states(env, _states(n))
    r64, d64, b64 = st = tc._downloaded(env)
    m = env.robot_model
    link_mass = np.array(m.rb_mass[-9:], dtype=np.float64)
    link_mass[env._arm_link_rb.index(env.gripper_idx)] += float(env.mass_params_tensor[0, 4])
    refs = [bd.reference(m, r64[e, :3], r64[e, 3:7], d64[e, :, 0], b64[e], link_mass) for e in range(n)]
    return env, refs, st, link_mass


def _launch_body(env, which=("J", "M")):
    """A direct C-ABI call into sentinel-framed buffers: {name: [n, ...] tensor} of the outputs asked for."""
    n = env.num_envs
    shape = {"J": (n, 27, 6, 26), "M": (n, 26, 26)}
    bufs = {k: _framed(int(np.prod(shape[k]))) for k in which}
    ptr = lambda k: bufs[k].data_ptr() + 4 * FRAME if k in bufs else None
    rc = env.sim.L.wbc_sim_body_dynamics(env.sim.h, ptr("J"), ptr("M"), env.sim._stream())
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    return {k: _unframed(b, shape[k], k) for k, b in bufs.items()}


def _worst(got, refs, outputs, n):
    """{output: (largest ratio, env, entry)} of [n, ...] float64 arrays against the per-env references."""
    worst = {f: (0.0, 0, ()) for f in outputs}
    for e, (out, mag) in enumerate(refs):
        for f in outputs:
            r, at = bd.ratio(got[f][e], out[f], mag[f])
            if r > worst[f][0]:
                worst[f] = (r, e, at)
    print(f"n={n}: largest |kernel - ref| / (2^-24 mag): " + ", ".join(f"{f} {w[0]:.3g} (env {w[1]}, entry {w[2]}; C = {CONST[f]:g})" for f, w in worst.items()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_and_entry_of_J_and_M(n):
    env, refs, _, _ = _case(n)
    keys = ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")
    before = [env.sim.tensor(k).clone() for k in keys]
    got = _launch_body(env)
    J, M = got["J"].double().cpu().numpy(), got["M"].double().cpu().numpy()
    worst = _worst({"J": J, "M": M}, refs, ("J", "M"), n)                     # structural entries: equalities, inside bd.ratio
    for f, w in worst.items():
        assert w[0] <= CONST[f], (f, w)
    Js, Ms = _structure(env.robot_model)
    assert np.all(J[:, Js] == 0) and np.all(M[:, Ms] == 0) and np.all(J[:, :, :, FINGERS] == 0)
    # symmetry: bit for bit outside the 6 x 6 root block (both triangles are the same product), within the bound inside it
    outside = np.ones((26, 26), dtype=bool); outside[:6, :6] = False
    assert np.array_equal(M[:, outside], M.transpose(0, 2, 1)[:, outside])
    for e, (_, mag) in enumerate(refs):
        skew = np.abs(M[e, :6, :6] - M[e, :6, :6].T)
        assert np.all(skew <= CONST["M"] * EPS * mag["M"][:6, :6]), (e, float((skew / (EPS * mag["M"][:6, :6])).max()))
    # one output at a time has the bits of the joint call; the Python entry points are the same calls
    assert torch.equal(_launch_body(env, ("J",))["J"], got["J"]) and torch.equal(_launch_body(env, ("M",))["M"], got["M"])
    env.refresh_jacobian_tensors(); env.refresh_mass_matrix_tensors()
    torch.cuda.synchronize()
    assert torch.equal(env.jacobian_whole, got["J"]) and torch.equal(env.mm_whole, got["M"])
    # q and -q are the same attitude: the same bits
    if n > len(_edge_states()):
        assert torch.equal(got["J"][n - 2], got["J"][n - 1]) and torch.equal(got["M"][n - 2], got["M"][n - 1])
    # the sim's state is read, never written
    for k, t in zip(keys, before):
        assert torch.equal(env.sim.tensor(k), t), k


@pytest.mark.gpu
def test_translating_the_root_leaves_every_bit():
    env, _, _, _ = _case(64)
    want = _launch_body(env)
    root0 = env.sim.tensor("ROOT_STATES").clone()
    try:
        root = root0.clone(); root[:, 0, 0:3] += torch.tensor([-57.0, 23.0, 4.5], device="cuda")
        env.sim.set_root_state(root.contiguous())
        moved = _launch_body(env)
    finally:
        env.sim.set_root_state(root0.contiguous())
        torch.cuda.synchronize()
    for k in want:
        assert bool(want[k].abs().sum() > 0) and torch.equal(moved[k], want[k]), k
    assert all(torch.equal(v, want[k]) for k, v in _launch_body(env).items())
