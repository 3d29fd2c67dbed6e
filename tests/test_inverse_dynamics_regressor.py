"""Body-parameter regressor of whole-body inverse dynamics, tau = Y(q, nu, nudot) pi (wbc_sim_inverse_dynamics_regressor and
wbc_sim_forward_dynamics_sensitivity, csrc/wbc_arm_kernel.hip; definitions in include/wbc_sim.h). The CPU tests pin the fp64
restatement tests/regressor_reference.py to inverse_dynamics_reference.py (the sum, every column by linearity, the native columns by
central differences, the sparsity, an identification); the GPU tests hold the kernel to that restatement element-wise, to the existing
inverse-dynamics kernel, to its own structure and invariances, and the sensitivity call to the fp64 mass matrix in residual form.

Element-wise bound of the GPU tests: |kernel - ref| <= C * 2^-24 * mag, mag the restatement's magnitude array (next to every entry the
sum of the absolute values of the terms that make it up), C = C_Y for the linear columns and C_N for the native ones. The constants
follow the convention of tests/test_inverse_dynamics.py: 4 x the larger of the fp32 yardstick's largest ratio K_ref (numpy float32, the
same chain, measured on the CPU on the GPU tests' own states) and the kernel's largest ratio measured on an MI355X, rounded up to a
power of two; the measured ratios stand next to the constants."""
import copy
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import arm_codegen
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import regressor_reference as rr
import whole_body_reference as wb
from test_inverse_dynamics import C_ID, _env, _random_body_params, _random_state
from wbc_amd import abi
from wbc_amd.abi import REGRESSOR_NATIVE, linear_body_params          # new with the regressor: every test here needs them

NCOL, NB, NP, EPS = 26, 19, 10, 2.0 ** -24
FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(NCOL) if c not in FINGERS]
TILT = (0.7, -1.3, -9.5)
SENTINEL = 12345.0
# Largest |x - ref| / (2^-24 mag) over the cases of test_kernel_matches_reference_elementwise (n = 1, 13, 64; both state families;
# nudot given and NULL; tilted gravity at n = 64):
#   linear columns: fp32 yardstick K_ref = 8.02 (CPU), kernel 9.03 on an MI355X (n = 1: 2.6, n = 13: 5.4, n = 64: 9.03);  4 x 9.03 rounds up to 64.
#   native columns: fp32 yardstick K_ref = 8.02 (CPU), kernel 9.03 on an MI355X (n = 1: 2.8, n = 13: 5.4, n = 64: 9.03);  4 x 9.03 rounds up to 64.
# No entry class dominates: the largest ratio sits at another (row, body, column) in every case (a force row of a thigh's first moment, a
# leg joint's row of a calf's inertia, a root-moment row of the root's or a hip's parameters, a force row of the gripper's first moment).
C_Y = 64.0
C_N = 64.0
assert C_Y <= 4096 and C_N <= 4096


# ------------------------------------------------------------------------------------------------------------ shared states
def _nudot(rng):
    return np.r_[rng.uniform(-10, 10, 6), rng.uniform(-50, 50, 20)]


def _cpu_state(seed):
    """One seeded state of the families of tests/test_inverse_dynamics.py: near / far, nudot given / zero, gravity plain / tilted."""
    rng = np.random.default_rng(seed)
    pos, quat, q, nu = _random_state(rng, far=seed % 2 == 1)
    bp = _random_body_params(MODEL(), rng)
    nudot = _nudot(rng) if seed % 4 < 2 else None
    g = TILT if seed % 8 >= 4 else idr.GRAVITY
    return pos, quat, q, nu, nudot, bp, g


@functools.lru_cache(maxsize=None)
def MODEL():
    return abi.load_default_model()


@functools.lru_cache(maxsize=None)
def _case(n):
    """The GPU tests' states for n envs, rounded to fp32 as the sim holds them: env e is of the far family when e is odd. Returns a dict of
    float64 arrays: pos, quat, q, nu, nudot, and the randomisation (dmass, dcom, gdmass) with the body_params it gives."""
    m = MODEL()
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    out = {k: [] for k in ("pos", "quat", "q", "nu", "nudot", "dmass", "dcom", "gdmass")}
    for e in range(n):
        rng = np.random.default_rng(1000 * n + e)
        pos, quat, q, nu = _random_state(rng, far=e % 2 == 1)
        for k, v in zip(out, (pos, quat, q, nu, _nudot(rng), rng.uniform(-0.5, 2.5), rng.uniform(-0.1, 0.1, 3), rng.uniform(0, 0.1))):
            out[k].append(f32(v))
    out = {k: np.array(v) for k, v in out.items()}
    out["bp"] = abi.body_params_from_randomisation(m, out["dmass"], out["dcom"], out["gdmass"]).astype(np.float64)
    out["gravity"] = TILT if n == 64 else idr.GRAVITY
    return out


@functools.lru_cache(maxsize=None)
def _case_reference(n, with_nudot, dtype=np.float64):
    """(Y, mag) [n, 26, 19, 10] of the restatement on _case(n), linear columns."""
    c, m = _case(n), MODEL()
    res = [rr.regressor(m, c["quat"][e], c["q"][e], c["nu"][e], c["nudot"][e] if with_nudot else None, c["gravity"], dtype) for e in range(n)]
    return tuple(np.array([r[i] for r in res]) for i in range(2))


def _native(Y, mag, bp):
    """(Yn, magn): the native columns of every env at body_params bp [n, 20]."""
    res = [rr.native(Y[e], mag[e], rr.theta_of(MODEL(), bp[e])) for e in range(len(Y))]
    return tuple(np.array([r[i] for r in res]) for i in range(2))


def _ratio(got, ref, mag):
    """Largest |got - ref| / (2^-24 mag); entries whose magnitude is 0 must be exactly 0."""
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    return float((np.abs(got - ref)[~zero] / (EPS * mag[~zero])).max())


def _with_theta(model, b, theta_b):
    """A copy of the model whose moving body b has the inertial parameters theta_b (m, c, I_c)."""
    m2 = copy.copy(model)
    m2.mass, m2.com, m2.inertia = np.array(model.mass, dtype=np.float64), np.array(model.com, dtype=np.float64), np.array(model.inertia, dtype=np.float64)
    m2.mass[b], m2.com[b], m2.inertia[b] = theta_b[0], theta_b[1:4], theta_b[4:10]
    return m2


def _id_with(model, state, b, theta_b):
    """idr.inverse_dynamics with body b's parameters replaced (the root and the gripper body through body_params)."""
    pos, quat, q, nu, nudot, bp, g = state
    gb = model.gripper_piece["body"]
    if b in (0, gb):
        bp = np.array(bp)
        bp[0:10] = theta_b if b == 0 else bp[0:10]
        bp[10:20] = theta_b if b == gb else bp[10:20]
        return idr.inverse_dynamics(model, pos, quat, q, nu, nudot, bp, g)[0]
    return idr.inverse_dynamics(_with_theta(model, b, theta_b), pos, quat, q, nu, nudot, bp, g)[0]


# ------------------------------------------------------------------------------------------------------------ CPU: restatement
def test_regressor_times_parameters_is_inverse_dynamics():
    """(a) sum_b Y_b pi_b == idr.inverse_dynamics over 40 seeded states: worst |difference| / max|tau| 7.3e-15."""
    m = MODEL()
    worst = 0.0
    for seed in range(40):
        pos, quat, q, nu, nudot, bp, g = _cpu_state(seed)
        Y, mag = rr.regressor(m, quat, q, nu, nudot, g)
        pi = linear_body_params(m, bp)[0]
        assert np.array_equal(pi, rr.pi_from_theta(rr.theta_of(m, bp)))
        tau, _ = idr.inverse_dynamics(m, pos, quat, q, nu, nudot, bp, g)
        got = np.einsum("cbk,bk->c", Y, pi)
        err = np.abs(got - tau).max() / np.abs(tau).max()
        worst = max(worst, err)
        assert err <= 1e-13, (seed, err)
        assert np.all(np.abs(Y) <= mag * (1 + 1e-12)) and np.all(Y[FINGERS] == 0) and np.all(mag[FINGERS] == 0)
    print(f"Y pi - ID: worst relative difference {worst:.3g}")


def test_every_linear_column_is_a_difference_of_inverse_dynamics():
    """(b) Y[:, b, k] == ID(pi + e_k) - ID(pi) with both parameter sets mapped back to (m, c, I_c): linearity is exact, the difference
    holds to the rounding of the two torques (worst 9.1e-13 N m against torques of a few hundred)."""
    m = MODEL()
    worst = 0.0
    for seed in (0, 1, 6):
        state = _cpu_state(seed)
        pos, quat, q, nu, nudot, bp, g = state
        Y, _ = rr.regressor(m, quat, q, nu, nudot, g)
        pi = linear_body_params(m, bp)[0]
        for b in range(NB):
            base = _id_with(m, state, b, rr.theta_from_pi(pi[b]))
            for k in range(NP):
                pk = pi[b].copy(); pk[k] += 1.0
                col = _id_with(m, state, b, rr.theta_from_pi(pk)) - base
                err = np.abs(col - Y[:, b, k]).max()
                worst = max(worst, err)
                assert err <= 1e-10, (seed, b, k, err)
    print(f"linear columns against differences of ID: worst {worst:.3g}")


def test_native_columns_are_central_differences():
    """(c) d tau / d (m, c, I_c) against central differences of idr.inverse_dynamics in theta (tau is quadratic in c and linear in m and
    I_c, so the central difference is exact to rounding). Measured: worst |difference| / (1 + max|column|) = 1.24e-11 with steps of 1e-3;
    asserted at 10 x that."""
    m = MODEL()
    h = 1e-3
    worst = 0.0
    for seed in (2, 3, 5):
        state = _cpu_state(seed)
        pos, quat, q, nu, nudot, bp, g = state
        theta = rr.theta_of(m, bp)
        Y, mag = rr.regressor(m, quat, q, nu, nudot, g)
        Yn, _ = rr.native(Y, mag, theta)
        for b in range(NB):
            for k in range(NP):
                tp, tm = theta[b].copy(), theta[b].copy()
                tp[k] += h; tm[k] -= h
                col = (_id_with(m, state, b, tp) - _id_with(m, state, b, tm)) / (2 * h)
                err = np.abs(col - Yn[:, b, k]).max() / (1 + np.abs(Yn[:, b, k]).max())
                worst = max(worst, err)
    print(f"native columns against central differences: worst {worst:.3g}")
    assert worst <= 1.24e-10, worst


def test_sparsity_is_the_ancestor_masks():
    """(d) An entry is structurally zero exactly where the body is not in the subtree the row's coordinate moves."""
    m = MODEL()
    mask = rr.subtree_mask(m)
    assert mask[0:6].all() and not mask[FINGERS].any() and mask.sum() == 159
    for b in range(NB):
        anc = wb.ancestors(m, b)
        for d, a in enumerate(wb.dof_body(m)):
            assert mask[6 + d, b] == (a in anc and a > 0)
    seen = np.zeros_like(mask)
    for seed in range(6):
        pos, quat, q, nu, nudot, bp, g = _cpu_state(seed)
        Y, mag = rr.regressor(m, quat, q, nu, _nudot(np.random.default_rng(seed)), g)
        assert np.all(Y[~mask] == 0) and np.all(mag[~mask] == 0)
        seen |= (Y != 0).any(axis=2)
    assert np.array_equal(seen, mask)


def _identify(Ys, taus, pi_all, bodies):
    """Least squares for the linear parameters of `bodies` from stacked live rows, the other bodies' parameters known; columns scaled to
    unit norm. Returns (pi_hat [len(bodies), 10], condition number of the scaled matrix)."""
    others = [b for b in range(NB) if b not in bodies]
    A = np.concatenate([Y[LIVE][:, bodies].reshape(len(LIVE), -1) for Y in Ys])
    rhs = np.concatenate([t[LIVE] - np.einsum("cbk,bk->c", Y[LIVE][:, others], pi_all[others]) for Y, t in zip(Ys, taus)])
    s = np.linalg.norm(A, axis=0)
    x, *_ = np.linalg.lstsq(A / s, rhs, rcond=None)
    return (x / s).reshape(len(bodies), NP), float(np.linalg.cond(A / s))


def _group_error(pi_hat, pi):
    """Largest relative error over the groups (m | m c | Ibar) of every body."""
    return max(np.linalg.norm(pi_hat[b, sl] - pi[b, sl]) / np.linalg.norm(pi[b, sl]) for b in range(len(pi)) for sl in (slice(0, 1), slice(1, 4), slice(4, 10)))


def _identification_states(seed0=100, k=8):
    """k seeded states of one env (one randomisation): both families, angular velocities and accelerations that differ in every state."""
    m = MODEL()
    bp = _random_body_params(m, np.random.default_rng(seed0))
    out = []
    for i in range(k):
        rng = np.random.default_rng(seed0 + 1 + i)
        pos, quat, q, nu = _random_state(rng, far=i % 2 == 1)
        out.append((pos, quat, q, nu, _nudot(rng)))
    return bp, out


def test_identification_recovers_root_and_gripper_parameters():
    """(e) 8 states x 24 live rows against the 20 linear parameters of the root and the gripper body: the fp64 reference recovers them to
    4.3e-13 relative per group (m | m c | Ibar); condition number of the column-scaled stack 6.2."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp, states = _identification_states()
    pi = linear_body_params(m, bp)[0]
    Ys = [rr.regressor(m, quat, q, nu, nd)[0] for pos, quat, q, nu, nd in states]
    taus = [idr.inverse_dynamics(m, pos, quat, q, nu, nd, bp)[0] for pos, quat, q, nu, nd in states]
    pi_hat, cond = _identify(Ys, taus, pi, [0, gb])
    err = _group_error(pi_hat, pi[[0, gb]])
    print(f"identification (fp64): condition number {cond:.3g}, worst relative group error {err:.3g}")
    assert err <= 1e-8, err
    theta_hat = rr.theta_from_pi(pi_hat)
    assert np.abs(theta_hat[0] - bp[0:10]).max() <= 1e-8 and np.abs(theta_hat[1] - bp[10:20]).max() <= 1e-8


def test_fp32_yardstick_sits_inside_the_bounds():
    """K_ref: the numpy-float32 chain's largest ratio on the GPU tests' states; the constants hold 4 x it."""
    kl = kn = 0.0
    for n in (1, 13, 64):
        for with_nudot in (True, False):
            Y, mag = _case_reference(n, with_nudot)
            Yn, magn = _native(Y, mag, _case(n)["bp"])
            Y32, mag32 = _case_reference(n, with_nudot, np.float32)
            Yn32, _ = _native(Y32, mag32, _case(n)["bp"])
            assert Y32.dtype == np.float32 and Yn32.dtype == np.float32
            kl, kn = max(kl, _ratio(Y32.astype(np.float64), Y, mag)), max(kn, _ratio(Yn32.astype(np.float64), Yn, magn))
    print(f"fp32 yardstick: K_ref linear {kl:.3g}, native {kn:.3g}")
    assert 4 * kl <= C_Y and 4 * kn <= C_N, (kl, kn)


def test_null_and_bad_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    assert L.wbc_sim_inverse_dynamics_regressor(None, None, 0, None, C.addressof(buf), 0, None) == -1
    assert b"wbc_sim_inverse_dynamics_regressor" in L.wbc_last_error() and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_forward_dynamics_sensitivity(None, None, 0, None, C.addressof(buf), C.addressof(buf), C.addressof(buf), 0, None) == -1
    assert b"wbc_sim_forward_dynamics_sensitivity" in L.wbc_last_error() and b"NULL" in L.wbc_last_error()
    assert abi.REGRESSOR_NATIVE == 4 and abi.DERIV_TRANSPOSED == 2 and abi.SOLVE_ARMATURE == 1


# (LDS bytes, scratch bytes, waves per SIMD that the VGPR count allows) of every kernel the file held before the regressor.
PARENT_CODEGEN = {
    "wbc_arm_dynamics_kernel": (4608, 224, 5), "wbc_body_dynamics_kernel": (4832, 0, 8), "wbc_inverse_dynamics_kernel": (2736, 0, 4),
    "wbc_mass_solve_kernel": (8000, 0, 8), "wbc_body_accel_kernel": (0, 0, 7), "wbc_constraint_rhs_kernel": (1032, 0, 7),
    "wbc_constraint_solve_kernel": (8880, 0, 7), "wbc_centroidal_kernel": (5312, 0, 8), "wbc_dynamics_derivatives_kernel": (17784, 0, 3),
    "wbc_derivatives_transpose_kernel": (0, 0, 8), "wbc_constraint_tangent_kernel": (3832, 0, 4),
    "wbc_constraint_derivatives_solve_kernel": (8736, 0, 7), "wbc_taskid_rhs_kernel": (1152, 0, 7), "wbc_taskid_solve_kernel": (16644, 0, 8),
    "wbc_taskqp_solve_kernel": (22336, 0, 5)}


def _waves(vgprs):
    """Waves per SIMD of a wave64 kernel on gfx950: 512 VGPRs per lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


def test_regressor_kernel_codegen():
    """(f) The new kernel: no scratch, no flat memory instructions, LDS for 8 workgroups per CU, 64 lanes. The kernels that were there:
    LDS, scratch and register class as before."""
    k = "wbc_inverse_dynamics_regressor_kernel"
    assert arm_codegen.meta(k, "private_segment_fixed_size") == 0
    assert arm_codegen.meta(k, "group_segment_fixed_size") <= 20480
    assert arm_codegen.meta(k, "max_flat_workgroup_size") == 64
    body = arm_codegen.body(k)
    assert "s_endpgm" in body and re.search(r"\bglobal_store_dwordx4\b", body)
    assert not re.search(r"\bflat_", body) and "scratch_" not in body
    for name, want in PARENT_CODEGEN.items():
        got = (arm_codegen.meta(name, "group_segment_fixed_size"), arm_codegen.meta(name, "private_segment_fixed_size"),
               _waves(arm_codegen.meta(name, "vgpr_count")))
        assert got == want, (name, got, want)


# ------------------------------------------------------------------------------------------------------------ GPU: the kernel
def _gpu_env(n):
    """An env holding _case(n): the randomisation through set_env_params, the states written into the sim."""
    c = _case(n)
    env = _env(n, seed=2, steps=0, gravity=c["gravity"] if n == 64 else None)
    env.sim.set_env_params(base_dmass=c["dmass"], base_dcom=c["dcom"], gripper_dmass=c["gdmass"])
    _set_states(env, c["pos"], c["quat"], c["q"], c["nu"])
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(bp, c["bp"], rtol=1e-6, atol=1e-9)   # the randomisation asked for; the references use the sim's own fp32 values
    return env, torch.tensor(c["nudot"], dtype=torch.float32, device="cuda").contiguous(), bp


def _set_states(env, pos, quat, q, nu, shift=(0.0, 0.0, 0.0)):
    root = env.sim.tensor("ROOT_STATES").clone()
    dof = env.sim.tensor("DOF_STATE").clone()
    for e in range(env.num_envs):
        root[e, 0] = torch.tensor(np.concatenate([pos[e] + np.asarray(shift), quat[e], nu[e][:6]]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q[e], nu[e][6:]], -1), dtype=torch.float32)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    torch.cuda.synchronize()


def _gripper(env):
    return int(env.robot_model.gripper_piece["body"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_kernel_matches_reference_elementwise(n):
    """Every entry of every env, linear and native columns, nudot given and NULL; the measured ratios stand next to C_Y and C_N. Also the
    identity with the existing kernel: Y_kernel pi - tau_kernel within the sum of both allowances."""
    env, nudot, bp = _gpu_env(n)
    c, m = _case(n), env.robot_model
    mask = rr.subtree_mask(m)
    pi = linear_body_params(m, bp)
    ratios = {}
    for with_nudot in (True, False):
        nd = nudot if with_nudot else None
        Y = env.sim.inverse_dynamics_regressor(nudot=nd)
        Yn = env.sim.inverse_dynamics_regressor(nudot=nd, native=True)
        tau = env.inverse_dynamics(nd)
        torch.cuda.synchronize()
        assert Y.shape == (n, NCOL, NB, NP) and Yn.shape == (n, NCOL, NB, NP)
        Y, Yn, tau = (t.cpu().numpy().astype(np.float64) for t in (Y, Yn, tau))
        ref, mag = _case_reference(n, with_nudot)
        refn, magn = _native(ref, mag, bp)
        # every structural entry is exercised (m: 0 at a joint's own body; without nudot and tilt the root's h columns of the z moment are 0)
        assert not with_nudot or np.all(mag[:, mask].reshape(n, -1, NP)[..., 1:4].max(axis=0) > 0)
        assert np.all(Y[:, ~mask] == 0) and np.all(Y[:, FINGERS] == 0) and np.all(Yn[:, ~mask] == 0)
        ratios["Y" + ("" if with_nudot else "(h)")] = _ratio(Y, ref, mag)
        ratios["native" + ("" if with_nudot else "(h)")] = _ratio(Yn, refn, magn)
        # identity: the kernel's Y against the existing kernel's tau
        got = np.einsum("ncbk,nbk->nc", Y, pi)
        tmag = np.array([idr.inverse_dynamics(m, c["pos"][e], c["quat"][e], c["q"][e], c["nu"][e], c["nudot"][e] if with_nudot else None,
                                              bp[e], c["gravity"])[1] for e in range(n)])
        allow = EPS * (C_Y * np.einsum("ncbk,nbk->nc", mag, np.abs(pi)) + C_ID * tmag)
        assert np.all(np.abs(got - tau) <= allow), float((np.abs(got - tau) / np.maximum(allow, 1e-300)).max())
        where = np.unravel_index(np.argmax(np.abs(Y - ref) / np.maximum(EPS * mag, 1e-300) * (mag > 0)), Y.shape)
        print(f"regressor n={n} nudot={with_nudot}: the largest linear ratio is at (env, row, body, column) {tuple(int(i) for i in where)}")
    print(f"regressor n={n}: largest |kernel - ref| / (2^-24 mag): {ratios}")
    assert max(ratios["Y"], ratios["Y(h)"]) <= C_Y and max(ratios["native"], ratios["native(h)"]) <= C_N, ratios


@pytest.mark.gpu
def test_structure_subset_transpose_and_translation():
    """Structural zeros and finger rows exactly 0.0; a subset call is the slices of the full call, the transposed output the transpose, and
    a translated robot gives the same bits; the native call for (root, gripper) lines up with BODY_PARAMS."""
    n = 13
    env, nudot, _ = _gpu_env(n)
    c, m = _case(n), env.robot_model
    mask = torch.tensor(rr.subtree_mask(m), device="cuda")
    full = env.sim.inverse_dynamics_regressor(nudot=nudot)
    fulln = env.sim.inverse_dynamics_regressor(nudot=nudot, native=True)
    assert bool((full[:, ~mask] == 0).all()) and bool((full[:, FINGERS] == 0).all()) and bool((full[:, :3, :, 4:] == 0).all())
    assert bool((full[:, mask] != 0).any(dim=-1).all())
    assert torch.equal(env.body_parameter_regressor(nudot), full)
    gb = _gripper(env)
    for bodies in ([0, gb], [gb, 3, 0, 17, 9], [5], list(range(NB))[::-1], list(range(10))):
        for native, whole in ((False, full), (True, fulln)):
            sub = env.sim.inverse_dynamics_regressor(bodies, nudot=nudot, native=native)
            assert sub.shape == (n, NCOL, len(bodies), NP) and torch.equal(sub, whole[:, :, bodies])
            subt = env.sim.inverse_dynamics_regressor(bodies, nudot=nudot, native=native, transposed=True)
            assert subt.shape == (n, len(bodies) * NP, NCOL)
            assert torch.equal(subt, sub.reshape(n, NCOL, len(bodies) * NP).transpose(1, 2))
    sens = env.randomised_parameter_sensitivity(nudot)
    assert sens.shape == (n, NCOL, 20) and torch.equal(sens, fulln[:, :, [0, gb]].reshape(n, NCOL, 20))
    assert torch.equal(env.sim.inverse_dynamics_regressor(), env.sim.inverse_dynamics_regressor(nudot=torch.zeros_like(nudot)))
    # translation: the same states 110 m away
    _set_states(env, c["pos"], c["quat"], c["q"], c["nu"], shift=(3.0, 110.0, 0.0))
    assert float((env.root_states[:, 1] - torch.tensor(c["pos"][:, 1] + 110.0, device="cuda")).abs().max()) < 1e-4
    assert torch.equal(env.sim.inverse_dynamics_regressor(nudot=nudot), full)
    assert torch.equal(env.sim.inverse_dynamics_regressor(nudot=nudot, native=True), fulln)


@pytest.mark.gpu
@pytest.mark.parametrize("armature", [False, True])
@pytest.mark.parametrize("nbodies", [2, 19])
def test_sensitivity_residual(nbodies, armature):
    """Every column X of dnudot_dpi against fp64 in residual form: |(M_ref + A) X + Y_ref(nudot_kernel)| within the mass solve's
    C_S 2^-24 row scale for that right-hand side plus the regressor's own allowance; nudot the bits of forward_dynamics. Two bodies are
    one solve launch, nineteen six (the last one ragged); the native columns with two bodies, the linear ones with nineteen. Measured
    largest residual / (2^-24 row scale), the regressor's allowance not used: 19.6 and 32 (two bodies, without / with the armature), 81.9
    and 117 (nineteen)."""
    n = 13
    env, _, bp = _gpu_env(n)
    c, m = _case(n), env.robot_model
    native = nbodies == 2
    bodies = [0, _gripper(env)] if nbodies == 2 else None
    tau = torch.tensor(msr.force_rhs(np.random.default_rng(5), (n,)), dtype=torch.float32, device="cuda").contiguous()
    nd, X = env.sim.forward_dynamics_sensitivity(bodies, tau, armature=armature, native=native)
    assert torch.equal(nd, env.sim.forward_dynamics(tau, armature=armature))
    assert X.shape == (n, nbodies * NP, NCOL)
    X, nd64 = X.cpu().numpy().astype(np.float64), nd.cpu().numpy().astype(np.float64)
    assert np.isfinite(X).all() and np.all(X[..., FINGERS] == 0)
    arm = msr.armature_vector(env.tcfg) if armature else None
    sel = [0, _gripper(env)] if nbodies == 2 else list(range(NB))
    worst = 0.0
    for e in range(n):
        M = msr.mass_matrix(m, c["pos"][e], c["quat"][e], c["q"][e], bp[e], arm)
        Y, mag = rr.regressor(m, c["quat"][e], c["q"][e], c["nu"][e], nd64[e], c["gravity"])
        if native:
            Y, mag = rr.native(Y, mag, rr.theta_of(m, bp[e]))
        b = -Y[:, sel].reshape(NCOL, -1).T                                   # [K, 26]: one right-hand side per parameter
        allow = (C_N if native else C_Y) * EPS * mag[:, sel].reshape(NCOL, -1).T
        scale = msr.row_scale(M, X[e], b)
        r = msr.residual(M, X[e], b)
        assert np.all(r <= msr.C_S * EPS * scale + allow), (e, float((r / np.maximum(msr.C_S * EPS * scale + allow, 1e-300)).max()))
        worst = max(worst, float((r[:, LIVE] / (EPS * scale[:, LIVE] + 1e-300)).max()))
    print(f"sensitivity nbodies={nbodies} armature={armature}: largest residual / (2^-24 row scale) = {worst:.3g}")


@pytest.mark.gpu
def test_identification_on_the_gpu():
    """A known randomisation through set_env_params, 8 states (one env each), tau from the existing kernel and Y from the new one; least
    squares in float64 on the host recovers BODY_PARAMS. Bound: 4 x the recovery error of the fp32 yardstick (numpy float32 Y and
    numpy float32 inverse dynamics) on the same states, per group (m | c | I_c) of both bodies relative to the group's norm. Measured:
    yardstick 6.96e-6 (bound 2.78e-5), the two kernels 1.89e-5; the worst group is the gripper body's I_c in both."""
    n = 8
    m = MODEL()
    gb = m.gripper_piece["body"]
    _, states = _identification_states()
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    states = [tuple(f32(x) for x in s) for s in states]
    dm, dcom, gd = np.full(n, 1.7, np.float32), np.tile(np.float32([0.04, -0.07, 0.02]), (n, 1)), np.full(n, 0.08, np.float32)
    env = _env(n, seed=2, steps=0)
    env.sim.set_env_params(base_dmass=dm, base_dcom=dcom, gripper_dmass=gd)
    _set_states(env, *[np.array([s[i] for s in states]) for i in range(4)])
    nudot = torch.tensor(np.array([s[4] for s in states]), dtype=torch.float32, device="cuda").contiguous()
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    assert np.all(bp == bp[0]) and bp[0, 0] > m.mass[0] + 1.6
    Y = env.body_parameter_regressor(nudot).cpu().numpy().astype(np.float64)
    tau = env.inverse_dynamics(nudot).cpu().numpy().astype(np.float64)
    theta = rr.theta_of(m, bp[0])
    pi = rr.pi_from_theta(theta)
    want = theta[[0, gb]]

    def error(Ys, taus):
        th = rr.theta_from_pi(_identify(Ys, taus, pi, [0, gb])[0])
        return max(np.linalg.norm(th[b, sl] - want[b, sl]) / np.linalg.norm(want[b, sl]) for b in range(2) for sl in (slice(0, 1), slice(1, 4), slice(4, 10)))
    yard = error([rr.regressor(m, s[1], s[2], s[3], s[4], dtype=np.float32)[0].astype(np.float64) for s in states],
                 [rr.inverse_dynamics_yardstick(m, s[1], s[2], s[3], s[4], theta).astype(np.float64) for s in states])
    got = error(list(Y), list(tau))
    print(f"identification on the GPU: recovery error {got:.3g}, fp32 yardstick {yard:.3g}")
    assert got <= 4 * yard, (got, yard)


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched():
    """Every -1 case of both entry points, one call at a time: the status, the word in wbc_last_error() under the entry point's own name,
    and at the end every poisoned buffer as it was."""
    n = 13
    env, nudot, _ = _gpu_env(n)
    L, h = env.sim.L, env.sim.h
    Y = torch.full((n, NCOL, NB, NP), SENTINEL, device="cuda")
    X, W = torch.full((n, NB * NP, NCOL), SENTINEL, device="cuda"), torch.full((n, NB * NP, NCOL), SENTINEL, device="cuda")
    nd = torch.full((n, NCOL), SENTINEL, device="cuda")
    idx = lambda *b: (C.c_int32 * len(b))(*b)
    gb = _gripper(env)
    # wbc_sim_inverse_dynamics_regressor
    names = ("sim", "bodies", "nbodies", "nudot", "Y", "flags", "stream")
    base = dict(sim=h, bodies=None, nbodies=0, nudot=nudot.data_ptr(), Y=Y.data_ptr(), flags=0, stream=None)
    call = lambda **kw: L.wbc_sim_inverse_dynamics_regressor(*[kw.get(k, base[k]) for k in names])
    bad_bodies = [dict(nbodies=2), dict(bodies=idx(0), nbodies=0), dict(bodies=idx(0), nbodies=-1), dict(bodies=idx(*range(NB), 0), nbodies=NB + 1),
                  dict(bodies=idx(0, NB), nbodies=2), dict(bodies=idx(0, -1), nbodies=2), dict(bodies=idx(3, 5, 3), nbodies=3)]
    refusals = [(dict(sim=None), b"NULL"), (dict(Y=None), b"NULL")] + [(kw, b"bodies") for kw in bad_bodies]
    refusals += [(dict(flags=f), b"flag") for f in (abi.SOLVE_ARMATURE, 8, abi.DERIV_TRANSPOSED | REGRESSOR_NATIVE | 16)]
    refusals += [(dict(nudot=base["nudot"] + off), b"aligned") for off in (1, 2, 3)]
    refusals += [(dict(Y=base["Y"] + off), b"aligned") for off in (1, 2, 3, 4, 8, 12)]          # Y: 16 bytes
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        err = L.wbc_last_error()
        assert word in err and b"wbc_sim_inverse_dynamics_regressor: " in err, (kw, err)
    # wbc_sim_forward_dynamics_sensitivity
    names_s = ("sim", "bodies", "nbodies", "tau", "nudot", "X", "W", "flags", "stream")
    base_s = dict(sim=h, bodies=None, nbodies=0, tau=nudot.data_ptr(), nudot=nd.data_ptr(), X=X.data_ptr(), W=W.data_ptr(), flags=0, stream=None)
    call_s = lambda **kw: L.wbc_sim_forward_dynamics_sensitivity(*[kw.get(k, base_s[k]) for k in names_s])
    refusals = [(dict(sim=None), b"NULL"), (dict(nudot=None), b"NULL"), (dict(X=None), b"NULL"), (dict(W=None), b"NULL")]
    refusals += [(kw, b"bodies") for kw in bad_bodies]
    refusals += [(dict(flags=f), b"flag") for f in (abi.DERIV_TRANSPOSED, 8, abi.SOLVE_ARMATURE | REGRESSOR_NATIVE | 16)]
    refusals += [({k: base_s[k] + off}, b"aligned") for k in ("tau", "nudot", "X") for off in (1, 2, 3)]
    refusals += [(dict(W=base_s["W"] + off), b"aligned") for off in (1, 2, 3, 4, 8, 12)]        # the workspace: 16 bytes
    last = 4 * (n * NB * NP * NCOL - NCOL)                                                       # the last 26 floats of a block
    refusals += [(dict(W=base_s["X"] + 16 * NCOL), b"overlap"), (dict(X=base_s["W"] + last), b"overlap"),
                 (dict(nudot=base_s["W"] + last), b"overlap"), (dict(nudot=base_s["X"]), b"overlap"),
                 (dict(bodies=idx(0, gb), nbodies=2, W=base_s["X"] + 4 * (n * 2 * NP * NCOL - 4)), b"overlap")]
    for kw, word in refusals:
        assert call_s(**kw) == -1, kw
        err = L.wbc_last_error()
        assert word in err and b"wbc_sim_forward_dynamics_sensitivity: " in err, (kw, err)
    torch.cuda.synchronize()
    for t in (Y, X, W, nd):
        assert bool((t == SENTINEL).all())
    # the same buffers are filled by good calls; blocks that only touch are no overlap (two bodies: the workspace right behind the result)
    assert call() == 0
    assert call_s(bodies=idx(0, gb), nbodies=2, W=base_s["X"] + 4 * n * 2 * NP * NCOL) == 0
    torch.cuda.synchronize()
    assert torch.equal(Y, env.sim.inverse_dynamics_regressor(nudot=nudot))
    want_nd, want_X = env.sim.forward_dynamics_sensitivity([0, gb], nudot)
    assert torch.equal(nd, want_nd) and torch.equal(X.view(-1)[:n * 2 * NP * NCOL].view(n, 2 * NP, NCOL), want_X)
