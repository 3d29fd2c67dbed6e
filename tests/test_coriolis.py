"""The Coriolis matrix C(q, nu), dM/dt, the generalised momentum p = M nu, C^T nu (wbc_sim_coriolis: wbc_coriolis_kernel and
wbc_momentum_kernel in csrc/wbc_arm_kernel.hip) and the momentum observer (wbc_sim_momentum_observer); definitions in include/wbc_sim.h.
The CPU tests pin the fp64 brute-force sum of tests/coriolis_reference.py to what exists -- inverse dynamics, the mass matrix and its
central difference, the fp64 forward dynamics -- and measure the fp32 yardstick; the GPU tests hold the kernels to the reference entry by
entry, to their structure as equalities, to the sibling kernels and to the observer's recursion.

Bound: every entry of every output satisfies |kernel - ref| <= C 2^-24 mag, mag the reference's magnitude about the root's own origin.
C is 4 x the larger of K_ref (the fp32 yardstick's largest ratio over 64 states of each of the two families below, measured on the CPU
and asserted there) and the kernel's largest ratio on an MI355X (n = 1, 13, 64), rounded up to a power of two:

    output     K_ref     kernel's largest ratio     C
    cmat       2.65      4.88  (n = 64)             32
    mdot       1.63      2.44  (n = 64)             16
    p          2.66      6.98  (n = 64)             32
    ctnu       2.06      4.05  (n = 64)             32

Against the sibling kernels the largest difference is 0.006 of the summed allowances for cmat nu (inverse dynamics minus gravity) and
0.0008 for p (mm_whole nu); the observer's state stays within 0.05 of its allowance of the fp64 recursion.

State families: member `seed` is test_inverse_dynamics._random_state with random body params, "far" with the root near (3, 110, 0). In
the GPU cases env e holds member e of the near (e even) or far (e odd) family; n = 64 runs under the tilted gravity (0.7, -1.3, -9.5).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import coriolis_reference as cor
import inverse_dynamics_reference as idr
import whole_body_reference as wb
from wbc_amd import abi

EPS, FAMILIES = cor.EPS, cor.FAMILIES
FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(26) if c not in FINGERS]
SENTINEL = 12345.0
TILTED = (0.7, -1.3, -9.5)
SIZES = {"cmat": 26 * 26, "mdot": 26 * 26, "vec": 2 * 26}
# K_ref, the kernel's largest ratio on the MI355X (the docstring's table) and the constant
K_REF = {"cmat": 2.65, "mdot": 1.63, "p": 2.66, "ctnu": 2.06}
K_GPU = {"cmat": 4.88, "mdot": 2.44, "p": 6.98, "ctnu": 4.05}
CONST = {"cmat": 32.0, "mdot": 16.0, "p": 32.0, "ctnu": 32.0}
assert all(CONST[f] == 2.0 ** np.ceil(np.log2(4 * max(K_REF[f], K_GPU[f]))) and CONST[f] <= 4096 for f in FAMILIES)
# The sibling kernels' allowances, restated: |tau - ref|_k <= C_ID 2^-24 mag_k (tests/test_inverse_dynamics.py) and
# |mm - ref| <= 1e-5 max |M_ref| per entry (tests/test_whole_body_dynamics.py).
C_ID = 4096.0
MM_REL = 1e-5
# Bounds of the CPU checks: what the definition was measured to hold to in fp64 on states of test_inverse_dynamics._random_state (the
# near family), times 4; next to each, the largest value over the states of the test below.
TOL_CNU = 4 * 4e-14           # |C nu - (h - g)|                                                          (1.2e-13)
TOL_MDOT = 4 * 8e-10          # |C + C^T - central difference of mass_matrix along nu|, step 1e-5         (8.0e-10)
TOL_POINT = 4 * 9e-15         # |brute-force sum about the world origin, or a point nearby - about the root origin|   (1.1e-14)
TOL_VEC = 4 * 4e-15           # |C^T nu, p - the matrix forms|                                            (3.6e-15)
# The last one was measured as 3e-9; the margin is 16 here, because this module's difference runs over whole RK4 steps of the brute-force
# sum, whose own rounding (2^-53 x the terms' sizes of some tens / the step) is what is left at a step of 1e-6.
TOL_PDOT = 16 * 3e-9          # |central difference of p along the fp64 forward dynamics - (tau + C^T nu - g)|, step 1e-6   (2.2e-8)


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _state(seed, far):
    """(pos, quat, q, nu, body_params) of member `seed` of a family."""
    import test_inverse_dynamics as tid
    rng = np.random.default_rng(4100 + seed)
    pos, quat, q, nu = tid._random_state(rng, far=far)
    return pos, quat, q, nu, tid._random_body_params(_model(), rng)


def _ancestor_pairs(model):
    """bool [26, 26]: both coordinates live and one's body an ancestor-or-self of the other's."""
    body = [0] * 6 + wb.dof_body(model)
    ok = np.zeros((26, 26), dtype=bool)
    for r in LIVE:
        for c in LIVE:
            ok[r, c] = body[r] in wb.ancestors(model, body[c]) or body[c] in wb.ancestors(model, body[r])
    return ok


# ------------------------------------------------------------------------------------------------------------ CPU
def test_null_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.wbc_sim_coriolis(None, p, p, p, None) == -1
    assert L.wbc_last_error().startswith(b"wbc_sim_coriolis: ") and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_momentum_observer(None, None, 10.0, 0.01, 0, p, None) == -1
    assert L.wbc_last_error().startswith(b"wbc_sim_momentum_observer: ") and b"NULL" in L.wbc_last_error()
    assert all(x == 0.0 for x in buf)


def test_coriolis_kernels_codegen():
    """The code object's metadata alone: no scratch, one wavefront per workgroup, the LDS sizes DESIGN.md states (two envs per
    workgroup: 12264 bytes with the 26 x 26 tile lying over the body tables, 3040 bytes for the vector kernel)."""
    for kernel, lds in (("wbc_coriolis_kernel", 12264), ("wbc_momentum_kernel", 3040)):
        assert arm_codegen.meta(kernel, "private_segment_fixed_size") == 0
        assert arm_codegen.meta(kernel, "max_flat_workgroup_size") == 64
        assert arm_codegen.meta(kernel, "group_segment_fixed_size") == lds
        body = arm_codegen.body(kernel)
        assert "s_endpgm" in body and "scratch_" not in body
    assert "global_store_dwordx4" in arm_codegen.body("wbc_coriolis_kernel")
    assert "global_store_dwordx4" not in arm_codegen.body("wbc_momentum_kernel")


def test_reference_is_the_velocity_product_term_and_the_mass_matrix_rate():
    """C nu == h - g of inverse_dynamics_reference; C + C^T == the central difference of whole_body_reference.mass_matrix along nu;
    C^T nu and p == the matrix forms; the sparsity pattern."""
    import test_centroidal as tc
    m = _model()
    pairs = _ancestor_pairs(m)
    worst = np.zeros(3)
    step = 1e-5
    for seed in range(12):
        pos, quat, q, nu, bp = _state(seed, far=False)
        out, mag = cor.coriolis(m, pos, quat, q, nu, bp)
        Cm = out["cmat"]
        h, _ = idr.bias_forces(m, pos, quat, q, nu, bp)
        g, _ = idr.gravity_forces(m, pos, quat, q, bp)
        worst[0] = max(worst[0], np.abs(Cm @ nu - (h - g)).max())
        side = [wb.mass_matrix(m, pos + s * step * nu[0:3], tc._rotated(quat, s * step * nu[3:6]), q + s * step * nu[6:], bp) for s in (1.0, -1.0)]
        worst[1] = max(worst[1], np.abs(out["mdot"] - (side[0] - side[1]) / (2 * step)).max())
        M = wb.mass_matrix(m, pos, quat, q, bp)
        worst[2] = max(worst[2], np.abs(Cm.T @ nu - out["ctnu"]).max(), np.abs(M @ nu - out["p"]).max())
        assert np.all(out["mdot"] == out["mdot"].T)
        # sparsity: the fingers, the pairs of which neither moves the other, and the block [0:3, 0:3]
        assert np.all(Cm[FINGERS] == 0) and np.all(Cm[:, FINGERS] == 0) and np.all(mag["cmat"][FINGERS] == 0) and np.all(mag["cmat"][:, FINGERS] == 0)
        assert np.all(Cm[~pairs] == 0) and np.all(mag["cmat"][~pairs] == 0) and np.all(mag["cmat"][3:][pairs[3:]] > 0)
        assert np.all(Cm[0:3, 0:3] == 0)
        assert np.abs(Cm[:, 0:3]).max() <= 1e-15 * mag["cmat"][:, 0:3].max()      # in exact arithmetic the whole of the first three columns
        assert np.all(out["p"][FINGERS] == 0) and np.all(out["ctnu"][FINGERS] == 0) and np.all(mag["p"][LIVE] > 0)
    print(f"coriolis reference: |C nu - (h - g)| {worst[0]:.3g}, |C + C^T - dM/dt| {worst[1]:.3g}, vectors vs matrix forms {worst[2]:.3g}")
    assert worst[0] <= TOL_CNU and worst[1] <= TOL_MDOT and worst[2] <= TOL_VEC


def test_reference_does_not_depend_on_the_point_the_moments_are_taken_about():
    """The brute-force sum about the world origin and about a random point inside the robot against the one about the root origin (which the tree form of
    the kernel uses): the values do not move."""
    m = _model()
    worst = 0.0
    for seed in range(8):
        pos, quat, q, nu, bp = _state(seed, far=False)
        out, _ = cor.coriolis(m, pos, quat, q, nu, bp)
        rng = np.random.default_rng(seed)
        for origin in (np.zeros(3), pos + 0.3 * rng.normal(size=3)):
            o2, m2 = cor.coriolis(m, pos, quat, q, nu, bp, origin=origin)
            for f in FAMILIES:
                worst = max(worst, float(np.abs(o2[f] - out[f]).max()))
    print(f"coriolis reference: largest |value about another point - value about the root origin| {worst:.3g}")
    assert worst <= TOL_POINT


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output family: the fp32 yardstick's largest ratio over 64 members of each state family."""
    m = _model()
    k = {f: 0.0 for f in FAMILIES}
    for far in (False, True):
        for seed in range(64):
            pos, quat, q, nu, bp = _state(seed, far)
            out, mag = cor.coriolis(m, pos, quat, q, nu, bp)
            y, _ = cor.coriolis(m, pos, quat, q, nu, bp, dtype=np.float32)
            for f in FAMILIES:
                k[f] = max(k[f], cor.largest_ratio(y[f], out[f], mag[f]))
    return k


def test_fp32_yardsticks_are_the_ones_the_constants_were_taken_from():
    k = _yardsticks()
    print("coriolis yardsticks: " + ", ".join(f"{f} K_ref = {k[f]:.3g} (C = {CONST[f]:g})" for f in FAMILIES))
    for f in FAMILIES:
        assert abs(k[f] - K_REF[f]) <= 0.25 * K_REF[f], (f, k[f])          # a largest ratio moves with the summation order of the BLAS at hand
        assert 4 * k[f] <= CONST[f] <= 4096


def _forward_dynamics(m, x, tau, bp):
    """d/dt of x = (pos, quat, q, nu) under the generalised forces tau, fp64: nudot = M^-1 (tau - h) on the live coordinates."""
    import test_inverse_dynamics as tid
    pos, quat, q, nu = x[0:3], x[3:7], x[7:27], x[27:53]
    quat = quat / np.linalg.norm(quat)
    M = wb.mass_matrix(m, pos, quat, q, bp)
    h, _ = idr.bias_forces(m, pos, quat, q, nu, bp)
    nudot = np.zeros(26)
    nudot[LIVE] = np.linalg.solve(M[np.ix_(LIVE, LIVE)], (tau - h)[LIVE])
    return np.r_[nu[0:3], 0.5 * tid._quat_mul(np.r_[nu[3:6], 0.0], quat), nu[6:], nudot]


def _rk4(f, x, dt):
    k1 = f(x); k2 = f(x + 0.5 * dt * k1); k3 = f(x + 0.5 * dt * k2); k4 = f(x + dt * k3)
    return x + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def test_reference_momentum_obeys_its_equation_along_the_forward_dynamics():
    """d/dt p = tau + C^T nu - g: the central difference of p over one RK4 step forward and one back along the fp64 forward dynamics
    under tau. At step 1e-6 rounding dominates; from 2e-3 to 1e-3 the error falls as step^2."""
    m = _model()
    worst, falls = 0.0, 0.0
    for seed in range(4):
        pos, quat, q, nu, bp = _state(seed, far=False)
        tau = np.zeros(26); tau[0:24] = np.random.default_rng(seed).uniform(-3, 3, 24)
        x0 = np.r_[pos, quat, q, nu]
        x0[27 + 24:53] = 0.0
        o, _ = cor.coriolis(m, pos, quat, q, x0[27:53], bp, matrices=False)
        g, _ = idr.gravity_forces(m, pos, quat, q, bp)
        want = tau + o["ctnu"] - g
        f = lambda y: _forward_dynamics(m, y, tau, bp)
        errs = []
        for step in (1e-6, 1e-3, 2e-3):
            side = []
            for sgn in (1.0, -1.0):
                x = _rk4(f, x0, sgn * step)
                side.append(cor.coriolis(m, x[0:3], x[3:7] / np.linalg.norm(x[3:7]), x[7:27], x[27:53], bp, matrices=False)[0]["p"])
            errs.append(float(np.abs((side[0] - side[1]) / (2 * step) - want)[LIVE].max()))
        worst, falls = max(worst, errs[0]), max(falls, errs[1] / errs[2])
    print(f"coriolis reference: |dp/dt - (tau + C^T nu - g)| at step 1e-6 {worst:.3g}; error at 1e-3 / error at 2e-3 {falls:.3g}")
    assert worst <= TOL_PDOT and falls < 0.3


def _observed(m, x0, tau, tau_ext, bp, gain, dt, steps):
    """The residuals [steps + 1, 26] of the observer sampled every dt along the RK4 trajectory from x0 under tau + tau_ext."""
    x, out = x0.copy(), []
    state = None
    for k in range(steps + 1):
        pos, quat, q, nu = x[0:3], x[3:7] / np.linalg.norm(x[3:7]), x[7:27], x[27:53]
        o, _ = cor.coriolis(m, pos, quat, q, nu, bp, matrices=False)
        g, _ = idr.gravity_forces(m, pos, quat, q, bp)
        state = cor.observer_step(state, o["p"], o["ctnu"], g, tau, gain, dt, reset=k == 0)
        out.append(state[1])
        x = _rk4(lambda y: _forward_dynamics(m, y, tau + tau_ext, bp), x, dt)
    return np.array(out)


def test_observer_residual_rises_towards_a_constant_external_torque():
    """d/dt p = tau + C^T nu - g + tau_ext along the fp64 forward dynamics: the residual follows (1 - (1 - gain dt)^k) tau_ext up to
    the discretisation error of the explicit update, which is measured at dt and dt / 2 and has to shrink (first order: about half)."""
    m = _model()
    pos, quat, q, nu, bp = _state(3, far=False)
    rng = np.random.default_rng(77)
    tau, tau_ext = np.zeros(26), np.zeros(26)
    tau[6:24] = rng.uniform(-3, 3, 18)
    tau_ext[LIVE] = rng.uniform(1, 2, 24) * rng.choice([-1.0, 1.0], 24)
    x0 = np.r_[pos, quat, q, nu]
    x0[7 + 18:27] = 0.0; x0[27 + 24:53] = 0.0                    # the locked fingers stay where they are
    gain, dt, steps = 50.0, 2e-3, 16
    errs = []
    for div in (1, 2):
        r = _observed(m, x0, tau, tau_ext, bp, gain, dt / div, steps * div)
        k = np.arange(steps * div + 1)[:, None]
        want = (1.0 - (1.0 - gain * dt / div) ** k) * tau_ext[None]
        errs.append(float(np.abs(r - want).max()))
        gap = np.abs(tau_ext[None] - r)[:, LIVE]
        assert np.all(r[0] == 0) and np.all(r[:, FINGERS] == 0)
        assert np.all(np.diff(gap, axis=0) < 0), "monotone approach, coordinate by coordinate"
        assert np.all(gap[-1] < 0.25 * np.abs(tau_ext[LIVE]))         # 1 - 0.9^16 = 0.81 of the way
    print(f"observer: largest |residual - (1 - (1 - gain dt)^k) tau_ext| at dt {errs[0]:.3g}, at dt / 2 {errs[1]:.3g} (|tau_ext| 1..2)")
    assert errs[1] < 0.75 * errs[0] and errs[0] < 0.25


# ------------------------------------------------------------------------------------------------------------ GPU
def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


def _set_states(env, states):
    root, dof = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    for e, (pos, quat, q, nu, _bp) in enumerate(states):
        root[e, 0] = torch.tensor(np.concatenate([pos, quat, nu[0:6]]), dtype=torch.float32)
        dof[e] = torch.tensor(np.stack([q, nu[6:]], -1), dtype=torch.float32)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    env.sim.tensor("BODY_PARAMS").copy_(torch.tensor(np.array([s[4] for s in states]), dtype=torch.float32))
    torch.cuda.synchronize()


def _downloaded(env):
    """(root [N, 13], dof [N, 20, 2], body_params [N, 20]) of the sim's fp32 state, as float64."""
    return (env.sim.tensor("ROOT_STATES")[:, 0].cpu().numpy().astype(np.float64), env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64),
            env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64))


def _args(env, st, e):
    r64, d64, b64 = st
    return (env.robot_model, r64[e, :3], r64[e, 3:7], d64[e, :, 0], np.r_[r64[e, 7:13], d64[e, :, 1]], b64[e])


@functools.lru_cache(maxsize=None)
def _case(n):
    """An env whose robot e holds member e of the near (e even) or far (e odd) family, and the fp64 reference of every env at the sim's
    DOWNLOADED fp32 state. Computed once and left unchanged."""
    import test_inverse_dynamics as tid
    env = tid._env(n, seed=5, steps=0, gravity=TILTED if n == 64 else None)
    _set_states(env, [_state(e, far=e % 2 == 1) for e in range(n)])
    st = _downloaded(env)
    refs = [cor.coriolis(*_args(env, st, e)) for e in range(n)]
    return env, refs, st


def _launch(env, which=("cmat", "mdot", "vec")):
    """A direct C-ABI call into sentinel-framed buffers; returns {name: [n, ...] tensor} of the outputs asked for."""
    n = env.num_envs
    bufs = {k: _sentinel_buffer(n * SIZES[k]) for k in which}
    ptr = lambda k: bufs[k].data_ptr() if k in bufs else None
    rc = env.sim.L.wbc_sim_coriolis(env.sim.h, ptr("cmat"), ptr("mdot"), ptr("vec"), None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[n * SIZES[k]:] == SENTINEL).all()), k
    shape = {"cmat": (n, 26, 26), "mdot": (n, 26, 26), "vec": (n, 2, 26)}
    return {k: b[:n * SIZES[k]].view(shape[k]).clone() for k, b in bufs.items()}


def _ratios(got, refs):
    g = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    worst = {f: 0.0 for f in FAMILIES}
    for e, (out, mag) in enumerate(refs):
        mine = {"cmat": g["cmat"][e], "mdot": g["mdot"][e], "p": g["vec"][e, 0], "ctnu": g["vec"][e, 1]}
        for f, x in mine.items():
            worst[f] = max(worst[f], cor.largest_ratio(x, out[f], mag[f]))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_and_entry_of_every_output(n):
    env, refs, _ = _case(n)
    before = [env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")]
    got = _launch(env)
    worst = _ratios(got, refs)
    print(f"coriolis n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")
    for f, w in worst.items():
        assert w <= CONST[f], (f, w)
    Cm, Md, vec = got["cmat"], got["mdot"], got["vec"]
    # structure, as equalities
    pairs = torch.tensor(_ancestor_pairs(env.robot_model), device="cuda")
    assert bool((Cm[:, FINGERS] == 0).all()) and bool((Cm[:, :, FINGERS] == 0).all()) and bool((vec[:, :, FINGERS] == 0).all())
    assert bool((Cm[:, 0:3, 0:3] == 0).all()) and bool((Cm[:, :, 0:3] == 0).all())
    assert bool((Cm[:, ~pairs] == 0).all()) and bool((Md[:, ~pairs] == 0).all())
    assert bool((Cm[:, pairs] != 0).any())
    assert torch.equal(Md, Md.transpose(1, 2)) and torch.equal(Md, Cm + Cm.transpose(1, 2))
    # every subset of the outputs has the bits of the full call (vec alone: the vector kernel) and writes nothing else
    for which in (("cmat",), ("mdot",), ("vec",), ("cmat", "vec"), ("mdot", "vec"), ("cmat", "mdot")):
        part = _launch(env, which)
        for k in which:
            assert torch.equal(part[k], got[k]), (which, k)
    # the Python entry points are the same calls
    a, b, c = env.sim.coriolis()
    assert torch.equal(a, Cm) and torch.equal(b, Md) and torch.equal(c, vec)
    only = env.sim.coriolis(vec=torch.empty_like(vec))
    assert len(only) == 1 and torch.equal(only[0], vec)
    assert torch.equal(env.coriolis_matrix(), Cm) and torch.equal(env.mass_matrix_rate(), Md) and torch.equal(env.generalized_momentum(), vec[:, 0])
    torch.cuda.synchronize()
    # the sim's state is read, never written
    for k, t in zip(("ROOT_STATES", "DOF_STATE", "BODY_PARAMS"), before):
        assert torch.equal(env.sim.tensor(k), t), k


@pytest.mark.gpu
def test_translation_and_finger_velocities_leave_every_bit():
    n = 64
    env, _, _ = _case(n)
    want = _launch(env)
    root0, dof0 = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    try:
        root = root0.clone(); root[:, 0, 0:3] += torch.tensor([-57.0, 23.0, 4.5], device="cuda")
        env.sim.set_root_state(root.contiguous())
        moved = _launch(env)
        dof = dof0.clone(); dof[:, 18:, 1] = torch.tensor([7.0, -3.0], device="cuda")
        env.sim.set_dof_state(dof.contiguous())
        fingers = _launch(env)
        alone = _launch(env, ("vec",))
    finally:
        env.sim.set_root_state(root0.contiguous()); env.sim.set_dof_state(dof0.contiguous())
        torch.cuda.synchronize()
    for k in want:
        assert bool(want[k].abs().sum() > 0) and torch.equal(moved[k], want[k]) and torch.equal(fingers[k], want[k]), k
    assert torch.equal(alone["vec"], want["vec"])
    assert all(torch.equal(v, want[k]) for k, v in _launch(env).items())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_agrees_with_the_sibling_kernels(n):
    """cmat @ nu against inverse_dynamics() - gravity_forces(), p against mm_whole @ nu: each difference within the sum of both sides'
    bounds, the product's in units of the sum's magnitude |ref magnitudes| @ |nu|."""
    env, refs, st = _case(n)
    got = _launch(env)
    env.refresh_mass_matrix_tensors()
    h, grav = env.inverse_dynamics(), env.gravity_forces()
    torch.cuda.synchronize()
    Cm, p = got["cmat"].double().cpu().numpy(), got["vec"][:, 0].double().cpu().numpy()
    M, cn = env.mm_whole.double().cpu().numpy(), (h.double() - grav.double()).cpu().numpy()
    g = [float(x) for x in env.tcfg.gravity]
    worst = [0.0, 0.0]
    for e in range(n):
        out, mag = refs[e]
        m, pos, quat, q, nu, bp = _args(env, st, e)
        _, mh = idr.bias_forces(m, pos, quat, q, nu, bp, g)
        _, mg = idr.gravity_forces(m, pos, quat, q, bp, g)
        allow = CONST["cmat"] * EPS * (mag["cmat"] @ np.abs(nu)) + C_ID * EPS * (mh + mg)
        diff = np.abs(Cm[e] @ nu - cn[e])
        assert np.all(diff[FINGERS] == 0) and np.all(diff[LIVE] <= allow[LIVE]), ("cmat nu", e, float((diff[LIVE] / allow[LIVE]).max()))
        worst[0] = max(worst[0], float((diff[LIVE] / allow[LIVE]).max()))
        allow = CONST["p"] * EPS * mag["p"] + MM_REL * np.abs(wb.mass_matrix(m, pos, quat, q, bp)).max() * np.abs(nu).sum()
        diff = np.abs(p[e] - M[e] @ nu)
        assert np.all(diff[FINGERS] == 0) and np.all(diff[LIVE] <= allow[LIVE]), ("p", e, float((diff[LIVE] / allow[LIVE]).max()))
        worst[1] = max(worst[1], float((diff[LIVE] / allow[LIVE]).max()))
    print(f"coriolis n={n} vs siblings: largest difference / allowance: cmat nu vs h - g {worst[0]:.3g}, p vs mm_whole nu {worst[1]:.3g}")


@pytest.mark.gpu
def test_observer_follows_the_recursion_from_its_own_previous_state():
    """Three updates, a different state of the robots before each: after every one `state` is the fp64 recursion restarted from the
    kernel's own previous state, within the vector constants (and the gravity kernel's, times dt)."""
    import test_inverse_dynamics as tid
    n, gain, dt = 13, 40.0, 0.02
    env = tid._env(n, seed=7, steps=0, gravity=TILTED)
    g3 = [float(x) for x in env.tcfg.gravity]
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    tau = ((torch.rand(n, 26, device="cuda", generator=gen) * 2 - 1) * 5).contiguous()
    t64 = tau.double().cpu().numpy()
    state = None
    for step in range(3):
        _set_states(env, [_state(100 * step + e, far=e % 2 == 1) for e in range(n)])
        prev = None if state is None else state.double().cpu().numpy()
        state = env.sim.momentum_observer(tau, gain, dt, reset=step == 0)
        vec = env.sim.coriolis(vec=torch.empty(n, 2, 26, device="cuda"))[0]
        torch.cuda.synchronize()
        got = state.double().cpu().numpy()
        assert state.shape == (n, 2, 26) and bool((state[:, :, FINGERS] == 0).all())
        if step == 0:
            assert torch.equal(state[:, 0], vec[:, 0]) and bool((state[:, 1] == 0).all())
            continue
        st = _downloaded(env)
        worst = 0.0
        for e in range(n):
            m, pos, quat, q, nu, bp = _args(env, st, e)
            o, mag = cor.coriolis(m, pos, quat, q, nu, bp, matrices=False)
            grav, mgrav = idr.gravity_forces(m, pos, quat, q, bp, g3)
            tl = t64[e].copy(); tl[FINGERS] = 0.0
            want = cor.observer_step(prev[e], o["p"], o["ctnu"], grav, tl, gain, dt)
            mi, mr = cor.observer_magnitude(prev[e], mag["p"], mag["ctnu"], 0 * mgrav, tl, gain, dt)
            cv = max(CONST["p"], CONST["ctnu"])
            allow_i = cv * EPS * mi + C_ID * EPS * dt * mgrav
            allow_r = cv * EPS * mr + gain * C_ID * EPS * dt * mgrav
            for x, w, a in ((got[e, 0], want[0], allow_i), (got[e, 1], want[1], allow_r)):
                d = np.abs(x - w)
                assert np.all(d[LIVE] <= a[LIVE]), (step, e, float((d[LIVE] / a[LIVE]).max()))
                worst = max(worst, float((d[LIVE] / a[LIVE]).max()))
        print(f"observer step {step}: largest difference / allowance {worst:.3g}")
    # the env's own entry point: the first call starts the observer, the residual is the second row of its state
    r = env.external_torque_estimate(gain=10.0, reset=True)
    assert r.shape == (n, 26) and bool((r == 0).all())
    r = env.external_torque_estimate(gain=10.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(r).all()) and bool((r[:, FINGERS] == 0).all()) and bool((r[:, LIVE] != 0).any())


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env, _, _ = _case(n)
    want = env.sim.coriolis()
    tau = torch.ones(n, 26, device="cuda")
    st0 = env.sim.momentum_observer(tau, 20.0, 0.01, state=torch.zeros(n, 2, 26, device="cuda"), reset=True).clone()
    want_state = env.sim.momentum_observer(tau, 20.0, 0.01, state=st0.clone()).clone()
    outs = [torch.zeros_like(t) for t in want]
    st = st0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream
        env.sim.coriolis(*outs)
        env.sim.momentum_observer(tau, 20.0, 0.01, state=st.clone())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in outs:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.coriolis(*outs)
        env.sim.momentum_observer(tau, 20.0, 0.01, state=st)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want)) and torch.equal(st, want_state)


@pytest.mark.gpu
def test_every_refusal_leaves_the_buffers_untouched():
    n = 13
    env, _, _ = _case(n)
    L, h = env.sim.L, env.sim.h
    bufs = {k: _sentinel_buffer(n * SIZES[k]) for k in SIZES}
    names = ("sim", "cmat", "mdot", "vec", "stream")
    base = dict(sim=h, stream=None, **{k: b.data_ptr() for k, b in bufs.items()})
    call = lambda **kw: L.wbc_sim_coriolis(*[kw.get(k, base[k]) for k in names])
    refusals = [(dict(sim=None), b"NULL"), (dict(cmat=None, mdot=None, vec=None), b"NULL")]
    refusals += [({k: bufs[k].data_ptr() + off}, b"aligned") for k in ("cmat", "mdot") for off in (1, 2, 4, 8, 12)]
    refusals += [(dict(vec=bufs["vec"].data_ptr() + off), b"aligned") for off in (1, 2, 3)]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_coriolis: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    # the observer
    state, tau = _sentinel_buffer(n * 52), _sentinel_buffer(n * 26)
    onames = ("sim", "tau", "gain", "dt", "flags", "state", "stream")
    obase = dict(sim=h, tau=tau.data_ptr(), gain=10.0, dt=0.01, flags=0, state=state.data_ptr(), stream=None)
    ocall = lambda **kw: L.wbc_sim_momentum_observer(*[kw.get(k, obase[k]) for k in onames])
    orefusals = [(dict(sim=None), b"NULL"), (dict(state=None), b"NULL"), (dict(flags=2), b"flag"), (dict(flags=-2), b"flag"),
                 (dict(gain=0.0), b"gain"), (dict(gain=-1.0), b"gain"), (dict(gain=float("nan")), b"gain"), (dict(gain=float("inf")), b"gain"),
                 (dict(dt=0.0), b"dt"), (dict(dt=-0.01), b"dt"), (dict(dt=float("nan")), b"dt"),
                 (dict(gain=200.0, dt=0.01), b"below 1"), (dict(gain=50.0, dt=0.5), b"below 1")]
    orefusals += [(dict(tau=tau.data_ptr() + off), b"aligned") for off in (1, 2, 3)]
    orefusals += [(dict(state=state.data_ptr() + off), b"aligned") for off in (1, 2, 3)]
    for kw, word in orefusals:
        assert ocall(**kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_momentum_observer: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for b in list(bufs.values()) + [state, tau]:
        assert bool((b == SENTINEL).all())
    # vec needs 4-byte alignment only; a NULL tau is zeros; a reset reads neither tau nor the old state
    want = _launch(env)
    assert call(cmat=None, mdot=None, vec=bufs["vec"].data_ptr() + 4) == 0
    assert ocall(tau=None, flags=abi.OBSERVER_RESET, state=state.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    v = bufs["vec"]
    assert torch.equal(v[1:1 + n * 52].view(n, 2, 26), want["vec"]) and float(v[0]) == SENTINEL and bool((v[1 + n * 52:] == SENTINEL).all())
    s = state[1:1 + n * 52].view(n, 2, 26)
    assert torch.equal(s[:, 0], want["vec"][:, 0]) and bool((s[:, 1] == 0).all()) and float(state[0]) == SENTINEL
    assert bool((state[1 + n * 52:] == SENTINEL).all()) and bool((bufs["cmat"] == SENTINEL).all()) and bool((bufs["mdot"] == SENTINEL).all())


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_calls():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        for _ in range(5):
            if use:
                env.sim.coriolis(); env.external_torque_estimate(gain=5.0)
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.coriolis_matrix(); env.mass_matrix_rate(); env.generalized_momentum()
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
