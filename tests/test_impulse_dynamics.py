"""Contact impulses and post-impact velocities (wbc_sim_impulse_dynamics; csrc/wbc_arm_kernel.hip, definitions in include/wbc_sim.h):
    M (nu+ - nu) = iota + sum_r J_r^T Lambda_r ,    J_r nu+ + damping Lambda_r = vdes_r - e_r (u_r - vdes_r) ,   u_r = J_r nu.
The CPU tests pin the fp64 reference of tests/impulse_reference.py to its own residuals, to the free jump nu + M^-1 iota, to the
projector and energy identities, and measure the fp32 yardstick; the GPU tests hold the kernels' own outputs to the fp64 system row by
row, to their exact guarantees and to their invariances.

Bounds (impulse_reference.py, residual form, EPS = 2^-24): K_ref is the fp32 yardstick's largest ratio over 60 members of _family below
(asserted <= C / 16 on the CPU), C the smallest power of two >= 16 K_ref and not below 32, and the last column the kernel's largest
ratio on an MI355X (n = 1, 13, 64 and every case of the GPU tests):

    rows                                         K_ref     C      kernel's largest ratio
    momentum rows (C_P)                          0.665     32     0.902
    contact rows (C_V)                           9.21      256    8.05
    energy (C_E)                                 0.256     32     0.388
    map rows |P nu - nu+| (C_M)                  0.633     32     0.798
    |Jc P| for e = 0, damping = 0 (C_J)          49.5      1024   19.0

The pre-impact contact velocity u enters the contact rows. Two forms were run through the yardstick over the same family: the velocity
walk (omega and the origin's velocity relative to the root's linear motion, carried down the tree) and the 24-term product
fl(J) fl(nu). The largest |u_f32 - u_ref| / (2^-24 sum_c |J_ic| |nu_c|) is 4.76 for the walk and 2.43 for the product, and the contact
rows' K_ref is 9.75 with the walk and 9.21 with the product. The kernel uses the product (asserted to be the smaller on both counts).

The impulses iota of the family and of the GPU cases are sized by each coordinate's own inertia (_impulse_rhs, which says why and what
a first form of the cases measured).

The largest condition number of the diagonally scaled Delassus matrix is 85.2 over the CPU family and 4.16 over the GPU cases
(asserted <= 1000 for both). Plastic touchdown applied twice: the second call's largest impulse is 0.0083 of its allowance.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import arm_codegen
import impulse_reference as ir
import mass_solve_reference as msr
from wbc_amd import abi

FINGERS, LIVE, EPS = ir.FINGERS, ir.LIVE, ir.EPS
C_P, C_V, C_E, C_M, C_J = ir.C_P, ir.C_V, ir.C_E, ir.C_M, ir.C_J
COND_MAX = 1000.0
SENTINEL = 12345.0
RESTITUTIONS = (0.0, 0.5, 1.0)


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


def _f32(a):
    return None if a is None else np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


JUMP = np.r_[np.full(3, 1.0), np.full(3, 2.0), np.full(20, 3.0)]                 # the velocity ranges of test_mass_solve._random_state


def _velocity_jumps(rng, shape):
    """[..., 26] velocity changes, uniform within the ranges the states' own velocities are drawn from (1 m/s, 2 rad/s, 3 rad/s)."""
    return rng.uniform(-1, 1, tuple(shape) + (26,)) * JUMP


def _impulse_rhs(M, jumps):
    """Generalised impulses [..., 26], fp32 values: iota_c = M_cc jump_c, the impulse that changes coordinate c's velocity by jump_c if
    it acted on that coordinate alone (linear rows about +-15 N s on this robot). So a push is as large as the motion the state already
    has, coordinate by coordinate, whatever the coordinate's inertia: an impulse drawn in N m s without regard to it (0.5 N m s, say)
    would send the wrist joints, whose inertias are near 1e-4 kg m^2, to thousands of rad/s. At such a velocity the absolute error
    of a Jacobian entry that is small by cancellation (the gripper's origin lies on the wrist-roll axis; its lever is the difference of
    two points half a metre from the root, so fp32 leaves about 3e-8 m of it) reaches 1e-4 m/s in a contact row, and no scale made of
    |J_ic| |nu_c| covers that: a first form of these cases, which drew the impulses that way, measured 280 x 2^-24 of the contact
    rows' scale on an MI355X (n = 64, feet + gripper, env 42, a gripper row, wrist roll at 5484 rad/s), all of it (J_ref - J_kernel) dnu."""
    return _f32(np.diagonal(M, axis1=-2, axis2=-1) * jumps)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_null_and_bad_arguments_are_rejected_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 2)(3, 7)
    p = (C.addressof(buf) + 15) & ~15                                             # 16-byte aligned, 48 floats behind it
    call = lambda **kw: L.wbc_sim_impulse_dynamics(*[kw.get(k, d) for k, d in (
        ("sim", None), ("rb", idx), ("k", 2), ("active", None), ("e", None), ("vdes", None), ("iota", None), ("damping", 0.0), ("flags", 0),
        ("nu_plus", p), ("lam", None), ("den", None), ("map", None), ("ws", p), ("stream", None))])
    assert call() == -1
    assert b"wbc_sim_impulse_dynamics: sim is NULL" in L.wbc_last_error()
    sim = None                                                                     # the argument checks that need no sim come first
    for kw, word in ((dict(rb=None), b"NULL"), (dict(nu_plus=None), b"NULL"), (dict(ws=None), b"NULL"),
                     (dict(k=0), b"nbodies"), (dict(k=6), b"nbodies"),
                     (dict(damping=-1.0), b"damping"), (dict(damping=float("nan")), b"damping"), (dict(damping=float("inf")), b"damping"),
                     (dict(flags=2), b"flag"), (dict(nu_plus=p + 2), b"4-byte"), (dict(iota=p + 1), b"4-byte"), (dict(lam=p + 2), b"4-byte"),
                     (dict(map=p + 8), b"16-byte")):
        assert call(sim=sim, **kw) == -1, kw
        msg = L.wbc_last_error()
        assert msg.startswith(b"wbc_sim_impulse_dynamics: ") and word in msg, (kw, msg)
    assert L.wbc_sim_impulse_dynamics_workspace_floats(10, 4) == 10 * 2 * 13 * 26
    for bad in ((10, 0), (10, 6), (0, 4), (-1, 4)):
        assert L.wbc_sim_impulse_dynamics_workspace_floats(*bad) == 0


def test_new_kernels_codegen():
    """Both kernels (and the map variant of the solve) exist, no scratch, no flat memory instructions, static LDS within the 20 kB that
    keep eight workgroups per CU; the variant without the map asks for no more LDS than the sibling solve."""
    for kernel in ("wbc_impulse_rhs_kernel", "wbc_impulse_solve_kernel", "wbc_impulse_solve_map_kernel"):
        assert arm_codegen.meta(kernel, "private_segment_fixed_size") == 0, kernel
        assert arm_codegen.meta(kernel, "max_flat_workgroup_size") == 64, kernel
        assert arm_codegen.meta(kernel, "group_segment_fixed_size") <= 20 * 1024, kernel
        body = arm_codegen.body(kernel)
        assert "s_endpgm" in body and re.search(r"\bglobal_store_dword", body), kernel
        assert not re.search(r"\bflat_", body) and "scratch_" not in body, kernel
    assert (arm_codegen.meta("wbc_impulse_solve_kernel", "group_segment_fixed_size")
            <= arm_codegen.meta("wbc_constraint_solve_kernel", "group_segment_fixed_size"))
    assert re.search(r"\bglobal_store_dwordx4", arm_codegen.body("wbc_impulse_solve_map_kernel"))


def _family(m, seed, arm_vec):
    """One member of the family the yardstick runs over, modelled on test_constrained_dynamics._family (the same state and
    body-parameter generators): (state, bodies, on [3K], e [3K], vdes [3K] or None, velocity jumps [26] of iota or None (_impulse_rhs), damping, armature or None).
    seed % 3: feet with 0..4 of them active (every count) / feet + gripper with per-body restitution / gripper alone."""
    rng = np.random.default_rng(500 + seed)
    pos, quat, q, nu = _random_state(rng)
    bp = _random_body_params(m, rng)
    feet, grip = _bodies(m)
    bodies = [feet, feet + [grip], [grip]][seed % 3]
    K = len(bodies)
    active = np.ones(K, dtype=bool)
    if seed % 3 == 0:
        active[:] = False
        active[rng.permutation(4)[:(seed // 3) % 5]] = True
    e = np.full(K, RESTITUTIONS[(seed // 3) % 3])
    if seed % 3 == 1:
        e = rng.choice(RESTITUTIONS, K)
    vdes = _f32(rng.uniform(-1, 1, 3 * K)) if seed % 5 < 3 else None
    jumps = _velocity_jumps(rng, ()) if seed % 7 < 4 else None
    damping = 1e-3 if seed % 4 == 3 else 0.0
    return (pos, quat, q, nu, bp), bodies, np.repeat(active, 3), np.repeat(e, 3), vdes, jumps, damping, (arm_vec if seed % 2 else None)


def _system(m, state, bodies, on, armature):
    pos, quat, q, nu, bp = state
    M = msr.mass_matrix(m, pos, quat, q, bp, armature)
    Jc, u = ir.contact_rows(m, pos, quat, q, nu, bodies, on[::3])
    return M, Jc, u


def _jp_ratio(r, s, on):
    """Largest |Jc P| / (2^-24 scale) over the active rows; where the scale is 0 (a column no active row depends on) so is Jc P."""
    r, s = r[on][:, LIVE], s[on][:, LIVE]
    assert np.all(r[s == 0] == 0) and np.any(s > 0)
    return float((r[s > 0] / (EPS * s[s > 0])).max())


def _model_and_armature():
    from wbc_amd.config import WidowGo1RoughCfg
    m = abi.load_default_model()
    return m, msr.armature_vector(abi.fill_task_cfg(WidowGo1RoughCfg(), m))


def test_reference_satisfies_both_residuals_and_reduces_to_the_free_jump(robot):
    m = robot["model"]
    A = msr.armature_vector(robot["tcfg"])
    for seed in range(15):
        state, bodies, on, e, vdes, jumps, damping, arm = _family(m, seed, A)
        nu = state[3]
        M, Jc, u = _system(m, state, bodies, on, arm)
        iota = None if jumps is None else _impulse_rhs(M, jumps)
        t = np.where(on, ir.target(u, e, vdes), 0.0)
        nu_plus, lam = ir.solve_with_mask(M, Jc, nu, t, iota, damping, on)
        assert np.all(nu_plus[FINGERS] == 0) and np.all(lam[~on] == 0)
        r, s = ir.momentum_residual_and_scale(M, nu, nu_plus, iota, Jc, lam)
        assert np.all(r[LIVE] <= 1e-10 * s[LIVE])
        r, s = ir.contact_residual_and_scale(Jc, nu, nu_plus, lam, t, np.where(on, e, 0.0), damping)
        assert np.all(r[on] <= 1e-10 * s[on]) and np.all(r[~on] == 0)
        # the walk's u is the Jacobian's
        uw = ir.contact_velocities(m, state[1], state[2], nu, bodies)
        assert np.abs(uw - u).max() <= 1e-12 * max(1.0, np.abs(u).max())
        free, lam0 = ir.solve_with_mask(M, Jc, nu, t, iota, damping, np.zeros_like(on))
        want = np.where(np.isin(np.arange(26), FINGERS), 0.0, nu) + msr.solve(M, np.zeros(26) if iota is None else iota)
        assert np.all(lam0 == 0) and np.abs(free - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        # nu+ = P nu + (the affine part), and P alone where there is none
        P = ir.impact_map(M, Jc, e, damping, on)
        assert np.all(P[FINGERS] == 0) and np.all(P[:, FINGERS] == 0)
        lin, _ = ir.solve_with_mask(M, Jc, nu, np.where(on, ir.target(u, e, None), 0.0), None, damping, on)
        assert np.abs(P @ nu - lin).max() <= 1e-10 * max(1.0, np.abs(nu).max())


def test_reference_projector_and_energy_identities(robot):
    m = robot["model"]
    A = msr.armature_vector(robot["tcfg"])
    seen_loss = 0
    for seed in range(30):
        state, bodies, on, _e, _vdes, _iota, damping, arm = _family(m, seed, A)
        nu = state[3]
        M, Jc, u = _system(m, state, bodies, on, arm)
        zero = np.zeros(len(on))
        P = ir.impact_map(M, Jc, zero, 0.0, on)
        assert np.abs(P @ P - P).max() <= 1e-10 * max(1.0, np.abs(P).max())
        r, s = ir.jp_residual_and_scale(M, Jc, P, on)
        assert np.all(r[on] <= 1e-10 * np.maximum(s[on], 1e-300))
        for e in (0.0, 0.3, 0.5, 1.0):
            t = np.where(on, ir.target(u, np.full(len(on), e), None), 0.0)
            nu_plus, lam = ir.solve_with_mask(M, Jc, nu, t, None, damping, on)
            dT = ir.delta_energy(M, nu, nu_plus)
            scale = ir.energy_scale(M, nu, nu_plus)
            assert dT <= 1e-12 * scale, (seed, e, dT)
            assert abs(dT - ir.energy_identity(lam, np.where(on, u, 0.0), e, damping)) <= 1e-12 * scale
            seen_loss += dT < -1e-3 * scale
    assert seen_loss >= 30


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref of the five bounds, the two forms of u and the largest scaled condition number, over 60 members of _family."""
    m, A = _model_and_armature()
    k = dict(momentum=0.0, contact=0.0, energy=0.0, map=0.0, jp=0.0, u_walk=0.0, u_product=0.0, contact_walk=0.0, cond=0.0)
    seen = dict(counts=set(), e=set(), vdes=set(), iota=set(), damping=set(), armature=set())
    for seed in range(60):
        state, bodies, on, e, vdes, jumps, damping, arm = _family(m, seed, A)
        pos, quat, q, nu, _bp = state
        nu32 = _f32(nu)
        M, Jc, _ = _system(m, state, bodies, on, arm)
        iota = None if jumps is None else _impulse_rhs(M, jumps)
        Jall, u = ir.contact_rows(m, pos, quat, q, nu32, bodies)
        seen["counts"].add((len(bodies), int(on.sum()) // 3)); seen["e"] |= set(e[on].tolist()); seen["vdes"].add(vdes is None)
        seen["iota"].add(iota is None); seen["damping"].add(damping); seen["armature"].add(arm is None)
        k["cond"] = max(k["cond"], ir.delassus_condition(M, Jc, damping, on))
        e_on, vd_on = np.where(on, e, 0.0), (None if vdes is None else np.where(on, vdes, 0.0))
        t = np.where(on, ir.target(u, e, vdes), 0.0)
        mag = ir.velocity_magnitude(Jall, nu32)
        u_forms = {"walk": ir.contact_velocities(m, quat, q, nu32, bodies, dtype=np.float32), "product": ir.product_f32(Jall, nu32)}
        for form, u32 in u_forms.items():
            k["u_" + form] = max(k["u_" + form], float((np.abs(u32 - u) / (EPS * mag)).max()))
        for form, u32 in u_forms.items():
            nu_plus, lam, den, P = ir.yardstick_f32(M, Jc, u32, nu32, e_on, vd_on, iota, damping, on, want_map=form == "product")
            if on.any():
                r, s = ir.contact_residual_and_scale(Jc, nu32, nu_plus, lam, t, e_on, damping)
                key = "contact" if form == "product" else "contact_walk"
                k[key] = max(k[key], float((r[on] / (EPS * s[on])).max()))
            if form != "product":
                continue
            r, s = ir.momentum_residual_and_scale(M, nu32, nu_plus, iota, Jc, lam)
            k["momentum"] = max(k["momentum"], float((r[LIVE] / (EPS * s[LIVE])).max()))
            k["energy"] = max(k["energy"], abs(den - ir.delta_energy(M, nu32, nu_plus)) / (EPS * ir.energy_scale(M, nu32, nu_plus, iota)))
            if vdes is None and iota is None:
                r, s = ir.map_residual_and_scale(M, P, nu32, nu_plus)
                k["map"] = max(k["map"], float((r[LIVE] / (EPS * s[LIVE])).max()))
        if on.any():                                                                # the plastic map of the same rows, without damping
            _, _, _, P0 = ir.yardstick_f32(M, Jc, np.zeros(len(on)), nu32, np.zeros(len(on)), None, None, 0.0, on)
            r, s = ir.jp_residual_and_scale(M, Jc, P0, on)
            k["jp"] = max(k["jp"], _jp_ratio(r, s, on))
    assert {(4, c) for c in range(5)} <= seen["counts"] and (5, 5) in seen["counts"] and (1, 1) in seen["counts"]
    assert seen["e"] == set(RESTITUTIONS) and seen["damping"] == {0.0, 1e-3}
    assert all(seen[key] == {True, False} for key in ("vdes", "iota", "armature"))
    return k


def test_fp32_yardsticks_sit_well_inside_the_bounds():
    k = _yardsticks()
    print("yardsticks: " + ", ".join(f"{name} {v:.4g}" for name, v in k.items()) + f"; constants {ir.CONSTANTS}")
    for name, c in ir.CONSTANTS.items():
        assert k[name] <= c / 16, (name, k[name], c)
        assert c == ir.constant_for(k[name]), (name, k[name], c)
    # the form of u the kernel uses, the product, is the one with the smaller ratio, alone and through the contact rows
    assert k["u_product"] <= k["u_walk"] and k["contact"] <= k["contact_walk"]


def test_delassus_conditioning_of_the_family():
    assert _yardsticks()["cond"] <= COND_MAX


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _case(n):
    """test_mass_solve._case(n)'s env and M_ref plus, per env, the fp64 linear Jacobian rows of the feet and the gripper [n, 5, 3, 26]
    and the fp32 state's nu [n, 26]. Computed once and left unchanged."""
    import test_mass_solve as tms
    import whole_body_reference as wb
    env, M, _, _, (root, q, qd, _bp) = tms._case(n)
    m = env.robot_model
    feet, grip = _bodies(m)
    J = np.array([wb.jacobian(m, root[e, :3], root[e, 3:7], q[e])[feet + [grip], 0:3] for e in range(n)])
    return env, M, J, np.concatenate([root[:, 7:13], qd], axis=1)


def _sentinel_buffer(numel, tail=8):
    return torch.full((numel + tail,), SENTINEL, dtype=torch.float32, device="cuda")


def _masks(n, K):
    """Stance masks [n, K] u8: env e has the feet of the bits of e % 16 active (all 16 patterns, so every count 0..4, at n = 64; none
    active at env 0 of every n), a fifth body active on odd envs."""
    e = torch.arange(n, device="cuda")
    return torch.stack([((e >> k) & 1) if k < 4 else (e & 1) for k in range(K)], 1).to(torch.uint8).contiguous()


_WORST = {"momentum": 0.0, "contact": 0.0, "energy": 0.0, "map": 0.0, "jp": 0.0, "cond": 0.0}


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def _check(n, rows, active, e, vdes, iota, damping, armature, nu_plus, lam, den=None, P=None):
    """The bounds for every env and row, from the kernel's own outputs against the fp64 system; rows: indices into _case's five bodies.
    e [n, K] / vdes [n, K, 3] / iota [n, 26]: numpy or None, with zeros (not NaN) where inactive. Returns the largest ratios."""
    env, M, J, nu = _case(n)
    if armature:
        M = M + np.diag(msr.armature_vector(env.tcfg))
    K = len(rows)
    npl, lm = _np(nu_plus), _np(lam).reshape(n, 3 * K)
    assert np.isfinite(npl).all() and np.isfinite(lm).all() and np.all(npl[:, FINGERS] == 0)
    act = np.ones((n, K), dtype=bool) if active is None else _np(active).astype(bool)
    dn, Pk = _np(den), _np(P)
    w = dict.fromkeys(("momentum", "contact", "energy", "map", "jp"), 0.0)
    for i in range(n):
        on = np.repeat(act[i], 3)
        assert np.all(lm[i][~on] == 0)
        Jall = J[i, rows].reshape(3 * K, 26)
        Jc, u = Jall * on[:, None], Jall @ nu[i]
        er = np.where(on, np.repeat(np.zeros(K) if e is None else e[i], 3), 0.0)
        vd = None if vdes is None else np.where(on, vdes[i].reshape(3 * K), 0.0)
        io = None if iota is None else np.where(np.isin(np.arange(26), FINGERS), 0.0, iota[i])
        t = np.where(on, ir.target(u, er, vd), 0.0)
        cond = ir.delassus_condition(M[i], Jc, damping, on)
        assert cond <= COND_MAX, (i, cond)
        _WORST["cond"] = max(_WORST["cond"], cond)
        r, s = ir.momentum_residual_and_scale(M[i], nu[i], npl[i], io, Jc, lm[i])
        assert np.all(s[LIVE] > 0)
        assert np.all(r[LIVE] <= C_P * EPS * s[LIVE]), ("momentum", i, float((r[LIVE] / (EPS * s[LIVE])).max()))
        w["momentum"] = max(w["momentum"], float((r[LIVE] / (EPS * s[LIVE])).max()))
        if on.any():
            r, s = ir.contact_residual_and_scale(Jc, nu[i], npl[i], lm[i], t, er, damping)
            assert np.all(s[on] > 0)
            assert np.all(r[on] <= C_V * EPS * s[on]), ("contact", i, float((r[on] / (EPS * s[on])).max()))
            w["contact"] = max(w["contact"], float((r[on] / (EPS * s[on])).max()))
        if dn is not None:
            r, s = abs(dn[i] - ir.delta_energy(M[i], nu[i], npl[i])), ir.energy_scale(M[i], nu[i], npl[i], io)
            assert r <= C_E * EPS * s, ("energy", i, r / (EPS * s))
            w["energy"] = max(w["energy"], r / (EPS * s))
        if Pk is not None:
            assert np.isfinite(Pk[i]).all() and np.all(Pk[i][FINGERS] == 0) and np.all(Pk[i][:, FINGERS] == 0)
            if vdes is None and iota is None:
                r, s = ir.map_residual_and_scale(M[i], Pk[i], nu[i], npl[i])
                assert np.all(r[LIVE] <= C_M * EPS * s[LIVE]), ("map", i, float((r[LIVE] / (EPS * s[LIVE])).max()))
                w["map"] = max(w["map"], float((r[LIVE] / (EPS * s[LIVE])).max()))
            if on.any() and damping == 0.0 and not er.any():
                r, s = ir.jp_residual_and_scale(M[i], Jc, Pk[i], on)
                assert np.all(r[on] <= C_J * EPS * s[on]), ("jp", i, _jp_ratio(r, s, on))
                w["jp"] = max(w["jp"], _jp_ratio(r, s, on))
            if not on.any():
                assert np.array_equal(Pk[i][np.ix_(LIVE, LIVE)], np.eye(len(LIVE)))
    for key, v in w.items():
        _WORST[key] = max(_WORST[key], v)
    return w


def _raw_call(sim, bodies, active, e, vdes, iota, damping, armature, want_lam=True, want_den=True, want_map=False):
    """wbc_sim_impulse_dynamics through ctypes into sentinel-tailed buffers; returns (nu_plus, lam, den, P) views (None where not asked
    for) after checking that nothing was written past any of them or into an output that was not handed in."""
    L, n, K = sim.L, sim.num_envs, len(bodies)
    nws = int(L.wbc_sim_impulse_dynamics_workspace_floats(n, K))
    assert nws == n * 2 * (3 * K + 1) * 26
    sizes = dict(nu=n * 26, lam=n * 3 * K, den=n, map=n * 676, ws=nws)
    buf = {k: _sentinel_buffer(v) for k, v in sizes.items()}
    ptr = lambda t: t.data_ptr() if t is not None else None
    rc = L.wbc_sim_impulse_dynamics(sim.h, (C.c_int32 * K)(*bodies), K, ptr(active), ptr(e), ptr(vdes), ptr(iota), damping, 1 if armature else 0,
                                    buf["nu"].data_ptr(), buf["lam"].data_ptr() if want_lam else None,
                                    buf["den"].data_ptr() if want_den else None, buf["map"].data_ptr() if want_map else None,
                                    buf["ws"].data_ptr(), None)
    assert rc == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    for k, v in sizes.items():
        assert bool((buf[k][v:] == SENTINEL).all()), k
    for k, asked in (("lam", want_lam), ("den", want_den), ("map", want_map)):
        assert asked or bool((buf[k] == SENTINEL).all()), k
    return (buf["nu"][:n * 26].view(n, 26), buf["lam"][:n * 3 * K].view(n, K, 3) if want_lam else None,
            buf["den"][:n] if want_den else None, buf["map"][:n * 676].view(n, 26, 26) if want_map else None)


CASES = ["feet", "feet_masked", "feet_gripper_vdes", "gripper", "armature", "damping", "iota_only", "impulse_null"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [1, 13, 64])
def test_impulse_dynamics_every_env_and_row(n, case):
    env = _case(n)[0]
    sim = env.sim
    feet, grip = _bodies(env.robot_model)
    rng = np.random.default_rng(211)
    dev = dict(dtype=torch.float32, device="cuda")
    rows, active, e, vdes, iota, damping, armature = [0, 1, 2, 3], None, None, None, None, 0.0, False
    if case == "feet_masked":
        active = _masks(n, 4)
        e = torch.full((n, 4), 0.5, **dev)
        vdes = torch.tensor(rng.uniform(-1, 1, (n, 4, 3)), **dev)
    elif case == "feet_gripper_vdes":
        rows = [0, 1, 2, 3, 4]
        e = torch.tensor(rng.choice(RESTITUTIONS, (n, 5)), **dev)
        vdes = torch.tensor(rng.uniform(-1, 1, (n, 5, 3)), **dev)
        iota = torch.tensor(_impulse_rhs(_case(n)[1], _velocity_jumps(rng, (n,))), **dev)
    elif case == "gripper":
        rows = [4]
        e = torch.ones((n, 1), **dev)
    elif case == "armature":
        armature = True
        iota = torch.tensor(_impulse_rhs(_case(n)[1], _velocity_jumps(rng, (n,))), **dev)
    elif case == "damping":
        damping = 1e-3
        e = torch.full((n, 4), 0.5, **dev)
    elif case == "iota_only":
        active = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
        iota = torch.tensor(_impulse_rhs(_case(n)[1], _velocity_jumps(rng, (n,))), **dev)
    bodies = [(feet + [grip])[r] for r in rows]
    e_in, v_in = e, vdes
    if case == "feet_masked":                                                      # NaN where inactive: never loaded into arithmetic
        e_in, v_in = e.clone(), vdes.clone()
        e_in[active == 0] = float("nan")
        v_in[active == 0] = float("nan")
    nu_plus, lam, den, _ = _raw_call(sim, bodies, active, e_in, v_in, iota, damping, armature, want_lam=case != "impulse_null")
    nu2, lam2, den2, P = _raw_call(sim, bodies, active, e_in, v_in, iota, damping, armature, want_map=True)
    # the outputs with and without the map agree bit for bit
    assert torch.equal(nu_plus, nu2) and torch.equal(den, den2) and (lam is None or torch.equal(lam, lam2))
    # the Python entry point is the same call
    kw = dict(active=None if active is None else active.bool(), restitution=e_in, vel_des=v_in, impulse_ext=iota, damping=damping,
              armature=armature)
    if case == "damping":
        kw["restitution"] = 0.5                                                    # a Python float is broadcast
    r = sim.impulse_dynamics(bodies, want_map=True, want_energy=True, **kw)
    assert torch.equal(r["nu_plus"], nu2) and torch.equal(r["impulse"], lam2) and torch.equal(r["denergy"], den2) and torch.equal(r["dnu_dnu"], P)
    r = sim.impulse_dynamics(bodies, workspace=torch.empty(int(sim.L.wbc_sim_impulse_dynamics_workspace_floats(n, len(rows))), **dev), **kw)
    assert set(r) == {"nu_plus", "impulse"} and torch.equal(r["nu_plus"], nu2) and torch.equal(r["impulse"], lam2)
    if case == "feet":
        a, b, c = env.touchdown_impact()
        assert torch.equal(a, nu2) and torch.equal(b, lam2) and torch.equal(c, den2) and torch.equal(env.impact_map(), P)
    if case == "feet_masked":
        a, b, c = env.touchdown_impact(stance=active.bool(), restitution=0.25)
        er = np.full((n, 4), 0.25)
        _check(n, rows, active, er, None, None, 0.0, False, a, b, c, env.impact_map(stance=active.bool(), restitution=0.25))
    w = _check(n, rows, active, _np(e), _np(vdes), _np(iota), damping, armature, nu2, lam2, den2, P)
    print(f"impulse dynamics n={n} {case}: largest ratios {({k: round(v, 3) for k, v in w.items()})}; running maxima "
          f"{({k: round(v, 3) for k, v in _WORST.items()})}")
    if case == "iota_only":                                                        # no active body: the free jump, no impulses
        assert bool((lam2 == 0).all())


@pytest.mark.gpu
def test_exact_guarantees_with_no_active_body_and_no_iota():
    n = 13
    env, _, _, nu = _case(n)
    feet, grip = _bodies(env.robot_model)
    none = torch.zeros((n, 5), dtype=torch.uint8, device="cuda")
    nan = torch.full((n, 5, 3), float("nan"), dtype=torch.float32, device="cuda")
    nu_plus, lam, den, P = _raw_call(env.sim, feet + [grip], none, nan[:, :, 0].contiguous(), nan, None, 1e-3, True, want_map=True)
    state = torch.tensor(nu, dtype=torch.float32, device="cuda")
    assert torch.equal(nu_plus[:, LIVE].view(torch.int32), state[:, LIVE].view(torch.int32))
    assert bool((nu_plus[:, FINGERS] == 0).all()) and bool((lam == 0).all()) and bool((den == 0).all())
    eye = torch.zeros(26, 26, device="cuda")
    eye[LIVE, LIVE] = 1.0
    assert bool((P == eye).all())


@pytest.mark.gpu
@pytest.mark.parametrize("e", RESTITUTIONS)
def test_an_impact_never_adds_energy(e):
    """0 <= e <= 1, no iota, surfaces at rest: denergy <= its allowance, < 0 wherever the reference's loss exceeds 100 allowances, and
    within the allowance of 0 for e = 1 without damping."""
    n = 64
    env, M, J, nu = _case(n)
    feet, _ = _bodies(env.robot_model)
    for damping in (0.0, 1e-3):
        r = env.sim.impulse_dynamics(feet, restitution=e, damping=damping, want_energy=True)
        torch.cuda.synchronize()
        den, npl = _np(r["denergy"]), _np(r["nu_plus"])
        lost = 0
        for i in range(n):
            allow = C_E * EPS * ir.energy_scale(M[i], nu[i], npl[i])
            assert den[i] <= allow, (i, den[i], allow)
            Jc = J[i, :4].reshape(12, 26)
            on = np.ones(12, dtype=bool)
            ref_plus, _ = ir.solve_with_mask(M[i], Jc, nu[i], ir.target(Jc @ nu[i], np.full(12, e), None), None, damping, on)
            if ir.delta_energy(M[i], nu[i], ref_plus) < -100 * allow:
                assert den[i] < 0, (i, den[i])
                lost += 1
            if e == 1.0 and damping == 0.0:
                assert abs(den[i]) <= allow, (i, den[i], allow)
        assert lost >= n // 2 or e == 1.0, (e, damping, lost)                  # the strict sign is checked somewhere


@pytest.mark.gpu
def test_a_plastic_touchdown_applied_twice_gives_no_second_impulse():
    """touchdown_impact(apply=True) leaves J nu+ = r with |r_i| <= C_V 2^-24 scale_i (the contact rows' bound); the second call answers
    with Lambda = -A^-1 r up to its own rounding of the same form, so |Lambda_2| <= C_V 2^-24 |A^-1| (scale_1 + scale_2): the first
    call's impulse magnitude |A^-1| |u| with |u| replaced by the rows' scales."""
    import test_inverse_dynamics as tid
    import whole_body_reference as wb
    n = 13
    env = tid._env(n, seed=7, steps=6)
    m = env.robot_model
    feet, _ = _bodies(m)
    root0, dof0 = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    nu1, lam1, _ = env.touchdown_impact()                                          # the default leaves the sim as it is
    assert torch.equal(env.sim.tensor("ROOT_STATES"), root0) and torch.equal(env.sim.tensor("DOF_STATE"), dof0)
    nu1b, lam1b, _ = env.touchdown_impact(apply=True)
    torch.cuda.synchronize()
    assert torch.equal(nu1, nu1b) and torch.equal(lam1, lam1b)
    root1, dof1 = env.sim.tensor("ROOT_STATES"), env.sim.tensor("DOF_STATE")
    assert torch.equal(root1[:, 0, :7], root0[:, 0, :7]) and torch.equal(root1[:, 1], root0[:, 1]) and torch.equal(dof1[..., 0], dof0[..., 0])
    assert torch.equal(root1[:, 0, 7:13], nu1[:, :6]) and torch.equal(dof1[:, :-2, 1], nu1[:, 6:-2]) and torch.equal(dof1[:, -2:], dof0[:, -2:])
    nu2, lam2, _ = env.touchdown_impact()
    torch.cuda.synchronize()
    root, q = _np(root0[:, 0]), _np(dof0[..., 0])
    bp = _np(env.sim.tensor("BODY_PARAMS"))
    v0, v1, v2, l1, l2 = np.concatenate([root[:, 7:13], _np(dof0[..., 1])], 1), _np(nu1), _np(nu2), _np(lam1).reshape(n, 12), _np(lam2).reshape(n, 12)
    worst = 0.0
    for i in range(n):
        M = wb.mass_matrix(m, root[i, :3], root[i, 3:7], q[i], bp[i])
        Jc = wb.jacobian(m, root[i, :3], root[i, 3:7], q[i])[feet, 0:3].reshape(12, 26)
        assert ir.delassus_condition(M, Jc, 0.0, np.ones(12, dtype=bool)) <= COND_MAX
        zero = np.zeros(12)
        _, s1 = ir.contact_residual_and_scale(Jc, v0[i], v1[i], l1[i], zero, zero, 0.0)
        _, s2 = ir.contact_residual_and_scale(Jc, v1[i], v2[i], l2[i], zero, zero, 0.0)
        Ainv = np.linalg.inv(Jc[:, LIVE] @ np.linalg.solve(M[np.ix_(LIVE, LIVE)], Jc[:, LIVE].T))
        allow = C_V * EPS * (np.abs(Ainv) @ (s1 + s2))
        assert np.abs(l1[i]).max() > 10 * allow.max(), (i, np.abs(l1[i]).max(), allow.max())   # the allowance is small beside the first impulses
        assert np.all(np.abs(l2[i]) <= allow), (i, float((np.abs(l2[i]) / allow).max()))
        worst = max(worst, float((np.abs(l2[i]) / allow).max()))
    print(f"plastic touchdown twice: largest |second impulse| / allowance = {worst:.3g}")


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    feet, grip = _bodies(robot["model"])
    rng = np.random.default_rng(223)
    dev = dict(dtype=torch.float32, device="cuda")
    vdes, iota = torch.tensor(rng.uniform(-1, 1, (n, 5, 3)), **dev), torch.tensor(_impulse_rhs(_case(n)[1], _velocity_jumps(rng, (n,))), **dev)
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        assert float((env.root_states[:, 1] - (-2.0 + shift[1])).abs().max()) < 1e-4
        r = env.sim.impulse_dynamics(feet + [grip], active=_masks(n, 5), restitution=0.5, vel_des=vdes, impulse_ext=iota, damping=1e-3,
                                     want_map=True, want_energy=True)
        torch.cuda.synchronize()
        outs.append([r[k].clone() for k in ("nu_plus", "impulse", "denergy", "dnu_dnu")])
    for x, y in zip(*outs):
        assert bool(x.abs().sum() > 0) and torch.equal(x, y)


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env = _case(n)[0]
    feet, grip = _bodies(env.robot_model)
    bodies = feet + [grip]
    dev = dict(dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(227)
    iota, e = torch.tensor(_impulse_rhs(_case(n)[1], _velocity_jumps(rng, (n,))), **dev), torch.full((n, 5), 0.5, **dev)
    kw = dict(active=_masks(n, 5), restitution=e, impulse_ext=iota, damping=1e-3, want_map=True, want_energy=True)
    want = env.sim.impulse_dynamics(bodies, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # warm-up off the default stream (the workspace exists already)
        env.sim.impulse_dynamics(bodies, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = env.sim.impulse_dynamics(bodies, **kw)
    for t in got.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
        assert bool(want[k].abs().sum() > 0) and torch.equal(got[k], want[k]), k


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env = _case(n)[0]
    m = env.robot_model
    feet, grip = _bodies(m)
    L, h = env.sim.L, env.sim.h
    K = 4
    nu, lam, den, P = _sentinel_buffer(n * 26), _sentinel_buffer(n * 15), _sentinel_buffer(n), _sentinel_buffer(n * 676)
    ws = _sentinel_buffer(int(L.wbc_sim_impulse_dynamics_workspace_floats(n, 5)))
    x = torch.ones(n, 26, device="cuda")
    idx = (C.c_int32 * 5)(*(feet + [grip]))
    same_body = next(r for r in range(27) if r != feet[0] and m.rb_body[r] == m.rb_body[feet[0]])   # e.g. the calf the foot is fixed to
    call = lambda **kw: L.wbc_sim_impulse_dynamics(*[kw.get(k, d) for k, d in (
        ("sim", h), ("rb", idx), ("k", K), ("active", None), ("e", None), ("vdes", None), ("iota", x.data_ptr()), ("damping", 0.0), ("flags", 0),
        ("nu", nu.data_ptr()), ("lam", lam.data_ptr()), ("den", den.data_ptr()), ("map", P.data_ptr()), ("ws", ws.data_ptr()), ("stream", None))])
    refusals = [
        (dict(sim=None), b"NULL"), (dict(rb=None), b"NULL"), (dict(nu=None), b"NULL"), (dict(ws=None), b"NULL"),
        (dict(k=0), b"nbodies"), (dict(k=6), b"nbodies"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], 27, feet[3])), b"index"), (dict(rb=(C.c_int32 * 4)(feet[0], -1, feet[2], feet[3])), b"index"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(rb=(C.c_int32 * 4)(feet[0], feet[1], same_body, feet[3])), b"same moving body"),
        (dict(damping=-1e-3), b"damping"), (dict(damping=float("inf")), b"damping"), (dict(damping=float("nan")), b"damping"),
        (dict(flags=2), b"flag"),
        (dict(e=x.data_ptr() + 2), b"4-byte"), (dict(vdes=x.data_ptr() + 1), b"4-byte"), (dict(iota=x.data_ptr() + 2), b"4-byte"),
        (dict(nu=nu.data_ptr() + 2), b"4-byte"), (dict(lam=lam.data_ptr() + 3), b"4-byte"), (dict(den=den.data_ptr() + 1), b"4-byte"),
        (dict(map=P.data_ptr() + 2), b"4-byte"), (dict(ws=ws.data_ptr() + 2), b"4-byte"),
        (dict(map=P.data_ptr() + 4), b"16-byte"), (dict(map=P.data_ptr() + 8), b"16-byte"),
    ]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        msg = L.wbc_last_error()
        assert msg.startswith(b"wbc_sim_impulse_dynamics: ") and word in msg, (kw, msg)
    torch.cuda.synchronize()
    for t in (nu, lam, den, P, ws):
        assert bool((t == SENTINEL).all())
    # 4-byte alignment is all the other pointers need: outputs one float into their buffers (the map 16 bytes in)
    want = env.sim.impulse_dynamics(feet, impulse_ext=x, want_map=True, want_energy=True)
    assert call(nu=nu.data_ptr() + 4, lam=lam.data_ptr() + 4, den=den.data_ptr() + 4, map=P.data_ptr() + 16, ws=ws.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(nu[1:1 + n * 26].view(n, 26), want["nu_plus"]) and float(nu[0]) == SENTINEL
    assert torch.equal(lam[1:1 + n * 12].view(n, 4, 3), want["impulse"]) and float(lam[0]) == SENTINEL
    assert torch.equal(den[1:1 + n], want["denergy"]) and float(den[0]) == SENTINEL and float(ws[0]) == SENTINEL
    assert torch.equal(P[4:4 + n * 676].view(n, 26, 26), want["dnu_dnu"]) and bool((P[:4] == SENTINEL).all())


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
                env.touchdown_impact(stance=env.get_foot_contacts(), push=b); env.impact_map()
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.sim.impulse_dynamics(feet + [grip], restitution=0.5, armature=True, damping=1e-3, want_map=True, want_energy=True)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
