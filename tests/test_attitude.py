"""The attitude filter (wbc_sim_attitude_filter: wbc_attitude_filter_kernel in csrc/wbc_attitude_kernel.hip; the text both implement is
the comment in include/wbc_sim.h). The CPU tests pin the fp64 restatement of tests/attitude_reference.py to properties of the equations
and measure the fp32 yardstick; the GPU tests hold the kernel to the reference entry by entry.

Bound: every entry of a continuous output satisfies |kernel - ref| <= C 2^-24 mag, mag as attitude_reference's docstring lists it. C is
4 x K_ref rounded up to a power of two, K_ref the largest ratio of the reference run in fp32 against itself in fp64 over the judged cases
(every call of every chain: SIZES x COMBOS x NCALLS), measured on the CPU and asserted there; it never comes from the kernel. The table
with the kernel's own largest ratios on an MI355X is in DESIGN.md (K_GPU below repeats it for the record).

The status words match exactly except in THIN cases, judged from the fp64 reference alone: a reset from the accelerometer whose
d = 1 + m . w_0 is within THIN_BOUND of WBC_ATTITUDE_ANTIPARALLEL. d is a sum of four terms of size at most 1 formed from a vector
normalised in fp32: 8 x 2^-24 covers their roundings with a margin. Such an env is left out of that call's comparison."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import attitude_reference as ar
from wbc_amd import abi
from wbc_amd.abi import WbcAttitudeCfg  # noqa: F401  (this file is about wbc_sim_attitude_filter: none of it means anything without the call)

SENTINEL, ISENTINEL = 12345.0, -7777
EPS = 2.0 ** -24
F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)                  # noqa: E731
E = 64                                                                               # envs per wavefront of the layout that ships: lane = env
SIZES = (1, E - 1, E, E + 1, 2 * E + 2)
# (accel given, K, gyro given, q_init given)
COMBOS = tuple(itertools.product((True, False), (0, 1, 4), (True, False), (True, False)))
NCALLS = 4                                                                           # a reset of all, a plain call, a masked reset, a plain call
THIN_BOUND = 8 * EPS
THIN_CAP = 0.01
GRAVITY = (0.0, 0.0, -9.81)

# K_ref (measured by test_fp32_yardstick_is_where_the_constants_came_from), the kernel's largest ratio on the MI355X (for the record: no
# bound comes from it) and the constant
K_REF = {"q": 20.2, "b": 147.0, "P": 6140.0, "gyro_out": 66.5, "gravity_body": 37.2, "nis": 62.1}
K_GPU = {"q": 19.0, "b": 109.0, "P": 6250.0, "gyro_out": 70.6, "gravity_body": 37.2, "nis": 44.1}
_pow2 = lambda k: float(2.0 ** np.ceil(np.log2(4 * k)))                             # noqa: E731
CONST = {k: _pow2(v) for k, v in K_REF.items()}


def _cfg(**kw):
    """The kernel receives the cfg as floats: the references use the same rounded values."""
    base = dict(dt=0.02, sigma_g=0.005, sigma_b=1e-4, sigma_a=0.02, kappa_a=100.0, p0_theta=0.25, p0_b=1e-3)
    base.update(kw)
    return {k: float(np.float32(base[k])) for k in ar.CFG_FIELDS}


def _make_cfg(cfg, **kw):
    c = dict(cfg, **kw)
    return abi.WbcAttitudeCfg(*[c[k] for k in ar.CFG_FIELDS])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rand_quat(rng, n):
    return _unit(rng.normal(size=(n, 4)))


# ---------------------------------------------------------------------------------------------------- properties of the equations (CPU)
def test_constant_rate_integrates_to_the_exponential():
    """With constant omega, b = 0 and no measurement, k calls give q0 (x) exp(k omega dt) to fp64 rounding."""
    rng = np.random.default_rng(0)
    n, k = 16, 50
    cfg = _cfg()
    q0 = _rand_quat(rng, n)
    w = rng.uniform(-3, 3, (n, 3))
    q, b, P = q0.copy(), np.zeros((n, 3)), np.tile(np.eye(6) * 1e-3, (n, 1, 1))
    for _ in range(k):
        o = ar.update(cfg, q, b, P, w)
        q, b, P = o["q"], o["b"], o["P"]
        assert (o["status"] == ar.STATUS_OK).all() and (o["b"] == 0).all()
    want = ar.quat_mul(q0, ar.exp_closed(w * (k * cfg["dt"])))
    assert np.abs(q - want).max() < 200 * 2.0 ** -53 * k
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 4 * 2.0 ** -53


def test_zero_rotation_leaves_the_quaternion_bit_for_bit():
    """exp(0) is (0, 0, 0, 1) exactly and q (x) exp(0) has q's bits, in both precisions; the call then divides by sqrt(q . q), so the
    quaternions here are fixed points of normalise (what a call writes, normalised again until it no longer moves: at most a few times)."""
    rng = np.random.default_rng(1)
    for D in (np.float64, np.float32):
        assert np.array_equal(ar.exp_quat(np.zeros((3, 3), dtype=D)), np.tile(np.array([0, 0, 0, 1], dtype=D), (3, 1)))
        q = _rand_quat(rng, 64).astype(D)
        assert np.array_equal(ar.quat_mul(q, ar.exp_quat(np.zeros((64, 3), dtype=D))), q)
        for _ in range(8):
            q = ar.normalise(q)
        keep = np.array_equal(ar.normalise(q), q)
        fixed = (ar.normalise(q) == q).all(axis=1)
        assert fixed.sum() >= 32, (D, int(fixed.sum()), keep)
        q = q[fixed]
        n = q.shape[0]
        b = rng.uniform(-0.1, 0.1, (n, 3)).astype(D)
        o = ar.update(_cfg(), q, b, np.tile(np.eye(6, dtype=D) * D(1e-3), (n, 1, 1)), b.copy(), dtype=D)        # gyro = b: omega = 0
        assert o["q"].dtype == D and np.array_equal(o["q"], q) and np.array_equal(o["b"], b)


def test_series_and_closed_form_agree_on_both_sides_of_the_switch():
    rng = np.random.default_rng(2)
    d = _unit(rng.normal(size=(200, 3)))
    for scale in (0.25, 0.5, 0.999, 1.001, 2.0, 4.0):
        phi = d * (ar.SWITCH * scale)
        a, b = ar.exp_series(phi), ar.exp_closed(phi)
        # the series' first dropped terms: |phi|^5 / 3840 in the vector part, |phi|^4 / 384 in the scalar
        assert np.abs(a - b).max() < 4 * 2.0 ** -53 + (ar.SWITCH * scale) ** 4 / 384
        got = ar.exp_quat(phi)
        assert np.array_equal(got, a if scale < 1 else b)
    a32, b64 = ar.exp_series((d * 0.9e-4).astype(np.float32)), ar.exp_closed(d * 0.9e-4)
    assert np.abs(a32 - b64).max() < 2 * EPS


def _true_error(q_hat, b_hat, q_true, b_true):
    Re = np.einsum("nji,njk->nik", ar.quat_to_mat(q_hat), ar.quat_to_mat(q_true))
    return np.concatenate([ar.log_mat(Re), b_true - b_hat], axis=1)


def test_transition_matrix_is_the_derivative_of_the_propagated_error():
    """Phi equals the central difference of the propagated error (log of R_hat^T R_true, b_true - b) with respect to (dtheta, db)."""
    rng = np.random.default_rng(3)
    n, dt, h = 8, 0.02, 1e-5
    q, b, gyro = _rand_quat(rng, n), rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-3, 3, (n, 3))
    step = lambda qq, bb, om: ar.normalise(ar.quat_mul(qq, ar.exp_quat((om - bb) * dt)))      # noqa: E731
    q_hat = step(q, b, gyro)
    F = ar.transition(ar.exp_quat((gyro - b) * dt), dt)
    num = np.zeros((n, 6, 6))
    for j in range(6):
        side = []
        for s in (+1, -1):
            dx = np.zeros((n, 6)); dx[:, j] = s * h
            qt = ar.normalise(ar.quat_mul(q, ar.exp_quat(dx[:, :3])))                     # R_true = R(q) exp([dtheta]x)
            bt = b + dx[:, 3:]
            side.append(_true_error(q_hat, b, step(qt, bt, gyro), bt))                    # the true gyro rate: gyro - b_true
        num[:, :, j] = (side[0] - side[1]) / (2 * h)
    # first order in dt: the bias block of the exact derivative is -dt times the left Jacobian of the step, I + O(|phi|)
    assert np.abs(num[:, :3, :3] - F[:, :3, :3]).max() < 1e-8
    assert np.abs(num[:, :3, 3:] - F[:, :3, 3:]).max() < dt * (3 * np.sqrt(3) * dt)
    assert np.abs(num[:, 3:, :] - F[:, 3:, :]).max() < 1e-9
    slow = rng.uniform(-1e-3, 1e-3, (n, 3))
    F = ar.transition(ar.exp_quat(slow * dt), dt)
    assert np.abs(F[:, :3, :3] - np.eye(3)).max() < 1e-4 and np.abs(F[:, :3, 3:] + dt * np.eye(3)).max() == 0


def test_measurement_jacobian_is_the_derivative_of_the_predicted_direction():
    rng = np.random.default_rng(4)
    n, h = 8, 1e-5
    q, w = _rand_quat(rng, n), _unit(rng.normal(size=(n, 3)))
    mh, H = ar.measurement_jacobian(q, w)
    assert np.abs(H[:, :, 3:]).max() == 0
    for j in range(3):
        side = []
        for s in (+1, -1):
            d = np.zeros((n, 3)); d[:, j] = s * h
            side.append(ar.measurement_jacobian(ar.normalise(ar.quat_mul(q, ar.exp_quat(d))), w)[0])
        assert np.abs((side[0] - side[1]) / (2 * h) - H[:, :, j]).max() < 1e-9


def _random_state(rng, n):
    A = rng.normal(size=(n, 6, 6)) * np.array([0.1, 0.1, 0.1, 0.01, 0.01, 0.01])[None, :, None]
    P = A @ np.swapaxes(A, 1, 2) + np.diag([1e-4] * 3 + [1e-6] * 3)
    return _rand_quat(rng, n), rng.uniform(-0.05, 0.05, (n, 3)), ar.sym_lower(P)


def test_one_update_is_the_textbook_gain_and_the_joseph_form():
    rng = np.random.default_rng(5)
    n = 32
    q, b, P = _random_state(rng, n)
    w, u, r = _unit(rng.normal(size=(n, 3))), rng.normal(size=(n, 3)) * 3, rng.uniform(1e-4, 1e-2, n)
    res = ar.correct(q, b, P, w, u, r)
    assert not res["zero"].any() and not res["pivot"].any()
    H, S, e = res["H"], res["S"], res["e"]
    K = P @ np.swapaxes(H, 1, 2) @ np.linalg.inv(S)
    dx = np.einsum("nij,nj->ni", K, e)
    I = np.eye(6)
    P_plain = (I - K @ H) @ P
    P_joseph = (I - K @ H) @ P @ np.swapaxes(I - K @ H, 1, 2) + K @ (r[:, None, None] * np.eye(3)) @ np.swapaxes(K, 1, 2)
    scale = np.abs(P).max(axis=(1, 2), keepdims=True)
    assert (np.abs(res["P"] - P_plain) / scale).max() < 1e-12 and (np.abs(res["P"] - P_joseph) / scale).max() < 1e-12
    assert np.abs(res["b"] - (b + dx[:, 3:])).max() < 1e-13
    assert np.abs(res["q"] - ar.normalise(ar.quat_mul(q, ar.exp_quat(dx[:, :3])))).max() < 1e-13
    assert np.abs(res["nis"] - np.einsum("ni,nij,nj->n", e, np.linalg.inv(S), e)).max() < 1e-9 * res["nis"].max()
    assert np.array_equal(res["P"], np.swapaxes(res["P"], 1, 2))


def test_accelerometer_alone_leaves_the_heading_with_isotropic_covariance():
    """With P_tt = p I and no attitude-bias coupling the correction dx_theta is perpendicular to the predicted gravity direction: no turn about
    gravity."""
    rng = np.random.default_rng(6)
    n = 32
    q = _rand_quat(rng, n)
    P = np.tile(np.diag([0.04] * 3 + [1e-4] * 3), (n, 1, 1))
    up, _ = ar.up_vector(GRAVITY, np.float64)
    w = np.tile(up, (n, 1))
    u = 9.81 * _unit(np.einsum("nji,j->ni", ar.quat_to_mat(q), up) + 0.2 * rng.normal(size=(n, 3)))
    res = ar.correct(q, np.zeros((n, 3)), P, w, u, np.full(n, 4e-4))
    dx = np.einsum("nrc,nr->nc", res["W"], res["y"])
    mh = ar.measurement_jacobian(q, w)[0]
    assert np.abs(dx[:, :3]).max() > 0.05 and np.abs(np.einsum("ni,ni->n", dx[:, :3], mh)).max() < 1e-15
    # the rotation that was applied moves R^T w about an axis perpendicular to it: the world heading of the trunk's x axis about gravity
    # changes only through the tilt
    dq = ar.quat_mul(np.concatenate([-q[:, :3], q[:, 3:]], axis=1), res["q"])
    axis = dq[:, :3] / np.linalg.norm(dq[:, :3], axis=1, keepdims=True)
    assert np.abs(np.einsum("ni,ni->n", axis, mh)).max() < 1e-12


@functools.lru_cache(maxsize=None)
def _scripted(aux, steps=3000, n=4, seed=0):
    """The scripted motion: a slowly varying rotation, gyro noise 0.002 rad/s and bias (0.02, -0.01, 0.03) rad/s, accelerometer noise
    0.05 m/s^2, a start 0.45 rad off; with aux a noisy heading vector (the world x axis). Returns the errors at the start and the end."""
    rng = np.random.default_rng(seed)
    cfg = _cfg()
    dt = cfg["dt"]
    bias = np.array([0.02, -0.01, 0.03])
    g = np.array(GRAVITY)
    north = np.array([1.0, 0.0, 0.0])
    qt = np.tile(_unit(np.array([[0.1, -0.2, 0.3, 0.9]])), (n, 1))
    q = ar.normalise(ar.quat_mul(qt, ar.exp_quat(0.45 * _unit(rng.normal(size=(n, 3))))))
    b, P = np.zeros((n, 3)), np.tile(np.diag([cfg["p0_theta"]] * 3 + [cfg["p0_b"]] * 3), (n, 1, 1))

    def errors():
        R, Rt = ar.quat_to_mat(q), ar.quat_to_mat(qt)
        ang = np.linalg.norm(ar.log_mat(np.einsum("nji,njk->nik", R, Rt)), axis=1)
        tilt = np.arccos(np.clip(np.einsum("ni,ni->n", R[:, 2, :], Rt[:, 2, :]), -1, 1))       # between the two R^T z
        gb = Rt[:, 2, :]
        be = b - bias
        along = np.einsum("ni,ni->n", be, gb)
        return dict(angle=ang, tilt=tilt, bias_across=np.linalg.norm(be - along[:, None] * gb, axis=1), bias_along=np.abs(along))

    first = errors()
    min_eig, asym = np.inf, 0.0
    for k in range(steps):
        t = k * dt
        w = np.tile(np.array([0.5 * np.sin(0.7 * t), 0.4 * np.cos(0.5 * t), 0.3 * np.sin(0.3 * t + 1)]), (n, 1))
        qt = ar.normalise(ar.quat_mul(qt, ar.exp_quat(w * dt)))
        R = ar.quat_to_mat(qt)
        gyro = w + bias + 0.002 * rng.normal(size=(n, 3))
        accel = np.einsum("nji,j->ni", R, -g) + 0.05 * rng.normal(size=(n, 3))
        kw = {}
        if aux:
            hb = np.einsum("nji,j->ni", R, north) + 0.01 * rng.normal(size=(n, 3))
            kw = dict(aux_body=hb[:, None], aux_world=np.tile(north, (n, 1, 1)), aux_sigma=np.full((n, 1), 0.02))
        o = ar.update(cfg, q, b, P, gyro, accel=accel, gravity=GRAVITY, **kw)
        q, b, P = o["q"], o["b"], o["P"]
        assert (o["status"] == ar.STATUS_OK).all()
        min_eig = min(min_eig, float(np.linalg.eigvalsh(P).min()))
        asym = max(asym, float(np.abs(P - np.swapaxes(P, 1, 2)).max()))
    return first, errors(), min_eig, asym


def test_scripted_motion_converges():
    """With the accelerometer alone the tilt error and the bias across gravity shrink below a twentieth and a tenth of where they started;
    with one heading vector the full angle error and the bias along gravity do too. (The motion turns the trunk, so the accelerometer
    alone also sees the bias along gravity over time; only the heading itself stays unobserved.)"""
    first, last, _, _ = _scripted(False)
    print(f"attitude, scripted motion, accelerometer alone: tilt {first['tilt'].max():.3g} -> {last['tilt'].max():.3g} rad, angle "
          f"{first['angle'].max():.3g} -> {last['angle'].max():.3g} rad, bias across gravity {first['bias_across'].max():.3g} -> "
          f"{last['bias_across'].max():.3g} rad/s")
    assert (last["tilt"] < first["tilt"] / 20).all() and (last["bias_across"] < first["bias_across"] / 10).all()
    first, last, _, _ = _scripted(True)
    print(f"attitude, scripted motion, with a heading vector: angle {first['angle'].max():.3g} -> {last['angle'].max():.3g} rad, bias "
          f"along gravity {first['bias_along'].max():.3g} -> {last['bias_along'].max():.3g} rad/s")
    assert (last["angle"] < first["angle"] / 20).all() and (last["tilt"] < first["tilt"] / 20).all()
    assert (last["bias_across"] < first["bias_across"] / 10).all() and (last["bias_along"] < first["bias_along"] / 10).all()


def test_covariance_stays_symmetric_and_positive_over_3000_updates():
    for aux in (False, True):
        _, _, min_eig, asym = _scripted(aux)
        print(f"attitude, 3000 updates (aux {aux}): smallest eigenvalue of P {min_eig:.3g}, largest asymmetry {asym:g}")
        assert min_eig > 0 and asym == 0


def test_reset_from_the_accelerometer_fixes_the_tilt_with_zero_yaw():
    rng = np.random.default_rng(7)
    n = 256
    up, _ = ar.up_vector(GRAVITY, np.float64)
    accel = rng.normal(size=(n, 3)) * rng.uniform(1, 20, (n, 1))
    o = ar.update(_cfg(), np.full((n, 4), np.nan), np.full((n, 3), np.nan), np.full((n, 6, 6), np.nan), np.zeros((n, 3)), accel=accel, reset=True)
    assert (o["status"] == ar.STATUS_RESET).all() and (o["b"] == 0).all()
    c = _cfg()
    assert np.array_equal(o["P"], np.tile(np.diag([c["p0_theta"]] * 3 + [c["p0_b"]] * 3), (n, 1, 1)))
    m = _unit(accel)
    assert np.abs(np.einsum("nij,nj->ni", ar.quat_to_mat(o["q"]), m) - up).max() < 1e-13          # R(q) m = w
    assert np.abs(np.einsum("ni,i->n", o["q"][:, :3], up)).max() < 1e-15                          # the rotation's axis is horizontal: zero yaw
    assert np.abs(o["gravity_body"] + m).max() < 1e-13 and (o["nis"] == 0).all()
    # neither input: the identity; q_init: normalised
    o = ar.update(_cfg(), np.zeros((3, 4)), np.zeros((3, 3)), np.zeros((3, 6, 6)), np.ones((3, 3)), reset=True)
    assert np.array_equal(o["q"], np.tile([0.0, 0, 0, 1], (3, 1))) and np.array_equal(o["gyro_out"], np.ones((3, 3)))
    qi = rng.normal(size=(5, 4)) * 3
    o = ar.update(_cfg(), np.zeros((5, 4)), np.zeros((5, 3)), np.zeros((5, 6, 6)), np.ones((5, 3)), accel=accel[:5], q_init=qi, reset=True)
    assert np.array_equal(o["q"], ar.normalise(qi))


def test_reset_at_and_next_to_the_antiparallel_direction():
    """m = -w exactly takes the half turn about the stated axis; one ulp off it (d far below the threshold) too; just above the threshold the
    shortest rotation, which is still a rotation with R(q) m = w."""
    for D, tol in ((np.float64, 1e-9), (np.float32, 1e-3)):
        up, _ = ar.up_vector(GRAVITY, D)
        assert np.array_equal(up, np.array([0, 0, 1], dtype=D)) and np.array_equal(ar.half_axis(up), np.array([0, -1, 0], dtype=D))
        down = np.array([0.0, 0.0, -9.81])
        off = down.copy(); off[0] = np.spacing(D(9.81))
        wide = np.array([9.81 * 3e-3, 0.0, -9.81])                                     # d = 1 - cos(3e-3) = 4.5e-6 > 1e-6
        accel = np.stack([down, off, wide, -down])
        o = ar.update(_cfg(), np.zeros((4, 4)), np.zeros((4, 3)), np.zeros((4, 6, 6)), np.zeros((4, 3)), accel=accel, reset=True, dtype=D)
        assert o["status"].tolist() == [ar.STATUS_RESET | ar.INFO_HALF_TURN] * 2 + [ar.STATUS_RESET] * 2
        assert np.array_equal(o["q"][:2], np.tile(np.array([0, -1, 0, 0], dtype=D), (2, 1)))
        R = ar.quat_to_mat(o["q"].astype(np.float64))
        assert np.abs(np.einsum("nij,nj->ni", R, _unit(accel)) - np.array([0, 0, 1.0])).max() < tol * 10
        assert np.array_equal(o["q"][3], np.array([0, 0, 0, 1], dtype=D))
    # a tilted gravity picks the other axis where |up_x| > 0.9
    up, _ = ar.up_vector((-9.0, 0.0, -1.0), np.float64)
    h = ar.half_axis(up)
    assert abs(up[0]) > 0.9 and abs(h @ up) < 1e-15 and abs(np.linalg.norm(h) - 1) < 1e-15 and h[1] == 0


def test_kappa_acts_only_through_the_accelerometers_length():
    rng = np.random.default_rng(8)
    n = 16
    q, b, P = _random_state(rng, n)
    gyro = rng.uniform(-1, 1, (n, 3))
    m = _unit(rng.normal(size=(n, 3)))
    gn = float(ar.up_vector(GRAVITY, np.float64)[1])
    base = ar.update(_cfg(kappa_a=0.0), q, b, P, gyro, accel=m * gn)
    same = ar.update(_cfg(kappa_a=1e4), q, b, P, gyro, accel=m * gn)
    for k in ar.OUTPUTS:
        assert np.abs(base[k] - same[k]).max() <= 1e-9 * max(1.0, np.abs(base[k]).max()), k     # |accel| = |g| to rounding: (1e-16)^2 kappa
    long0 = ar.update(_cfg(kappa_a=0.0), q, b, P, gyro, accel=m * gn * 1.5)
    long1 = ar.update(_cfg(kappa_a=100.0), q, b, P, gyro, accel=m * gn * 1.5)
    assert np.abs(long0["q"] - base["q"]).max() < 1e-12                                 # without kappa the length does not matter
    # with it r = sigma_a^2 (1 + 100 / 4) = 26 sigma_a^2: the same call with sigma_a scaled and |accel| = |g|
    scaled = ar.update(_cfg(kappa_a=0.0, sigma_a=_cfg()["sigma_a"] * np.sqrt(26.0)), q, b, P, gyro, accel=m * gn)
    assert np.abs(long1["q"] - scaled["q"]).max() < 1e-6 and np.abs(long1["P"] - scaled["P"]).max() < 1e-7
    assert (long1["nis"][:, 0] < long0["nis"][:, 0]).all()


def test_skipped_entries_zero_vectors_and_non_finite_inputs():
    rng = np.random.default_rng(9)
    n = 12
    q, b, P = _random_state(rng, n)
    gyro, accel = rng.uniform(-1, 1, (n, 3)), 9.81 * _unit(rng.normal(size=(n, 3)))
    body, world, sigma = rng.normal(size=(n, 3, 3)), rng.normal(size=(n, 3, 3)), rng.uniform(0.01, 0.1, (n, 3))
    want = ar.update(_cfg(), q, b, P, gyro, accel=accel, aux_body=body[:, [0, 2]], aux_world=world[:, [0, 2]], aux_sigma=sigma[:, [0, 2]])
    # a sigma <= 0 entry: the bits of the call without it, even with NaN in its vectors
    for s in (0.0, -1.0):
        sg, bd, wd = sigma.copy(), body.copy(), world.copy()
        sg[:, 1] = s; bd[:, 1] = np.nan; wd[:, 1] = np.inf
        got = ar.update(_cfg(), q, b, P, gyro, accel=accel, aux_body=bd, aux_world=wd, aux_sigma=sg)
        for k in ("q", "b", "P", "gyro_out", "gravity_body"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["nis"][:, [0, 1, 3]], want["nis"]) and (got["nis"][:, 2] == 0).all()
        assert (got["status"] == ar.STATUS_OK).all()
    # a zero u is skipped with its bit, for the accelerometer and for an aux entry (and a zero world vector likewise)
    a0, b0, w0 = accel.copy(), body.copy(), world.copy()
    a0[0] = 0; b0[1, 2] = 0; w0[2, 0] = 0
    got = ar.update(_cfg(), q, b, P, gyro, accel=a0, aux_body=b0, aux_world=w0, aux_sigma=sigma)
    assert got["status"][:4].tolist() == [ar.INFO_ZERO, ar.INFO_ZERO << 3, ar.INFO_ZERO << 1, 0]
    assert got["nis"][0, 0] == 0 and got["nis"][1, 3] == 0 and got["nis"][2, 1] == 0 and (got["nis"][3] > 0).all()
    alone = ar.update(_cfg(), q, b, P, gyro, aux_body=body, aux_world=world, aux_sigma=sigma)
    assert np.array_equal(got["q"][0], alone["q"][0]) and np.array_equal(got["P"][0], alone["P"][0])
    # a failed pivot (an enormous negative-definite "covariance") skips the measurement, keeps the predicted state and says so
    Pn = P.copy(); Pn[5] = -np.eye(6)
    got = ar.update(_cfg(), q, b, Pn, gyro, accel=accel)
    pred = ar.update(_cfg(), q, b, Pn, gyro)
    assert got["status"][5] == (ar.STATUS_FAILED_PIVOT | ar.INFO_PIVOT) and got["nis"][5, 0] == 0
    assert np.array_equal(got["q"][5], pred["q"][5]) and np.array_equal(got["P"][5], pred["P"][5]) and (np.delete(got["status"], 5) == 0).all()
    # a non-finite input that is read fails that env alone; one that is not read does not
    plain = ar.update(_cfg(), q, b, P, gyro, accel=accel, aux_body=body, aux_world=world, aux_sigma=sigma)
    g1, a1, b1, w1, s1, q1, bb1, P1 = (v.copy() for v in (gyro, accel, body, world, sigma, q, b, P))
    g1[0, 1] = np.nan; a1[1, 2] = np.inf; b1[2, 1, 0] = np.nan; w1[3, 2, 2] = -np.inf; s1[4, 0] = np.nan; q1[5, 3] = np.nan; bb1[6, 0] = np.inf
    P1[7, 4, 2] = np.nan                                                               # the lower triangle is read
    P1[8, 2, 4] = np.nan                                                               # the upper is not
    got = ar.update(_cfg(), q1, bb1, P1, g1, accel=a1, aux_body=b1, aux_world=w1, aux_sigma=s1)
    assert got["status"][:8].tolist() == [ar.STATUS_FAILED] * 8 and (got["status"][8:] == 0).all()
    for k in ("gyro_out", "gravity_body", "nis"):
        assert (got[k][:8] == 0).all() and np.array_equal(got[k][8:], plain[k][8:]), k
    for k, src in (("q", q1), ("b", bb1), ("P", P1)):
        assert np.array_equal(got[k][:8], src[:8], equal_nan=True) and np.array_equal(got[k][8:], plain[k][8:]), k
    # a reset env reads neither its state nor the aux inputs
    mask = np.zeros(n, dtype=np.int32); mask[[2, 3, 4, 5, 6, 7]] = 1
    got = ar.update(_cfg(), q1, bb1, P1, gyro, accel=accel, aux_body=b1, aux_world=w1, aux_sigma=s1, reset_mask=mask)
    assert (got["status"][[2, 3, 4, 5, 6, 7]] == ar.STATUS_RESET).all()
    bad_qi = np.tile([0.0, 0, 0, 1], (n, 1)); bad_qi[2] = 0; bad_qi[3, 1] = np.nan
    got = ar.update(_cfg(), q, b, P, gyro, accel=accel, q_init=bad_qi, reset_mask=mask)
    assert got["status"][[2, 3]].tolist() == [ar.STATUS_FAILED] * 2 and np.array_equal(got["q"][[2, 3]], q[[2, 3]])


# ---------------------------------------------------------------------------------------------------- the C ABI without a device
_INPUTS = ("gyro", "accel", "aux_body", "aux_world", "aux_sigma", "reset_mask", "q_init")
_STATE = ("q", "b", "P")
_OUTS = ("gyro_out", "gravity_body", "nis", "status")
_NAMES = ("sim", "cfg", "gyro", "accel", "aux_body", "aux_world", "aux_sigma", "num_aux", "reset_mask", "q_init", "flags") + _STATE + _OUTS + ("stream",)


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_attitude_filter(*[C.byref(args[k]) if isinstance(args[k], abi.WbcAttitudeCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device():
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    import re
    import __graft_entry__ as g
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    assert "wbc_sim_attitude_filter" in EXPORTED_SYMBOLS and hasattr(L, "wbc_sim_attitude_filter")
    assert "wbc_attitude_kernel.hip" in g.SOURCES and "wbc_attitude.h" in g.HEADERS
    # the mirror against the header's struct: the same fields in the same order, all floats
    header = open(g.ROOT + "/include/wbc_sim.h").read()
    body = re.search(r"typedef struct \{([^}]*)\} wbc_attitude_cfg;", header).group(1)
    fields = [name.strip() for decl in re.findall(r"float ([^;]*);", body) for name in decl.split(",")]
    assert fields == list(ar.CFG_FIELDS) == [f for f, _ in abi.WbcAttitudeCfg._fields_] and abi.AttitudeCfg is abi.WbcAttitudeCfg
    assert C.sizeof(abi.WbcAttitudeCfg) == 4 * len(fields) == 28
    assert [getattr(abi.WbcAttitudeCfg, f).offset for f in fields] == [4 * i for i in range(7)]
    for name, mine in (("RESET", 1), ("MAX_AUX", ar.MAX_AUX), ("STATUS_MASK", ar.STATUS_MASK), ("STATUS_OK", ar.STATUS_OK),
                       ("STATUS_RESET", ar.STATUS_RESET), ("STATUS_FAILED", ar.STATUS_FAILED), ("STATUS_FAILED_PIVOT", ar.STATUS_FAILED_PIVOT),
                       ("INFO_ZERO", ar.INFO_ZERO), ("INFO_PIVOT", ar.INFO_PIVOT), ("INFO_HALF_TURN", ar.INFO_HALF_TURN)):
        assert int(re.search(r"#define WBC_ATTITUDE_%s (\d+)" % name, header).group(1)) == getattr(abi, "ATTITUDE_" + name) == mine, name
    assert float(re.search(r"#define WBC_ATTITUDE_ANTIPARALLEL ([0-9.e-]+)f", header).group(1)) == abi.ATTITUDE_ANTIPARALLEL == ar.ANTIPARALLEL
    assert len(L.wbc_sim_attitude_filter.argtypes) == len(_NAMES)
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    good = _cfg()
    base = dict(sim=None, cfg=_make_cfg(good), num_aux=2, flags=0, stream=None, **{k: p + 256 * i for i, k in enumerate(_INPUTS + _STATE + _OUTS)})
    nan, inf = float("nan"), float("inf")
    refusals = [(dict(cfg=None), b"NULL"), (dict(q=None), b"NULL"), (dict(b=None), b"NULL"), (dict(P=None), b"NULL"),
                (dict(num_aux=-1), b"num_aux"), (dict(num_aux=5), b"num_aux"), (dict(aux_body=None), b"aux_"), (dict(aux_world=None), b"aux_"),
                (dict(aux_sigma=None), b"aux_"), (dict(flags=2), b"flag"), (dict(flags=-1), b"flag")]
    for field, word in (("dt", b"dt"), ("sigma_g", b"sigma"), ("sigma_b", b"sigma"), ("sigma_a", b"sigma"), ("p0_theta", b"variance"), ("p0_b", b"variance")):
        refusals += [(dict(cfg=_make_cfg(good, **{field: bad})), word) for bad in (0.0, -1.0, nan, inf)]
    refusals += [(dict(cfg=_make_cfg(good, kappa_a=bad)), b"kappa_a") for bad in (-1e-3, nan, inf)]
    refusals += [({k: base[k] + off}, b"aligned") for k in _INPUTS + _STATE + _OUTS for off in (1, 2, 3)]
    assert len(refusals) > 75
    passing = [dict(), dict(num_aux=0, aux_body=None, aux_world=None, aux_sigma=None), dict(gyro=None, accel=None, reset_mask=None, q_init=None),
               dict(flags=abi.ATTITUDE_RESET), dict(cfg=_make_cfg(good, kappa_a=0.0)), dict(gyro_out=None, gravity_body=None, nis=None, status=None)]
    for kw, word in refusals + [(kw, b"sim is NULL") for kw in passing]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_attitude_filter: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def test_attitude_kernel_codegen():
    """The translation unit's metadata: one kernel, no scratch, a workgroup of 64, at most 128 VGPRs. Nothing else is looked at."""
    import os
    import re
    import subprocess
    import tempfile
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    source = "wbc_attitude_kernel.hip"
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "attitude.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        text = open(out).read()
    entry = text[text.index("amdhsa.kernels:"):]
    assert len(re.findall(r"\.name:\s+\w+\n", entry)) == 1 and re.search(r"\.name:\s+wbc_attitude_filter_kernel\n", entry)
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))          # noqa: E731
    print(f"wbc_attitude_filter_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64 and meta("vgpr_count") <= 128


# ---------------------------------------------------------------------------------------------------- the judged cases
def _inputs(n, combo, call, state):
    """fp32-representable inputs of call `call` of the chain for n envs; `state` (q, b, P) is what the call starts from (None: a reset of
    all, which reads none). Every fifth env has |accel| far from |g|, every seventh a rotation step below the series' switch."""
    with_accel, K, with_gyro, with_qinit = COMBOS[combo]
    rng = np.random.default_rng([n, combo, call])
    idx = np.arange(n)
    reset = True if call == 0 else ((idx % 3 == 1).astype(np.int32) if call == 2 else None)
    rs = np.ones(n, dtype=bool) if reset is True else (np.zeros(n, dtype=bool) if reset is None else reset != 0)
    if state is None:
        q, b, P = np.full((n, 4), np.nan), np.full((n, 3), np.nan), np.full((n, 6, 6), np.nan)
        q_true = _rand_quat(rng, n)
    else:
        q, b, P = (np.array(v, copy=True) for v in state)
        P[:, np.triu_indices(6, 1)[0], np.triu_indices(6, 1)[1]] = np.nan              # only the lower triangle is read
        q_true = ar.normalise(ar.quat_mul(np.where(rs[:, None], _rand_quat(rng, n), q), ar.exp_quat(0.1 * rng.normal(size=(n, 3)))))
    R = ar.quat_to_mat(q_true)
    gyro = rng.uniform(-2, 2, (n, 3))
    slow = idx % 7 == 3
    gyro[slow] = np.where(rs[slow, None], 0.0, np.nan_to_num(b[slow])) + rng.uniform(-2e-3, 2e-3, (int(slow.sum()), 3))
    inp = dict(q=F32(q), b=F32(b), P=F32(P), reset=reset)
    if with_gyro:
        inp["gyro"] = F32(gyro)
    else:                                                                              # the sim's quaternion (any) and world angular velocity
        qs = F32(_rand_quat(rng, n) * rng.uniform(0.99, 1.01, (n, 1)))
        inp["sim_quat"], inp["sim_ang_vel"] = qs, F32(np.einsum("nij,nj->ni", ar.quat_to_mat(ar.normalise(qs)), gyro))
    if with_accel:
        scale = np.where(idx % 5 == 2, np.where(idx % 2 == 0, 0.3, 2.5), 1.0 + 0.02 * rng.normal(size=n))
        inp["accel"] = F32((np.einsum("nji,j->ni", R, -np.array(GRAVITY)) + 0.2 * rng.normal(size=(n, 3))) * scale[:, None])
    if K:
        world = rng.normal(size=(n, K, 3)) * rng.uniform(0.5, 2, (n, K, 1))
        body = (np.einsum("nji,nkj->nki", R, _unit(world)) + 0.05 * rng.normal(size=(n, K, 3))) * rng.uniform(0.5, 2, (n, K, 1))
        sigma = rng.uniform(0.02, 0.1, (n, K))
        if K == 4:                                                                     # one sigma <= 0 among the four, its vectors never read
            off = idx % 4
            sigma[idx, off] = np.where(idx % 2 == 0, 0.0, -1.0)
            body[idx, off] = np.nan; world[idx, off] = np.nan
        inp.update(aux_body=F32(body), aux_world=F32(world), aux_sigma=F32(sigma))
    if with_qinit and reset is not None:
        inp["q_init"] = F32(_rand_quat(rng, n) * rng.uniform(0.5, 2, (n, 1)))
    return inp


def _ref(cfg, inp, dtype=np.float64):
    gyro, gmag = (inp["gyro"], None) if "gyro" in inp else ar.sim_gyro(inp["sim_quat"], inp["sim_ang_vel"], dtype)
    reset = inp.get("reset")
    return ar.update(cfg, inp["q"], inp["b"], inp["P"], gyro, accel=inp.get("accel"), aux_body=inp.get("aux_body"), aux_world=inp.get("aux_world"),
                     aux_sigma=inp.get("aux_sigma"), reset_mask=None if reset is True else reset, q_init=inp.get("q_init"), reset=reset is True,
                     gravity=GRAVITY, gyro_mag=gmag, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _chain(n, combo):
    """(cfg, [(inputs, fp64 reference)] per call): every call starts from the previous call's reference state, rounded to fp32."""
    cfg = _cfg()
    calls, state = [], None
    for call in range(NCALLS):
        inp = _inputs(n, combo, call, state)
        ref = _ref(cfg, inp)
        calls.append((inp, ref))
        state = (ref["q"], ref["b"], ref["P"])
    return cfg, calls


def judge(ref):
    """keep [N]: the envs whose outputs are judged; the others are thin (a reset from the accelerometer next to the antiparallel threshold)."""
    d = ref["diag"]["d"]
    return ~(np.isfinite(d) & (np.abs(d - ar.ANTIPARALLEL) <= THIN_BOUND))


def compare(got, ref, const=None, who=""):
    """Assert the bound on every continuous output present in `got` and the status words exactly, over the kept envs; returns the ratios."""
    const = const or CONST
    keep = judge(ref)
    sub = lambda d: {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in d.items()}       # noqa: E731
    r_ = dict(sub(ref), mag=sub(ref["mag"]))
    g_ = {k: np.asarray(got[k])[keep] for k in ar.OUTPUTS + ("status",) if got.get(k) is not None}
    r = ar.ratios(g_, r_)
    for k, v in r.items():
        assert v <= const[k], (who, k, v, const[k])
    if "status" in g_:
        assert np.array_equal(g_["status"], r_["status"]), (who, g_["status"], r_["status"])
    return r


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output over every judged call and the thin env-cases, the fp32 reference's status words held to fp64 on the way."""
    worst = {k: 0.0 for k in ar.OUTPUTS}
    thin = [0, 0]
    seen = dict(slow=0, far=0, skipped=0, reset_accel=0, reset_identity=0, reset_qinit=0)
    big = {k: float("inf") for k in ar.OUTPUTS}
    for n in SIZES:
        for combo in range(len(COMBOS)):
            cfg, calls = _chain(n, combo)
            for j, (inp, ref) in enumerate(calls):
                assert ((ref["status"] & ar.STATUS_MASK) != ar.STATUS_FAILED).all() and ((ref["status"] & ar.STATUS_MASK) != ar.STATUS_FAILED_PIVOT).all()
                r = compare(_ref(cfg, inp, dtype=np.float32), ref, const=big, who=(n, COMBOS[combo], j))
                worst = {k: max(worst[k], r[k]) for k in worst}
                keep = judge(ref)
                thin[0] += int((~keep).sum()); thin[1] += keep.size
                rs = (ref["status"] & ar.STATUS_MASK) == ar.STATUS_RESET
                seen["reset_qinit"] += int(rs.sum()) if "q_init" in inp else 0
                seen["reset_accel"] += int(rs.sum()) if "q_init" not in inp and "accel" in inp else 0
                seen["reset_identity"] += int(rs.sum()) if "q_init" not in inp and "accel" not in inp else 0
                seen["skipped"] += int((inp["aux_sigma"] <= 0).sum()) if "aux_sigma" in inp else 0
                if "accel" in inp:
                    seen["far"] += int((np.abs(np.linalg.norm(inp["accel"], axis=1) / 9.81 - 1) > 0.5).sum())
                if "gyro" in inp and j in (1, 3):
                    seen["slow"] += int((np.linalg.norm((inp["gyro"] - inp["b"]) * cfg["dt"], axis=1) < ar.SWITCH).sum())
    return worst, thin, seen


def test_fp32_yardstick_is_where_the_constants_came_from():
    worst, _, _ = _yardsticks()
    print("attitude yardsticks: " + ", ".join(f"{k} K_ref = {worst[k]:.3g} (C = {CONST[k]:g})" for k in worst))
    for k in K_REF:
        assert abs(worst[k] - K_REF[k]) <= 0.25 * K_REF[k], (k, worst[k])
        assert 4 * worst[k] <= CONST[k]


def test_thin_cases_stay_under_the_cap():
    _, thin, seen = _yardsticks()
    print(f"attitude thin env-cases: {thin[0]} of {thin[1]}; in the judged cases: {seen}")
    assert thin[0] <= THIN_CAP * thin[1], thin
    assert all(v > 0 for v in seen.values()), seen                                     # and the cases are not vacuous


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _env(n, seed=5):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    return WidowGo1(cfg, sim_device="cuda:0", seed=seed)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


FRAME = 8


def _shapes(K):
    return {"q": ((4,), torch.float32), "b": ((3,), torch.float32), "P": ((6, 6), torch.float32), "gyro_out": ((3,), torch.float32),
            "gravity_body": ((3,), torch.float32), "nis": ((1 + K,), torch.float32), "status": ((), torch.int32)}


def _load_sim(env, inp):
    """The sim's own root state from the inputs of a NULL-gyro case."""
    root = env.sim.tensor("ROOT_STATES").clone()
    root[:, 0, 3:7] = _dev(inp["sim_quat"]); root[:, 0, 10:13] = _dev(inp["sim_ang_vel"])
    env.sim.set_root_state(root.contiguous())
    torch.cuda.synchronize()


def _call(env, cfg, inp, which=_OUTS, tensors=None):
    """A direct C-ABI call into buffers with sentinel frames on both sides (the state starts from inp's); returns {name: [n, ...] tensor}
    of the state and the outputs asked for. Inputs missing from inp are handed over as NULL (a NULL gyro: load the sim first)."""
    n = env.num_envs
    K = inp["aux_sigma"].shape[1] if "aux_sigma" in inp else 0
    shapes = _shapes(K)
    size = {k: int(np.prod(s, dtype=np.int64)) for k, (s, _) in shapes.items()}
    sent = lambda dt: SENTINEL if dt == torch.float32 else ISENTINEL                   # noqa: E731
    bufs = {}
    for name in _STATE + tuple(which):
        dt = shapes[name][1]
        bufs[name] = torch.full((FRAME + n * size[name] + FRAME,), sent(dt), dtype=dt, device="cuda")
    body = lambda name: bufs[name][FRAME:FRAME + n * size[name]]                       # noqa: E731
    for name in _STATE:
        body(name).copy_(_dev(inp[name]).reshape(-1))
    reset = inp.get("reset")
    tens = {k: _dev(inp.get(k)) for k in _INPUTS if k != "reset_mask"}
    tens["reset_mask"] = _dev(reset, torch.int32) if reset is not None and reset is not True else None
    tens.update(tensors or {})
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None          # noqa: E731
    out = lambda name: body(name).data_ptr() if name in bufs else None                 # noqa: E731
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_attitude_filter(env.sim.h, C.byref(c), ptr(tens["gyro"]), ptr(tens["accel"]), ptr(tens["aux_body"]), ptr(tens["aux_world"]),
                                           ptr(tens["aux_sigma"]), K, ptr(tens["reset_mask"]), ptr(tens["q_init"]),
                                           abi.ATTITUDE_RESET if reset is True else 0, *[out(k) for k in _STATE + _OUTS], None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        s = sent(shapes[name][1])
        assert bool((b[:FRAME] == s).all()) and bool((b[FRAME + n * size[name]:] == s).all()), name
    return {name: body(name).view((n,) + shapes[name][0]).clone() for name in bufs}


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_entry_against_fp64(n):
    env = _env(n)
    worst = {k: 0.0 for k in ar.OUTPUTS}
    for combo in range(len(COMBOS)):
        cfg, calls = _chain(n, combo)
        for j, (inp, ref) in enumerate(calls):
            if "gyro" not in inp:
                _load_sim(env, inp)
            got = _np(_call(env, cfg, inp))
            assert all(np.isfinite(got[k].astype(np.float64)[:, np.tril_indices(6)[0], np.tril_indices(6)[1]] if k == "P" else got[k].astype(np.float64)).all()
                       for k in got)
            r = compare(got, ref, who=(n, COMBOS[combo], j))
            worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"attitude n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")


@pytest.mark.gpu
def test_outputs_one_at_a_time_two_runs_a_graph_a_null_gyro_and_the_sim_untouched():
    n = 2 * E + 2
    combo = COMBOS.index((True, 4, False, True))                                       # every input, the gyro from the sim
    env = _env(n)
    cfg, calls = _chain(n, combo)
    inp = calls[2][0]                                                                  # the masked reset: both kinds of env in one launch
    _load_sim(env, inp)
    before = {name: env.sim.tensor(name).clone() for name in abi.TENSOR_IDS}
    want = _call(env, cfg, inp)
    assert _same(want, _call(env, cfg, inp))                                           # two runs: the same bits
    for name in _OUTS:
        got = _call(env, cfg, inp, which=(name,))
        assert _same(got, {k: want[k] for k in got}), name
    got = _call(env, cfg, inp, which=())
    assert _same(got, {k: want[k] for k in got})
    assert bool(torch.equal(want["P"], want["P"].transpose(1, 2)))                     # written bit-symmetric from a lower triangle
    # NULL gyro: the bits of the call on a copy of what the rule computes, which a reset hands out as gyro_out = gyro - 0
    rule = _call(env, cfg, dict(inp, reset=True), which=("gyro_out",))["gyro_out"]
    assert _same(_call(env, cfg, inp, tensors=dict(gyro=rule.clone())), want)
    compare(_np(want), calls[2][1], who="NULL gyro")
    # a captured graph replays the eager bits
    c = _make_cfg(cfg)
    t = {k: _dev(inp[k]) for k in ("accel", "aux_body", "aux_world", "aux_sigma", "q_init")}
    t["reset_mask"] = _dev(inp["reset"], torch.int32)
    state0 = {k: _dev(inp[k]) for k in _STATE}
    state = {k: v.clone() for k, v in state0.items()}
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _shapes(4).items() if k not in _STATE}
    call = lambda: env.sim.attitude_filter(c, state["q"], state["b"], state["P"], **t, **outs)     # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                     # warm-up off the default stream
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for k in _STATE:
        state[k].copy_(state0[k])
    with torch.cuda.graph(graph):
        call()
    for k in _STATE:
        state[k].copy_(state0[k])
    for o in outs.values():
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(dict(state, **outs), want)
    for name, t0 in before.items():
        assert torch.equal(_bits(env.sim.tensor(name)), _bits(t0)), name


@pytest.mark.gpu
def test_failed_envs_keep_their_state_and_the_special_resets():
    n = 2 * E + 2
    combo = COMBOS.index((True, 4, True, False))
    env = _env(n)
    cfg, calls = _chain(n, combo)
    inp, _ = calls[1]
    bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in inp.items()}
    rows = [0, 1, 63, 64, 65, 100, 128, 129]
    live = lambda e: [k for k in range(4) if k != e % 4][0]                            # noqa: E731  an aux entry of env e that is read
    bad["gyro"][0, 1] = np.nan; bad["accel"][1, 2] = np.inf; bad["aux_body"][63, live(63), 0] = np.nan; bad["aux_world"][64, live(64), 2] = -np.inf
    bad["aux_sigma"][65, live(65)] = np.nan; bad["q"][100, 3] = np.nan; bad["b"][128, 0] = np.inf; bad["P"][129, 4, 2] = np.nan
    ref = _ref(cfg, bad)
    assert ref["status"][rows].tolist() == [ar.STATUS_FAILED] * len(rows)
    got = _call(env, cfg, bad)
    plain = _call(env, cfg, inp)
    ok = torch.tensor(np.delete(np.arange(n), rows), device="cuda")
    for k in got:                                                                      # their neighbours: the bits of the launch without them
        assert torch.equal(_bits(got[k][ok]), _bits(plain[k][ok])), k
    g = _np(got)
    assert g["status"][rows].tolist() == [ar.STATUS_FAILED] * len(rows)
    for k in ("gyro_out", "gravity_body", "nis"):
        assert (g[k][rows] == 0).all(), k
    low = np.tril(np.ones((6, 6), dtype=bool))
    for k in ("q", "b"):
        assert np.array_equal(g[k][rows], bad[k][rows].astype(np.float32), equal_nan=True), k
    assert np.array_equal(g["P"][rows][:, low], bad["P"][rows].astype(np.float32)[:, low], equal_nan=True)
    # the resets that random inputs do not reach: exactly antiparallel, a zero accelerometer, and a zero u in a plain call
    acc = np.array(inp["accel"], copy=True)
    acc[0] = (0.0, 0.0, -9.81); acc[1] = 0.0
    spec = dict(inp, accel=acc, reset=True)
    ref = _ref(cfg, spec)
    got = _np(_call(env, cfg, spec))
    assert ref["status"][:2].tolist() == [ar.STATUS_RESET | ar.INFO_HALF_TURN, ar.STATUS_RESET | ar.INFO_ZERO]
    assert np.array_equal(got["q"][:2], np.array([[0, -1, 0, 0], [0, 0, 0, 1]], dtype=np.float32))
    compare(got, ref, who="special resets")
    body = np.array(inp["aux_body"], copy=True)
    body[2, live(2)] = 0.0
    spec = dict(inp, accel=acc, aux_body=body)
    ref = _ref(cfg, spec)
    assert ref["status"][:3].tolist() == [0, ar.INFO_ZERO, ar.INFO_ZERO << (1 + live(2))]
    compare(_np(_call(env, cfg, spec)), ref, who="zero vectors")


@functools.lru_cache(maxsize=None)
def _long_chain(n=E + 1, steps=200):
    """A scripted rotation with fp32-representable inputs and, per step, the fp64 chain's state and the fp32 reference chain's drift."""
    rng = np.random.default_rng(11)
    cfg = _cfg()
    dt = cfg["dt"]
    north = np.array([1.0, 0.0, 0.0])
    qt = _rand_quat(rng, n)
    q0 = F32(ar.normalise(ar.quat_mul(qt, ar.exp_quat(0.3 * _unit(rng.normal(size=(n, 3)))))))
    s64 = (q0, np.zeros((n, 3)), np.tile(np.diag([cfg["p0_theta"]] * 3 + [cfg["p0_b"]] * 3), (n, 1, 1)))
    s32 = tuple(v.astype(np.float32) for v in s64)
    inputs, states, drift = [], [], {k: 0.0 for k in _STATE}
    for k in range(steps):
        t = k * dt
        w = np.tile(np.array([0.5 * np.sin(0.7 * t), 0.4 * np.cos(0.5 * t), 0.3 * np.sin(0.3 * t + 1)]), (n, 1))
        qt = ar.normalise(ar.quat_mul(qt, ar.exp_quat(w * dt)))
        R = ar.quat_to_mat(qt)
        inp = dict(gyro=F32(w + np.array([0.02, -0.01, 0.03]) + 0.002 * rng.normal(size=(n, 3))),
                   accel=F32(np.einsum("nji,j->ni", R, -np.array(GRAVITY)) + 0.05 * rng.normal(size=(n, 3))),
                   aux_body=F32(np.einsum("nji,j->ni", R, north) + 0.01 * rng.normal(size=(n, 3)))[:, None],
                   aux_world=np.tile(north, (n, 1, 1)), aux_sigma=F32(np.full((n, 1), 0.02)))
        o64 = ar.update(cfg, *s64, gravity=GRAVITY, **inp)
        o32 = ar.update(cfg, *s32, gravity=GRAVITY, dtype=np.float32, **inp)
        s64, s32 = tuple(o64[k_] for k_ in _STATE), tuple(o32[k_] for k_ in _STATE)
        inputs.append(inp); states.append(s64)
        for i, k_ in enumerate(_STATE):
            scale = np.abs(s64[i]).reshape(n, -1).max(axis=1).reshape((n,) + (1,) * (s64[i].ndim - 1))
            drift[k_] = max(drift[k_], float((np.abs(s32[i].astype(np.float64) - s64[i]) / scale).max()))
    return cfg, q0, inputs, states, drift


def test_long_chain_yardstick_is_finite_and_small():
    """The fp32 reference's own drift from the fp64 chain over 200 updates, relative to the env's largest entry of q, b and P: the GPU
    test's bound is 4 x this."""
    _, _, _, _, drift = _long_chain()
    print(f"attitude, 200 chained updates: the fp32 reference's drift relative to the largest entry: {drift}")
    assert all(0 < v < 1e-2 for v in drift.values())


@pytest.mark.gpu
def test_long_chain_on_the_kernels_own_state():
    cfg, q0, inputs, states, drift = _long_chain()
    n = q0.shape[0]
    env = _env(n)
    c = _make_cfg(cfg)
    q, b, P = _dev(q0), torch.zeros((n, 3), device="cuda"), _dev(np.tile(np.diag([cfg["p0_theta"]] * 3 + [cfg["p0_b"]] * 3), (n, 1, 1)))
    status = torch.zeros((n,), dtype=torch.int32, device="cuda")
    dev = [{k: _dev(v) for k, v in inp.items()} for inp in inputs]
    worst = {k: 0.0 for k in _STATE}
    for k, (t, want) in enumerate(zip(dev, states)):
        env.sim.attitude_filter(c, q, b, P, status=status, **t)
        if k % 10 == 9 or k == len(dev) - 1:
            torch.cuda.synchronize()
            assert bool((status == 0).all()) and bool(torch.equal(P, P.transpose(1, 2))) and bool((torch.diagonal(P, dim1=1, dim2=2) > 0).all())
            for i, (name, got) in enumerate((("q", q), ("b", b), ("P", P))):
                scale = np.abs(want[i]).reshape(n, -1).max(axis=1).reshape((n,) + (1,) * (want[i].ndim - 1))
                worst[name] = max(worst[name], float((np.abs(got.cpu().numpy().astype(np.float64) - want[i]) / scale).max()))
    print(f"attitude, 200 chained kernel calls: drift relative to the largest entry {worst}; the fp32 reference's {drift}")
    for name in _STATE:
        assert worst[name] <= 4 * drift[name], (name, worst[name], drift[name])


@pytest.mark.gpu
def test_attitude_on_the_simulator_feeds_the_leg_odometry():
    """8 envs on the plane, 50 control steps of standing under a joint PD; an ImuModel with a gyro bias of 0.02 rad/s and the heading vector.
    The kernel is held, call by call on the logged inputs and from its own previous state, to the fp64 reference within 4 x the fp32
    reference's own largest ratio on those inputs (rounded up to a power of two); att.quat and att.gyro feed BaseStateEstimator.update to
    finite outputs and defined status words. The errors against the sim's quaternion and the bias error are printed, not asserted."""
    from wbc_amd.envs import AttitudeEstimator, ImuModel
    n = 8
    env = _env(n, seed=9)
    env.reset()
    env.reset_buf.zero_()
    est = env.base_state_estimator()
    att = env.attitude_estimator()
    imu = env.imu(gyro_bias=0.02, gyro_noise=0.002, accel_noise=0.05, heading_noise=0.01, seed=4)
    assert isinstance(att, AttitudeEstimator) and isinstance(imu, ImuModel)
    assert bool((att.status == abi.ATTITUDE_STATUS_RESET).all()) and torch.equal(att.bias, torch.zeros_like(att.bias))
    cfg = {k: float(getattr(att.cfg, k)) for k in ar.CFG_FIELDS}
    q0 = env.default_dof_pos.to(torch.float32).reshape(1, -1).expand(n, -1).clone()
    decimation = int(env.cfg.control.decimation)
    host = lambda t: t.cpu().numpy().astype(np.float64)                                # noqa: E731
    known = ar.STATUS_MASK | 31 * ar.INFO_ZERO | 31 * ar.INFO_PIVOT | ar.INFO_HALF_TURN
    logs = []
    for step in range(50):
        ds = env.sim.tensor("DOF_STATE")
        tau = (40.0 * (q0 - ds[:, :, 0]) - 1.0 * ds[:, :, 1]).clamp(-30.0, 30.0).contiguous()
        env.sim.set_dof_forces(tau)
        for _ in range(decimation):
            env.sim.simulate()
        gyro, accel, heading = imu.read()
        before = (host(att.quat), host(att.bias), host(att.P))
        att.update(gyro=gyro, accel=accel, aux=(heading, imu.heading_world, 0.05))
        est.update(quat=att.quat, gyro=att.gyro, accel=accel)
        torch.cuda.synchronize()
        li = att.last_inputs
        logs.append(dict(q=before[0], b=before[1], P=before[2], gyro=host(li["gyro"]), accel=host(li["accel"]), aux_body=host(li["aux_body"]),
                         aux_world=host(li["aux_world"]), aux_sigma=host(li["aux_sigma"]), reset=li["reset_mask"].cpu().numpy(), q_init=host(li["q_init"]),
                         got=_np(dict(q=att.quat, b=att.bias, P=att.P, gyro_out=att.gyro, gravity_body=att.gravity_body, nis=att.nis, status=att.status))))
        for name in ("quat", "bias", "P", "gyro", "gravity_body", "nis"):
            assert bool(torch.isfinite(getattr(att, name)).all()), (step, name)
        assert bool(((att.status & ~known) == 0).all()) and bool(((att.status & ar.STATUS_MASK) != ar.STATUS_FAILED).all())
        assert bool(torch.isfinite(est.x).all()) and bool(torch.isfinite(est.base_lin_vel).all())
        assert set(est.status.cpu().tolist()) <= {abi.ESTIMATOR_STATUS_OK, abi.ESTIMATOR_STATUS_RESET, abi.ESTIMATOR_STATUS_FAILED}
    gravity = tuple(float(g) for g in env.tcfg.gravity)
    k_sim = {k: 0.0 for k in ar.OUTPUTS}
    refs = []
    for lg in logs:
        kw = dict(accel=lg["accel"], aux_body=lg["aux_body"], aux_world=lg["aux_world"], aux_sigma=lg["aux_sigma"], reset_mask=lg["reset"],
                  q_init=lg["q_init"], gravity=gravity)
        ref = ar.update(cfg, lg["q"], lg["b"], lg["P"], lg["gyro"], **kw)
        r = ar.ratios(ar.update(cfg, lg["q"], lg["b"], lg["P"], lg["gyro"], dtype=np.float32, **kw), ref)
        k_sim = {k: max(k_sim[k], r[k]) for k in k_sim}
        refs.append(ref)
    const = {k: _pow2(max(v, 0.25)) for k, v in k_sim.items()}
    worst = {k: 0.0 for k in ar.OUTPUTS}
    for step, (lg, ref) in enumerate(zip(logs, refs)):
        r = compare(lg["got"], ref, const=const, who=("sim", step))
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"attitude on the simulator: K_ref {k_sim}, C {const}, kernel's largest ratios {worst}")
    R, Rt = ar.quat_to_mat(host(att.quat)), ar.quat_to_mat(ar.normalise(host(env.base_quat)))
    tilt = np.arccos(np.clip(np.einsum("ni,ni->n", R[:, 2, :], Rt[:, 2, :]), -1, 1))
    head = np.arctan2(R[:, 1, 0], R[:, 0, 0]) - np.arctan2(Rt[:, 1, 0], Rt[:, 0, 0])
    print(f"attitude on the simulator after 50 steps: tilt error {tilt.max():.3g} rad, heading error {np.abs(np.arctan2(np.sin(head), np.cos(head))).max():.3g} rad, "
          f"bias error {np.abs(host(att.bias) - 0.02).max():.3g} rad/s (bias 0.02)")
    # a partial reset leaves the others as they are
    keep = (att.quat.clone(), att.bias.clone(), att.P.clone())
    att.reset(env_ids=[1, 5])
    torch.cuda.synchronize()
    rest = [0, 2, 3, 4, 6, 7]
    assert all(torch.equal(t[rest], k[rest]) for t, k in zip((att.quat, att.bias, att.P), keep))
    assert bool((att.status[[1, 5]] == abi.ATTITUDE_STATUS_RESET).all()) and bool((att.bias[[1, 5]] == 0).all())
    att.reset(from_accel=True, accel=imu.read()[1])
    torch.cuda.synchronize()
    assert bool(((att.status & ar.STATUS_MASK) == abi.ATTITUDE_STATUS_RESET).all())
