"""Leg-odometry Kalman filter (wbc_sim_leg_odometry: wbc_leg_odometry_kernel in csrc/wbc_estimator_kernel.hip; definitions in
include/wbc_sim.h): the base's position and velocity and the four foot origins from orientation, gyro, joint state, accelerometer, contact
flags and foot heights. The CPU tests pin the fp64 restatement of tests/estimator_reference.py to properties of the equations -- it
recovers the truth on a consistent log, P+ is the Joseph form, swing rows vanish like 1 / kappa, the NIS averages m -- and measure the fp32
yardstick; the GPU tests hold the kernel to the reference entry by entry.

Bound: every entry of x, P, vel_body and nis satisfies |kernel - ref| <= C 2^-24 mag, mag the size of the terms summed into the entry as
estimator_reference.update returns it. C is 4 x K_ref rounded up to a power of two, K_ref the largest ratio of the reference run in fp32
against itself in fp64 over the judged cases, measured on the CPU and asserted there; it never comes from the kernel.

ONE UPDATE (n = 1, 13, 130; nine contact patterns x with / without height rows x with / without accel; CFG_ONE):

    output     K_ref     kernel's largest ratio on an MI355X     C
    x          2996      1981  (n = 130)                         16384
    P          12.7      14.4  (n = 130)                         64
    vel_body   168       18.1  (n = 130)                         1024
    nis        163       312   (n = 130)                         1024

x's K_ref is large because a random P of order 0.05 against measurement variances of 2.5e-5 makes S ill-conditioned (about 1e4, and 1e7
with swing rows inflated by kappa = 1000); the fp32 reference shows the same.

300 UPDATES of the consistent log with fp32-rounded inputs (n = 13, CFG_RUN; x and P after the last update):

    x          37        39.8                                    256
    P          24800     13744                                   131072

kappa is 1e9 there so that the swing feet's velocity rows, which no consistent log can satisfy, move v by less than fp32 resolves (the
kernel's v is within 2.7 x 2^-24 mag of the truth); a touch-down then cancels a foot variance of order 1 down to sigma_r^2, which is
why P's long-run constant is large. The smallest eigenvalue of the kernel's P over the run is 6.2e-7.

ON THE SIMULATOR the states exist on the GPU alone: that test measures K_ref by the same rule from the reference's fp32 run on the
logged inputs (32 / 102 / 3.5 / 0.07 for x / P / vel_body / nis; the kernel's 7.0 / 89 / 5.1 / 0.11).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import estimator_reference as er
from wbc_amd import abi

SENTINEL, ISENTINEL = 12345.0, -7777
SIZES = (1, 13, 130)
NX = er.NX
F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)                  # noqa: E731
GRAVITY = (0.0, 0.0, float(np.float32(-9.81)))


def _cfg(**kw):
    """The kernel receives the cfg as floats: the references use the same rounded values."""
    base = dict(dt=0.02, sigma_p=0.02, sigma_v=0.5, sigma_f=0.02, sigma_r=0.005, sigma_rdot=0.1, sigma_z=0.005, kappa=1000.0, p0_p=1e-4,
                p0_v=0.25, p0_f=1e-4)
    base.update(kw)
    return {k: float(np.float32(base[k])) for k in er.CFG_FIELDS}


CFG_ONE = _cfg()
CFG_RUN = _cfg(sigma_f=1e-4, kappa=1e9)
# test 2 runs in fp64 alone. No log can make a swing foot's rows consistent (its velocity row measures the foot's own motion, its position row
# a foothold that is being carried along), and they move (p, v) by O(1 / kappa) per update (test_swing_rows_vanish_like_one_over_kappa); a
# touch-down snaps p_i onto its measurement up to sigma_r^2 / (dt sigma_f^2 kappa) of the stale offset. Both are below 1e-9 with kappa = 1e12 and
# the foot process noise of CFG_ONE.
CFG_EXACT = dict(CFG_ONE, kappa=float(np.float32(1e12)))
RUN_STEPS, RUN_N, RUN_SEED = 300, 13, 1

# K_ref (measured by test_fp32_yardstick_is_where_the_constants_came_from), the kernel's largest ratio on the MI355X (for the record: no
# bound comes from it) and the constant
K_REF = {"x": 2996.0, "P": 12.7, "vel_body": 168.0, "nis": 163.0}
K_GPU = {"x": 1981.0, "P": 14.4, "vel_body": 18.1, "nis": 312.0}
LONG_K_REF = {"x": 37.0, "P": 24800.0}
LONG_K_GPU = {"x": 39.8, "P": 13744.0}
_pow2 = lambda k: float(2.0 ** np.ceil(np.log2(4 * k)))                             # noqa: E731
CONST = {k: _pow2(v) for k, v in K_REF.items()}
LONG_CONST = {k: _pow2(v) for k, v in LONG_K_REF.items()}
# static LDS bytes (per env: P 18 x 19, W 28 x 19, S 28 x 29, D 32, x 18, the legs' 4 x 6 and 4 floats; two envs per workgroup) as DESIGN.md states
LDS_BYTES = 2 * 4 * (18 * 19 + 28 * 19 + 28 * 29 + 32 + 18 + 24 + 4)

PATTERNS = [("all stance", (1, 1, 1, 1)), ("all swing", (0, 0, 0, 0)), ("FL", (1, 0, 0, 0)), ("FR", (0, 1, 0, 0)), ("RL", (0, 0, 1, 0)),
            ("RR", (0, 0, 0, 1)), ("FL+RR", (1, 0, 0, 1)), ("FR+RL", (0, 1, 1, 0)), ("half", (0.5, 0.5, 0.5, 0.5))]
COMBOS = [(p, heights, accel) for p in range(len(PATTERNS)) for heights in (True, False) for accel in (True, False)]


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _sym32(P):
    """fp32 values, exactly symmetric."""
    P = F32(P)
    return np.tril(P) + np.transpose(np.tril(P, -1), (0, 2, 1))


def one_update_inputs(n, combo, seed=0):
    """fp32-representable inputs of one update for n envs: joint states inside the limits, random orientations and gyros, a random
    positive-definite P (a Gram matrix plus the diagonal) and random x with the feet near where the legs put them."""
    m = _model()
    pattern, heights, accel = COMBOS[combo]
    rng = np.random.default_rng(7000 + 100 * combo + n + 1000003 * seed)
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    lo, hi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    dof = np.stack([lo + (hi - lo) * rng.uniform(0.05, 0.95, (n, 20)), rng.uniform(-3, 3, (n, 20))], axis=-1)
    inp = dict(quat=F32(quat), gyro=F32(rng.uniform(-2, 2, (n, 3))), dof=F32(dof),
               contact=F32(np.broadcast_to(np.array(PATTERNS[pattern][1], dtype=np.float64), (n, 4))),
               accel=F32(rng.normal(size=(n, 3)) * 3 + np.array([0, 0, 9.81])) if accel else None,
               foot_height=F32(rng.uniform(-0.05, 0.05, (n, 4))) if heights else None)
    _, r, _, _ = er.measurement(m, inp["quat"], inp["gyro"], inp["dof"])
    p = rng.uniform(-2, 2, (n, 3)); p[:, 2] = rng.uniform(0.2, 0.5, n)
    x = np.concatenate([p, rng.uniform(-1, 1, (n, 3)), (p[:, None, :] + r + rng.normal(size=(n, 4, 3)) * 0.03).reshape(n, 12)], axis=1)
    G = rng.normal(size=(n, NX, NX)) * 0.05
    P = G @ np.transpose(G, (0, 2, 1)) + np.eye(NX) * rng.uniform(0.005, 0.02, (n, NX))[:, None, :]
    inp.update(x=F32(x), P=_sym32(P))
    return inp


def _ref(inp, cfg=CFG_ONE, dtype=np.float64, **kw):
    return er.update(_model(), cfg, inp["x"], inp["P"], inp["quat"], inp["gyro"], inp["dof"], inp["contact"], accel=inp.get("accel"),
                     foot_height=inp.get("foot_height"), gravity=GRAVITY, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def _log():
    """The consistent log of tests 2, 4 and 10. Computed once and left unchanged."""
    return er.consistent_log(_model(), RUN_N, RUN_STEPS, CFG_RUN["dt"], seed=RUN_SEED, gravity=GRAVITY)


@functools.lru_cache(maxsize=None)
def _long_reference():
    """The fp64 reference after RUN_STEPS updates of the fp32-rounded log."""
    return er.run_log(_model(), CFG_RUN, _log(), RUN_STEPS, gravity=GRAVITY, cast=F32)


# ------------------------------------------------------------------------------------------------------------ CPU
_INPUTS = ("quat", "gyro", "dof", "accel", "contact", "foot_height", "reset_mask", "p_init")
_NAMES = ("sim", "cfg") + _INPUTS + ("flags", "x", "P", "vel_body", "nis", "status", "stream")


def _make_cfg(cfg=CFG_ONE, **kw):
    return abi.WbcEstimatorCfg(*[dict(cfg, **kw)[k] for k in er.CFG_FIELDS])


def _refusals(base):
    """[(arguments that differ from the good call `base`, a word of the message)]: every refusal of wbc_sim_leg_odometry but the NULL sim.
    The cfg structs are kept alive by the list's own entries."""
    out = [(dict(cfg=None), b"NULL"), (dict(contact=None), b"NULL"), (dict(x=None), b"NULL"), (dict(P=None), b"NULL"),
           (dict(flags=2), b"flag"), (dict(flags=-1), b"flag")]
    for field in ("dt", "sigma_p", "sigma_v", "sigma_f", "sigma_r", "sigma_rdot", "sigma_z", "p0_p", "p0_v", "p0_f"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            out.append((dict(cfg=_make_cfg(**{field: bad})), b"dt" if field == "dt" else (b"sigma" if field.startswith("sigma") else b"variance")))
    out += [(dict(cfg=_make_cfg(kappa=bad)), b"kappa") for bad in (-1e-3, float("nan"), float("inf"))]
    out += [({k: base[k] + off}, b"aligned") for k in _INPUTS + ("x", "P", "vel_body", "nis", "status") for off in (1, 2, 3)]
    return out


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_leg_odometry(*[C.byref(args[k]) if isinstance(args[k], abi.WbcEstimatorCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device(robot):
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    assert "wbc_sim_leg_odometry" in EXPORTED_SYMBOLS and hasattr(L, "wbc_sim_leg_odometry")
    assert C.sizeof(abi.WbcEstimatorCfg) == 4 * len(er.CFG_FIELDS) and [f for f, _ in abi.WbcEstimatorCfg._fields_] == list(er.CFG_FIELDS)
    assert (abi.ESTIMATOR_STATUS_OK, abi.ESTIMATOR_STATUS_RESET, abi.ESTIMATOR_STATUS_FAILED) == (er.STATUS_OK, er.STATUS_RESET, er.STATUS_FAILED)
    assert abi.ESTIMATOR_RESET == 1 and abi.ESTIMATOR_NX == NX
    assert tuple(float(g) for g in robot["tcfg"].gravity) == GRAVITY
    buf = (C.c_float * 512)()
    p = C.addressof(buf)
    base = dict(sim=None, cfg=_make_cfg(), flags=0, stream=None, x=p, P=p + 128, vel_body=p + 256, nis=p + 384, status=p + 512,
                **{k: p + 640 + 64 * i for i, k in enumerate(_INPUTS)})
    for kw, word in _refusals(base) + [(dict(), b"sim is NULL"), (dict(flags=abi.ESTIMATOR_RESET), b"sim is NULL")]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_leg_odometry: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def test_reference_recovers_the_truth_on_a_consistent_log():
    """A property of the equations: on a log whose prediction is exact and whose stance rows agree with it, p and v stay at the truth."""
    m, log = _model(), _log()
    k = 199
    scale_p, scale_v = np.abs(log["p"][:200]).max(), np.abs(log["v"][:200]).max()
    assert np.abs(log["v"][k]).max() > 0.05 and scale_v > 0.1                          # the base is moving where it is judged
    assert 0.3 < log["contact"].mean() < 0.8 and set(np.unique(log["contact"])) == {0.0, 1.0}
    out = er.run_log(m, CFG_EXACT, log, 200, heights=True, gravity=GRAVITY)
    ep, ev = np.abs(out["x"][:, 0:3] - log["p"][k]).max(), np.abs(out["x"][:, 3:6] - log["v"][k]).max()
    print(f"consistent log, 200 updates with heights: |p - truth| = {ep:.3g} of {scale_p:.3g}, |v - truth| = {ev:.3g} of {scale_v:.3g}")
    assert ep <= 1e-9 * scale_p and ev <= 1e-9 * scale_v and (out["status"] == er.STATUS_OK).all()
    out = er.run_log(m, CFG_EXACT, log, 200, heights=False, gravity=GRAVITY)
    ev = np.abs(out["x"][:, 3:6] - log["v"][k]).max()
    stance = log["contact"][k] == 1.0
    rel = (out["x"][:, None, 0:3] - out["x"][:, 6:].reshape(-1, 4, 3)) - (log["p"][k][:, None, :] - log["foot"][k])
    er_ = np.abs(rel[stance]).max()
    print(f"consistent log, 200 updates without heights: |v - truth| = {ev:.3g}, |(p - p_i) - truth| over stance feet = {er_:.3g}")
    assert ev <= 1e-9 * scale_v and er_ <= 1e-9 * er.reach(m).max() and stance.sum() >= 2 * RUN_N


def test_p_plus_is_the_joseph_form():
    for combo in (0, 1, 17, 34):
        inp = one_update_inputs(13, combo)
        out = _ref(inp)
        m = out["S"].shape[1]
        Cm = er.selection(m)
        K = out["K"]
        I_KC = np.eye(NX) - K @ Cm
        joseph = I_KC @ out["P_pred"] @ np.transpose(I_KC, (0, 2, 1)) + np.einsum("njk,nk,nlk->njl", K, out["Rm"], K)
        assert np.abs(out["P"] - joseph).max() <= 1e-12 * np.abs(out["P_pred"]).max(), combo
        assert np.array_equal(out["P"], np.transpose(out["P"], (0, 2, 1)))
        # and the gain is the textbook one
        assert np.abs(K - out["P_pred"] @ Cm.T @ np.linalg.inv(out["S"])).max() <= 1e-9 * np.abs(K).max()


def test_swing_rows_vanish_like_one_over_kappa():
    inp = one_update_inputs(13, 4)                                                      # all swing, heights, accel
    moved = []
    for kappa in (1e6, 1e8, 1e10):
        out = _ref(inp, cfg=dict(CFG_ONE, kappa=kappa))
        moved.append(np.abs(out["x"][:, 0:6] - out["x_pred"][:, 0:6]).max())
    print("all swing: largest move of (p, v) away from the prediction at kappa = 1e6, 1e8, 1e10:", moved)
    assert moved[0] < 1e-2 and all(0.005 < b / a < 0.02 for a, b in zip(moved, moved[1:]))


def test_nis_of_residuals_drawn_from_s_averages_m():
    """NIS = e^T S^-1 e of e ~ N(0, S) is chi-square with m degrees of freedom: mean m, variance 2 m. Over N = 4000 draws the mean lies
    within 5 standard errors, 5 sqrt(2 m / N), of m."""
    draws = 4000
    for combo in (0, 2):                                                               # m = 28 and m = 24
        inp = one_update_inputs(draws, combo)
        out = _ref(inp)
        m = out["S"].shape[1]
        rng = np.random.default_rng(5)
        e = np.einsum("nij,nj->ni", out["L"], rng.normal(size=(draws, m)))
        y = er.forward(out["L"], e[:, :, None])[:, :, 0]
        nis = (y * y).sum(-1)
        print(f"m = {m}: mean NIS over {draws} draws {nis.mean():.3f}")
        assert abs(nis.mean() - m) <= 5 * np.sqrt(2 * m / draws)


@functools.lru_cache(maxsize=None)
def _yardsticks():
    one = {k: 0.0 for k in er.OUTPUTS}
    for n in SIZES:
        for combo in range(len(COMBOS)):
            inp = one_update_inputs(n, combo)
            r = er.ratios(_ref(inp, dtype=np.float32), _ref(inp))
            one = {k: max(one[k], r[k]) for k in one}
    long = er.ratios(er.run_log(_model(), CFG_RUN, _log(), RUN_STEPS, gravity=GRAVITY, cast=F32, dtype=np.float32), _long_reference())
    return one, {k: long[k] for k in LONG_K_REF}


def test_fp32_yardstick_is_where_the_constants_came_from():
    one, long = _yardsticks()
    print("estimator yardsticks, one update: " + ", ".join(f"{k} K_ref = {one[k]:.3g} (C = {CONST[k]:g})" for k in one))
    print("estimator yardsticks, %d updates: " % RUN_STEPS + ", ".join(f"{k} K_ref = {long[k]:.3g} (C = {LONG_CONST[k]:g})" for k in long))
    for got, want, const in ((one, K_REF, CONST), (long, LONG_K_REF, LONG_CONST)):
        for k in want:
            assert abs(got[k] - want[k]) <= 0.25 * want[k], (k, got[k])               # a largest ratio moves with the summation order of the BLAS at hand
            assert 4 * got[k] <= const[k]


@functools.lru_cache(maxsize=None)
def _kernel_assembly():
    """csrc/wbc_estimator_kernel.hip compiled to gfx950 assembly with the build's own flags."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    if not os.path.exists(arm_codegen.HIPCC):
        pytest.skip("hipcc not installed")
    source = "wbc_estimator_kernel.hip"
    assert source in g.SOURCES and "wbc_estimator.h" in g.HEADERS
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "estimator.s")
        subprocess.check_call([arm_codegen.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        return open(out).read()


def test_estimator_kernel_codegen():
    """One kernel, no scratch, a single wavefront per workgroup and therefore no s_barrier, the static LDS DESIGN.md states, at most 128 VGPRs."""
    import re
    text = _kernel_assembly()
    assert text.count(".amdhsa_kernel ") == 1
    entry = text[text.index("amdhsa.kernels:"):]
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))
    assert re.search(r"\.name:\s+wbc_leg_odometry_kernel\n", entry)
    print(f"wbc_leg_odometry_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64
    assert meta("group_segment_fixed_size") == LDS_BYTES and LDS_BYTES // 2 < 8192 and meta("vgpr_count") <= 128
    body = text[text.index("\nwbc_leg_odometry_kernel:"):]
    body = body[:body.index(".Lfunc_end")]
    assert "s_endpgm" in body and "scratch_" not in body and "s_barrier" not in body


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _env(n, seed=5):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    return WidowGo1(cfg, sim_device="cuda:0", seed=seed)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


_SHAPES = {"x": (NX,), "P": (NX, NX), "vel_body": (3,), "nis": (), "status": ()}


def _call(env, inp, cfg=CFG_ONE, which=("vel_body", "nis", "status"), flags=0, x=None, P=None):
    """A direct C-ABI call into sentinel-framed buffers (x and P start from inp's, or from the tensors given); returns {name: [n, ...]
    tensor} of x, P and the outputs asked for. Inputs missing from inp, or None, are handed over as NULL."""
    n = env.num_envs
    size = {k: int(np.prod(s, dtype=np.int64)) for k, s in _SHAPES.items()}
    bufs = {}
    for name in ("x", "P") + tuple(which):
        bufs[name] = torch.full((n * size[name] + 8,), ISENTINEL if name == "status" else SENTINEL, dtype=torch.int32 if name == "status" else torch.float32, device="cuda")
    bufs["x"][:n * NX] = (_dev(inp["x"]) if x is None else x).reshape(-1)
    bufs["P"][:n * NX * NX] = (_dev(inp["P"]) if P is None else P).reshape(-1)
    tens = {k: _dev(inp.get(k), torch.int32 if k == "reset_mask" else torch.float32) for k in _INPUTS}
    ptr = lambda d, k: d[k].data_ptr() if d.get(k) is not None else None
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_leg_odometry(env.sim.h, C.byref(c), *[ptr(tens, k) for k in _INPUTS], flags, ptr(bufs, "x"), ptr(bufs, "P"),
                                        ptr(bufs, "vel_body"), ptr(bufs, "nis"), ptr(bufs, "status"), None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert bool((b[n * size[name]:] == (ISENTINEL if name == "status" else SENTINEL)).all()), name
    return {name: b[:n * size[name]].view((n,) + _SHAPES[name]).clone() for name, b in bufs.items()}


def _np(got):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in got.items() if k != "status"}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_one_update_every_entry_against_fp64(n):
    env = _env(n)
    worst = {k: 0.0 for k in er.OUTPUTS}
    for combo in range(len(COMBOS)):
        inp = one_update_inputs(n, combo)
        ref, got = _ref(inp), _call(env, inp)
        r = er.ratios(_np(got), ref)
        worst = {k: max(worst[k], r[k]) for k in worst}
        assert bool(torch.isfinite(got["x"]).all()) and bool(torch.isfinite(got["P"]).all())
        assert got["status"].cpu().numpy().tolist() == ref["status"].tolist() and (ref["status"] == er.STATUS_OK).all()
        assert torch.equal(got["P"], got["P"].transpose(1, 2)), COMBOS[combo]
        for k in er.OUTPUTS:
            assert r[k] <= CONST[k], (COMBOS[combo], k, r[k])
    print(f"estimator one update n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")


@pytest.mark.gpu
def test_null_inputs_mean_the_sims_state():
    n = 130
    env = _env(n)
    inp = one_update_inputs(n, 0)
    rng = np.random.default_rng(11)
    root = env.sim.tensor("ROOT_STATES").clone()
    # the first half: orientations whose rotation matrices are signed identities, where R^T w is exact in any arithmetic
    flips = np.array([[0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    quat = inp["quat"].copy()
    quat[: n // 2] = flips[np.arange(n // 2) % 4]
    w_world = F32(rng.uniform(-2, 2, (n, 3)))
    R = er.quat_to_mat(quat)
    w_world[n // 2:] = 0.0                                                              # general orientations: no angular velocity, R^T 0 = 0
    gyro = np.einsum("nji,nj->ni", R, w_world)
    assert np.array_equal(F32(gyro), gyro)
    root[:, 0, 3:7] = _dev(quat); root[:, 0, 10:13] = _dev(w_world)
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(_dev(inp["dof"]))
    torch.cuda.synchronize()
    inp = dict(inp, quat=quat, gyro=gyro)
    want = _call(env, inp)
    for drop in (("quat",), ("gyro",), ("dof",), ("quat", "gyro", "dof")):
        got = _call(env, {k: v for k, v in inp.items() if k not in drop})
        for k in want:
            assert torch.equal(got[k], want[k]), (drop, k)
    # general orientations with a gyro from the sim: against fp64, with R^T w formed there
    quat, w_world = one_update_inputs(n, 0)["quat"], F32(rng.uniform(-2, 2, (n, 3)))
    root[:, 0, 3:7] = _dev(quat); root[:, 0, 10:13] = _dev(w_world)
    env.sim.set_root_state(root.contiguous())
    torch.cuda.synchronize()
    inp = dict(inp, quat=quat, gyro=np.einsum("nji,nj->ni", er.quat_to_mat(quat), w_world))
    got = _call(env, {k: v for k, v in inp.items() if k not in ("quat", "gyro", "dof")})
    r = er.ratios(_np(got), _ref(inp))
    print(f"estimator, gyro and orientation from the sim: largest ratios {r}")
    assert all(r[k] <= CONST[k] for k in er.OUTPUTS), r


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_reset_by_mask_and_by_flag(n):
    env = _env(n)
    inp = one_update_inputs(n, 0)
    rng = np.random.default_rng(12)
    mask = (rng.random(n) < 0.4).astype(np.int32) * rng.integers(1, 9, n).astype(np.int32)   # any non-zero entry resets
    if n > 1:
        mask[0], mask[1] = 0, 5
    p_init = F32(rng.uniform(-3, 3, (n, 3)))
    plain = _call(env, inp)
    for p0 in (p_init, None):
        got = _call(env, dict(inp, reset_mask=mask, p_init=p0))
        ref = _ref(inp, reset=mask, p_init=p0)
        hit = torch.tensor(mask != 0, device="cuda")
        assert got["status"].cpu().numpy().tolist() == np.where(mask != 0, er.STATUS_RESET, er.STATUS_OK).tolist()
        for k in got:                                                               # the unmasked envs: the bits of the call without a mask
            assert torch.equal(got[k][~hit], plain[k][~hit]), k
        g = _np(got)
        rs = mask != 0
        want_p = np.zeros((n, 3)) if p0 is None else p0
        assert np.array_equal(g["x"][rs, 0:3], want_p[rs]) and (g["x"][rs, 3:6] == 0).all() and (g["vel_body"][rs] == 0).all() and (g["nis"][rs] == 0).all()
        assert np.array_equal(g["P"][rs], np.broadcast_to(ref["P"][rs][:1], ref["P"][rs].shape)) if rs.any() else True
        r = er.ratios(g, ref)
        assert all(r[k] <= CONST[k] for k in er.OUTPUTS), r                          # the p_i = p + r_i among them
    got = _call(env, dict(inp, p_init=p_init), flags=abi.ESTIMATOR_RESET)
    ref = _ref(inp, reset=True, p_init=p_init)
    assert bool((got["status"] == er.STATUS_RESET).all())
    r = er.ratios(_np(got), ref)
    assert all(r[k] <= CONST[k] for k in er.OUTPUTS), r
    diag = np.array([CFG_ONE["p0_p"]] * 3 + [CFG_ONE["p0_v"]] * 3 + [CFG_ONE["p0_f"]] * 12)
    assert np.array_equal(_np(got)["P"], np.broadcast_to(np.diag(diag), (n, NX, NX)))
    # a reset env's x and P are not read: garbage in them does not matter
    junk = _call(env, dict(inp, p_init=p_init), flags=abi.ESTIMATOR_RESET, x=torch.full((n, NX), float("nan"), device="cuda"),
                 P=torch.full((n, NX, NX), float("nan"), device="cuda"))
    assert all(torch.equal(junk[k], got[k]) for k in got)


@pytest.mark.gpu
def test_failed_factorisation_keeps_the_prediction():
    n = 130
    env = _env(n)
    for combo in (0, 3):
        inp = one_update_inputs(n, combo)
        broken = np.array([0, 1, 31, 32, 33, 64, 97, 129])
        P = inp["P"].copy()
        for i, e in enumerate(broken):
            j = (0, 3, 8, 17, 5, 1, 7, 4)[i]
            P[e, j, j] = -50.0                                                         # S's own diagonal turns negative
        got = _call(env, dict(inp, P=P))
        ref = _ref(dict(inp, P=P))
        assert ref["status"][broken].tolist() == [er.STATUS_FAILED] * len(broken) and (np.delete(ref["status"], broken) == er.STATUS_OK).all()
        assert got["status"].cpu().numpy().tolist() == ref["status"].tolist()
        assert all(bool(torch.isfinite(got[k]).all()) for k in ("x", "P", "vel_body", "nis"))
        g = _np(got)
        r = er.ratios(g, ref)                                                       # the failed envs: (x-, P-) as the reference predicts them
        assert all(r[k] <= CONST[k] for k in er.OUTPUTS), r
        assert (g["nis"][broken] == 0).all()
        ok = torch.tensor(np.delete(np.arange(n), broken), device="cuda")
        plain = _call(env, inp)
        for k in got:                                                               # their neighbours: the bits of the launch without them
            assert torch.equal(got[k][ok], plain[k][ok]), k


@pytest.mark.gpu
def test_three_hundred_updates_of_the_consistent_log():
    env, log, ref = _env(RUN_N), _log(), _long_reference()
    s = log["start"]
    start = dict(quat=F32(s["quat"]), gyro=F32(s["gyro"]), dof=F32(s["dof"]), contact=F32(s["contact"]), p_init=F32(log["p0"]),
                 x=np.zeros((RUN_N, NX)), P=np.zeros((RUN_N, NX, NX)))
    got = _call(env, start, cfg=CFG_RUN, flags=abi.ESTIMATOR_RESET)
    x, P = got["x"], got["P"]
    dev = {k: _dev(F32(log[k])) for k in ("quat", "gyro", "dof", "accel", "contact", "foot_height")}
    cfg = _make_cfg(CFG_RUN)
    status = torch.zeros(RUN_N, dtype=torch.int32, device="cuda")
    history = torch.empty((RUN_STEPS, RUN_N, NX, NX), device="cuda")
    for k in range(RUN_STEPS):
        env.sim.leg_odometry(cfg, x, P, dev["contact"][k], quat=dev["quat"][k], gyro=dev["gyro"][k], dof=dev["dof"][k], accel=dev["accel"][k],
                             foot_height=dev["foot_height"][k], status=status)
        history[k] = P
    torch.cuda.synchronize()
    assert bool((status == er.STATUS_OK).all())
    assert torch.equal(history, history.transpose(2, 3))                               # bit-symmetric after every update
    eig = np.linalg.eigvalsh(history.cpu().numpy().astype(np.float64))
    print(f"estimator, {RUN_STEPS} updates: smallest eigenvalue of P over the run {eig.min():.3g}")
    assert eig.min() > 0
    g = dict(x=x.cpu().numpy().astype(np.float64), P=P.cpu().numpy().astype(np.float64))
    r = {k: er.ratios(dict(g, vel_body=ref["vel_body"], nis=ref["nis"]), ref)[k] for k in ("x", "P")}
    v_err = np.abs(g["x"][:, 3:6] - log["v"][RUN_STEPS - 1]) / (er.EPS * ref["mag"]["x"][:, 3:6])
    print(f"estimator, {RUN_STEPS} updates: largest |kernel - ref| / (2^-24 mag): {r}; |v - truth| / (2^-24 mag) {v_err.max():.3g}")
    assert all(r[k] <= LONG_CONST[k] for k in r), r
    assert v_err.max() <= LONG_CONST["x"]


@pytest.mark.gpu
def test_on_the_simulator_against_the_replayed_reference():
    """Every update of BaseStateEstimator.update() with its defaults, replayed in fp64 from the tensors the call was handed (x and P before it
    among them). Measured on an MI355X: see DESIGN.md; the error against the true base_lin_vel is printed, not asserted."""
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    n = 64
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    env = WidowGo1(cfg, sim_device="cuda:0", seed=9)
    env.sim.tensor("EPISODE_LENGTH")[::7] = int(env.max_episode_length) - torch.arange(5, 5 + len(range(0, n, 7)) * 6, 6, device="cuda")   # time-outs mid-run
    est = env.base_state_estimator()
    c = {k: float(getattr(est.cfg, k)) for k in er.CFG_FIELDS}
    assert abs(c["dt"] - env.dt) < 1e-9
    gen = torch.Generator(device="cuda"); gen.manual_seed(77)
    worst, k_ref, resets, errs = {k: 0.0 for k in er.OUTPUTS}, {k: 0.0 for k in er.OUTPUTS}, 0, []
    host = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float64)
    for phase in ("zero actions", "seeded actions"):
        err = []
        for _ in range(40):
            a = torch.zeros(n, 18, device="cuda") if phase == "zero actions" else torch.randn(n, 18, device="cuda", generator=gen) * 0.8
            env.step(a)
            x0, P0 = host(est.x), host(est.P)
            est.update()
            torch.cuda.synchronize()
            li = est.last_inputs
            assert li["quat"] is None and li["gyro"] is None and li["dof"] is None        # the defaults: the sim's state
            root = host(env.sim.tensor("ROOT_STATES"))[:, 0]
            gyro = np.einsum("nji,nj->ni", er.quat_to_mat(root[:, 3:7]), root[:, 10:13])
            args = (env.robot_model, c, x0, P0, root[:, 3:7], gyro, host(env.sim.tensor("DOF_STATE")), host(li["contact"]))
            kw = dict(accel=host(li["accel"]), foot_height=host(li["foot_height"]), gravity=GRAVITY, reset=host(li["reset_mask"]), p_init=host(li["p_init"]))
            ref = er.update(*args, **kw)
            got = dict(x=host(est.x), P=host(est.P), vel_body=host(est.base_lin_vel), nis=host(est.nis))
            assert est.status.cpu().numpy().tolist() == ref["status"].tolist()
            resets += int((ref["status"] == er.STATUS_RESET).sum())
            r = er.ratios(got, ref)
            worst = {k: max(worst[k], r[k]) for k in worst}
            y = er.ratios(er.update(*args, dtype=np.float32, **kw), ref)                # the yardstick on the same logged inputs
            k_ref = {k: max(k_ref[k], y[k]) for k in k_ref}
            assert torch.equal(est.position, est.x[:, 0:3]) and torch.equal(est.foot_positions.reshape(n, 12), est.x[:, 6:])
            err.append((est.base_lin_vel - env.base_lin_vel).abs().max(dim=1).values.cpu().numpy())
        errs.append(np.array(err))
    print(f"estimator on the simulator, 2 x 40 steps of {n} envs, {resets} resets: largest |kernel - ref| / (2^-24 mag) {worst}")
    for phase, e in zip(("zero actions", "seeded actions"), errs):
        print(f"  {phase}: |base_lin_vel estimate - true base_lin_vel| (m/s), max over axes: mean {e.mean():.4f}, 95th percentile "
              f"{np.percentile(e, 95):.4f}, max {e.max():.4f}")
    # these states exist on the GPU alone, so their K_ref cannot be among the constants above: it is measured here, by the same rule, from the
    # reference's own fp32 run on the logged inputs (never from the kernel)
    # (with a floor of 4: a different summation order cannot be held to less than a few roundings of the terms)
    const = {k: max(_pow2(max(k_ref[k], 1e-3)), 4.0) for k in er.OUTPUTS}
    print(f"  K_ref on the logged inputs {k_ref}, constants {const}")
    assert resets > 0
    assert all(worst[k] <= const[k] for k in er.OUTPUTS), (worst, const)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_partial_outputs_have_the_bits_of_the_full_launch(n):
    env = _env(n)
    inp = one_update_inputs(n, 5)
    before = [env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")]
    want = _call(env, inp)
    for which in ((), ("vel_body",), ("nis",), ("status",), ("vel_body", "status"), ("nis", "status")):
        got = _call(env, inp, which=which)
        assert set(got) == {"x", "P"} | set(which)
        for k in got:
            assert torch.equal(got[k], want[k]), (which, k)
    x, P = _dev(inp["x"]), _dev(inp["P"])
    outs = env.sim.leg_odometry(_make_cfg(), x, P, _dev(inp["contact"]), quat=_dev(inp["quat"]),
                                gyro=_dev(inp["gyro"]), dof=_dev(inp["dof"]), accel=_dev(inp["accel"]), foot_height=_dev(inp["foot_height"]))
    assert len(outs) == 5 and all(torch.equal(a, want[k]) for a, k in zip(outs, ("x", "P", "vel_body", "nis", "status")))
    torch.cuda.synchronize()
    for k, t in zip(("ROOT_STATES", "DOF_STATE", "BODY_PARAMS"), before):
        assert torch.equal(env.sim.tensor(k), t), k                                   # the sim's state is read, never written


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env = _env(n)
    inp = one_update_inputs(n, 0)
    want = _call(env, inp)
    cfg = _make_cfg()
    t = {k: _dev(inp[k]) for k in ("quat", "gyro", "dof", "accel", "contact", "foot_height")}
    x, P = _dev(inp["x"]), _dev(inp["P"])
    outs = [torch.zeros_like(want[k]) for k in ("vel_body", "nis", "status")]
    call = lambda: env.sim.leg_odometry(cfg, x, P, t["contact"], quat=t["quat"], gyro=t["gyro"], dof=t["dof"], accel=t["accel"],
                                        foot_height=t["foot_height"], vel_body=outs[0], nis=outs[1], status=outs[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                     # warm-up off the default stream
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    x.copy_(_dev(inp["x"])); P.copy_(_dev(inp["P"]))                                   # the update is in place: start the replay where `want` started
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, want[k]) for a, k in zip([x, P] + outs, ("x", "P", "vel_body", "nis", "status")))


@pytest.mark.gpu
def test_every_refusal_leaves_the_buffers_untouched():
    n = 13
    env = _env(n)
    L, h = env.sim.L, env.sim.h
    inp = one_update_inputs(n, 0)
    size = {"x": NX, "P": NX * NX, "vel_body": 3, "nis": 1, "status": 1}
    bufs = {k: torch.full((n * size[k] + 8,), SENTINEL, dtype=torch.float32, device="cuda") for k in ("x", "P", "vel_body", "nis")}
    bufs["status"] = torch.full((n + 8,), ISENTINEL, dtype=torch.int32, device="cuda")
    tens = {k: _dev(inp[k]) for k in ("quat", "gyro", "dof", "accel", "contact", "foot_height")}
    tens["reset_mask"] = torch.zeros(n, dtype=torch.int32, device="cuda"); tens["p_init"] = torch.zeros(n, 3, device="cuda")
    base = dict(sim=h, cfg=_make_cfg(), flags=0, stream=None, **{k: t.data_ptr() for k, t in tens.items()}, **{k: b.data_ptr() for k, b in bufs.items()})
    call = lambda **kw: _raw_call(L, base, **kw)
    for kw, word in _refusals(base) + [(dict(sim=None), b"sim is NULL")]:
        assert call(**kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_leg_odometry: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == (ISENTINEL if k == "status" else SENTINEL)).all()), k
    # kappa = 0 is allowed, and 4-byte alignment is enough
    zero = _make_cfg(kappa=0.0)
    bufs["x"][1:1 + n * NX] = _dev(inp["x"]).reshape(-1); bufs["P"][1:1 + n * NX * NX] = _dev(inp["P"]).reshape(-1)
    assert call(cfg=zero, x=bufs["x"].data_ptr() + 4, P=bufs["P"].data_ptr() + 4, vel_body=None, nis=None, status=None) == 0
    torch.cuda.synchronize()
    ref = _ref(inp, cfg=dict(CFG_ONE, kappa=0.0))
    got = dict(x=bufs["x"][1:1 + n * NX].view(n, NX).cpu().numpy().astype(np.float64), P=bufs["P"][1:1 + n * NX * NX].view(n, NX, NX).cpu().numpy().astype(np.float64),
               vel_body=ref["vel_body"], nis=ref["nis"])
    r = er.ratios(got, ref)
    assert r["x"] <= CONST["x"] and r["P"] <= CONST["P"], r
    assert float(bufs["x"][0]) == SENTINEL and bool((bufs["x"][1 + n * NX:] == SENTINEL).all()) and bool((bufs["P"][1 + n * NX * NX:] == SENTINEL).all())
    assert all(bool((bufs[k] == (ISENTINEL if k == "status" else SENTINEL)).all()) for k in ("vel_body", "nis", "status"))


@pytest.mark.gpu
def test_step_is_untouched_by_the_estimator():
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    n = 64
    finals = []
    for use in (False, True):
        cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
        env = WidowGo1(cfg, sim_device="cuda:0", seed=6)
        est = env.base_state_estimator(kappa=100.0) if use else None
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        for k in range(5):
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                before = [env.sim.tensor(t).clone() for t in ("ROOT_STATES", "DOF_STATE")]
                est.update()
                if k == 2:                                                          # a partial reset: the listed envs, and nothing else
                    kept = [t.clone() for t in (est.x, est.P, est.base_lin_vel, est.nis, est.status)]
                    ids = [0, 5, 63]
                    est.reset(ids)
                    rest = torch.ones(n, dtype=torch.bool, device="cuda"); rest[ids] = False
                    assert all(torch.equal(t[rest], b[rest]) for t, b in zip((est.x, est.P, est.base_lin_vel, est.nis, est.status), kept))
                    assert bool((est.status[ids] == er.STATUS_RESET).all()) and torch.equal(est.position[ids], env.root_states[ids, 0:3])
                    assert bool((est.velocity[ids] == 0).all()) and bool((est.P[ids] == torch.diag_embed(est.P[ids].diagonal(dim1=1, dim2=2))).all())
                torch.cuda.synchronize()
                assert all(torch.equal(env.sim.tensor(t), b) for t, b in zip(("ROOT_STATES", "DOF_STATE"), before))
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)
