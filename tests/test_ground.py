"""Ground plane, normals and foot heights from the footholds (wbc_sim_ground_estimate: wbc_ground_estimate_kernel in
csrc/wbc_ground_kernel.hip; the text both implement is the comment in include/wbc_sim.h). The CPU tests pin the fp64 restatement of
tests/ground_reference.py to properties of the equations and measure the fp32 yardstick; the GPU tests hold the kernel to the reference
entry by entry.

Bound: every entry of a continuous output and of the state satisfies |kernel - ref| <= C 2^-24 mag, mag as ground_reference's docstring
lists it (anchored quantities from |d_i| and |m_i - cbar|, not from |m_i|). C is 4 x K_ref rounded up to a power of two, K_ref the largest
ratio of the reference run in fp32 against itself in fp64 over the judged cases (every call of every chain: SIZES x COMBOS x NCALLS),
measured on the CPU and asserted there; it never comes from the kernel.

    output      K_ref    kernel's largest ratio on an MI355X    C
    normal      0.633    0.729  (n = 17)                        4
    ground      0.765    0.691  (n = 64)                        4
    residual    0.855    0.855  (n = 63)                        4
    trunk       1.01     0.744  (n = 15)                        8
    theta_ref   0.758    0.846  (n = 130)                       4
    query_z     0.875    0.763  (n = 130)                       4
    state       3.35     3.36   (n = 17)                        16

Thin env-cases: 21 of 8904 (the cap is 1 %). Over 200 chained calls on its own state the kernel's largest ratios against the fp64 chain are
the fp32 reference's own (state 43 777 against 48 516, ground 1.73 against 1.10, the others equal to three digits). On the simulator (8 envs,
40 control steps, the yardstick measured in the test from the logged inputs): K_ref at most 1.43 (trunk), the kernel the same to the digits
printed; |ground - FOOT_RADIUS| <= 0.003 mm, the largest |residual| 0.001 mm, the normal world z.

The judged cases: n in SIZES, Q in {0, 1, 5} and NULL / given quat, dof, base_pos (COMBOS), every fifth env 900 m from the origin in x and
y (every tenth with no standing foot in the plain calls, so that its fit runs on stored points alone and its magnitudes hold no |b|: the
kernel's centring is judged there), every seventh env of the second call with its four contact points moved to within 1 mm of a line (no
posture puts four feet on a line), trunks tilted by up to 0.7 rad about each axis so that the slopes reach beyond slope_max = 0.45, and four chained
calls, each from the previous reference state rounded to fp32: a reset of all, a plain call, a masked reset, a plain call.

Info bits match exactly except in THIN env-cases, judged from the fp64 reference alone (judge()): a contact within 2^-24 of c_on, |a|
within C_state 2^-24 mag of slope_max, the pivot d1 within its bound of 0. A thin env is left out; the cap is 1 % of the env-cases."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import estimator_reference as er
import ground_reference as gr
from wbc_amd import abi
from wbc_amd.abi import WbcGroundCfg  # noqa: F401  (this file is about wbc_sim_ground_estimate: none of it means anything without the call)

SENTINEL, ISENTINEL = 12345.0, -7777
EPS = 2.0 ** -24
F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)                  # noqa: E731
SIZES = (1, 15, 16, 17, 63, 64, 65, 130)
# (the inputs handed over as NULL, Q)
COMBOS = (((), 0), (("quat",), 1), (("dof",), 5), (("base_pos",), 1), (("quat", "dof", "base_pos"), 5), ((), 5))
NCALLS = 4
THIN_CAP = 0.01
FAR = 900.0

# K_ref (measured by test_fp32_yardstick_is_where_the_constants_came_from), the kernel's largest ratio on the MI355X (for the record: no
# bound comes from it) and the constant
K_REF = {"normal": 0.633, "ground": 0.765, "residual": 0.855, "trunk": 1.01, "theta_ref": 0.758, "query_z": 0.875, "state": 3.35}
K_GPU = {"normal": 0.729, "ground": 0.691, "residual": 0.855, "trunk": 0.744, "theta_ref": 0.846, "query_z": 0.763, "state": 3.36}
_pow2 = lambda k: float(2.0 ** np.ceil(np.log2(4 * k)))                             # noqa: E731
CONST = {k: _pow2(v) for k, v in K_REF.items()}


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _cfg(**kw):
    """The kernel receives the cfg as floats: the references use the same rounded values."""
    base = {"dt": 0.02, "c_on": 0.5, "tau_age": 0.3, "lambda": 0.01, "slope_max": 0.45, "tilt_gain": 0.8}
    base.update(kw)
    return {k: float(np.float32(base[k])) for k in gr.CFG_FIELDS}


def _make_cfg(cfg, **kw):
    c = dict(cfg, **kw)
    return abi.WbcGroundCfg(*[c[k] for k in gr.CFG_FIELDS])


def _inputs(n, combo, call=0):
    """fp32-representable inputs of call number `call` of a chain: trunks tilted by up to 0.7 rad about each axis at every heading, leg
    joints inside their limits, both moving a little from call to call, contacts either side of c_on; every fifth env 900 m out, every
    tenth with no standing foot in the plain calls."""
    m = _model()
    env_rng = np.random.default_rng(9000 + 31 * combo + n)                               # the env's place, heading, tilt and posture: one per chain
    rng = np.random.default_rng(9000 + 31 * combo + 1009 * (call + 1) + n)               # what moves from call to call
    b = np.stack([env_rng.uniform(-2, 2, n), env_rng.uniform(-2, 2, n), env_rng.uniform(0.25, 0.4, n)], axis=-1)
    b[::5, 0:2] += FAR
    b += rng.uniform(-0.03, 0.03, (n, 3))
    yaw, rp = env_rng.uniform(-np.pi, np.pi, n), env_rng.uniform(-0.7, 0.7, (n, 2))
    dlo, dhi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    q = dlo + (dhi - dlo) * env_rng.uniform(0.2, 0.8, (n, 20)) + rng.uniform(-0.1, 0.1, (n, 20))
    rng, step_rng = env_rng, rng
    # the far envs: a freshly latched foot there carries |b| = 900 in its magnitude, which makes the band around slope_max that counts as
    # thin wide (it grows with the slope); they stand near the default posture, every tenth pitched by 0.15 .. 0.25 rad (slopes near 0.2)
    # and the others by 0.85 .. 0.95 rad (slopes above 1), so that both sides of the clamp are met there and the band is not
    nf = len(q[::5])
    q[::5] = np.asarray(er.STAND) + rng.uniform(-0.01, 0.01, (nf, 20))
    rp[::5, 0] = rng.uniform(-0.02, 0.02, nf)
    rp[::5, 1] = np.where(np.arange(nf) % 2 == 0, rng.uniform(0.15, 0.25, nf), rng.uniform(0.85, 0.95, nf)) * rng.choice([-1.0, 1.0], nf)
    ang = np.linalg.norm(rp, axis=1)                                                     # a tilt by |rp| about (rp, 0) in the heading frame, then the yaw
    tx, ty, tw = rp[:, 0] / ang * np.sin(ang / 2), rp[:, 1] / ang * np.sin(ang / 2), np.cos(ang / 2)
    yz, yw = np.sin(yaw / 2), np.cos(yaw / 2)
    quat = np.stack([yw * tx - yz * ty, yw * ty + yz * tx, yz * tw, yw * tw], axis=-1)
    rng = step_rng
    quat *= rng.uniform(0.8, 1.2, (n, 1))                                                # normalised in the call
    dof = F32(np.stack([q, rng.uniform(-2, 2, (n, 20))], axis=-1))
    contact = np.where(rng.random((n, 4)) < 0.5, rng.uniform(0.55, 1.0, (n, 4)), rng.uniform(0.0, 0.45, (n, 4)))
    if call in (1, 3):
        contact[::10] = rng.uniform(0.0, 0.45, (len(contact[::10]), 4))
        contact[::7] = rng.uniform(0.0, 0.45, (len(contact[::7]), 4))
    mask = (rng.random(n) < 0.3).astype(np.int32) * rng.integers(1, 5, n).astype(np.int32)
    nq = COMBOS[combo][1]
    query = b[:, None, 0:2] + rng.uniform(-0.6, 0.6, (n, nq, 2))
    return dict(base_pos=F32(b), quat=F32(quat), dof=dof, contact=F32(contact), mask=mask, query_xy=F32(query) if nq else None)


def _collinear(state, rng):
    """Every seventh env's four contact points moved to within 1 mm of a line through its foot 0's point."""
    state = np.array(state, copy=True)
    n = state.shape[0]
    for e in range(0, n, 7):
        u = rng.normal(size=3); u[2] *= 0.3; u /= np.linalg.norm(u)
        m0 = state[e, 0:3].copy()
        for i in range(4):
            state[e, 5 * i:5 * i + 3] = m0 + (i / 3.0 - 0.4) * 0.6 * u + rng.uniform(-1e-3, 1e-3, 3) / np.sqrt(3.0)
    return state


def _ref(cfg, inp, dtype=np.float64):
    return gr.estimate(_model(), cfg, inp["state"], inp["quat"], inp["dof"], inp["base_pos"], inp["contact"], reset=inp.get("reset"),
                       query_xy=inp.get("query_xy"), dtype=dtype)


@functools.lru_cache(maxsize=None)
def _chain(n, combo):
    """[(inputs, fp64 reference)] of NCALLS calls: a reset of every env, a plain call, a masked reset, a plain call, each from the previous
    reference's state rounded to fp32 (the second call's with every seventh env's points on a line). Computed once and left unchanged."""
    cfg = _cfg()
    state = np.zeros((n, gr.NS))
    calls = []
    for j in range(NCALLS):
        inp = _inputs(n, combo, j)
        if j == 1:
            state = _collinear(state, np.random.default_rng(77 + n + combo))
        inp["state"] = F32(state)
        if j == 0:
            inp["reset"] = True
        elif j == 2:
            inp["reset"] = inp["mask"]
        ref = _ref(cfg, inp)
        calls.append((inp, ref))
        state = ref["state"]
    return cfg, calls


def judge(cfg, ref, const=None):
    """From the fp64 reference alone: env_ok [N], False for a thin env and for a failed one."""
    const = CONST if const is None else const
    d = ref["diag"]
    ok = (np.abs(d["contact"] - cfg["c_on"]) >= EPS).all(1)
    ok &= np.abs(d["slope"] - cfg["slope_max"]) >= const["state"] * EPS * d["slope_mag"]
    ok &= ~(np.abs(d["pivot"]) < const["state"] * EPS * d["pivot_mag"]) | ~d["fit"]["ok"]
    return ok & ~d["failed"]


def compare(got, ref, cfg, const=None, who=""):
    """Hold `got` (numpy, any float type) to the fp64 reference: the info word exactly and the continuous entries within the bound, outside
    thin env-cases. Returns (the largest ratios, thin env-cases, env-cases)."""
    const = CONST if const is None else const
    ok = judge(cfg, ref, const)
    assert np.array_equal(np.asarray(got["info"]).astype(np.int64)[ok], ref["info"][ok]), who
    r = gr.ratios(got, ref, ok)
    for k in gr.OUTPUTS:
        assert r[k] <= const[k], (who, k, r[k])
    return r, int((~ok & ~ref["diag"]["failed"]).sum()), ok.size


# ------------------------------------------------------------------------------------------------------------ CPU
_INPUTS = ("quat", "dof", "base_pos", "contact", "reset_mask", "query_xy")
_OUTS = ("normal", "ground", "residual", "trunk", "theta_ref", "query_z", "info")
_NAMES = ("sim", "cfg") + _INPUTS + ("num_query", "flags", "state") + _OUTS + ("stream",)


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_ground_estimate(*[C.byref(args[k]) if isinstance(args[k], abi.WbcGroundCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device():
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    import re
    import __graft_entry__ as g
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    assert "wbc_sim_ground_estimate" in EXPORTED_SYMBOLS and hasattr(L, "wbc_sim_ground_estimate")
    assert "wbc_ground_kernel.hip" in g.SOURCES and "wbc_ground.h" in g.HEADERS
    # the mirror against the header's struct: the same fields in the same order, all floats
    header = open(g.ROOT + "/include/wbc_sim.h").read()
    body = re.search(r"typedef struct \{([^}]*)\} wbc_ground_cfg;", header).group(1)
    fields = [name.strip() for decl in re.findall(r"float ([^;]*);", body) for name in decl.split(",")]
    assert fields == list(gr.CFG_FIELDS) == [f for f, _ in abi.WbcGroundCfg._fields_]
    assert C.sizeof(abi.WbcGroundCfg) == 4 * len(fields) == 24
    assert [getattr(abi.WbcGroundCfg, f).offset for f in fields] == [0, 4, 8, 12, 16, 20]
    assert all(t is abi.f32 for _, t in abi.WbcGroundCfg._fields_)
    assert (abi.GROUND_NS, abi.GROUND_RESET, abi.GROUND_SERIES) == (gr.NS, 1, gr.SERIES)
    assert (abi.GROUND_INFO_RESET, abi.GROUND_INFO_FAILED, abi.GROUND_INFO_DEGENERATE, abi.GROUND_INFO_CLAMPED, abi.GROUND_INFO_LATCHED) == (
        gr.INFO_RESET, gr.INFO_FAILED, gr.INFO_DEGENERATE, gr.INFO_CLAMPED, gr.INFO_LATCHED)
    for name in ("NS", "RESET", "INFO_RESET", "INFO_FAILED", "INFO_DEGENERATE", "INFO_CLAMPED", "INFO_LATCHED"):
        assert int(re.search(r"#define WBC_GROUND_%s (\d+)" % name, header).group(1)) == getattr(abi, "GROUND_" + name), name
    assert float(re.search(r"#define WBC_GROUND_SERIES ([0-9.e-]+)f", header).group(1)) == abi.GROUND_SERIES
    assert len(L.wbc_sim_ground_estimate.argtypes) == len(_NAMES)
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    good = _cfg()
    base = dict(sim=None, cfg=_make_cfg(good), num_query=3, flags=0, stream=None, state=p,
                **{k: p + 512 * (1 + i) for i, k in enumerate(_INPUTS + _OUTS)})
    mk = lambda **kw: _make_cfg(good, **kw)                                          # noqa: E731
    nan, inf = float("nan"), float("inf")
    refusals = [(dict(cfg=None), b"NULL"), (dict(state=None), b"NULL"), (dict(contact=None), b"NULL"), (dict(flags=2), b"flag"), (dict(flags=-1), b"flag")]
    for field in ("dt", "tau_age", "lambda", "slope_max"):
        refusals += [(dict(cfg=mk(**{field: bad})), field.encode()) for bad in (0.0, -1.0, nan, inf)]
    refusals += [(dict(cfg=mk(c_on=bad)), b"c_on") for bad in (nan, inf, -inf)]
    refusals += [(dict(cfg=mk(tilt_gain=bad)), b"tilt_gain") for bad in (-0.01, 1.01, nan, inf)]
    refusals += [(dict(num_query=-1), b"num_query"), (dict(num_query=0), b"num_query"), (dict(num_query=-1, query_xy=None), b"num_query")]
    refusals += [({k: base[k] + off}, b"aligned") for k in _INPUTS + ("state",) + _OUTS for off in (1, 2, 3)]
    assert len(refusals) > 70
    accepted = [dict(), dict(flags=abi.GROUND_RESET), dict(query_xy=None, num_query=0), dict(query_xy=None, num_query=7),
                dict(cfg=mk(tilt_gain=0.0, c_on=-3.0)), dict(cfg=mk(tilt_gain=1.0)),
                {k: None for k in ("quat", "dof", "base_pos", "reset_mask", "query_xy") + _OUTS}]
    for kw, word in refusals + [(kw, b"sim is NULL") for kw in accepted]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_ground_estimate: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def _points_call(m, t=None, a_prev=None, **kw):
    """The fit alone on contact points m [N, 4, 3]."""
    m = np.asarray(m, dtype=np.float64)
    n = m.shape[0]
    return gr.fit(m, np.zeros((n, 4)) if t is None else t, np.zeros((n, 2)) if a_prev is None else a_prev, _cfg(**kw))


def test_an_exact_plane_is_returned_and_the_normal_is_orthogonal_to_it():
    """Four footholds on z = h + alpha x + beta y, a reset and lambda -> small: (alpha, beta) and `ground` to fp64 rounding; the normal is
    unit and orthogonal to both in-plane directions; theta_ref rotates world z onto n."""
    rng = np.random.default_rng(3)
    n = 64
    inp = _inputs(n, 0)
    cfg = _cfg(slope_max=10.0, tilt_gain=1.0, **{"lambda": 1e-30})
    p, R, _ = gr.foot_positions(_model(), inp["quat"], inp["dof"], inp["base_pos"])
    # the true plane through three of the feet; the fourth foot's joints are left alone, so the reset's fit is tested on points put on
    # the plane through fit() below and the kinematics through `ground` against the fit's own plane
    h, al, be = rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    xy = rng.uniform(-0.4, 0.4, (n, 4, 2)) + inp["base_pos"][:, None, 0:2]
    m = np.concatenate([xy, (h[:, None] + al[:, None] * xy[:, :, 0] + be[:, None] * xy[:, :, 1])[:, :, None]], axis=-1)
    F = _points_call(m, slope_max=10.0, **{"lambda": 1e-30})
    scale = 1.0 + np.abs(m[:, :, 2]).max(1)
    cond = np.linalg.cond(np.stack([np.stack([F["A00"], F["A10"]], -1), np.stack([F["A10"], F["A11"]], -1)], -2))
    assert F["ok"].all() and not F["clamped"].any()
    tol = 1e-13 * cond * scale                                                         # the heights' own rounding (2^-52 scale) through the solve
    assert (np.abs(F["a"][:, 0] - al) <= tol).all() and (np.abs(F["a"][:, 1] - be) <= tol).all()
    # the whole call after a reset: every foot is a foothold, `ground` is the fitted plane at the feet, and for a foot ON the plane its own height
    ref = _ref(cfg, dict(inp, state=np.zeros((n, gr.NS)), reset=True))
    a, st = ref["diag"]["a"], ref["state"]
    z = st[:, 22, None] + a[:, 0, None] * (p[:, :, 0] - st[:, 20, None]) + a[:, 1, None] * (p[:, :, 1] - st[:, 21, None])
    near = np.abs(inp["base_pos"][:, 0]) < 10
    assert np.abs(ref["ground"] - z)[near].max() < 1e-13 and np.abs(ref["ground"] - z).max() < 1e-10       # 900 m: the stored anchor's own rounding
    assert np.abs(ref["residual"] - (p[:, :, 2] - ref["ground"])).max() < 1e-12                  # every m_i = p_i
    nrm = ref["normal"][:, 0]
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-15 and (ref["normal"] == nrm[:, None, :]).all()
    tx = np.stack([np.ones(n), np.zeros(n), a[:, 0]], -1); ty = np.stack([np.zeros(n), np.ones(n), a[:, 1]], -1)
    assert np.abs((nrm * tx).sum(1)).max() < 1e-15 and np.abs((nrm * ty).sum(1)).max() < 1e-15 and (nrm[:, 2] > 0).all()
    # theta_ref (tilt_gain 1) is the rotation vector that takes world z onto n: Rodrigues on (0, 0, 1)
    th = ref["theta_ref"]
    ang = np.linalg.norm(th, axis=1)
    k = th / ang[:, None]
    ez = np.array([0.0, 0.0, 1.0])
    rot = ez * np.cos(ang)[:, None] + np.cross(k, ez) * np.sin(ang)[:, None] + k * (k @ ez)[:, None] * (1 - np.cos(ang))[:, None]
    assert np.abs(rot - nrm).max() < 1e-14 and (th[:, 2] == 0).all()
    # the trunk block: the clearance along the normal and the slopes in the heading frame
    zb = ref["trunk"][:, 0]
    assert np.abs(ref["trunk"][:, 1] - (inp["base_pos"][:, 2] - zb) * nrm[:, 2]).max() < 1e-15 and (ref["trunk"][:, 4:] == 0).all()
    hd = R[:, 0:2, 0] / np.linalg.norm(R[:, 0:2, 0], axis=1, keepdims=True)
    assert np.abs(ref["trunk"][:, 2] - (a * hd).sum(1)).max() < 1e-15
    assert np.abs(ref["trunk"][:, 2] ** 2 + ref["trunk"][:, 3] ** 2 - (a * a).sum(1)).max() < 1e-14


def test_tilt_series_meets_the_closed_form_and_a_flat_plane_is_exact():
    s = np.array([0.0, 1e-9, 0.5e-4, 0.999e-4, np.nextafter(gr.SERIES, 0), gr.SERIES, 1.001e-4, 2e-4, 1e-3])
    g = gr.tilt_factor(s)
    with np.errstate(all="ignore"):
        closed = np.where(s > 0, np.arctan(s) / np.where(s > 0, s, 1), 1.0)
    assert np.abs(g - closed).max() <= 2 ** -52 and g[0] == 1.0                       # s^4 / 5 <= 2e-17 below the switch
    assert np.abs(gr.tilt_factor(s.astype(np.float32), np.float32) - closed).max() <= 2 ** -23
    # a = 0: four footholds at one height
    n = 5
    m = np.random.default_rng(1).uniform(-1, 1, (n, 4, 3)); m[:, :, 2] = 0.3
    for dtype in (np.float64, np.float32):
        inp = _inputs(n, 0)
        st = np.zeros((n, gr.NS)); st[:, :20] = np.concatenate([m, np.zeros((n, 4, 2))], -1).reshape(n, 20)
        ref = _ref(_cfg(), dict(inp, state=st, contact=np.zeros((n, 4))), dtype=dtype)
        assert (ref["state"][:, 23:25] == 0).all() and (ref["theta_ref"] == 0).all() and (ref["trunk"][:, 2:] == 0).all()
        assert (ref["normal"] == np.array([0.0, 0.0, 1.0])).all() and (ref["residual"] == 0).all()
        assert np.array_equal(ref["ground"], np.full((n, 4), 0.3, dtype=dtype)) and (ref["info"] == 0).all()


def test_translation_moves_the_anchor_and_nothing_else():
    n = 40
    cfg, calls = _chain(n, 5)
    inp, ref = calls[1]
    shift = np.array([16.0, -32.0, 0.5])                                               # exact in fp64 on fp32 inputs
    moved = dict(inp, base_pos=inp["base_pos"] + shift, query_xy=inp["query_xy"] + shift[0:2])
    st = inp["state"].copy()
    for i in range(4):
        st[:, 5 * i:5 * i + 3] += shift
    got = _ref(cfg, dict(moved, state=st))
    assert np.abs(got["state"][:, 20:22] - ref["state"][:, 20:22] - shift[0:2]).max() < 1e-12
    assert np.abs(got["state"][:, 22] - ref["state"][:, 22] - shift[2]).max() < 1e-13
    tol = 1e-10                                                                        # the rounding of b + R fk at the two places, times the conditioning
    for k in ("normal", "residual", "theta_ref"):
        assert np.abs(got[k] - ref[k]).max() < tol, k
    assert np.abs(got["state"][:, 23:25] - ref["state"][:, 23:25]).max() < tol and np.array_equal(got["info"], ref["info"])
    assert np.abs(got["ground"] - ref["ground"] - shift[2]).max() < tol and np.abs(got["query_z"] - ref["query_z"] - shift[2]).max() < tol
    assert np.abs(got["trunk"][:, 0] - ref["trunk"][:, 0] - shift[2]).max() < tol and np.abs(got["trunk"][:, 1:] - ref["trunk"][:, 1:]).max() < tol


def test_collinear_and_coincident_footholds_keep_the_prior_slope():
    """lambda > 0 and exactly collinear footholds: the slope along the line tends to the line's own, the slope across it is a_prev's; four
    equal footholds return a_prev."""
    rng = np.random.default_rng(5)
    n = 32
    ang = rng.uniform(0, 2 * np.pi, n)
    u = np.stack([np.cos(ang), np.sin(ang)], -1); v = np.stack([-u[:, 1], u[:, 0]], -1)
    sline = rng.uniform(-0.3, 0.3, n)
    pos = np.array([-0.3, -0.1, 0.1, 0.3])
    m = np.zeros((n, 4, 3))
    m[:, :, 0:2] = rng.uniform(-5, 5, (n, 1, 2)) + pos[None, :, None] * u[:, None, :]
    m[:, :, 2] = 0.2 + sline[:, None] * pos[None, :]
    ap = rng.uniform(-0.3, 0.3, (n, 2))
    lam = float(np.float32(1e-3))                                                      # as the cfg hands it over
    F = _points_call(m, a_prev=ap, slope_max=10.0, **{"lambda": lam})
    assert F["ok"].all()
    across, along = (F["a"] * v).sum(1), (F["a"] * u).sum(1)
    assert np.abs(across - (ap * v).sum(1)).max() < 1e-12
    sig = (pos ** 2).sum()                                                            # sum w d^2 along the line, W = 4
    want = (sig * sline + 4 * lam * (ap * u).sum(1)) / (sig + 4 * lam)
    assert np.abs(along - want).max() < 1e-12
    same = np.repeat(rng.uniform(-3, 3, (n, 1, 3)), 4, axis=1)
    F = _points_call(same, a_prev=ap, slope_max=10.0, **{"lambda": lam})
    assert F["ok"].all() and np.abs(F["a"] - ap).max() < 1e-15


def test_repeated_calls_converge_at_the_rate_of_the_lambda_term():
    """Fixed footholds, nobody standing, equal ages: a_k - a_ls = M^k (a_0 - a_ls) with M = (S + lw I)^-1 lw, so in S's eigenbasis the
    error shrinks by lw / (sigma_j + lw) per call, towards the least-squares plane."""
    rng = np.random.default_rng(8)
    n = 16
    inp = _inputs(n, 0)
    cfg = _cfg(slope_max=10.0, **{"lambda": 0.02})
    m = np.concatenate([rng.uniform(-0.4, 0.4, (n, 4, 2)), rng.uniform(0.0, 0.2, (n, 4, 1))], -1)
    st = np.zeros((n, gr.NS)); st[:, :20] = np.concatenate([m, np.zeros((n, 4, 2))], -1).reshape(n, 20)
    st[:, 23:25] = rng.uniform(-0.5, 0.5, (n, 2))
    d = m - m.mean(1, keepdims=True)
    S = np.einsum("nfu,nfv->nuv", d[:, :, 0:2], d[:, :, 0:2])
    a_ls = np.linalg.solve(S, np.einsum("nfu,nf->nu", d[:, :, 0:2], d[:, :, 2])[:, :, None])[:, :, 0]
    M = np.linalg.solve(S + 4 * cfg["lambda"] * np.eye(2), 4 * cfg["lambda"] * np.eye(2)[None].repeat(n, 0))
    err0 = st[:, 23:25] - a_ls
    Mk = np.eye(2)[None].repeat(n, 0)
    for k in range(1, 13):
        ref = _ref(cfg, dict(inp, state=st, contact=np.zeros((n, 4))))
        st = ref["state"]
        Mk = Mk @ M
        assert np.abs((st[:, 23:25] - a_ls) - np.einsum("nuv,nv->nu", Mk, err0)).max() < 1e-12, k
    rate = np.linalg.eigvalsh(M).max(1)
    assert (np.linalg.norm(st[:, 23:25] - a_ls, axis=1) <= rate ** 12 * np.linalg.norm(err0, axis=1) * (1 + 1e-9) + 1e-13).all() and (rate < 1).all()


def test_a_foot_that_never_stands_again_loses_weight_exponentially():
    n = 4
    inp = _inputs(n, 0)
    cfg = _cfg()
    contact = np.ones((n, 4)); contact[:, 2] = 0.0
    st = _ref(cfg, dict(inp, state=np.zeros((n, gr.NS)), reset=True, contact=np.ones((n, 4))))["state"]
    for k in range(1, 40):
        ref = _ref(cfg, dict(inp, state=st, contact=contact))
        st = ref["state"]
        w = ref["diag"]["w"]
        assert np.abs(st[:, 13] - k * cfg["dt"]).max() < 1e-12 and (st[:, [3, 8, 18]] == 0).all()
        assert np.abs(w[:, 2] - np.exp(-k * cfg["dt"] / cfg["tau_age"])).max() < 1e-13 and (w[:, [0, 1, 3]] == 1).all()
        assert ((ref["info"] & ~gr.INFO_CLAMPED) == (gr.INFO_LATCHED * (1 + 2 + 8))).all()
    # ages that would underflow exp(-t / tau) one by one: the weights are relative to the youngest foot, W >= 1
    st[:, [3, 8, 13, 18]] = np.array([4000.0, 4000.3, 4000.6, 5000.0])
    ref = _ref(cfg, dict(inp, state=st, contact=np.zeros((n, 4))))
    assert ((ref["info"] & ~gr.INFO_CLAMPED) == 0).all() and np.isfinite(ref["state"]).all() and (ref["diag"]["W"] >= 1).all()
    assert np.abs(ref["diag"]["w"][:, 1] - np.exp(-0.3 / cfg["tau_age"])).max() < 1e-9


def test_a_scripted_trot_up_a_ramp_finds_the_slope_within_a_gait_period():
    """A trot on a 0.2 ramp (z = 0.2 x + r, feet placed on it by the script; the trunk 0.3 m above it moves at 0.5 m/s): the footholds
    are handed over through the state's own mechanism -- a standing foot's joints put it on the ramp, a swinging foot is lifted. After one
    gait period the slope is within 10 % of the truth, and `ground` under the swinging feet is off the true surface by no more than the
    fit's own residual plus the height error of the feet that were put down (1 mm)."""
    m = _model()
    slope, period, dt = 0.2, 0.4, 0.02
    cfg = _cfg(dt=dt, slope_max=1.0)
    n = 2
    rng = np.random.default_rng(12)
    legs = er.legs(m)
    q_prev = None
    _, _, _, dofs = er.leg_kinematics(m, np.zeros((1, 20)), None, jac=True)
    hips = np.array([chain[0][2] for chain, _ in legs])                               # the hip joints' offsets in the trunk,
    hips[:, 1] += 0.08 * np.sign(hips[:, 1])                                          # and the feet a thigh's offset further out

    def solve_leg(f, target, q0):
        """Newton on the leg's three joints so that fk_f(q) = target (trunk axes)."""
        q = q0.copy()
        for _ in range(30):
            full = np.zeros((1, 20)); full[0, dofs[f]] = q
            fk, _, J, _ = er.leg_kinematics(m, full, None, jac=True)
            err = target - fk[0, f]
            if np.abs(err).max() < 1e-13:
                break
            q = q + np.linalg.solve(J[0, f], err)
        assert np.abs(err).max() < 1e-10
        return q

    stand_q = np.array([0.0, 0.8, -1.5])
    state = np.zeros((n, gr.NS))
    quat = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n, 1))
    steps = int(round(1.5 * period / dt))
    foothold = None
    for k in range(steps + 1):
        tnow = k * dt
        b = np.stack([0.5 * tnow + np.arange(n) * 1.0, 0.1 * np.arange(n), np.zeros(n)], -1)
        b[:, 2] = 0.3 + slope * b[:, 0]
        phase = (tnow / period) % 1.0
        standing = np.array([phase < 0.5, phase >= 0.5, phase >= 0.5, phase < 0.5])    # FL + RR, then FR + RL
        if foothold is None:
            foothold = b[:, None, :] + hips[None] + np.array([0.0, 0.0, 0.0])
            foothold[:, :, 2] = slope * foothold[:, :, 0] + rng.uniform(-1e-3, 1e-3, (n, 4))
        q = np.zeros((n, 20))
        target = np.zeros((n, 4, 3))
        for f in range(4):
            if standing[f]:
                target[:, f] = foothold[:, f]
            else:                                                                    # swing: above a point ahead of the hip; it lands there
                nxt = b + hips[f] + np.array([0.1, 0.0, 0.0])
                nxt[:, 2] = slope * nxt[:, 0] + rng.uniform(-1e-3, 1e-3, n)
                foothold[:, f] = nxt
                target[:, f] = nxt + np.array([0.0, 0.0, 0.05])
            for e in range(n):
                q[e, dofs[f]] = solve_leg(f, target[e, f] - b[e], stand_q if k == 0 else q_prev[e, dofs[f]])
        q_prev = q
        dof = np.stack([q, np.zeros_like(q)], -1)
        ref = gr.estimate(m, cfg, state, quat, dof, b, standing[None].repeat(n, 0).astype(float), reset=True if k == 0 else None)
        state = ref["state"]
        if tnow >= period:
            a = ref["diag"]["a"]
            print(f"ramp t = {tnow:.2f} s: a1 / truth {a[:, 0] / slope}, |a2| {np.abs(a[:, 1])}, largest |residual| {np.abs(ref['residual']).max():.2e}")
            assert (np.abs(a[:, 0] / slope - 1) <= 0.1).all() and (np.abs(a[:, 1]) <= 0.1 * slope).all()
            sw = ~standing
            true_z = slope * target[:, :, 0]
            off = np.abs(ref["ground"] - true_z)[:, sw]
            bound = np.abs(ref["residual"]).max(1, keepdims=True) * 2 + 2e-3
            assert (off <= bound).all(), (off, bound)


def test_clamped_and_degenerate_bits_appear_where_they_should():
    rng = np.random.default_rng(21)
    n = 200
    xy = rng.uniform(-0.4, 0.4, (n, 4, 2))
    al, be = rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n)
    m = np.concatenate([xy, (al[:, None] * xy[:, :, 0] + be[:, None] * xy[:, :, 1])[:, :, None]], -1)
    F = _points_call(m, slope_max=0.45, **{"lambda": 1e-9})
    true = np.hypot(al, be)
    edge = np.abs(true - 0.45) < 1e-3
    assert np.array_equal(F["clamped"][~edge], (true > 0.45)[~edge]) and F["clamped"].any() and (~F["clamped"]).any()
    got = np.hypot(F["a"][:, 0], F["a"][:, 1])
    assert np.abs(got[F["clamped"]] - np.float32(0.45)).max() < 1e-15 and np.array_equal(F["a"][~F["clamped"]], F["a_fit"][~F["clamped"]])
    cl = F["clamped"]
    assert np.abs(F["a"][cl, 0] * F["a_fit"][cl, 1] - F["a"][cl, 1] * F["a_fit"][cl, 0]).max() < 1e-15     # the direction is kept
    # DEGENERATE: a failed pivot alone -- footholds so far apart that the sums overflow; collinear, coincident and far-away ones are not
    inp = _inputs(6, 0)
    st = np.zeros((6, gr.NS))
    pts = rng.uniform(-0.3, 0.3, (6, 4, 3))
    pts[1] *= 1e200; pts[2, :, 0:2] = pts[2, :1, 0:2] + np.arange(4)[:, None] * np.array([0.1, 0.05]); pts[3] = pts[3, :1]; pts[4, :, 0:2] += 1e6
    st[:, :20] = np.concatenate([pts, np.zeros((6, 4, 2))], -1).reshape(6, 20)
    st[:, 23:25] = [0.1, -0.2]
    ref = _ref(_cfg(slope_max=100.0), dict(inp, state=st, contact=np.zeros((6, 4))))
    assert ref["info"].tolist() == [0, gr.INFO_DEGENERATE, 0, 0, 0, 0]
    assert np.array_equal(ref["state"][1, 23:25], st[1, 23:25]) and np.isfinite(ref["state"][1, 20:23]).all()
    with np.errstate(all="ignore"):
        ref32 = _ref(_cfg(slope_max=100.0), dict(inp, state=np.where(np.abs(st) > 1e30, np.sign(st) * 1e25, st), contact=np.zeros((6, 4))), dtype=np.float32)
    assert ref32["info"].tolist() == [0, gr.INFO_DEGENERATE, 0, 0, 0, 0]


def _spoil(inp, rows):
    """One non-finite value that is read in each of the first len(rows) - 3 rows, and three that are never read in the last three."""
    bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in inp.items()}
    _, _, dofs = gr.foot_positions(_model(), inp["quat"], inp["dof"], inp["base_pos"])
    r = rows
    bad["base_pos"][r[0], 1] = np.nan; bad["quat"][r[1], 3] = np.inf; bad["dof"][r[2], dofs[1, 2], 0] = np.nan; bad["contact"][r[3], 2] = np.nan
    bad["state"][r[4], 5 * 2 + 1] = np.nan; bad["state"][r[5], 5 * 1 + 3] = np.inf; bad["state"][r[6], 23] = np.nan; bad["state"][r[7], 24] = -np.inf
    bad["query_xy"][r[8], 3, 1] = np.nan
    bad["dof"][r[9], dofs[0, 0], 1] = np.nan; bad["state"][r[10], 4] = np.nan; bad["state"][r[11], 21] = np.inf   # a velocity, a reserved float, the anchor
    return bad


def test_non_finite_inputs_fail_the_env_alone():
    n = 14
    cfg, calls = _chain(17, 5)
    inp = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in calls[1][0].items()}
    good = _ref(cfg, inp)
    bad = _spoil(inp, list(range(12)))
    o = _ref(cfg, bad)
    assert o["info"][:9].tolist() == [gr.INFO_FAILED] * 9 and np.array_equal(o["info"][9:], good["info"][9:])
    for k in _OUTS[:-1]:
        assert (o[k][:9] == 0).all() and np.array_equal(o[k][9:], good[k][9:]), k
    assert np.array_equal(o["state"][:9], bad["state"][:9], equal_nan=True) and np.array_equal(o["state"][9:], good["state"][9:])
    # a reset env does not read its state
    o = _ref(cfg, dict(bad, reset=np.array([0] * 4 + [1] * 4 + [0] * 6)))
    assert (o["info"][4:8] & gr.INFO_FAILED == 0).all() and (o["info"][4:8] & gr.INFO_RESET != 0).all() and np.isfinite(o["state"][4:8]).all()


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output over every judged call, the thin env-cases and what the cases hold, the fp32 reference's info held to fp64 on the way."""
    worst = {k: 0.0 for k in gr.OUTPUTS}
    thin = [0, 0]
    seen = dict(clamped=0, unclamped=0, latched=0, far_stored=0, collinear=0, reset=0)
    for n in SIZES:
        for combo in range(len(COMBOS)):
            cfg, calls = _chain(n, combo)
            for j, (inp, ref) in enumerate(calls):
                r32 = _ref(cfg, inp, dtype=np.float32)
                ok = judge(cfg, ref)
                assert np.array_equal(r32["info"][ok], ref["info"][ok]), (n, combo, j)
                r = gr.ratios(r32, ref, ok)
                worst = {k: max(worst[k], r[k]) for k in worst}
                thin[0] += int((~ok).sum()); thin[1] += ok.size
                assert not ref["diag"]["failed"].any() and ref["diag"]["fit"]["ok"].all()
                seen["clamped"] += int(ref["diag"]["fit"]["clamped"].sum()); seen["unclamped"] += int((~ref["diag"]["fit"]["clamped"]).sum())
                seen["latched"] += int(ref["diag"]["stand"].sum()); seen["reset"] += int((ref["info"] & gr.INFO_RESET != 0).sum())
                if j == 1:
                    fresh = ref["diag"]["stand"].any(1)
                    seen["far_stored"] += int((~fresh[::10]).sum())
                    d = ref["diag"]["fit"]["d"][::7, :, 0:2]
                    sv = np.linalg.svd(d, compute_uv=False)
                    assert (sv[:, 1] < 4e-3).all()                                       # within 1 mm of a line each
                    seen["collinear"] += d.shape[0]
    return worst, thin, seen


def test_fp32_yardstick_is_where_the_constants_came_from():
    worst, _, _ = _yardsticks()
    print("ground yardsticks: " + ", ".join(f"{k} K_ref = {worst[k]:.3g} (C = {CONST[k]:g})" for k in worst))
    for k in K_REF:
        assert abs(worst[k] - K_REF[k]) <= 0.25 * K_REF[k], (k, worst[k])
        assert 4 * worst[k] <= CONST[k]


def test_thin_cases_stay_under_the_cap():
    _, thin, seen = _yardsticks()
    print(f"ground thin env-cases: {thin[0]} of {thin[1]}; what the judged cases hold: {seen}")
    assert thin[0] <= THIN_CAP * thin[1], thin
    assert all(v > 0 for v in seen.values()), seen                                     # and the cases are not vacuous


@functools.lru_cache(maxsize=None)
def _kernel_assembly():
    """csrc/wbc_ground_kernel.hip compiled to gfx950 assembly with the build's own flags."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    source = "wbc_ground_kernel.hip"
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ground.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        return open(out).read()


def test_ground_kernel_codegen():
    """One kernel, no scratch, no LDS, a single wavefront per workgroup and no s_barrier, at most 128 VGPRs."""
    import re
    text = _kernel_assembly()
    assert text.count(".amdhsa_kernel ") == 1
    entry = text[text.index("amdhsa.kernels:"):]
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))          # noqa: E731
    assert re.search(r"\.name:\s+wbc_ground_estimate_kernel\n", entry)
    print(f"wbc_ground_estimate_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64
    assert meta("group_segment_fixed_size") == 0 and meta("vgpr_count") <= 128
    body = text[text.index("\nwbc_ground_estimate_kernel:"):]
    body = body[:body.index(".Lfunc_end")]
    assert "s_endpgm" in body and "scratch_" not in body and "s_barrier" not in body and "ds_read" not in body and "ds_write" not in body


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _env(n, seed=5):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    return WidowGo1(cfg, sim_device="cuda:0", seed=seed)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


def _shapes(nq):
    f, i = torch.float32, torch.int32
    return {"state": ((gr.NS,), f), "normal": ((4, 3), f), "ground": ((4,), f), "residual": ((4,), f), "trunk": ((6,), f), "theta_ref": ((3,), f),
            "query_z": ((nq,), f), "info": ((), i)}


def _sent(dtype):
    return {torch.float32: SENTINEL, torch.int32: ISENTINEL}[dtype]


def _load_sim(env, inp):
    """The sim's own root and joint state from the inputs."""
    root = env.sim.tensor("ROOT_STATES").clone()
    root[:, 0, 0:3] = _dev(inp["base_pos"]); root[:, 0, 3:7] = _dev(inp["quat"])
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(_dev(inp["dof"]))
    torch.cuda.synchronize()


PAD = 8


def _call(env, cfg, inp, which=_OUTS, null=()):
    """A direct C-ABI call into buffers with a sentinel frame on both sides (the state starts from inp's); returns {name: [n, ...] tensor}
    of the state and the outputs asked for. The inputs named in `null`, and those missing from inp, are handed over as NULL."""
    n = env.num_envs
    q = inp.get("query_xy")
    nq = 0 if q is None else q.shape[1]
    shapes = _shapes(nq)
    size = {k: int(np.prod(s, dtype=np.int64)) for k, (s, _) in shapes.items()}
    bufs = {}
    for name in ("state",) + tuple(which):
        dt = shapes[name][1]
        bufs[name] = torch.full((PAD + n * size[name] + PAD,), _sent(dt), dtype=dt, device="cuda")
    bufs["state"][PAD:PAD + n * gr.NS] = _dev(inp["state"]).reshape(-1)
    reset = inp.get("reset")
    flags = abi.GROUND_RESET if reset is True else 0
    tens = {k: _dev(inp.get(k)) for k in ("quat", "dof", "base_pos", "contact", "query_xy") if k not in null}
    tens["reset_mask"] = _dev(reset, torch.int32) if reset is not None and reset is not True else None
    ptr = lambda k: tens[k].data_ptr() if tens.get(k) is not None and tens[k].numel() > 0 else None     # noqa: E731
    out = lambda k: bufs[k].data_ptr() + PAD * 4 if k in bufs else None              # noqa: E731  (query_z with Q = 0: a pointer between two frames)
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_ground_estimate(env.sim.h, C.byref(c), ptr("quat"), ptr("dof"), ptr("base_pos"), ptr("contact"), ptr("reset_mask"),
                                           ptr("query_xy"), nq, flags, out("state"), *[out(k) for k in _OUTS], None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        s = _sent(shapes[name][1])
        assert bool((b[:PAD] == s).all()) and bool((b[PAD + n * size[name]:] == s).all()), name
    return {name: b[PAD:PAD + n * size[name]].view((n,) + shapes[name][0]).clone() for name, b in bufs.items()}


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_entry_against_fp64(n):
    env = _env(n)
    worst = {k: 0.0 for k in gr.OUTPUTS}
    for combo in range(len(COMBOS)):
        cfg, calls = _chain(n, combo)
        for j, (inp, ref) in enumerate(calls):
            null = COMBOS[combo][0]
            if null:
                _load_sim(env, inp)
            got = _np(_call(env, cfg, inp, null=null))
            assert all(np.isfinite(got[k].astype(np.float64)).all() for k in got)
            r, _, _ = compare(got, ref, cfg, who=(n, COMBOS[combo], j))
            worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"ground n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")


@pytest.mark.gpu
def test_outputs_one_at_a_time_two_runs_a_graph_and_the_sim_untouched():
    n, combo = 130, 5
    env = _env(n)
    cfg, calls = _chain(n, combo)
    inp = calls[1][0]
    _load_sim(env, inp)
    before = {name: env.sim.tensor(name).clone() for name in abi.TENSOR_IDS}
    want = _call(env, cfg, inp)
    again = _call(env, cfg, inp)
    assert all(torch.equal(want[k], again[k]) for k in want)                           # two runs: the same bits
    for name in _OUTS:
        got = _call(env, cfg, inp, which=(name,))
        assert torch.equal(got[name], want[name]) and torch.equal(got["state"], want["state"]), name
    got = _call(env, cfg, inp, which=())
    assert torch.equal(got["state"], want["state"])
    # Q = 0: query_z is handed over and nothing is written to it (the frames are checked in _call)
    got = _call(env, cfg, dict(inp, query_xy=None))
    assert all(torch.equal(got[k], want[k]) for k in want if k != "query_z") and got["query_z"].numel() == 0
    # a captured graph replays the eager bits
    c = _make_cfg(cfg)
    t = {k: _dev(inp[k]) for k in ("quat", "dof", "base_pos", "contact", "query_xy")}
    state0 = _dev(inp["state"])
    state = state0.clone()
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _shapes(inp["query_xy"].shape[1]).items() if k != "state"}
    call = lambda: env.sim.ground_estimate(c, state, **t, **outs)                      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                     # warm-up off the default stream
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    state.copy_(state0)
    with torch.cuda.graph(graph):
        call()
    state.copy_(state0)
    for o in outs.values():
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(state, want["state"]) and all(torch.equal(outs[k], want[k]) for k in outs)
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8)                       # noqa: E731
    for name, t0 in before.items():
        assert torch.equal(raw(env.sim.tensor(name)), raw(t0)), name


@pytest.mark.gpu
def test_null_inputs_give_the_bits_of_the_call_on_copies():
    n, combo = 130, 5
    env = _env(n)
    cfg, calls = _chain(n, combo)
    for j in (0, 3):
        inp, ref = calls[j]
        _load_sim(env, inp)
        want = _call(env, cfg, inp)
        for null in (("quat",), ("dof",), ("base_pos",), ("quat", "dof", "base_pos")):
            got = _call(env, cfg, inp, null=null)
            assert all(torch.equal(got[k], want[k]) for k in want), (j, null)
        compare(_np(got), ref, cfg, who="NULL inputs")


@pytest.mark.gpu
def test_failed_envs_write_zeros_and_keep_their_state():
    n, combo = 130, 5
    env = _env(n)
    cfg, calls = _chain(n, combo)
    inp, _ = calls[1]
    rows = [0, 1, 15, 16, 63, 64, 65, 100, 129, 2, 17, 66]
    bad = _spoil(inp, rows)
    ref = _ref(cfg, bad)
    rows = rows[:9]
    assert ref["info"][rows].tolist() == [gr.INFO_FAILED] * len(rows) and int((ref["info"] == gr.INFO_FAILED).sum()) == len(rows)
    got = _call(env, cfg, bad)
    plain = _call(env, cfg, inp)
    ok = torch.tensor(np.delete(np.arange(n), rows), device="cuda")
    for k in got:                                              # their neighbours, 2, 17 and 66 included: the bits of the launch without them
        assert torch.equal(got[k][ok], plain[k][ok]), k
    g = _np(got)
    assert g["info"][rows].tolist() == [gr.INFO_FAILED] * len(rows)
    for k in _OUTS[:-1]:
        assert (g[k][rows] == 0).all(), k
    assert np.array_equal(g["state"][rows], bad["state"][rows].astype(np.float32), equal_nan=True)


@pytest.mark.gpu
def test_drift_over_200_chained_calls():
    """200 calls, each from the kernel's own state: a walking trunk, contacts that come and go. Per output the kernel's largest ratio
    against the fp64 chain stays within 4 x that of the fp32 reference chained on its own state (at least 1: one rounding of the entry)."""
    n, steps = 17, 200
    env = _env(n)
    cfg = _cfg()
    base = _inputs(n, 5)
    rng = np.random.default_rng(4)
    s64 = s32 = np.zeros((n, gr.NS))
    sk = None
    k32 = {k: 0.0 for k in gr.OUTPUTS}
    kk = dict(k32)
    for j in range(steps):
        inp = dict(base)
        inp["base_pos"] = F32(base["base_pos"] + np.array([0.01 * j, 0.004 * j, 0.02 * np.sin(0.3 * j)]))
        dof = base["dof"].copy(); dof[:, :, 0] += 0.15 * np.sin(0.2 * j + np.arange(20))
        inp["dof"] = F32(dof)
        inp["contact"] = F32((rng.random((n, 4)) < 0.5).astype(float))
        inp["query_xy"] = F32(inp["base_pos"][:, None, 0:2] + base["query_xy"] - base["base_pos"][:, None, 0:2])
        if j == 0:
            inp["reset"] = True
        ref = _ref(cfg, dict(inp, state=s64))
        r32 = _ref(cfg, dict(inp, state=s32), dtype=np.float32)
        got = _np(_call(env, cfg, dict(inp, state=np.zeros((n, gr.NS)) if sk is None else sk)))
        assert np.array_equal(got["info"], ref["info"]) and np.array_equal(r32["info"], ref["info"]), j
        a, bq = gr.ratios(r32, ref), gr.ratios(got, ref)
        k32 = {k: max(k32[k], a[k]) for k in k32}; kk = {k: max(kk[k], bq[k]) for k in kk}
        s64, s32, sk = ref["state"], r32["state"].astype(np.float64), got["state"].astype(np.float64)
    print(f"ground drift over {steps} calls: fp32 reference {k32}, kernel {kk}")
    for k in gr.OUTPUTS:
        assert kk[k] <= 4 * max(k32[k], 1.0), (k, kk[k], k32[k])


@pytest.mark.gpu
def test_estimator_on_the_simulator_feeds_the_filter_and_the_detector():
    """8 envs on the plane: 40 control steps of standing under a joint PD with get_foot_contacts() as contact. The kernel is held, call by
    call on the logged inputs and from its own previous state, to the fp64 reference within 4 x the fp32 reference's own largest ratio on
    those inputs (rounded up to a power of two). On the flat plane every foot origin rests its radius above z = 0 less the contact's
    penetration, so `ground` is within 5 mm + the largest |residual| of abi.FOOT_RADIUS and the normal within (5 mm + the largest
    |residual|) / 0.1 m of world z (0.1 m: below half the smallest distance between two feet). gnd.ground feeds BaseStateEstimator.update
    and ContactDetector.update to finite outputs and defined status words."""
    from wbc_amd.envs import GroundEstimator
    n = 8
    env = _env(n, seed=9)
    env.reset()
    env.reset_buf.zero_()
    est, det, gnd = env.base_state_estimator(), env.contact_detector(), env.ground_estimator()
    assert isinstance(gnd, GroundEstimator) and gnd.plane.data_ptr() == gnd.state.data_ptr() + 4 * 20
    cfg = {k: float(getattr(gnd.cfg, k)) for k in gr.CFG_FIELDS}
    q0 = env.default_dof_pos.to(torch.float32).reshape(1, -1).expand(n, -1).clone()
    decimation = int(env.cfg.control.decimation)
    logs = []
    for step in range(40):
        ds = env.sim.tensor("DOF_STATE")
        tau = (40.0 * (q0 - ds[:, :, 0]) - 1.0 * ds[:, :, 1]).clamp(-30.0, 30.0).contiguous()
        env.sim.set_dof_forces(tau)
        for _ in range(decimation):
            env.sim.simulate()
        contact = env.get_foot_contacts().to(torch.float32)
        root = env.sim.tensor("ROOT_STATES")
        query = (root[:, 0, None, 0:2] + torch.tensor([[0.2, 0.1], [-0.2, -0.1]], device=root.device)).contiguous()
        before = gnd.state.clone()
        gnd.update(contact, query_xy=query)
        est.update(foot_height=gnd.ground)
        det.update(torques=tau, ground=gnd.ground, normal=gnd.normal)
        torch.cuda.synchronize()
        logs.append(dict(state=before.cpu().numpy().astype(np.float64), quat=root[:, 0, 3:7].cpu().numpy().astype(np.float64),
                         base_pos=root[:, 0, 0:3].cpu().numpy().astype(np.float64), dof=env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64),
                         contact=contact.cpu().numpy().astype(np.float64), query_xy=query.cpu().numpy().astype(np.float64),
                         reset=gnd.last_inputs["reset_mask"].cpu().numpy(),
                         got=_np(dict(state=gnd.state, normal=gnd.normal, ground=gnd.ground, residual=gnd.residual, trunk=gnd.trunk,
                                      theta_ref=gnd.theta_ref, query_z=gnd.query_z, info=gnd.info))))
        for name in ("state", "normal", "ground", "residual", "trunk", "theta_ref", "query_z"):
            assert bool(torch.isfinite(getattr(gnd, name)).all()), (step, name)
        assert bool(torch.isfinite(est.x).all()) and bool(torch.isfinite(det.prob).all()) and bool(torch.isfinite(det.terms).all())
        known = gr.INFO_RESET | gr.INFO_DEGENERATE | gr.INFO_CLAMPED | 15 * gr.INFO_LATCHED
        assert bool(((gnd.info & ~known) == 0).all())
        assert set(est.status.cpu().tolist()) <= {abi.ESTIMATOR_STATUS_OK, abi.ESTIMATOR_STATUS_RESET, abi.ESTIMATOR_STATUS_FAILED}
        assert bool((det.info & abi.CONTACT_INFO_FAILED == 0).all()) and set(det.contact.cpu().unique().tolist()) <= {0, 1}
    k_sim = {k: 0.0 for k in gr.OUTPUTS}
    refs = []
    for lg in logs:
        ref = _ref(cfg, lg)
        r32 = _ref(cfg, lg, dtype=np.float32)
        r = gr.ratios(r32, ref, judge(cfg, ref))
        k_sim = {k: max(k_sim[k], r[k]) for k in k_sim}
        refs.append(ref)
    const = {k: _pow2(max(v, 0.25)) for k, v in k_sim.items()}
    worst = {k: 0.0 for k in gr.OUTPUTS}
    for step, (lg, ref) in enumerate(zip(logs, refs)):
        r, _, _ = compare(lg["got"], ref, cfg, const=const, who=("sim", step))
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"ground on the simulator: K_ref {k_sim}, C {const}, kernel's largest ratios {worst}")
    last = logs[-1]["got"]
    res = float(np.abs(last["residual"]).max())
    off = float(np.abs(last["ground"] - abi.FOOT_RADIUS).max())
    tilt = float(np.arccos(np.clip(last["normal"][:, 0, 2], -1, 1)).max())
    print(f"ground on the simulator: |ground - FOOT_RADIUS| <= {off * 1e3:.3f} mm, largest |residual| {res * 1e3:.3f} mm, normal within {tilt:.2e} rad "
          f"of z, standing feet {logs[-1]['contact'].mean():.2f}")
    assert off <= 5e-3 + res and tilt <= (5e-3 + res) / 0.1
    # a partial reset leaves the others as they are
    keep_state = gnd.state.clone()
    gnd.reset(env_ids=[1, 5])
    torch.cuda.synchronize()
    rest = [0, 2, 3, 4, 6, 7]
    assert torch.equal(gnd.state[rest], keep_state[rest]) and bool((gnd.info[[1, 5]] & gr.INFO_RESET != 0).all())
    assert bool((gnd.state[[1, 5]][:, [3, 8, 13, 18]] == 0).all())                     # every contact point at its foot, age 0
