"""Gait clock, terrain-aware footholds and swing-foot references (wbc_sim_footstep_plan: wbc_footstep_plan_kernel in
csrc/wbc_footstep_kernel.hip; the text both implement is the comment in include/wbc_sim.h). The CPU tests pin the fp64 restatement of
tests/footstep_reference.py to properties of the equations and measure the fp32 yardstick; the GPU tests hold the kernel to the reference
entry by entry.

Bound: every entry of a continuous output satisfies |kernel - ref| <= C 2^-24 mag, mag as footstep_reference's docstring lists it. C is
4 x K_ref rounded up to a power of two, K_ref the largest ratio of the reference run in fp32 against itself in fp64 over the judged cases
(every call of every chain: SIZES x TERRAINS x COMBOS x NCALLS), measured on the CPU and asserted there; it never comes from the kernel.

    output      K_ref     kernel's largest ratio on an MI355X     C
    swing_ref   658       658   (n = 130, 24x24)                  4096
    swing_acc   73.6      71.9  (n = 130, 24x24)                  512
    foothold    14.7      15.4  (n = 130, 24x24)                  64
    foot_pos    13.8      13.8  (n = 130, 24x24)                  64
    state       13.8      13.8  (n = 130, 24x24)                  64

swing_ref's K_ref is large because its magnitude is the position scale alone: near a swing's ends b'' changes by 60 per unit of s, s carries
the phase's rounding divided by 1 - duty (five times it at duty 0.8), and the vertical acceleration multiplies that by (2 / T_sw)^2; the
kernel's largest ratio there is the fp32 reference's own to every printed digit. Thin foot-cases: 231, 232 and 384 of 21 440 on the plane,
the 2 x 2 and the 24 x 24 field (the cap is 5 %). 200 calls on the kernel's own state: the fp32 reference drifts 1.52e-6 from fp64 in
phase, the bound is 7.63e-6, the kernel drifts 1.52e-6; 36 of 10 452 foot-calls are thin.

Discrete outputs (stance, contact, schedule, the chosen candidate read back from foothold, info) match exactly except in THIN cases, judged
from the fp64 reference alone (judge()): a foot's or a stage's phase within PHASE_BOUND of duty, 0 (or 1) or, through s, of latch; the two
lowest costs of a search closer than the cost bound; a candidate's rough or n_z within its bound of its threshold; a query point within
the position bound of a grid line or of its cell's diagonal. A thin foot is left out of the foot's discrete and continuous outputs.
PHASE_BOUND: phase + offset and (phase + (k + 1/2) c) + offset are at most four fp32 roundings (the quotient c, the product, two sums) of
numbers below 4, each at most 2^-24 of 4 / 2: 8 x 2^-24 covers them; the n_z bound of 16 x 2^-24 covers the six roundings from the int16
samples to 1 / sqrt(.)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import estimator_reference as er
import footstep_reference as fr
from wbc_amd import abi
from wbc_amd.abi import WbcFootstepCfg  # noqa: F401  (this file is about wbc_sim_footstep_plan: none of it means anything without the call)

SENTINEL, ISENTINEL, USENTINEL = 12345.0, -7777, 201
EPS = 2.0 ** -24
F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)                  # noqa: E731
GRAVITY = (0.0, 0.0, float(np.float32(-9.81)))
GROUND_Z = 0.0
SIZES = (1, 3, 130)
TERRAINS = ("plane", "2x2", "24x24")
# (gait, duty, H, R): every H, R and gait of the issue, each with several of the others
COMBOS = (("stand", 1.0, 0, 0), ("trot", 0.5, 10, 1), ("walk", 0.75, 16, 3), ("trot", 0.6, 1, 3), ("walk", 0.75, 2, 1), ("trot", 0.5, 16, 0),
          ("stand", 1.0, 10, 3), ("trot", 0.4, 2, 3), ("walk", 0.8, 1, 0), ("trot", 0.5, 0, 1))
NCALLS = 4
# phases that put a trot's feet just after lift-off, mid-swing, past the latch and just before touchdown, and exactly 0
SPECIAL_PHASES = (0.0, 0.01, 0.25, 0.45, 0.495, 0.51, 0.75, 0.95, 0.995)

# K_ref (measured by test_fp32_yardstick_is_where_the_constants_came_from), the kernel's largest ratio on the MI355X (for the record: no
# bound comes from it) and the constant
K_REF = {"swing_ref": 658.0, "swing_acc": 73.6, "foothold": 14.7, "foot_pos": 13.8, "state": 13.8}
K_GPU = {"swing_ref": 658.0, "swing_acc": 71.9, "foothold": 15.4, "foot_pos": 13.8, "state": 13.8}
_pow2 = lambda k: float(2.0 ** np.ceil(np.log2(4 * k)))                             # noqa: E731
CONST = {k: _pow2(v) for k, v in K_REF.items()}
PHASE_BOUND = 8 * EPS * 4
NZ_BOUND = 16 * EPS
COST_CONST = 64.0            # cost = three products and two sums of terms that a position error of C_foothold 2^-24 moves by less than itself


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _cfg(**kw):
    """The kernel receives the cfg as floats: the references use the same rounded values."""
    base = dict(dt=0.02, period=0.5, duty=0.5, offset=fr.GAITS["trot"], horizon=10, mpc_dt=0.03,
                stance_offset=((0.19, 0.13), (0.19, -0.13), (-0.19, 0.13), (-0.19, -0.13)), k_v=0.03, com_height=0.3, max_reach=0.25,
                swing_height=0.08, latch=0.8, kp=400.0, kd=40.0, search_radius=1, search_step=0.04, probe_radius=0.03, w_dist=1.0, w_rough=10.0,
                w_slope=0.1, rough_max=0.03, nz_min=0.85)
    base.update(kw)
    out = {}
    for k in fr.CFG_FIELDS:
        v = base[k]
        out[k] = int(v) if k in ("horizon", "search_radius") else (F32(v).tolist() if k in ("offset", "stance_offset") else float(np.float32(v)))
    return out


def _combo_cfg(combo, **kw):
    gait, duty, H, R = COMBOS[combo]
    return _cfg(offset=fr.GAITS[gait], duty=duty, horizon=H, search_radius=R, **kw)


def _make_cfg(cfg, **kw):
    c = dict(cfg, **kw)
    return abi.WbcFootstepCfg(c["dt"], c["period"], c["duty"], (abi.f32 * 4)(*c["offset"]), c["horizon"], c["mpc_dt"],
                              ((abi.f32 * 2) * 4)(*[(abi.f32 * 2)(*r) for r in c["stance_offset"]]), c["k_v"], c["com_height"], c["max_reach"],
                              c["swing_height"], c["latch"], c["kp"], c["kd"], c["search_radius"], c["search_step"], c["probe_radius"],
                              c["w_dist"], c["w_rough"], c["w_slope"], c["rough_max"], c["nz_min"])


@functools.lru_cache(maxsize=None)
def _terrain(name):
    """None (the plane); the smallest legal heightfield, one cell of 2 m whose two triangles tilt differently; 24 x 24 samples of 0.1 m:
    blocks of 4 x 4 cells at multiples of 0.08 m (steps that a probe accepts or rejects), a gentle ramp over the first eight rows, a ramp
    too steep for nz_min in a corner, and one count of noise everywhere so that no two candidates tie."""
    if name == "plane":
        return None
    if name == "2x2":
        return dict(heights=np.array([[0, 6], [-4, 10]], dtype=np.int16), hs=float(np.float32(2.0)), vs=float(np.float32(0.005)),
                    t=tuple(F32((-1.0, -1.0, 0.02)).tolist()))
    rng = np.random.default_rng(3)
    h = np.kron(rng.integers(-2, 3, (6, 6)) * 16, np.ones((4, 4), dtype=np.int64))
    h[0:8] += 3 * np.arange(24)[None, :]
    h[16:24, 0:12] = 15 * np.arange(12)[None, :]
    h += rng.integers(-1, 2, (24, 24))
    return dict(heights=h.astype(np.int16), hs=float(np.float32(0.1)), vs=float(np.float32(0.005)), t=tuple(F32((-1.2, -1.2, 0.0)).tolist()))


def _span(name):
    """Base positions: inside the grid and beyond its border."""
    return {"plane": (-2.0, 2.0), "2x2": (-1.5, 1.5), "24x24": (-1.6, 1.5)}[name]


def _inputs(n, terrain, seed, call=0, dt=0.02):
    """fp32-representable inputs of call number `call` of a chain: near-upright trunks at every heading, legs inside their limits, moving
    as their velocities say from call to call."""
    m = _model()
    rng = np.random.default_rng(9000 + 17 * seed + n)
    lo, hi = _span(terrain)
    b = np.stack([rng.uniform(lo, hi, n), rng.uniform(lo, hi, n), rng.uniform(0.25, 0.4, n)], axis=-1)
    v = rng.uniform(-0.6, 0.6, (n, 3)); v[:, 2] *= 0.2
    yaw, rp = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.2, 0.2, (n, 2))
    quat = np.stack([np.sin(rp[:, 0] / 2) * np.cos(yaw / 2), np.sin(rp[:, 1] / 2) * np.cos(yaw / 2), np.sin(yaw / 2), np.cos(yaw / 2)], axis=-1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    dlo, dhi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    q, qd = dlo + (dhi - dlo) * rng.uniform(0.3, 0.7, (n, 20)), rng.uniform(-2, 2, (n, 20))
    special = np.array(SPECIAL_PHASES)
    phases = np.where(np.arange(n) < len(special), special[(np.arange(n) + seed) % len(special)], rng.uniform(0, 1, n))
    mask = (rng.random(n) < 0.2).astype(np.int32) * rng.integers(1, 5, n).astype(np.int32)
    t = call * dt
    return dict(base_pos=F32(b + v * t), base_vel=F32(v), quat=F32(quat), ang_vel=F32(rng.uniform(-1, 1, (n, 3))),
                dof=F32(np.stack([q + 0.3 * qd * t, qd], axis=-1)), vel_cmd=F32(rng.uniform(-0.6, 0.6, (n, 2))), yaw_rate=F32(rng.uniform(-1, 1, n)),
                phases=F32(phases), mask=mask, phase2=F32(rng.uniform(0, 1, n)))


def _ref(cfg, inp, terrain, dtype=np.float64, **kw):
    return fr.plan(_model(), cfg, inp["state"], inp["base_pos"], inp["base_vel"], inp["quat"], inp["ang_vel"], inp["dof"], vel_cmd=inp.get("vel_cmd"),
                   yaw_rate=inp.get("yaw_rate"), terrain=_terrain(terrain), gravity=GRAVITY, ground_z=GROUND_Z, reset=inp.get("reset"),
                   phase_init=inp.get("phase_init"), hold=inp.get("hold", False), dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def _chain(n, terrain, combo):
    """[(inputs, fp64 reference)] of NCALLS calls: a reset of every env at the dealt phases, a plain call, a masked reset, a plain call, each
    from the previous reference's state rounded to fp32. Computed once and left unchanged."""
    cfg = _combo_cfg(combo)
    state = np.zeros((n, fr.NS))
    calls = []
    for j in range(NCALLS):
        inp = _inputs(n, terrain, combo, j)
        inp["state"] = F32(state)
        if j == 0:
            inp.update(reset=True, phase_init=inp["phases"])
        elif j == 2:
            inp.update(reset=inp["mask"], phase_init=inp["phase2"])
        ref = _ref(cfg, inp, terrain)
        calls.append((inp, ref))
        state = ref["state"]
    return cfg, calls


def judge(cfg, ref):
    """From the fp64 reference alone: foot_ok [N, 4], stage_ok [N, H, 4], phase_ok [N] (the advanced phase is not at a wrap), and the
    masks `keep` of the continuous outputs' entries that are judged."""
    d, mag = ref["diag"], ref["mag"]
    n = d["phi"].shape[0]
    duty, latch = cfg["duty"], cfg["latch"]
    always = duty >= 1
    near = lambda x: (np.abs(x - duty) < PHASE_BOUND) | (x < PHASE_BOUND) | (x > 1 - PHASE_BOUND)    # noqa: E731
    foot_ok = np.ones((n, 4), dtype=bool)
    stage_ok = np.ones(d["stage_phase"].shape, dtype=bool)
    if not always:
        foot_ok &= ~near(d["phi"])
        foot_ok &= ~(~d["stand"] & (np.abs(d["s"] - latch) < PHASE_BOUND / (1 - duty)))
        stage_ok &= ~near(d["stage_phase"])
    pos_bound = CONST["foothold"] * EPS * mag["pos"]                                    # [N]
    with np.errstate(all="ignore"):
        cost = np.sort(d["cost"], axis=-1)
        gap = (cost[..., 1] - cost[..., 0]) if cost.shape[-1] > 1 else np.full(cost.shape[:-1], np.inf)
        tie = np.isfinite(cost[..., 0]) & ~(gap >= COST_CONST * EPS * mag["cost"])      # (inf - finite = inf: not a tie)
    edge = (np.abs(d["rough"] - cfg["rough_max"]) < pos_bound[:, None, None]).any(-1) | (np.abs(d["nz"] - cfg["nz_min"]) < NZ_BOUND).any(-1)
    line = d["margin"] < pos_bound[:, None]
    foot_ok &= ~(d["search"] & (tie | edge | line))
    adv = ref["state"][:, 0]
    phase_ok = (adv > PHASE_BOUND) & (adv < 1 - PHASE_BOUND)
    fk = foot_ok[:, :, None]
    st = np.ones((n, fr.NS), dtype=bool)
    st[:, 0] = phase_ok
    st[:, 4:] = np.repeat(foot_ok, 7, axis=1)
    H = d["stage_phase"].shape[1]
    keep = dict(swing_ref=np.broadcast_to(fk, (n, 4, 9)), swing_acc=np.broadcast_to(fk, (n, 4, 3)), foothold=np.broadcast_to(fk, (n, 4, 3)),
                foot_pos=np.broadcast_to((foot_ok & stage_ok.all(1))[:, None, :, None], (n, H, 4, 3)), state=st)
    return dict(foot_ok=foot_ok, stage_ok=stage_ok, phase_ok=phase_ok, keep=keep)


def _info_mask(foot_ok):
    """The info bits that are judged: a thin foot's NO_SAFE and LIFT bits are not."""
    bits = np.full(foot_ok.shape[0], fr.INFO_RESET | fr.INFO_FAILED, dtype=np.int64)
    for i in range(4):
        bits |= np.where(foot_ok[:, i], (fr.INFO_NO_SAFE << i) | (fr.INFO_LIFT << i), 0)
    return bits


def compare(got, ref, cfg, const=CONST, who=""):
    """Hold `got` (numpy, any float type) to the fp64 reference: discrete outputs exactly and continuous ones within the bound, outside thin
    cases. Returns (the largest ratios, thin foot-cases, foot-cases)."""
    j = judge(cfg, ref)
    fo, so = j["foot_ok"], j["stage_ok"]
    assert np.array_equal(np.asarray(got["stance"])[fo], ref["stance"][fo]), who
    assert np.array_equal(np.asarray(got["contact"], dtype=np.float64)[fo], ref["contact"][fo]), who
    assert np.array_equal(np.asarray(got["schedule"])[so], ref["schedule"][so]), who
    bits = _info_mask(fo)
    assert np.array_equal(np.asarray(got["info"]).astype(np.int64) & bits, ref["info"] & bits), who
    # the chosen candidate, read back from the foothold
    d = ref["diag"]
    picked = fo & (d["chosen"] >= 0)
    if picked.any():
        dist = np.abs(np.asarray(got["foothold"], dtype=np.float64)[:, :, None, 0:2] - d["cand"]).sum(-1)       # [N, 4, K]
        assert np.array_equal(np.argmin(dist, axis=-1)[picked], d["chosen"][picked]), who
    r = fr.ratios(got, ref, j["keep"])
    for k in fr.OUTPUTS:
        assert r[k] <= const[k], (who, k, r[k])
    thin = int((~(fo & so.all(1))).sum())
    return r, thin, fo.size


# ------------------------------------------------------------------------------------------------------------ CPU
_INPUTS = ("base_pos", "base_vel", "quat", "dof", "vel_cmd", "yaw_rate", "reset_mask", "phase_init")
_OUTS = ("stance", "contact", "schedule", "foot_pos", "foothold", "swing_ref", "swing_acc", "info")
_NAMES = ("sim", "cfg") + _INPUTS + ("flags", "state") + _OUTS + ("stream",)


def _refusals(base):
    """[(arguments that differ from the good call `base`, a word of the message)]: every refusal of wbc_sim_footstep_plan but the NULL sim."""
    good = _cfg()
    mk = lambda **kw: _make_cfg(good, **kw)                                          # noqa: E731
    nan, inf = float("nan"), float("inf")
    out = [(dict(cfg=None), b"NULL"), (dict(state=None), b"NULL"), (dict(flags=4), b"flag"), (dict(flags=-1), b"flag")]
    for field in ("dt", "period", "mpc_dt", "search_step", "probe_radius", "duty"):
        out += [(dict(cfg=mk(**{field: bad})), field.encode()) for bad in (0.0, -1.0, nan, inf)]
    for f in range(4):
        off = lambda bad: [bad if i == f else good["offset"][i] for i in range(4)]    # noqa: E731
        out += [(dict(cfg=mk(offset=off(bad))), b"offset") for bad in (-0.01, 1.0, nan, inf)]
        so = lambda bad: [[bad if (i, j) == (f, f % 2) else good["stance_offset"][i][j] for j in range(2)] for i in range(4)]   # noqa: E731
        out += [(dict(cfg=mk(stance_offset=so(bad))), b"stance_offset") for bad in (nan, inf)]
    out += [(dict(cfg=mk(horizon=bad)), b"horizon") for bad in (-1, 17)]
    out += [(dict(cfg=mk(search_radius=bad)), b"search_radius") for bad in (-1, 4)]
    for field, word in (("k_v", b"gain"), ("kp", b"gain"), ("kd", b"gain"), ("com_height", b"height"), ("swing_height", b"height"),
                        ("max_reach", b"reach"), ("w_dist", b"weight"), ("w_rough", b"weight"), ("w_slope", b"weight"),
                        ("rough_max", b"threshold"), ("nz_min", b"threshold")):
        out += [(dict(cfg=mk(**{field: bad})), word) for bad in (-1e-3, nan, inf)]
    out += [(dict(cfg=mk(latch=bad)), b"latch") for bad in (-0.01, 1.01, nan)]
    out += [({k: base[k] + off}, b"aligned") for k in _INPUTS + ("state", "contact", "foot_pos", "foothold", "swing_ref", "swing_acc", "info")
            for off in (1, 2, 3)]
    return out


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_footstep_plan(*[C.byref(args[k]) if isinstance(args[k], abi.WbcFootstepCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device():
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    import __graft_entry__ as g
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    assert "wbc_sim_footstep_plan" in EXPORTED_SYMBOLS and hasattr(L, "wbc_sim_footstep_plan")
    assert "wbc_footstep_kernel.hip" in g.SOURCES and "wbc_footstep.h" in g.HEADERS
    assert [f for f, _ in abi.WbcFootstepCfg._fields_] == list(fr.CFG_FIELDS) and C.sizeof(abi.WbcFootstepCfg) == 4 * 32
    assert (abi.FOOTSTEP_NS, abi.FOOTSTEP_MAX_RADIUS, abi.FOOTSTEP_RESET, abi.FOOTSTEP_HOLD) == (fr.NS, 3, 1, 2)
    assert (abi.FOOTSTEP_INFO_RESET, abi.FOOTSTEP_INFO_FAILED, abi.FOOTSTEP_INFO_NO_SAFE, abi.FOOTSTEP_INFO_LIFT) == (
        fr.INFO_RESET, fr.INFO_FAILED, fr.INFO_NO_SAFE, fr.INFO_LIFT)
    assert len(L.wbc_sim_footstep_plan.argtypes) == len(_NAMES)
    buf = (C.c_float * 2048)()
    p = C.addressof(buf)
    base = dict(sim=None, cfg=_make_cfg(_cfg()), flags=0, stream=None, state=p, **{k: p + 256 * (1 + i) for i, k in enumerate(_INPUTS + _OUTS)})
    refusals = _refusals(base)
    assert len(refusals) > 120
    for kw, word in refusals + [(dict(), b"sim is NULL"), (dict(flags=abi.FOOTSTEP_RESET | abi.FOOTSTEP_HOLD), b"sim is NULL"),
                                (dict(cfg=_make_cfg(_cfg(), horizon=0, mpc_dt=0.0)), b"sim is NULL"),      # mpc_dt is not looked at without stages
                                (dict(cfg=_make_cfg(_cfg(), duty=3.0, latch=1.0)), b"sim is NULL")]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_footstep_plan: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def test_schedule_reproduces_trot_schedule():
    from wbc_amd.envs import trot_schedule
    n = 400
    rng = np.random.default_rng(1)
    for duty, H, mpc_dt in ((0.5, 10, 0.03), (0.6, 16, 0.02), (0.35, 7, 0.05)):
        cfg = _cfg(duty=duty, horizon=H, mpc_dt=mpc_dt)
        phase = F32(rng.uniform(0, 1, n))
        inp = dict(_inputs(n, "plane", 0), state=np.zeros((n, fr.NS)), reset=True, phase_init=phase)
        ref = _ref(cfg, inp, "plane")
        clear = judge(cfg, ref)["stage_ok"] & (np.minimum(np.abs(ref["diag"]["stage_phase"] - cfg["duty"]), np.minimum(
            ref["diag"]["stage_phase"], 1 - ref["diag"]["stage_phase"])) >= 1e-3)
        want = trot_schedule(torch.tensor(phase, dtype=torch.float32), cfg["period"], cfg["duty"], H, cfg["mpc_dt"]).numpy()
        assert clear.mean() > 0.95 and np.array_equal(ref["schedule"][clear], want[clear])
        got32 = _ref(cfg, inp, "plane", dtype=np.float32)["schedule"]                  # the fp32 statements are trot_schedule's: every stage
        assert np.array_equal(got32, want)


def _swing_state(n, lift, target, phase):
    st = np.zeros((n, fr.NS))
    st[:, 0] = phase
    for i in range(4):
        st[:, 4 + 7 * i:7 + 7 * i], st[:, 7 + 7 * i:10 + 7 * i], st[:, 10 + 7 * i] = lift[:, i], target[:, i], 1.0
    return st


def test_swing_reference_ends_apex_and_derivatives():
    """s = 0: the lift-off position at rest; s -> 1: the target at rest; s = 1/2: the apex with no vertical velocity; and velocity and
    acceleration are the time derivatives of position and velocity by fp64 central differences."""
    n = 6
    rng = np.random.default_rng(2)
    cfg = _cfg(latch=0.0, horizon=0)                                                   # the stored target is kept
    T_sw = (1 - cfg["duty"]) * cfg["period"]
    lift, target = rng.uniform(-1, 1, (n, 4, 3)), rng.uniform(-1, 1, (n, 4, 3))
    inp0 = _inputs(n, "plane", 1)

    def at(phase):
        inp = dict(inp0, state=_swing_state(n, lift, target, phase), hold=True)
        return _ref(cfg, inp, "plane")
    # trot: feet 0 and 3 swing over phase [0.5, 1), feet 1 and 2 over [0, 0.5)
    for feet, phase0 in (((0, 3), 0.5), ((1, 2), 0.0)):
        feet = list(feet)
        o = at(phase0)                                                                 # s = 0 exactly
        assert not o["stance"][:, feet].any()
        assert np.array_equal(o["swing_ref"][:, feet, 0:3], lift[:, feet]) and (o["swing_ref"][:, feet, 3:] == 0).all()
        o = at(phase0 + 0.5 - 1e-9)                                                     # s = 1 - 2e-9
        assert np.abs(o["swing_ref"][:, feet, 0:3] - target[:, feet]).max() < 1e-7 and np.abs(o["swing_ref"][:, feet, 3:]).max() < 1e-4
        o = at(phase0 + 0.25)                                                           # s = 1/2
        za = np.maximum(lift[:, feet, 2], target[:, feet, 2]) + cfg["swing_height"]
        assert np.abs(o["swing_ref"][:, feet, 2] - za).max() < 1e-12 and np.abs(o["swing_ref"][:, feet, 5]).max() < 1e-9
        assert np.abs(o["swing_ref"][:, feet, 0:2] - 0.5 * (lift[:, feet, 0:2] + target[:, feet, 0:2])).max() < 1e-12
        for s in (0.07, 0.3, 0.49, 0.51, 0.8, 0.97):
            dphi = 1e-5
            h = dphi * cfg["period"]
            lo, mid, hi = at(phase0 + 0.5 * s - dphi), at(phase0 + 0.5 * s), at(phase0 + 0.5 * s + dphi)
            vel = (hi["swing_ref"][:, feet, 0:3] - lo["swing_ref"][:, feet, 0:3]) / (2 * h)
            acc = (hi["swing_ref"][:, feet, 3:6] - lo["swing_ref"][:, feet, 3:6]) / (2 * h)
            assert np.abs(vel - mid["swing_ref"][:, feet, 3:6]).max() < 1e-5 * 2 / T_sw, s
            assert np.abs(acc - mid["swing_ref"][:, feet, 6:9]).max() < 1e-5 * 2 / T_sw ** 2, s
            # swing_acc is the reference's acceleration plus the PD on the tracking error
            d = mid["diag"]
            want = mid["swing_ref"][:, feet, 6:9] + cfg["kp"] * (mid["swing_ref"][:, feet, 0:3] - d["p"][:, feet]) + cfg["kd"] * (mid["swing_ref"][:, feet, 3:6] - d["pd"][:, feet])
            assert np.abs(mid["swing_acc"][:, feet] - want).max() < 1e-9 * np.abs(want).max()


def test_nominal_foothold_closed_forms_and_the_plane():
    """On the plane the chosen candidate is the nominal; for a straight walk at the commanded velocity and for a pure turn the nominal is
    the closed form."""
    n = 40
    rng = np.random.default_rng(3)
    cfg = _cfg(search_radius=3, horizon=0, max_reach=10.0)
    inp = dict(_inputs(n, "plane", 2), state=np.zeros((n, fr.NS)), reset=True)
    inp["phase_init"] = F32(rng.uniform(0, 1, n))
    yaw = rng.uniform(-np.pi, np.pi, n)
    inp["quat"] = np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)], axis=-1)
    so = np.array(cfg["stance_offset"])
    rot = lambda a, x: np.stack([np.cos(a) * x[..., 0] - np.sin(a) * x[..., 1], np.sin(a) * x[..., 0] + np.cos(a) * x[..., 1]], axis=-1)   # noqa: E731
    # a straight walk: v = v_c, no yaw rate
    cmd = rng.uniform(-0.5, 0.5, (n, 2))
    vw = rot(yaw, cmd)
    walk = dict(inp, vel_cmd=cmd, yaw_rate=np.zeros(n), base_vel=np.concatenate([vw, np.zeros((n, 1))], axis=-1))
    o = _ref(cfg, walk, "plane")
    t = o["diag"]["t"]
    want = walk["base_pos"][:, None, 0:2] + vw[:, None] * t[..., None] + rot(yaw[:, None], so[None]) + 0.5 * cfg["duty"] * cfg["period"] * vw[:, None]
    assert np.abs(o["diag"]["nom"] - want).max() < 1e-12
    sw = ~o["diag"]["stand"]
    assert sw.any() and (o["diag"]["chosen"][o["diag"]["search"]] == 24).all() and (o["info"] & (15 * fr.INFO_NO_SAFE) == 0).all()
    at_nom = o["diag"]["stand"] | o["diag"]["search"]                                  # (a foot past the latch keeps its stored target)
    assert np.array_equal(o["foothold"][..., 0:2][at_nom], o["diag"]["nom"][at_nom]) and (o["foothold"][..., 2][at_nom] == GROUND_Z).all()
    # a pure turn: no velocity, no command
    wz = rng.uniform(-2, 2, n)
    turn = dict(inp, vel_cmd=np.zeros((n, 2)), yaw_rate=wz, base_vel=np.zeros((n, 3)))
    o = _ref(cfg, turn, "plane")
    t = o["diag"]["t"]
    want = turn["base_pos"][:, None, 0:2] + rot(yaw[:, None] + wz[:, None] * t, so[None])
    assert np.abs(o["diag"]["nom"] - want).max() < 1e-12
    # and the clamp on the added vector
    o = _ref(dict(cfg, max_reach=0.05), dict(walk, base_vel=walk["base_vel"] * 5), "plane")
    ln = np.linalg.norm(o["diag"]["add"], axis=-1)
    assert ln.max() <= 0.05 + 1e-12 and (np.abs(ln - 0.05) < 1e-12).sum() > n // 2


def test_search_avoids_a_step_and_reports_no_safe():
    """Next to a one-cell step of 2 rough_max no chosen foothold has a probe across the edge; the chosen cost is the least of the accepted
    candidates; NO_SAFE appears exactly where every candidate is rejected."""
    n = 300
    cfg = _cfg(search_radius=3, horizon=0, nz_min=0.0, probe_radius=0.15, search_step=0.04)
    hs, vs = 0.1, 0.005
    rise = int(round(2 * cfg["rough_max"] / vs))
    h = np.zeros((24, 24), dtype=np.int16)
    h[12:] = rise                                                                      # the step: the cell between rows 11 and 12
    T = dict(heights=h, hs=hs, vs=vs, t=(-1.2, -1.2, 0.0))
    xa, xb = -1.2 + 11 * hs, -1.2 + 12 * hs
    rng = np.random.default_rng(4)
    inp = dict(_inputs(n, "plane", 3), state=np.zeros((n, fr.NS)), reset=True)
    inp["phase_init"] = F32(rng.uniform(0, 1, n))
    inp["base_pos"][:, 0] = rng.uniform(xa - 0.5, xb + 0.5, n)
    inp["base_pos"][:, 1] = rng.uniform(-0.8, 0.8, n)
    o = fr.plan(_model(), cfg, inp["state"], inp["base_pos"], inp["base_vel"], inp["quat"], inp["ang_vel"], inp["dof"], vel_cmd=inp["vel_cmd"],
                yaw_rate=inp["yaw_rate"], terrain=T, gravity=GRAVITY, reset=True, phase_init=inp["phase_init"])
    d = o["diag"]
    pr = cfg["probe_radius"]
    across = lambda x: ((x >= xb) & (x - pr <= xa)) | ((x <= xa) & (x + pr >= xb))     # noqa: E731
    srch = d["search"]
    assert srch.sum() > 200
    assert across(d["nom"][..., 0][srch]).sum() > 20                                   # nominal footholds that the search had to move
    found = srch & (d["chosen"] >= 0)
    assert not across(o["foothold"][..., 0][found]).any()
    assert (d["chosen"][srch & across(d["nom"][..., 0])] != 24).all()
    best = np.take_along_axis(d["cost"], np.maximum(d["chosen"], 0)[..., None], axis=-1)[..., 0]
    assert (best[found][:, None] <= d["cost"][found]).all() and np.isfinite(best[found]).all()
    no_safe = np.stack([(o["info"] >> (4 + i)) & 1 for i in range(4)], axis=-1).astype(bool)
    assert np.array_equal(no_safe, srch & ~np.isfinite(d["cost"]).any(-1))
    # a ramp too steep for nz_min everywhere: every candidate rejected, the target is the nominal on the terrain
    steep = dict(heights=(np.arange(24)[:, None] * 15 + np.zeros((1, 24))).astype(np.int16), hs=hs, vs=vs, t=(-1.2, -1.2, 0.0))
    cfg2 = _cfg(search_radius=1, horizon=0)
    inp["base_pos"][:, 0] = rng.uniform(-0.6, 0.6, n)
    o = fr.plan(_model(), cfg2, inp["state"], inp["base_pos"], inp["base_vel"], inp["quat"], inp["ang_vel"], inp["dof"], terrain=steep,
                gravity=GRAVITY, reset=True, phase_init=inp["phase_init"])
    d = o["diag"]
    no_safe = np.stack([(o["info"] >> (4 + i)) & 1 for i in range(4)], axis=-1).astype(bool)
    assert d["search"].any() and np.array_equal(no_safe, d["search"]) and (d["chosen"][d["search"]] == -1).all()
    hn, _, _ = fr.terrain_query(steep, d["nom"][..., 0], d["nom"][..., 1])
    assert np.array_equal(o["foothold"][..., 0:2][d["search"]], d["nom"][d["search"]]) and np.array_equal(o["foothold"][..., 2][d["search"]], hn[d["search"]])


def test_stage_foot_positions_advance_by_a_period_of_the_command():
    n = 50
    rng = np.random.default_rng(5)
    cfg = _cfg(horizon=16, mpc_dt=0.1, search_radius=0)                                # 1.6 s: more than three periods
    inp = dict(_inputs(n, "plane", 4), state=np.zeros((n, fr.NS)), reset=True)
    inp["phase_init"] = F32(rng.uniform(0, 1, n))
    o = _ref(cfg, inp, "plane")
    vc, p, fh = o["diag"]["vc"], o["diag"]["p"], o["foothold"]
    seen = 0
    for e in range(n):
        for i in range(4):
            stages = [k for k in range(16) if o["schedule"][e, k, i]]
            vals = []
            for k in stages:
                v = o["foot_pos"][e, k, i]
                if not vals or not np.array_equal(vals[-1], v):
                    vals.append(v)
            if o["stance"][e, i] and o["schedule"][e, 0, i]:
                assert np.array_equal(vals[0], p[e, i])                                # the stance the foot is in now
                vals = vals[1:]
            assert len(vals) >= 2 and np.array_equal(vals[0], fh[e, i])
            for a, b in zip(vals, vals[1:]):
                assert np.abs(b - a - np.append(cfg["period"] * vc[e], 0.0)).max() < 1e-12
                seen += 1
            for k in range(16):                                                        # a swing stage: its next stance stage's value
                later = [kk for kk in stages if kk > k]
                if not o["schedule"][e, k, i] and later:
                    assert np.array_equal(o["foot_pos"][e, k, i], o["foot_pos"][e, later[0], i])
    assert seen > 2 * n


def test_hold_and_one_full_period_of_calls():
    """A HOLD call leaves the phase; the 64 calls of one period after a reset return the phase exactly (dt / period = 2^-6) and lift every
    foot exactly once, whether the reset found it standing or swinging."""
    n = 20
    rng = np.random.default_rng(6)
    lift_bits = lambda o: np.stack([(o["info"] >> (8 + i)) & 1 for i in range(4)], axis=-1)     # noqa: E731
    for gait, duty in (("trot", 0.5), ("walk", 0.75), ("pace", 0.6), ("bound", 0.4)):
        cfg = _cfg(offset=fr.GAITS[gait], duty=duty, dt=0.0078125, period=0.5, horizon=0)
        inp = dict(_inputs(n, "plane", 5), state=np.zeros((n, fr.NS)), reset=True)
        inp["phase_init"] = F32(rng.uniform(0, 1, n))
        held = _ref(cfg, dict(inp, hold=True), "plane")
        assert np.array_equal(held["state"][:, 0], inp["phase_init"])
        o = _ref(cfg, inp, "plane")
        assert np.array_equal(lift_bits(o), 1 - o["stance"]) and np.array_equal(o["state"][:, 10::7], 1.0 - o["stance"])
        start, state = o["state"][:, 0].copy(), o["state"]
        assert np.array_equal(start, (inp["phase_init"] + 0.0078125 / 0.5) % 1.0)
        lifts = np.zeros((n, 4), dtype=np.int64)
        for _ in range(64):
            o = _ref(cfg, dict(inp, state=state, reset=None), "plane")
            lifts += lift_bits(o)
            state = o["state"]
            again = _ref(cfg, dict(inp, state=state, reset=None, hold=True), "plane")
            assert np.array_equal(again["state"][:, 0], state[:, 0])
        assert np.array_equal(state[:, 0], start) and np.array_equal(lifts, np.ones((n, 4), dtype=np.int64))


def test_non_finite_inputs_fail_the_env_alone():
    n = 9
    cfg = _cfg()
    inp = dict(_inputs(n, "plane", 6), state=F32(np.random.default_rng(7).uniform(0, 0.9, (n, fr.NS))))
    good = _ref(cfg, inp, "plane")
    bad = {k: np.array(v, copy=True) for k, v in inp.items()}
    bad["base_pos"][0, 1] = np.nan; bad["base_vel"][1, 0] = np.inf; bad["quat"][2, 3] = np.nan; bad["dof"][3, 4, 0] = np.nan
    bad["vel_cmd"][4, 0] = np.inf; bad["yaw_rate"][5] = np.nan; bad["state"][6, 17] = np.nan; bad["ang_vel"][7, 2] = np.inf
    o = _ref(cfg, bad, "plane")
    assert o["info"][:8].tolist() == [fr.INFO_FAILED] * 8 and o["info"][8] == good["info"][8]
    for k in ("stance", "contact", "schedule", "foot_pos", "foothold", "swing_ref", "swing_acc"):
        assert (o[k][:8] == 0).all() and np.array_equal(o[k][8], good[k][8])
    assert np.array_equal(o["state"][:8], bad["state"][:8], equal_nan=True) and np.array_equal(o["state"][8], good["state"][8])


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output over every judged call, the thin foot-cases per terrain, and the fp32 reference's discrete outputs held to fp64."""
    worst = {k: 0.0 for k in fr.OUTPUTS}
    thin = {t: [0, 0] for t in TERRAINS}
    big = {k: 4.0 * 2 ** 20 for k in fr.OUTPUTS}                                       # the discrete checks; the ratios are measured, not bounded, here
    for terrain in TERRAINS:
        for n in SIZES:
            for combo in range(len(COMBOS)):
                cfg, calls = _chain(n, terrain, combo)
                for j, (inp, ref) in enumerate(calls):
                    r, t, total = compare(_ref(cfg, inp, terrain, dtype=np.float32), ref, cfg, const=big, who=(terrain, n, combo, j))
                    worst = {k: max(worst[k], r[k]) for k in worst}
                    thin[terrain][0] += t; thin[terrain][1] += total
    return worst, thin


def test_fp32_yardstick_is_where_the_constants_came_from():
    worst, _ = _yardsticks()
    print("footstep yardsticks: " + ", ".join(f"{k} K_ref = {worst[k]:.3g} (C = {CONST[k]:g})" for k in worst))
    for k in K_REF:
        assert abs(worst[k] - K_REF[k]) <= 0.25 * K_REF[k], (k, worst[k])
        assert 4 * worst[k] <= CONST[k]


def test_thin_cases_stay_under_the_cap():
    _, thin = _yardsticks()
    print("footstep thin foot-cases per terrain:", {t: f"{a} of {b}" for t, (a, b) in thin.items()})
    for t, (a, b) in thin.items():
        assert a <= 0.05 * b, (t, a, b)
    # and the cases are not vacuous: searches, rejections, NO_SAFE, both triangles and clamped queries all occur on the 24 x 24 field
    seen = dict(search=0, rejected=0, no_safe=0, moved=0)
    for n in SIZES:
        for combo in range(len(COMBOS)):
            for _, ref in _chain(n, "24x24", combo)[1]:
                d = ref["diag"]
                seen["search"] += int(d["search"].sum())
                seen["rejected"] += int((d["search"][..., None] & ~np.isfinite(d["cost"])).sum())
                seen["no_safe"] += int((d["chosen"] == -1).sum())
                seen["moved"] += int(((d["chosen"] >= 0) & (d["chosen"] != (d["cost"].shape[-1] - 1) // 2)).sum())
    print("24x24:", seen)
    assert all(v > 0 for v in seen.values()), seen


@functools.lru_cache(maxsize=None)
def _kernel_assembly():
    """csrc/wbc_footstep_kernel.hip compiled to gfx950 assembly with the build's own flags."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    if not os.path.exists(arm_codegen.HIPCC):
        pytest.skip("hipcc not installed")
    source = "wbc_footstep_kernel.hip"
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "footstep.s")
        subprocess.check_call([arm_codegen.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        return open(out).read()


def test_footstep_kernel_codegen():
    """One kernel, no scratch, a single wavefront per workgroup and therefore no s_barrier, at most 128 VGPRs, the static LDS DESIGN.md states."""
    import re
    text = _kernel_assembly()
    assert text.count(".amdhsa_kernel ") == 1
    entry = text[text.index("amdhsa.kernels:"):]
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))          # noqa: E731
    assert re.search(r"\.name:\s+wbc_footstep_plan_kernel\n", entry)
    print(f"wbc_footstep_plan_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64
    assert meta("group_segment_fixed_size") == 4 * (4 * 6 + 4 * 2 + 4 + 4 * 3 + 4 + 4 * 3) and meta("vgpr_count") <= 128
    body = text[text.index("\nwbc_footstep_plan_kernel:"):]
    body = body[:body.index(".Lfunc_end")]
    assert "s_endpgm" in body and "scratch_" not in body and "s_barrier" not in body


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _env(n, seed=5):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    return WidowGo1(cfg, sim_device="cuda:0", seed=seed)


_CURRENT_TERRAIN = {}


def _set_terrain(env, terrain):
    if _CURRENT_TERRAIN.get(id(env), "plane") == terrain:
        return
    T = _terrain(terrain)
    if T is None:
        env.sim.set_heightfield(None)
    else:
        env.sim.set_heightfield(T["heights"], T["hs"], T["vs"], *T["t"])
    _CURRENT_TERRAIN[id(env)] = terrain


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


def _shapes(H):
    return {"state": ((fr.NS,), torch.float32), "stance": ((4,), torch.uint8), "contact": ((4,), torch.float32), "schedule": ((H, 4), torch.uint8),
            "foot_pos": ((H, 4, 3), torch.float32), "foothold": ((4, 3), torch.float32), "swing_ref": ((4, 9), torch.float32),
            "swing_acc": ((4, 3), torch.float32), "info": ((), torch.int32)}


def _sent(dtype):
    return {torch.float32: SENTINEL, torch.int32: ISENTINEL, torch.uint8: USENTINEL}[dtype]


def _load_sim(env, inp):
    """The sim's own root and joint state from the inputs (the root's angular velocity is always read there)."""
    root = env.sim.tensor("ROOT_STATES").clone()
    root[:, 0, 0:3] = _dev(inp["base_pos"]); root[:, 0, 3:7] = _dev(inp["quat"]); root[:, 0, 7:10] = _dev(inp["base_vel"])
    root[:, 0, 10:13] = _dev(inp["ang_vel"])
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(_dev(inp["dof"]))
    torch.cuda.synchronize()


def _call(env, cfg, inp, which=_OUTS, null=(), load=True):
    """A direct C-ABI call into sentinel-framed buffers (the state starts from inp's); returns {name: [n, ...] tensor} of the state and the
    outputs asked for. The inputs named in `null`, and those missing from inp, are handed over as NULL."""
    n, H = env.num_envs, cfg["horizon"]
    if load:
        _load_sim(env, inp)
    shapes = _shapes(H)
    size = {k: int(np.prod(s, dtype=np.int64)) for k, (s, _) in shapes.items()}
    bufs = {}
    for name in ("state",) + tuple(which):
        dt = shapes[name][1]
        bufs[name] = torch.full((n * size[name] + 8,), _sent(dt), dtype=dt, device="cuda")
    bufs["state"][:n * fr.NS] = _dev(inp["state"]).reshape(-1)
    reset = inp.get("reset")
    flags = (abi.FOOTSTEP_RESET if reset is True else 0) | (abi.FOOTSTEP_HOLD if inp.get("hold") else 0)
    tens = {k: _dev(inp.get(k)) for k in _INPUTS if k not in null and k != "reset_mask"}
    tens["reset_mask"] = _dev(reset, torch.int32) if reset is not None and reset is not True else None
    ptr = lambda d, k: d[k].data_ptr() if d.get(k) is not None and d[k].numel() > 0 else None     # noqa: E731
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_footstep_plan(env.sim.h, C.byref(c), *[ptr(tens, k) for k in _INPUTS], flags, ptr(bufs, "state"),
                                         *[ptr(bufs, k) for k in _OUTS], None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert bool((b[n * size[name]:] == _sent(shapes[name][1])).all()), name
    return {name: b[:n * size[name]].view((n,) + shapes[name][0]).clone() for name, b in bufs.items()}


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("terrain", TERRAINS)
@pytest.mark.parametrize("n", SIZES)
def test_every_entry_against_fp64(n, terrain):
    env = _env(n)
    _set_terrain(env, terrain)
    worst = {k: 0.0 for k in fr.OUTPUTS}
    for combo in range(len(COMBOS)):
        cfg, calls = _chain(n, terrain, combo)
        for j, (inp, ref) in enumerate(calls):
            got = _np(_call(env, cfg, inp))
            assert all(np.isfinite(got[k].astype(np.float64)).all() for k in got)
            r, _, _ = compare(got, ref, cfg, who=(terrain, n, COMBOS[combo], j))
            worst = {k: max(worst[k], r[k]) for k in worst}
            zero = (inp["phases"] == 0.0) if j == 0 else np.zeros(n, dtype=bool)
            if COMBOS[combo][:2] == ("trot", 0.5) and zero.any():
                # phase exactly 0 (thin by the rule above, yet exact in any arithmetic): FL and RR stand at phi = 0, FR and RL lift off at
                # phi = 0.5 = duty with s = 0: the reference is the lift-off position, which is the foot's origin, at rest
                assert got["stance"][zero].tolist() == [[1, 0, 0, 1]] * int(zero.sum())
                assert (got["swing_ref"][zero][:, :, 3:] == 0).all() and (got["swing_acc"][zero][:, [0, 3]] == 0).all()
                lift = got["state"][zero][:, 4:].reshape(-1, 4, 7)[:, :, 0:3]
                assert np.array_equal(got["swing_ref"][zero][:, [1, 2], 0:3], lift[:, [1, 2]])
                assert (got["info"][zero] & (15 * fr.INFO_LIFT)) .tolist() == [6 * fr.INFO_LIFT] * int(zero.sum())
    print(f"footstep n={n} {terrain}: largest |kernel - ref| / (2^-24 mag): {worst}")


@pytest.mark.gpu
def test_outputs_one_at_a_time_two_runs_and_the_sim_untouched():
    n, terrain, combo = 130, "24x24", 2
    env = _env(n)
    _set_terrain(env, terrain)
    cfg, calls = _chain(n, terrain, combo)
    inp = calls[1][0]
    _load_sim(env, inp)
    before = {name: env.sim.tensor(name).clone() for name in abi.TENSOR_IDS}
    want = _call(env, cfg, inp, load=False)
    again = _call(env, cfg, inp, load=False)
    assert all(torch.equal(want[k], again[k]) for k in want)                           # two runs: the same bits
    for name in _OUTS:
        got = _call(env, cfg, inp, which=(name,), load=False)
        assert torch.equal(got[name], want[name]) and torch.equal(got["state"], want["state"]), name
    got = _call(env, cfg, inp, which=(), load=False)
    assert torch.equal(got["state"], want["state"])
    raw = lambda t: t.contiguous().reshape(-1).view(torch.uint8)                       # noqa: E731
    for name, t in before.items():
        assert torch.equal(raw(env.sim.tensor(name)), raw(t)), name


@pytest.mark.gpu
def test_null_inputs_mean_the_sims_state():
    n, terrain, combo = 130, "24x24", 1
    env = _env(n)
    _set_terrain(env, terrain)
    cfg, calls = _chain(n, terrain, combo)
    inp, ref = calls[3]
    want = _call(env, cfg, inp)
    # copies alone: position, velocity and joints are the same floats wherever they are read
    for null in (("base_pos",), ("base_vel",), ("dof",), ("base_pos", "base_vel", "dof")):
        got = _call(env, cfg, inp, null=null, load=False)
        assert all(torch.equal(got[k], want[k]) for k in want), null
    # the quaternion is normalised in the call either way: the same bits too, and within the bound of fp64 in any case
    got = _call(env, cfg, inp, null=("base_pos", "base_vel", "quat", "dof"), load=False)
    compare(_np(got), ref, cfg, who="NULL inputs")
    assert all(torch.equal(got[k], want[k]) for k in want)
    # no command at all
    inp0 = {k: v for k, v in inp.items() if k not in ("vel_cmd", "yaw_rate")}
    got = _call(env, cfg, inp0, null=("vel_cmd", "yaw_rate"), load=False)
    compare(_np(got), _ref(cfg, inp0, terrain), cfg, who="NULL command")


@pytest.mark.gpu
def test_failed_envs_write_zeros_and_keep_their_state():
    n, terrain, combo = 130, "plane", 1
    env = _env(n)
    _set_terrain(env, terrain)
    cfg, calls = _chain(n, terrain, combo)
    inp, _ = calls[1]
    bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in inp.items()}
    rows = [0, 1, 31, 64, 65, 100, 128, 129]
    bad["base_pos"][0, 1] = np.nan; bad["base_vel"][1, 0] = np.inf; bad["quat"][31, 3] = np.nan; bad["dof"][64, 4, 0] = np.nan
    bad["vel_cmd"][65, 0] = np.inf; bad["yaw_rate"][100] = np.nan; bad["state"][128, 17] = np.nan; bad["ang_vel"][129, 2] = np.inf
    ref = _ref(cfg, bad, terrain)
    assert ref["info"][rows].tolist() == [fr.INFO_FAILED] * len(rows)
    got = _call(env, cfg, bad)
    plain = _call(env, cfg, inp)
    ok = torch.tensor(np.delete(np.arange(n), rows), device="cuda")
    for k in got:                                                                      # their neighbours: the bits of the launch without them
        assert torch.equal(got[k][ok], plain[k][ok]), k
    g = _np(got)
    assert g["info"][rows].tolist() == [fr.INFO_FAILED] * len(rows)
    for k in _OUTS[:-1]:
        assert (g[k][rows] == 0).all(), k
    assert np.array_equal(g["state"][rows], bad["state"][rows].astype(np.float32), equal_nan=True)


@pytest.mark.gpu
def test_two_hundred_calls_track_the_reference():
    """Four periods of 50 calls on the kernel's own state: the phase within the accumulated fp32 bound, which is 4 x the fp32 reference's own
    largest drift from fp64 over the run rounded up to a power of two; stance and the swing flags exact outside thin cases (a foot phase
    within that bound, plus PHASE_BOUND, of duty or of a wrap)."""
    n, terrain = 13, "plane"
    env = _env(n)
    _set_terrain(env, terrain)
    cfg = _cfg(dt=0.01, period=0.5, horizon=0, search_radius=1)
    inp = dict(_inputs(n, terrain, 11), state=np.zeros((n, fr.NS)), reset=True)
    inp["phase_init"] = inp["phases"]
    circ = lambda a, b: np.abs((a - b + 0.5) % 1.0 - 0.5)                              # noqa: E731
    s64, s32 = inp["state"], inp["state"]
    got = _call(env, cfg, inp)
    drift, kernel_drift, thin, lifts = 0.0, [], 0, np.zeros((n, 4), dtype=np.int64)
    refs = []
    for j in range(201):
        step = dict(inp, state=s64) if j == 0 else dict(inp, state=s64, reset=None, phase_init=None)
        r64 = _ref(cfg, step, terrain)
        r32 = _ref(cfg, dict(step, state=s32), terrain, dtype=np.float32)
        s64, s32 = r64["state"], r32["state"].astype(np.float64)
        drift = max(drift, circ(s32[:, 0], s64[:, 0]).max())
        refs.append(r64)
    bound = float(2.0 ** np.ceil(np.log2(4 * max(drift, EPS))))
    state = None
    for j in range(201):
        step = inp if j == 0 else dict(inp, state=state, reset=None, phase_init=None)
        got = _np(_call(env, cfg, step, load=(j == 0)))
        state = got["state"].astype(np.float64)
        r64 = refs[j]
        kernel_drift.append(circ(state[:, 0], r64["state"][:, 0]).max())
        phi = r64["diag"]["phi"]
        near = (np.abs(phi - cfg["duty"]) < bound + PHASE_BOUND) | (phi < bound + PHASE_BOUND) | (phi > 1 - bound - PHASE_BOUND)
        thin += int(near.sum())
        assert np.array_equal(got["stance"][~near], r64["stance"][~near]), j
        assert np.array_equal(state[:, 10::7][~near], r64["state"][:, 10::7][~near]), j
        lifts += np.stack([(got["info"] >> (8 + i)) & 1 for i in range(4)], axis=-1)
    print(f"footstep 200 calls: fp32 reference's drift {drift:.3g}, bound {bound:.3g}, kernel's largest drift {max(kernel_drift):.3g}, thin foot-calls {thin}")
    assert max(kernel_drift) <= bound
    assert thin <= 0.05 * 201 * n * 4 and lifts.min() >= 4 and lifts.max() <= 5        # four periods: every foot lifted four times (five with the reset's)


@pytest.mark.gpu
def test_captured_graph_replays_the_eager_bits():
    n, terrain, combo = 130, "24x24", 2
    env = _env(n)
    _set_terrain(env, terrain)
    cfg, calls = _chain(n, terrain, combo)
    inp = calls[1][0]
    want = _call(env, cfg, inp)
    H = cfg["horizon"]
    c = _make_cfg(cfg)
    t = {k: _dev(inp[k]) for k in ("base_pos", "base_vel", "quat", "dof", "vel_cmd", "yaw_rate")}
    state0 = _dev(inp["state"])
    state = state0.clone()
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _shapes(H).items() if k != "state"}
    call = lambda: env.sim.footstep_plan(c, state, **t, **outs)                        # noqa: E731
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


@pytest.mark.gpu
def test_gait_planner_closes_the_loop_with_finite_outputs():
    """estimator -> planner -> MPC -> whole-body controller -> simulate on 8 envs for 20 control steps: every output finite, every status
    word one of its defined values. Nothing is asserted about how well the robot walks."""
    from wbc_amd.envs import FootstepPlanner
    env = _env(8, seed=9)
    _set_terrain(env, "plane")
    env.reset()
    est = env.base_state_estimator()
    planner = env.gait_planner("trot", period=0.5, duty=0.5, horizon=10)
    mpc = env.centroidal_mpc(horizon=10)
    assert isinstance(planner, FootstepPlanner) and planner.phase.shape == (8,) and bool((planner.phase == 0).all())
    so = np.array(FootstepPlanner.default_stance_offset(env))
    assert so.shape == (4, 2) and (so[:2, 0] > 0).all() and (so[2:, 0] < 0).all() and (so[::2, 1] > 0).all() and (so[1::2, 1] < 0).all()
    cmd = torch.tensor([[0.3, 0.0]], device="cuda").expand(8, 2).contiguous()
    wz = torch.zeros(8, device="cuda")
    known = fr.INFO_RESET | fr.INFO_FAILED | 15 * fr.INFO_NO_SAFE | 15 * fr.INFO_LIFT
    for step in range(20):
        est.update(contact=planner.contact)
        planner.update(cmd, wz, state=est)
        mpc.solve(planner.contact_schedule, cmd, wz, foot_positions=planner.foot_positions, state=est)
        tau, nudot, lam, info = env.whole_body_controller(base_acc=mpc.base_acc, swing_acc=planner.swing_acc, stance=planner.stance)
        env.sim.set_dof_forces(tau.contiguous())
        for _ in range(int(env.cfg.control.decimation)):
            env.sim.simulate()
        torch.cuda.synchronize()
        for name in ("state", "contact", "foot_positions", "footholds", "swing_ref", "swing_acc"):
            assert bool(torch.isfinite(getattr(planner, name)).all()), (step, name)
        assert bool(torch.isfinite(mpc.forces).all()) and bool(torch.isfinite(mpc.base_acc).all()) and bool(torch.isfinite(tau).all())
        assert bool(torch.isfinite(est.x).all())
        assert bool(((planner.info & ~known) == 0).all()) and bool((planner.info & fr.INFO_FAILED == 0).all())
        assert set(mpc.status.cpu().tolist()) <= {abi.MPC_STATUS_OK, abi.MPC_STATUS_ITERATIONS, abi.MPC_STATUS_FAILED}
        assert set(info["status"].cpu().tolist()) <= {0, 1, 2}
        assert set(est.status.cpu().tolist()) <= {abi.ESTIMATOR_STATUS_OK, abi.ESTIMATOR_STATUS_RESET, abi.ESTIMATOR_STATUS_FAILED}
        assert set(planner.stance.cpu().unique().tolist()) <= {0, 1}
    if not bool(env.reset_buf.any()):
        assert abs(float(planner.phase[0]) - (20 * env.dt / 0.5) % 1.0) < 1e-4
    # reset of some envs at a phase: the others keep theirs
    keep = planner.state.clone()
    planner.reset(env_ids=[1, 5], phase=0.25)
    torch.cuda.synchronize()
    assert planner.phase[[1, 5]].tolist() == [0.25, 0.25] and torch.equal(planner.state[[0, 2, 3, 4, 6, 7], 0], keep[[0, 2, 3, 4, 6, 7], 0])
