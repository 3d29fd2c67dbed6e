"""Contact detection from proprioception (wbc_sim_contact_detect: wbc_contact_detect_kernel in csrc/wbc_contact_kernel.hip; the text both
implement is the comment in include/wbc_sim.h). The CPU tests pin the fp64 restatement of tests/contact_reference.py to properties of the
equations and measure the fp32 yardstick; the GPU tests hold the kernel to the reference entry by entry.

Bound: every entry of a continuous output satisfies |kernel - ref| <= C 2^-24 mag, mag as contact_reference's docstring lists it. C is
4 x K_ref rounded up to a power of two, K_ref the largest ratio of the reference run in fp32 against itself in fp64 over the judged cases
(every call of every chain: SIZES x COMBOS x NCALLS), measured on the CPU and asserted there; it never comes from the kernel.

    output   K_ref    kernel's largest ratio on an MI355X    C
    prob     5.9      14.5  (n = 130)                        32
    terms    10.9     16.6  (n = 130)                        64
    force    75       46.8  (n = 130)                        512
    state    5.9      14.5  (n = 130)                        32

The kernel's prob ratio is above K_ref (and inside C): its P_f goes through the device's erff and its own FMA contraction of the 3 x 3 solve,
and prob's magnitude carries the force's error through Phi's slope (up to 0.05 per newton at sigma_f = 8 N). Thin foot-cases: 6 of 37 232
(the cap is 1 %). On the simulator (8 envs, 75 control steps, the yardstick measured in the test from the logged inputs): K_ref 1.6 / 5.5 /
13.5 / 1.6 (prob / terms / force / state), C 8 / 32 / 64 / 8, the kernel 1.03 / 3.72 / 9.64 / 1.03.

Discrete outputs (contact, stance, the info bits, the flag in state) match exactly except in THIN cases, judged from the fp64 reference
alone (judge()): the filtered p within C_prob 2^-24 mag of p_on or p_off; a foot's phase within PHASE_BOUND of duty or of a wrap (0 or 1),
or, through s, of early_min's or late_min's edge. A thin foot is left out of the foot's discrete and continuous outputs. PHASE_BOUND:
phase + offset is one fp32 rounding of a number below 2, frac another, the division by duty or 1 - duty a third: 8 x 2^-24 x 4 covers
them with the margin wbc_sim_footstep_plan's tests use. The dwell comparison t >= t_dwell is never thin: t_dwell = 0.05 is no multiple of
dt = 0.02, so t is at least 0.01 from it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contact_reference as cr
import estimator_reference as er
from wbc_amd import abi
from wbc_amd.abi import WbcContactCfg  # noqa: F401  (this file is about wbc_sim_contact_detect: none of it means anything without the call)

SENTINEL, ISENTINEL, USENTINEL = 12345.0, -7777, 201
EPS = 2.0 ** -24
F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)                  # noqa: E731
SIZES = (1, 15, 16, 17, 130)
# (force source, ground, phase, random normal): every combination of sources but none at all, both force sources with both kinds of normal
COMBOS = (("tau", True, True, False), ("tau", True, False, True), ("tau", False, True, True), ("tau", False, False, False),
          ("ff", True, True, True), ("ff", True, False, False), ("ff", False, True, False), ("ff", False, False, True),
          (None, True, True, False), (None, True, False, False), (None, False, True, False),
          ("tau", True, True, True), ("ff", True, True, False))
NCALLS = 4
PHASE_BOUND = 8 * EPS * 4
THIN_CAP = 0.01

# K_ref (measured by test_fp32_yardstick_is_where_the_constants_came_from), the kernel's largest ratio on the MI355X (for the record: no
# bound comes from it) and the constant
K_REF = {"prob": 5.9, "terms": 10.9, "force": 75.0, "state": 5.9}
K_GPU = {"prob": 14.5, "terms": 16.6, "force": 46.8, "state": 14.5}
_pow2 = lambda k: float(2.0 ** np.ceil(np.log2(4 * k)))                             # noqa: E731
CONST = {k: _pow2(v) for k, v in K_REF.items()}


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _cfg(**kw):
    """The kernel receives the cfg as floats: the references use the same rounded values."""
    base = dict(dt=0.02, duty=0.6, offset=(0.0, 0.5, 0.5, 0.0), sigma_phase=0.05, mu_z=0.01, sigma_z=0.01, mu_f=15.0, sigma_f=8.0, var_phase=0.25,
                var_z=0.05, var_f=0.05, alpha=0.5, p_on=0.6, p_off=0.4, t_dwell=0.05, early_min=0.5, late_min=0.2, damping=0.02)
    base.update(kw)
    return {k: (F32(base[k]).tolist() if k == "offset" else float(np.float32(base[k]))) for k in cr.CFG_FIELDS}


def _make_cfg(cfg, **kw):
    c = dict(cfg, **kw)
    return abi.WbcContactCfg(c["dt"], c["duty"], (abi.f32 * 4)(*c["offset"]), *[c[k] for k in cr.CFG_FIELDS[3:]])


def _postures(n, rng):
    """Leg joints inside their limits; every fifth env has one leg within 1 degree of a straight knee (the calf joint at 0, outside its
    limits, where the leg Jacobian loses a direction and the damping decides the force)."""
    m = _model()
    dlo, dhi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    q = dlo + (dhi - dlo) * rng.uniform(0.2, 0.8, (n, 20))
    _, _, _, dofs = er.leg_kinematics(m, q[:1], None, jac=True)
    for e in range(0, n, 5):
        q[e, dofs[(e // 5) % 4, 2]] = np.deg2rad(rng.uniform(-1.0, 1.0))
    return q, dofs


def _inputs(n, combo, call=0):
    """fp32-representable inputs of call number `call` of a chain: near-upright trunks at every heading, a plausible ground reaction on
    every foot turned into joint torques by the leg Jacobians (plus noise), feet within a few centimetres of the ground."""
    m = _model()
    rng = np.random.default_rng(7000 + 31 * combo + 1009 * call + n)
    b = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.25, 0.4, n)], axis=-1)
    yaw, rp = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.2, 0.2, (n, 2))
    quat = np.stack([np.sin(rp[:, 0] / 2) * np.cos(yaw / 2), np.sin(rp[:, 1] / 2) * np.cos(yaw / 2), np.sin(yaw / 2), np.cos(yaw / 2)], axis=-1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    quat *= rng.uniform(0.8, 1.2, (n, 1))                                                # normalised in the call
    q, dofs = _postures(n, rng)
    dof = F32(np.stack([q, rng.uniform(-2, 2, (n, 20))], axis=-1))
    b, quat = F32(b), F32(quat)
    P, J, _ = cr.leg_jacobians(m, quat, dof, b)
    f_true = np.stack([rng.uniform(-10, 10, (n, 4)), rng.uniform(-10, 10, (n, 4)), rng.uniform(-10, 60, (n, 4))], axis=-1)
    tau = rng.uniform(-3, 3, (n, 26))
    tau[:, 6 + dofs] += np.einsum("nfik,nfi->nfk", J, f_true)
    normal = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.3, 0.3, (n, 4, 3))
    normal *= rng.uniform(0.5, 2.0, (n, 4, 1))
    mask = (rng.random(n) < 0.3).astype(np.int32) * rng.integers(1, 5, n).astype(np.int32)
    return dict(base_pos=b, quat=quat, dof=dof, tau_ext=F32(tau), foot_force=F32(f_true + rng.uniform(-2, 2, (n, 4, 3))), normal=F32(normal),
                ground=F32(P[:, :, 2] - rng.uniform(-0.02, 0.05, (n, 4))), phase=F32(rng.uniform(0, 1, n)), p_init=F32(rng.uniform(0, 1, (n, 4))),
                p_init2=F32(rng.uniform(0, 1, (n, 4))), mask=mask)


def _select(inp, combo):
    """The inputs a combo hands over (the others are NULL)."""
    src, ground, phase, rnd_normal = COMBOS[combo]
    out = {k: inp[k] for k in ("base_pos", "quat", "dof", "state", "reset", "p_init") if k in inp}
    if src == "tau":
        out["tau_ext"] = inp["tau_ext"]
    if src == "ff":
        out["foot_force"] = inp["foot_force"]
    if rnd_normal:
        out["normal"] = inp["normal"]
    if ground:
        out["ground"] = inp["ground"]
    if phase:
        out["phase"] = inp["phase"]
    return out


def _ref(cfg, inp, dtype=np.float64):
    return cr.detect(_model(), cfg, inp["state"], inp["quat"], inp["dof"], inp["base_pos"], tau_ext=inp.get("tau_ext"),
                     foot_force_in=inp.get("foot_force"), normal=inp.get("normal"), ground=inp.get("ground"), phase=inp.get("phase"),
                     reset=inp.get("reset"), p_init=inp.get("p_init"), dtype=dtype)


@functools.lru_cache(maxsize=None)
def _chain(n, combo):
    """[(inputs, fp64 reference)] of NCALLS calls: a reset of every env with dealt p_init, a plain call, a masked reset, a plain call, each
    from the previous reference's state rounded to fp32. Computed once and left unchanged."""
    cfg = _cfg()
    state = np.zeros((n, cr.NS))
    calls = []
    for j in range(NCALLS):
        raw = _inputs(n, combo, j)
        raw["state"] = F32(state)
        if j == 0:
            raw["reset"] = True
        elif j == 2:
            raw.update(reset=raw["mask"], p_init=raw["p_init2"])
        else:
            raw.pop("p_init")
        inp = _select(raw, combo)
        ref = _ref(cfg, inp)
        calls.append((inp, ref))
        state = ref["state"]
    return cfg, calls


def judge(cfg, ref, const=None):
    """From the fp64 reference alone: foot_ok [N, 4] and the masks `keep` of the continuous outputs' entries that are judged."""
    const = CONST if const is None else const
    d = ref["diag"]
    n = d["p"].shape[0]
    bound = const["prob"] * EPS * d["pmag"]
    foot_ok = (np.abs(d["p"] - cfg["p_on"]) >= bound) & (np.abs(d["p"] - cfg["p_off"]) >= bound)
    if d["have_phase"]:
        duty, phi, s = cfg["duty"], d["phi"], d["s"]
        foot_ok &= (phi >= PHASE_BOUND) & (phi <= 1 - PHASE_BOUND)
        if duty < 1:
            foot_ok &= np.abs(phi - duty) >= PHASE_BOUND
        width = np.where(d["sched"], min(duty, 1.0), max(1 - duty, EPS))
        edge = np.where(d["sched"], cfg["late_min"], cfg["early_min"])
        foot_ok &= np.abs(s - edge) >= PHASE_BOUND / width
    foot_ok &= ~d["failed"][:, None]
    fk = foot_ok[:, :, None]
    keep = dict(prob=foot_ok, terms=np.broadcast_to(fk, (n, 4, 4)), force=np.broadcast_to(fk, (n, 4, 3)), state=np.repeat(foot_ok, 4, axis=1))
    return dict(foot_ok=foot_ok, keep=keep)


def _info_mask(foot_ok):
    """The info bits that are judged: a thin foot's own bits are not."""
    bits = np.full(foot_ok.shape[0], cr.INFO_RESET | cr.INFO_FAILED, dtype=np.int64)
    per_foot = cr.INFO_TOUCHDOWN | cr.INFO_LIFTOFF | cr.INFO_EARLY | cr.INFO_LATE | cr.INFO_FORCE_SINGULAR
    for i in range(4):
        bits |= np.where(foot_ok[:, i], per_foot << i, 0)
    return bits


def compare(got, ref, cfg, const=None, who=""):
    """Hold `got` (numpy, any float type) to the fp64 reference: discrete outputs exactly and continuous ones within the bound, outside thin
    cases. Returns (the largest ratios, thin foot-cases, foot-cases)."""
    const = CONST if const is None else const
    j = judge(cfg, ref, const)
    fo = j["foot_ok"]
    assert np.array_equal(np.asarray(got["contact"])[fo], ref["contact"][fo]), who
    assert np.array_equal(np.asarray(got["stance"])[fo], ref["stance"][fo]), who
    assert np.array_equal(np.asarray(got["state"], dtype=np.float64).reshape(-1, 4, 4)[:, :, 1][fo], ref["contact"][fo].astype(np.float64)), who
    bits = _info_mask(fo)
    assert np.array_equal(np.asarray(got["info"]).astype(np.int64) & bits, ref["info"] & bits), who
    r = cr.ratios(got, ref, j["keep"])
    for k in cr.OUTPUTS:
        assert r[k] <= const[k], (who, k, r[k])
    return r, int((~fo).sum()), fo.size


# ------------------------------------------------------------------------------------------------------------ CPU
_INPUTS = ("quat", "dof", "base_pos", "tau_ext", "foot_force", "normal", "ground", "phase", "reset_mask", "p_init")
_OUTS = ("prob", "contact", "stance", "force", "terms", "info")
_NAMES = ("sim", "cfg", "quat", "dof", "base_pos", "tau_ext", "tau_ext_stride", "foot_force", "normal", "ground", "phase", "phase_stride", "reset_mask",
          "p_init", "flags", "state") + _OUTS + ("stream",)


def _refusals(base):
    """[(arguments that differ from the good call `base`, a word of the message)]: every refusal of wbc_sim_contact_detect but the NULL sim."""
    good = _cfg()
    mk = lambda **kw: _make_cfg(good, **kw)                                          # noqa: E731
    nan, inf = float("nan"), float("inf")
    out = [(dict(cfg=None), b"NULL"), (dict(state=None), b"NULL"), (dict(flags=2), b"flag"), (dict(flags=-1), b"flag")]
    for field, word in (("dt", b"dt"), ("duty", b"duty"), ("sigma_phase", b"sigma"), ("sigma_z", b"sigma"), ("sigma_f", b"sigma"),
                        ("var_phase", b"var"), ("var_z", b"var"), ("var_f", b"var")):
        out += [(dict(cfg=mk(**{field: bad})), word) for bad in (0.0, -1.0, nan, inf)]
    for f in range(4):
        off = lambda bad: [bad if i == f else good["offset"][i] for i in range(4)]    # noqa: E731
        out += [(dict(cfg=mk(offset=off(bad))), b"offset") for bad in (-0.01, 1.0, nan, inf)]
    out += [(dict(cfg=mk(**{field: bad})), b"mu_") for field in ("mu_z", "mu_f") for bad in (nan, inf, -inf)]
    out += [(dict(cfg=mk(alpha=bad)), b"alpha") for bad in (0.0, -0.5, 1.01, nan, inf)]
    out += [(dict(cfg=mk(**{field: bad})), b"p_on") for field in ("p_on", "p_off") for bad in (nan, inf, -inf)]
    out += [(dict(cfg=mk(p_on=0.4, p_off=0.4)), b"above"), (dict(cfg=mk(p_on=0.3, p_off=0.4)), b"above")]
    out += [(dict(cfg=mk(**{field: bad})), field.encode()) for field in ("t_dwell", "damping") for bad in (-1e-3, nan, inf)]
    out += [(dict(cfg=mk(**{field: bad})), field.encode()) for field in ("early_min", "late_min") for bad in (-0.01, 1.01, nan)]
    out += [(dict(tau_ext=None, foot_force=None, ground=None, phase=None), b"no measurement source")]
    out += [(dict(), b"both")]                                                       # the base call hands over tau_ext and foot_force
    out += [(dict(foot_force=None, tau_ext_stride=bad), b"tau_ext_stride") for bad in (25, 0, -26)]
    out += [(dict(foot_force=None, phase_stride=bad), b"phase_stride") for bad in (0, -1)]
    out += [({"foot_force": None, k: base[k] + off}, b"aligned") for k in _INPUTS + ("state", "prob", "force", "terms", "info")
            if k != "foot_force" for off in (1, 2, 3)]
    out += [({"tau_ext": None, "foot_force": base["foot_force"] + off}, b"aligned") for off in (1, 2, 3)]
    return out


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_contact_detect(*[C.byref(args[k]) if isinstance(args[k], abi.WbcContactCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device():
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    import re
    import __graft_entry__ as g
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    assert "wbc_sim_contact_detect" in EXPORTED_SYMBOLS and hasattr(L, "wbc_sim_contact_detect")
    assert "wbc_contact_kernel.hip" in g.SOURCES and "wbc_contact.h" in g.HEADERS
    # the mirror against the header's struct: the same fields in the same order, all floats
    header = open(g.ROOT + "/include/wbc_sim.h").read()
    body = re.search(r"typedef struct \{([^}]*)\} wbc_contact_cfg;", header).group(1)
    fields = []
    for decl in re.findall(r"float ([^;]*);", body):
        for name in decl.split(","):
            name = name.strip()
            count = int(re.search(r"\[(\d+)\]", name).group(1)) if "[" in name else 1
            fields.append((name.split("[")[0], count))
    assert [f for f, _ in fields] == list(cr.CFG_FIELDS) == [f for f, _ in abi.WbcContactCfg._fields_]
    assert C.sizeof(abi.WbcContactCfg) == 4 * sum(c for _, c in fields) == 4 * 21
    assert abi.WbcContactCfg.offset.offset == 8 and abi.WbcContactCfg.sigma_phase.offset == 24 and abi.WbcContactCfg.damping.offset == 80
    assert (abi.CONTACT_NS, abi.CONTACT_RESET) == (cr.NS, 1)
    assert (abi.CONTACT_INFO_RESET, abi.CONTACT_INFO_FAILED, abi.CONTACT_INFO_TOUCHDOWN, abi.CONTACT_INFO_LIFTOFF, abi.CONTACT_INFO_EARLY,
            abi.CONTACT_INFO_LATE, abi.CONTACT_INFO_FORCE_SINGULAR) == (cr.INFO_RESET, cr.INFO_FAILED, cr.INFO_TOUCHDOWN, cr.INFO_LIFTOFF,
                                                                         cr.INFO_EARLY, cr.INFO_LATE, cr.INFO_FORCE_SINGULAR)
    for name in ("NS", "RESET", "INFO_RESET", "INFO_FAILED", "INFO_TOUCHDOWN", "INFO_LIFTOFF", "INFO_EARLY", "INFO_LATE", "INFO_FORCE_SINGULAR"):
        assert int(re.search(r"#define WBC_CONTACT_%s (\d+)" % name, header).group(1)) == getattr(abi, "CONTACT_" + name), name
    assert len(L.wbc_sim_contact_detect.argtypes) == len(_NAMES)
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    base = dict(sim=None, cfg=_make_cfg(_cfg()), flags=0, stream=None, state=p, tau_ext_stride=26, phase_stride=1,
                **{k: p + 512 * (1 + i) for i, k in enumerate(_INPUTS + _OUTS)})
    refusals = _refusals(base)
    assert len(refusals) > 120
    for kw, word in refusals + [(dict(foot_force=None), b"sim is NULL"), (dict(tau_ext=None, flags=abi.CONTACT_RESET), b"sim is NULL"),
                                (dict(foot_force=None, tau_ext_stride=52, phase_stride=32), b"sim is NULL"),
                                (dict(tau_ext=None, foot_force=None, ground=None, tau_ext_stride=0), b"sim is NULL"),   # a stride without its pointer is not looked at
                                (dict(tau_ext=None, foot_force=None, phase=None, phase_stride=0), b"sim is NULL"),
                                (dict(foot_force=None, cfg=_make_cfg(_cfg(), duty=3.0, alpha=1.0, t_dwell=0.0, damping=0.0)), b"sim is NULL")]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_contact_detect: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def test_force_solve_inverts_the_transposed_jacobian_and_stays_bounded():
    """With J from central differences of the reference's own forward kinematics, delta = 0 and tau = J^T f the solve returns f to fp64
    rounding on reachable postures; with delta > 0 the force never exceeds |tau| / (2 delta), a straight knee included."""
    m = _model()
    rng = np.random.default_rng(11)
    n = 64
    dlo, dhi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    q = dlo + (dhi - dlo) * rng.uniform(0.15, 0.85, (n, 20))
    dof = np.stack([q, np.zeros_like(q)], axis=-1)
    quat = rng.normal(size=(n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    b = rng.uniform(-1, 1, (n, 3))
    P, J, dofs = cr.leg_jacobians(m, quat, dof, b)
    h = 1e-6
    Jfd = np.zeros_like(J)
    for f in range(4):
        for k in range(3):
            dp, dm = dof.copy(), dof.copy()
            dp[:, dofs[f, k], 0] += h; dm[:, dofs[f, k], 0] -= h
            Jfd[:, f, :, k] = (cr.leg_jacobians(m, quat, dp, b)[0][:, f] - cr.leg_jacobians(m, quat, dm, b)[0][:, f]) / (2 * h)
    assert np.abs(Jfd - J).max() < 1e-8                                               # the analytic columns are the derivative of the foot origin
    force = rng.uniform(-50, 50, (n, 4, 3))
    tau = np.einsum("nfik,nfi->nfk", Jfd, force)
    got, ok, _ = cr.foot_force(Jfd, tau, 0.0)
    cond = np.linalg.cond(Jfd)
    assert ok.all() and (np.abs(got - force).max(-1) <= 1e-13 * cond ** 2 * np.abs(force).max(-1)).all() and np.abs(got - force).max() < 1e-8
    # damped: bounded by |tau| / (2 delta), the straight knee (calf joint at 0) included
    q2, dofs = _postures(n, rng)
    q2[::2, dofs[:, 2]] = 0.0
    dof2 = np.stack([q2, np.zeros_like(q2)], axis=-1)
    _, J2, _ = cr.leg_jacobians(m, quat, dof2, b)
    assert np.linalg.svd(J2[0], compute_uv=False)[:, 2].max() < 1e-12                 # straight: a direction is lost
    tau2 = rng.uniform(-30, 30, (n, 4, 3))
    for delta in (1e-3, 0.02, 0.5):
        f2, ok2, _ = cr.foot_force(J2, tau2, delta)
        assert ok2.all() and (np.linalg.norm(f2, axis=-1) <= np.linalg.norm(tau2, axis=-1) / (2 * delta) * (1 + 1e-9)).all(), delta
    # a failed pivot: f = 0 and the flag
    A = np.array([[[0.0, 0, 0], [0, 1, 0], [0, 0, 1]], [[1.0, 2, 0], [2, 4, 0], [0, 0, 1]], [[1.0, 0, 0], [0, 1, 2], [0, 2, 3]], [[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]]])
    assert not cr.chol3_solve(A, np.ones((4, 3)))[1].any()
    f3, ok3, _ = cr.foot_force(np.zeros((1, 3, 3)), np.ones((1, 3)), 0.0)
    assert not ok3.any() and (f3 == 0).all()


def test_prior_edges_symmetry_and_fusion():
    sigma = 0.05
    half = 0.5 * cr.erf(1 / (sigma * np.sqrt(2.0)))
    for duty in (0.3, 0.5, 0.6, 0.8):
        tiny = 1e-13
        lo, _, _ = cr.prior(np.array([duty - tiny, duty, 1.0 - tiny, 0.0]), duty, sigma)
        # the end of stance and the start of swing; the end of swing and the start of stance: one value, 1/2 erf(1 / (sigma sqrt 2))
        assert np.abs(lo - half).max() < 1e-9 and abs(float(half) - 0.5) < 1e-15
        s = np.linspace(0.01, 0.99, 99)
        st, sched, _ = cr.prior(s * duty, duty, sigma)
        assert sched.all() and np.abs(st - st[::-1]).max() < 1e-12 and st[49] > 1 - 1e-12          # symmetric about the middle of stance
        sw, sched, _ = cr.prior(duty + s * (1 - duty), duty, sigma)
        assert not sched.any() and np.abs(sw - sw[::-1]).max() < 1e-12 and sw[49] < 1e-12 and (sw >= 0).all() and (st <= 1).all()
    always, sched, s = cr.prior(np.array([0.0, 0.3, 0.99]), 1.0, sigma)
    assert sched.all() and np.allclose(s, [0.0, 0.3, 0.99])
    # fusion: between the smallest and the largest term; the term itself when it is alone
    n = 40
    cfg = _cfg(alpha=1.0, var_phase=0.3, var_z=0.02, var_f=0.11)
    for combo in range(len(COMBOS)):
        inp = _select(dict(_inputs(n, combo), state=np.zeros((n, cr.NS)), reset=True), combo)
        ref = _ref(cfg, inp)
        present = np.array([COMBOS[combo][2], COMBOS[combo][1], COMBOS[combo][0] is not None])
        tm = ref["terms"]
        assert (tm[:, :, :3][:, :, ~present] == 0).all()
        have = tm[:, :, :3][:, :, present]
        assert (tm[:, :, 3] >= have.min(-1) - 1e-15).all() and (tm[:, :, 3] <= have.max(-1) + 1e-15).all()
        if present.sum() == 1:
            assert np.abs(tm[:, :, 3] - have[:, :, 0]).max() <= 4 * 2.0 ** -53          # (P / var) / (1 / var): two roundings of a number below 1
        assert np.abs(ref["prob"] - tm[:, :, 3]).max() < 1e-15                         # alpha = 1: the filtered value is the fused one


def test_low_pass_closed_form():
    """After k calls with constant inputs p = P + (1 - alpha)^k (p_0 - P)."""
    n, combo = 12, 0
    cfg = _cfg(alpha=0.3, p_on=2.0, p_off=-1.0)                                        # the flag never switches
    raw = _inputs(n, combo)
    inp = _select(dict(raw, state=np.zeros((n, cr.NS)), reset=True), combo)
    p0 = raw["p_init"]
    state = None
    for k in range(1, 9):
        step = inp if k == 1 else dict(inp, state=state, reset=None, p_init=None)
        ref = _ref(cfg, step)
        state = ref["state"]
        P = ref["terms"][:, :, 3]
        assert np.abs(ref["prob"] - (P + (1 - cfg["alpha"]) ** k * (p0 - P))).max() < 1e-14, k
    assert np.allclose(ref["state"].reshape(n, 4, 4)[:, :, 2], cfg["t_dwell"] + 8 * cfg["dt"])


def _scripted(cfg, probs, phases=None, n_extra=0):
    """Drive the reference with a scripted sequence of fused probabilities for foot 0 of env 0 (alpha = 1, the force term alone, a measured
    normal force placed so that P_f is the wanted value); returns the per-call references."""
    from statistics import NormalDist
    n = 1 + n_extra
    base = _inputs(n, 5)
    state, refs = np.zeros((n, cr.NS)), []
    for j, pr in enumerate(probs):
        ff = np.zeros((n, 4, 3))
        ff[:, :, 2] = cfg["mu_f"] + cfg["sigma_f"] * NormalDist().inv_cdf(min(max(pr, 1e-12), 1 - 1e-12))
        ref = cr.detect(_model(), cfg, state, base["quat"], base["dof"], base["base_pos"], foot_force_in=ff,
                        phase=None if phases is None else np.full(n, phases[j]), reset=True if j == 0 else None,
                        p_init=np.zeros((n, 4)) if j == 0 else None)
        assert np.abs(ref["prob"] - pr).max() < 1e-9
        state = ref["state"]
        refs.append(ref)
    return refs


def test_flag_dwell_and_events_on_a_scripted_sequence():
    """dt 0.02, dwell 0.05 (no multiple of dt: the timer comparison is never thin). The flag never switches inside the dwell time, switches
    at the first eligible call, TOUCHDOWN / LIFTOFF appear on those calls only, EARLY / LATE exactly where the definition says and never
    without phase."""
    cfg = _cfg(alpha=1.0, var_f=1.0, var_phase=1e12, t_dwell=0.05, dt=0.02, p_on=0.6, p_off=0.4, duty=0.5, offset=(0.0, 0.0, 0.0, 0.0),
               early_min=0.5, late_min=0.2)
    # call 0: the reset at p_init 0: c = 0, the dwell served; 0.5 is inside the band. 1: 0.9 >= p_on at t = 0.09: touchdown. 2, 3: 0.1 <= p_off
    # but t = 0.02, 0.04 < dwell. 4: t = 0.06: lift-off, the first eligible call. 5, 6: 0.9 inside the dwell. 7: touchdown. 8, 9: inside the
    # band. 10: 0.39 <= p_off at t = 0.06: lift-off. 11, 12: nothing to switch. 13: 0.9 at t = 0.06: touchdown.
    probs = [0.5, 0.9, 0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 0.61, 0.5, 0.39, 0.39, 0.39, 0.9]
    want_c = [0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1]
    for phases in (None, [0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.45, 0.55, 0.7, 0.8, 0.9, 0.95, 0.05, 0.15]):
        refs = _scripted(cfg, probs, phases, n_extra=2)
        for foot in range(4):
            c = [int(r["contact"][0, foot]) for r in refs]
            td = [bool(r["info"][0] & (cr.INFO_TOUCHDOWN << foot)) for r in refs]
            lo = [bool(r["info"][0] & (cr.INFO_LIFTOFF << foot)) for r in refs]
            assert c == want_c, c
            assert [i for i, v in enumerate(td) if v] == [1, 7, 13] and [i for i, v in enumerate(lo) if v] == [4, 10]
            early = [bool(r["info"][0] & (cr.INFO_EARLY << foot)) for r in refs]
            late = [bool(r["info"][0] & (cr.INFO_LATE << foot)) for r in refs]
            if phases is None:
                assert not any(early) and not any(late)
                assert all(np.array_equal(r["stance"], r["contact"]) for r in refs)
                continue
            # duty 0.5: stance for phi < 0.5 with s = phi / 0.5, swing with s = (phi - 0.5) / 0.5
            want_late = [ph < 0.5 and ph / 0.5 >= cfg["late_min"] and ci == 0 for ph, ci in zip(phases, c)]
            want_early = [ph >= 0.5 and (ph - 0.5) / 0.5 >= cfg["early_min"] and ci == 1 for ph, ci in zip(phases, c)]
            assert late == want_late and early == want_early and any(late) and any(early)
            for r, ph, e, l in zip(refs, phases, early, late):
                assert int(r["stance"][0, foot]) == int(((ph < 0.5) or e) and not l)
        assert all((r["info"] & cr.INFO_RESET != 0).all() == (j == 0) for j, r in enumerate(refs))


def test_exact_threshold_hits():
    """Phi(0) = 1/2 exactly: a normal force of mu_f puts p on a threshold of 1/2. p >= p_on switches on, p <= p_off switches off; one ulp
    beyond the threshold does not."""
    n = 3
    base = _inputs(n, 5)
    up, down = float(np.nextafter(np.float32(0.5), np.float32(1))), float(np.nextafter(np.float32(0.5), np.float32(0)))
    for start, kw, want in ((0.0, dict(p_on=0.5, p_off=0.2), 1), (0.0, dict(p_on=up, p_off=0.2), 0),
                            (1.0, dict(p_on=0.8, p_off=0.5), 0), (1.0, dict(p_on=0.8, p_off=down), 1)):
        cfg = _cfg(alpha=1.0, var_f=1.0, **kw)
        ff = np.zeros((n, 4, 3)); ff[:, :, 2] = cfg["mu_f"]
        for dtype in (np.float64, np.float32):
            ref = cr.detect(_model(), cfg, np.zeros((n, cr.NS)), base["quat"], base["dof"], base["base_pos"], foot_force_in=ff, reset=True,
                            p_init=np.full((n, 4), start), dtype=dtype)
            assert (ref["prob"] == 0.5).all() and (ref["contact"] == want).all(), (kw, dtype)
            bit = cr.INFO_TOUCHDOWN if start == 0.0 else cr.INFO_LIFTOFF
            assert ((ref["info"] & (15 * bit)) == (15 * bit if want != int(start) else 0)).all()


def test_non_finite_inputs_fail_the_env_alone():
    n, combo = 12, 0
    cfg = _cfg()
    raw = dict(_inputs(n, combo), state=F32(np.random.default_rng(7).uniform(0, 0.9, (n, cr.NS))))
    raw.pop("p_init")
    inp = _select(raw, combo)
    good = _ref(cfg, inp)
    bad = {k: np.array(v, copy=True) for k, v in inp.items()}
    _, _, dofs = cr.leg_jacobians(_model(), inp["quat"], inp["dof"], inp["base_pos"])
    bad["base_pos"][0, 1] = np.nan; bad["quat"][1, 3] = np.inf; bad["dof"][2, dofs[1, 2], 0] = np.nan; bad["tau_ext"][3, 6 + dofs[2, 0]] = np.inf
    bad["ground"][4, 3] = np.nan; bad["phase"][5] = np.inf; bad["state"][6, 4 * 2 + 0] = np.nan; bad["state"][7, 4 * 1 + 2] = np.inf
    bad["state"][8, 4 * 3 + 1] = np.nan
    bad["dof"][9, dofs[0, 0], 1] = np.nan; bad["tau_ext"][10, 2] = np.nan; bad["state"][11, 3] = np.nan     # never read: a velocity, a root row, the reserved float
    o = _ref(cfg, bad)
    assert o["info"][:9].tolist() == [cr.INFO_FAILED] * 9 and np.array_equal(o["info"][9:], good["info"][9:])
    for k in ("prob", "contact", "stance", "force", "terms"):
        assert (o[k][:9] == 0).all() and np.array_equal(o[k][9:], good[k][9:]), k
    assert np.array_equal(o["state"][:9], bad["state"][:9], equal_nan=True) and np.array_equal(o["state"][9:], good["state"][9:])


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output over every judged call and the thin foot-cases, the fp32 reference's discrete outputs held to fp64 on the way."""
    worst = {k: 0.0 for k in cr.OUTPUTS}
    thin = [0, 0]
    big = {k: 4.0 * 2 ** 30 for k in cr.OUTPUTS}                                       # the discrete checks; the ratios are measured, not bounded, here
    big["prob"] = CONST["prob"]                                                        # thinness is judged with the shipped constant
    seen = dict(touchdown=0, liftoff=0, early=0, late=0, straight=0)
    for n in SIZES:
        for combo in range(len(COMBOS)):
            cfg, calls = _chain(n, combo)
            for j, (inp, ref) in enumerate(calls):
                r32 = _ref(cfg, inp, dtype=np.float32)
                j_ = judge(cfg, ref)
                r = cr.ratios(r32, ref, j_["keep"])
                fo = j_["foot_ok"]
                assert np.array_equal(r32["contact"][fo], ref["contact"][fo]) and np.array_equal(r32["stance"][fo], ref["stance"][fo])
                worst = {k: max(worst[k], r[k]) for k in worst}
                thin[0] += int((~fo).sum()); thin[1] += fo.size
                for k in ("touchdown", "liftoff", "early", "late"):
                    seen[k] += int(ref["diag"][k].sum())
                if inp.get("tau_ext") is not None:
                    seen["straight"] += int((np.linalg.svd(ref["diag"]["jac"], compute_uv=False)[..., 2] < 0.01).sum())
    return worst, thin, seen


def test_fp32_yardstick_is_where_the_constants_came_from():
    worst, _, _ = _yardsticks()
    print("contact yardsticks: " + ", ".join(f"{k} K_ref = {worst[k]:.3g} (C = {CONST[k]:g})" for k in worst))
    for k in K_REF:
        assert abs(worst[k] - K_REF[k]) <= 0.25 * K_REF[k], (k, worst[k])
        assert 4 * worst[k] <= CONST[k]


def test_thin_cases_stay_under_the_cap():
    _, thin, seen = _yardsticks()
    print(f"contact thin foot-cases: {thin[0]} of {thin[1]}; events in the judged cases: {seen}")
    assert thin[0] <= THIN_CAP * thin[1], thin
    assert all(v > 0 for v in seen.values()), seen                                     # and the cases are not vacuous


@functools.lru_cache(maxsize=None)
def _kernel_assembly():
    """csrc/wbc_contact_kernel.hip compiled to gfx950 assembly with the build's own flags."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    source = "wbc_contact_kernel.hip"
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "contact.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        return open(out).read()


def test_contact_kernel_codegen():
    """One kernel, no scratch, no LDS, a single wavefront per workgroup and no s_barrier, at most 128 VGPRs."""
    import re
    text = _kernel_assembly()
    assert text.count(".amdhsa_kernel ") == 1
    entry = text[text.index("amdhsa.kernels:"):]
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))          # noqa: E731
    assert re.search(r"\.name:\s+wbc_contact_detect_kernel\n", entry)
    print(f"wbc_contact_detect_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64
    assert meta("group_segment_fixed_size") == 0 and meta("vgpr_count") <= 128
    body = text[text.index("\nwbc_contact_detect_kernel:"):]
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


_SHAPES = {"state": ((cr.NS,), torch.float32), "prob": ((4,), torch.float32), "contact": ((4,), torch.uint8), "stance": ((4,), torch.uint8),
           "force": ((4, 3), torch.float32), "terms": ((4, 4), torch.float32), "info": ((), torch.int32)}


def _sent(dtype):
    return {torch.float32: SENTINEL, torch.int32: ISENTINEL, torch.uint8: USENTINEL}[dtype]


def _load_sim(env, inp):
    """The sim's own root and joint state from the inputs."""
    root = env.sim.tensor("ROOT_STATES").clone()
    root[:, 0, 0:3] = _dev(inp["base_pos"]); root[:, 0, 3:7] = _dev(inp["quat"])
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(_dev(inp["dof"]))
    torch.cuda.synchronize()


def _call(env, cfg, inp, which=_OUTS, null=(), tensors=None, strides=None):
    """A direct C-ABI call into sentinel-framed buffers (the state starts from inp's); returns {name: [n, ...] tensor} of the state and the
    outputs asked for. The inputs named in `null`, and those missing from inp, are handed over as NULL; `tensors` replaces device inputs
    (strided views), `strides` their strides."""
    n = env.num_envs
    size = {k: int(np.prod(s, dtype=np.int64)) for k, (s, _) in _SHAPES.items()}
    bufs = {}
    for name in ("state",) + tuple(which):
        dt = _SHAPES[name][1]
        bufs[name] = torch.full((n * size[name] + 8,), _sent(dt), dtype=dt, device="cuda")
    bufs["state"][:n * cr.NS] = _dev(inp["state"]).reshape(-1)
    reset = inp.get("reset")
    flags = abi.CONTACT_RESET if reset is True else 0
    tens = {k: _dev(inp.get(k)) for k in _INPUTS if k not in null and k != "reset_mask"}
    tens["reset_mask"] = _dev(reset, torch.int32) if reset is not None and reset is not True else None
    tens.update(tensors or {})
    st = dict(dict(tau_ext=26, phase=1), **(strides or {}))
    ptr = lambda d, k: d[k].data_ptr() if d.get(k) is not None and d[k].numel() > 0 else None     # noqa: E731
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_contact_detect(env.sim.h, C.byref(c), ptr(tens, "quat"), ptr(tens, "dof"), ptr(tens, "base_pos"), ptr(tens, "tau_ext"),
                                          st["tau_ext"], ptr(tens, "foot_force"), ptr(tens, "normal"), ptr(tens, "ground"), ptr(tens, "phase"),
                                          st["phase"], ptr(tens, "reset_mask"), ptr(tens, "p_init"), flags, ptr(bufs, "state"),
                                          *[ptr(bufs, k) for k in _OUTS], None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert bool((b[n * size[name]:] == _sent(_SHAPES[name][1])).all()), name
    return {name: b[:n * size[name]].view((n,) + _SHAPES[name][0]).clone() for name, b in bufs.items()}


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_entry_against_fp64(n):
    env = _env(n)
    worst = {k: 0.0 for k in cr.OUTPUTS}
    for combo in range(len(COMBOS)):
        cfg, calls = _chain(n, combo)
        for j, (inp, ref) in enumerate(calls):
            got = _np(_call(env, cfg, inp))
            assert all(np.isfinite(got[k].astype(np.float64)).all() for k in got)
            r, _, _ = compare(got, ref, cfg, who=(n, COMBOS[combo], j))
            worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"contact n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")


@pytest.mark.gpu
def test_outputs_one_at_a_time_two_runs_a_graph_and_the_sim_untouched():
    n, combo = 130, 0
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
    # a captured graph replays the eager bits
    c = _make_cfg(cfg)
    t = {k: _dev(inp[k]) for k in ("quat", "dof", "base_pos", "tau_ext", "ground", "phase")}
    state0 = _dev(inp["state"])
    state = state0.clone()
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _SHAPES.items() if k != "state"}
    call = lambda: env.sim.contact_detect(c, state, **t, **outs)                       # noqa: E731
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
def test_null_inputs_and_strided_views_give_the_same_bits():
    from wbc_amd.envs import FootstepPlanner  # noqa: F401
    n, combo = 130, 0
    env = _env(n)
    cfg, calls = _chain(n, combo)
    inp, ref = calls[3]
    _load_sim(env, inp)
    want = _call(env, cfg, inp)
    # NULL quat / dof / base_pos: the sim's tensors, which hold the same floats
    for null in (("quat",), ("dof",), ("base_pos",), ("quat", "dof", "base_pos")):
        got = _call(env, cfg, inp, null=null)
        assert all(torch.equal(got[k], want[k]) for k in want), null
    compare(_np(got), ref, cfg, who="NULL inputs")
    # tau_ext as the residual plane of an observer state [N, 2, 26], phase as element 0 of a planner state [N, 32]
    obs = torch.full((n, 2, 26), float("nan"), device="cuda")
    obs[:, 1] = _dev(inp["tau_ext"])
    plan = torch.full((n, abi.FOOTSTEP_NS), float("nan"), device="cuda")
    plan[:, 0] = _dev(inp["phase"])
    got = _call(env, cfg, inp, tensors=dict(tau_ext=obs[:, 1], phase=plan[:, 0]), strides=dict(tau_ext=52, phase=abi.FOOTSTEP_NS))
    assert all(torch.equal(got[k], want[k]) for k in want)
    # and through WbcSim.contact_detect, which takes the views as they stand
    state = _dev(inp["state"])
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _SHAPES.items() if k != "state"}
    env.sim.contact_detect(_make_cfg(cfg), state, tau_ext=obs[:, 1], ground=_dev(inp["ground"]), phase=plan[:, 0], **outs)
    torch.cuda.synchronize()
    assert torch.equal(state, want["state"]) and all(torch.equal(outs[k], want[k]) for k in outs)
    assert bool(torch.isnan(obs[:, 0]).all()) and bool(torch.isnan(plan[:, 1:]).all())


@pytest.mark.gpu
def test_failed_envs_write_zeros_and_keep_their_state():
    n, combo = 130, 0
    env = _env(n)
    cfg, calls = _chain(n, combo)
    inp, _ = calls[1]
    bad = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in inp.items()}
    _, _, dofs = cr.leg_jacobians(_model(), inp["quat"], inp["dof"], inp["base_pos"])
    rows = [0, 1, 15, 16, 64, 65, 100, 129]
    bad["base_pos"][0, 1] = np.nan; bad["quat"][1, 3] = np.inf; bad["dof"][15, dofs[1, 2], 0] = np.nan; bad["tau_ext"][16, 6 + dofs[2, 0]] = np.inf
    bad["ground"][64, 3] = np.nan; bad["phase"][65] = np.inf; bad["state"][100, 4 * 2 + 0] = np.nan; bad["state"][129, 4 * 1 + 2] = np.inf
    ref = _ref(cfg, bad)
    assert ref["info"][rows].tolist() == [cr.INFO_FAILED] * len(rows)
    got = _call(env, cfg, bad)
    plain = _call(env, cfg, inp)
    ok = torch.tensor(np.delete(np.arange(n), rows), device="cuda")
    for k in got:                                                                      # their neighbours: the bits of the launch without them
        assert torch.equal(got[k][ok], plain[k][ok]), k
    g = _np(got)
    assert g["info"][rows].tolist() == [cr.INFO_FAILED] * len(rows)
    for k in _OUTS[:-1]:
        assert (g[k][rows] == 0).all(), k
    assert np.array_equal(g["state"][rows], bad["state"][rows].astype(np.float32), equal_nan=True)


@pytest.mark.gpu
def test_detector_on_the_simulator_feeds_the_estimator_and_the_controller():
    """8 envs on the plane: 50 control steps of standing under a joint PD, then 25 with the front-left leg lifted. The kernel is held, call by
    call on the logged inputs and from its own previous state, to the fp64 reference within 4 x the fp32 reference's own largest ratio on
    those inputs (rounded up to a power of two); det.prob and det.stance feed BaseStateEstimator.update and whole_body_controller to finite
    outputs and defined status words. The agreement with the simulator's force sensors is printed, not asserted."""
    from wbc_amd.envs import ContactDetector
    n = 8
    env = _env(n, seed=9)
    env.reset()
    env.reset_buf.zero_()
    est = env.base_state_estimator()
    det = env.contact_detector()
    assert isinstance(det, ContactDetector) and det.observer_state is not env.sim.__dict__.get("_observer_state")
    assert det.tau_ext.data_ptr() == det.observer_state.data_ptr() + 4 * 26 and det.tau_ext.stride(0) == 52
    cfg = {k: ([float(v) for v in det.cfg.offset] if k == "offset" else float(getattr(det.cfg, k))) for k in cr.CFG_FIELDS}
    q0 = env.default_dof_pos.to(torch.float32).reshape(1, -1).expand(n, -1).clone()
    _, _, _, dofs = er.leg_kinematics(_model(), q0[:1].cpu().numpy().astype(np.float64), None, jac=True)
    decimation = int(env.cfg.control.decimation)
    known = (cr.INFO_RESET | cr.INFO_FAILED | 15 * cr.INFO_TOUCHDOWN | 15 * cr.INFO_LIFTOFF | 15 * cr.INFO_EARLY | 15 * cr.INFO_LATE |
             15 * cr.INFO_FORCE_SINGULAR)
    logs, agree, fz = [], [], []
    for step in range(75):
        target = q0.clone()
        if step >= 50:                                                                 # fold the front-left leg: thigh forward, knee bent further
            target[:, dofs[0, 1]] += 0.6
            target[:, dofs[0, 2]] -= 0.7
        ds = env.sim.tensor("DOF_STATE")
        tau = (40.0 * (target - ds[:, :, 0]) - 1.0 * ds[:, :, 1]).clamp(-30.0, 30.0).contiguous()
        env.sim.set_dof_forces(tau)
        for _ in range(decimation):
            env.sim.simulate()
        state_before = det.state.clone()
        det.update(torques=tau)
        est.update(contact=det.prob)
        t2, nudot, lam, info = env.whole_body_controller(stance=det.stance)
        torch.cuda.synchronize()
        li = det.last_inputs
        root = env.sim.tensor("ROOT_STATES")
        logs.append(dict(state=state_before.cpu().numpy().astype(np.float64), quat=root[:, 0, 3:7].cpu().numpy().astype(np.float64),
                         base_pos=root[:, 0, 0:3].cpu().numpy().astype(np.float64), dof=env.sim.tensor("DOF_STATE").cpu().numpy().astype(np.float64),
                         tau_ext=li["tau_ext"].cpu().numpy().astype(np.float64), ground=li["ground"].cpu().numpy().astype(np.float64),
                         reset=li["reset_mask"].cpu().numpy(), got=_np(dict(state=det.state, prob=det.prob, contact=det.contact, stance=det.stance,
                                                                           force=det.foot_forces, terms=det.terms, info=det.info))))
        for name in ("state", "prob", "foot_forces", "terms"):
            assert bool(torch.isfinite(getattr(det, name)).all()), (step, name)
        assert bool(torch.isfinite(est.x).all()) and bool(torch.isfinite(t2).all()) and bool(torch.isfinite(nudot).all())
        assert bool(((det.info & ~known) == 0).all()) and bool((det.info & cr.INFO_FAILED == 0).all())
        assert set(info["status"].cpu().tolist()) <= {0, 1, 2}
        assert set(est.status.cpu().tolist()) <= {abi.ESTIMATOR_STATUS_OK, abi.ESTIMATOR_STATUS_RESET, abi.ESTIMATOR_STATUS_FAILED}
        assert set(det.contact.cpu().unique().tolist()) <= {0, 1} and set(det.stance.cpu().unique().tolist()) <= {0, 1}
        assert torch.equal(det.stance, det.contact)                                    # no planner: no schedule
        truth = env.get_foot_contacts()
        agree.append(float((det.contact.bool() == truth.bool()).float().mean()))
        fz.append((float(det.foot_forces[:, :, 2].sum(1).mean()), float(env.sim.tensor("FORCE_SENSOR")[:, :, 2].sum(1).mean())))
    # the kernel against the reference on the logged inputs; the yardstick from the reference's fp32 run on the same inputs
    k_sim = {k: 0.0 for k in cr.OUTPUTS}
    refs = []
    for lg in logs:
        inp = dict(lg, p_init=None)
        ref = _ref(cfg, inp)
        r32 = _ref(cfg, inp, dtype=np.float32)
        keep = judge(cfg, ref)["keep"]
        r = cr.ratios(r32, ref, keep)
        k_sim = {k: max(k_sim[k], r[k]) for k in k_sim}
        refs.append(ref)
    const = {k: _pow2(max(v, 0.25)) for k, v in k_sim.items()}
    worst = {k: 0.0 for k in cr.OUTPUTS}
    for step, (lg, ref) in enumerate(zip(logs, refs)):
        r, _, _ = compare(lg["got"], ref, cfg, const=dict(const, prob=max(const["prob"], CONST["prob"])), who=("sim", step))
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"contact on the simulator: K_ref {k_sim}, C {const}, kernel's largest ratios {worst}")
    print(f"contact on the simulator: agreement of det.contact with get_foot_contacts: standing (steps 25..49) {np.mean(agree[25:50]):.3f}, "
          f"leg lifted (steps 60..74) {np.mean(agree[60:]):.3f}; sum f_z estimated / sensed at step 49: {fz[49][0]:.1f} / {fz[49][1]:.1f} N, "
          f"at step 74: {fz[74][0]:.1f} / {fz[74][1]:.1f} N")
    # a partial reset leaves the others as they are
    keep_state = det.state.clone()
    det.reset(env_ids=[1, 5])
    torch.cuda.synchronize()
    rest = [0, 2, 3, 4, 6, 7]
    assert torch.equal(det.state[rest], keep_state[rest]) and bool((det.info[[1, 5]] & cr.INFO_RESET != 0).all())
    assert bool((det.observer_state[[1, 5], 1] == 0).all())
