"""The leg controller (wbc_sim_leg_control: wbc_leg_control_kernel in csrc/wbc_legctl_kernel.hip; the text both implement is the comment in
include/wbc_sim.h). The CPU tests pin the fp64 restatement of tests/leg_control_reference.py to properties of the equations and measure the
fp32 yardstick; the GPU tests hold the kernel to the reference entry by entry.

Bound: every entry of a continuous output satisfies |kernel - ref| <= C 2^-24 mag, mag as leg_control_reference's docstring lists it. C is
4 x K_ref rounded up to a power of two, K_ref the largest ratio of the reference run in fp32 against itself in fp64 over the judged cases
(SIZES x COMBOS), measured on the CPU and asserted there; it never comes from the kernel.

    output      K_ref    kernel's largest ratio on an MI355X    C
    tau         13.7     13.7  (n = 16)                         64
    leg_force   2.42     3.21  (n = 17)                         16
    foot        3.06     4.27  (n = 130)                        16

The kernel's tau ratio equals K_ref to every digit: at the worst entry (a feed-forward torque at a nearly straight knee) the kernel and
the reference's fp32 run round alike. Its leg_force and foot ratios are above K_ref and inside C: the device's sincosf and the FMA
contraction of the walk differ from numpy's fp32. Thin cases: 0 of 10 740 (the cap is 1 %). On the simulator (8 envs in full stance,
forces and bias from whole_body_inverse_dynamics and inverse_dynamics, the yardstick measured in the test from the logged inputs): K_ref
21.0 / 0 / 1.06 (tau / leg_force / foot; leg_force is -f there, exact), C 128 / 1 / 8, the kernel 21.0 / 0 / 1.06, and the kernel's tau is
within 0.033 of the summed bound of that call's own torques.

The info bits match exactly except in THIN cases, judged from the fp64 reference alone (judge()): with the clip, a force component within
C_leg_force 2^-24 |f| of the edge it is compared with, or a stance input within 2^-24 of 0 (FORCE_CLIPPED asks for w > 0) or of 1 without
being that number (the planner's 0.0 and 1.0 are exact in every precision and are judged); with limits,
an unclamped torque within C_tau 2^-24 mag of +-limit. A thin leg's (or the arm's) bits are left out; the continuous outputs are judged
everywhere, since a clamp that goes the other way moves the value by no more than the bound. FF_SINGULAR needs a pivot that is not positive
at delta = 0, which rounding decides: it is pinned on the reference's factorisation alone, as FORCE_SINGULAR of wbc_sim_contact_detect was."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import contact_reference as cr
import estimator_reference as er
import leg_control_reference as lr
from wbc_amd import abi
from wbc_amd.abi import WbcLegControlCfg  # noqa: F401  (this file is about wbc_sim_leg_control: none of it means anything without the call)

F32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)   # noqa: E731
EPS = 2.0 ** -24
SENTINEL, ISENTINEL = 12345.0, 1234567
SIZES = (1, 15, 16, 17, 130)
# which optional inputs a case hands over: forces, swing_ref, stance, tau_bias, mass_matrix, acc_bias, arm_q_des, tau_limit, clip
COMBOS = ((1, 1, 1, 1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1, 1, 0, 0), (1, 1, 1, 1, 1, 0, 0, 1, 1), (1, 1, 1, 1, 0, 0, 1, 1, 0),
          (1, 0, 1, 1, 0, 0, 0, 1, 1), (1, 0, 0, 1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 1, 1, 0, 0, 0), (0, 1, 0, 0, 0, 0, 1, 1, 0),
          (0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 1, 1, 0, 1, 1), (0, 0, 1, 1, 0, 0, 1, 1, 0), (1, 1, 1, 0, 0, 0, 0, 0, 1))
_FLAGS = ("forces", "swing_ref", "stance", "tau_bias", "mass_matrix", "acc_bias", "arm_q_des", "tau_limit", "clip")
THIN_CAP = 0.01


def _pow2(x):
    return float(2 ** int(np.ceil(np.log2(x))))


# measured by test_fp32_yardstick_is_where_the_constants_came_from (the reference alone) / by the GPU tests on an MI355X (for the record)
K_REF = {"tau": 13.7, "leg_force": 2.42, "foot": 3.06}
K_GPU = {"tau": 13.7, "leg_force": 3.21, "foot": 4.27}
CONST = {k: _pow2(4 * v) for k, v in K_REF.items()}


@functools.lru_cache(maxsize=None)
def _model():
    return abi.load_default_model()


def _cfg(**kw):
    """The kernel receives the cfg as floats: the references use the same rounded values."""
    base = dict(kp=(400.0, 350.0, 500.0), kd=(8.0, 7.0, 10.0), kd_stance=0.2, damping=0.02, fz_min=0.0, fz_max=100.0, mu=0.5,
                kp_arm=(50.0, 50.0, 40.0, 20.0, 20.0, 10.0), kd_arm=(2.0, 2.0, 1.5, 1.0, 1.0, 0.5), arm_q_default=(0.0, 0.8, -0.9, 0.1, 0.3, -0.2))
    base.update(kw)
    return {k: (F32(base[k]).tolist() if n > 1 else float(np.float32(base[k]))) for k, n in zip(lr.CFG_FIELDS, lr.CFG_COUNTS)}


def _make_cfg(cfg, **kw):
    c = dict(cfg, **kw)
    return abi.WbcLegControlCfg(*[(abi.f32 * n)(*c[k]) if n > 1 else c[k] for k, n in zip(lr.CFG_FIELDS, lr.CFG_COUNTS)])


def _postures(n, rng):
    """Leg joints inside their limits; every fifth env has one leg within 1 degree of a straight knee (the calf joint at 0, outside its
    limits, where the leg Jacobian loses a direction and the damping decides the feed-forward)."""
    m = _model()
    dlo, dhi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    q = dlo + (dhi - dlo) * rng.uniform(0.2, 0.8, (n, 20))
    dofs = lr.dof_groups(m)[0]
    for e in range(0, n, 5):
        q[e, dofs[(e // 5) % 4, 2]] = np.deg2rad(rng.uniform(-1.0, 1.0))
    return q, dofs


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    """fp32-representable inputs: near-upright trunks at every heading that move and turn, foot forces that reach outside the friction
    pyramid, swing references a few centimetres from the feet, weights at 0, at 1 and between, limits that some torques reach."""
    m = _model()
    rng = np.random.default_rng(9100 + 131 * seed + n)
    b = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.25, 0.4, n)], axis=-1)
    yaw, rp = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.2, 0.2, (n, 2))
    quat = np.stack([np.sin(rp[:, 0] / 2) * np.cos(yaw / 2), np.sin(rp[:, 1] / 2) * np.cos(yaw / 2), np.sin(yaw / 2), np.cos(yaw / 2)], axis=-1)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    quat *= rng.uniform(0.8, 1.2, (n, 1))                                                # normalised in the call
    q, _ = _postures(n, rng)
    dof = F32(np.stack([q, rng.uniform(-2, 2, (n, 20))], axis=-1))
    b, quat = F32(b), F32(quat)
    v, w = F32(rng.uniform(-1, 1, (n, 3))), F32(rng.uniform(-1, 1, (n, 3)))
    P, _, _ = cr.leg_jacobians(m, quat, dof, b)
    forces = np.stack([rng.uniform(-40, 40, (n, 4)), rng.uniform(-40, 40, (n, 4)), rng.uniform(-20, 120, (n, 4))], axis=-1)
    swing = np.concatenate([P + rng.uniform(-0.05, 0.05, (n, 4, 3)), rng.uniform(-1, 1, (n, 4, 3)), rng.uniform(-20, 20, (n, 4, 3))], axis=-1)
    kind = rng.integers(0, 3, (n, 4))
    stance = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.uniform(-0.2, 1.2, (n, 4))))
    B = rng.uniform(-1, 1, (n, 26, 26))
    mm = 0.02 * np.einsum("nij,nkj->nik", B, B) + 0.02 * np.eye(26)
    return dict(base_pos=b, quat=quat, dof=dof, base_vel=v, ang_vel=w, forces=F32(forces), swing_ref=F32(swing), stance=F32(stance),
                tau_bias=F32(rng.uniform(-5, 5, (n, 26))), mass_matrix=F32(mm), acc_bias=F32(rng.uniform(-5, 5, (n, 27, 6))),
                arm_q_des=F32(rng.uniform(-1, 1, (n, 6))), tau_limit=F32(rng.uniform(5, 40, (n, 18))))


def _select(inp, combo):
    """(inputs handed over, clip) of a combo; the others are NULL."""
    flags = dict(zip(_FLAGS, COMBOS[combo]))
    out = {k: inp[k] for k in ("base_pos", "quat", "dof", "base_vel", "ang_vel")}
    out.update({k: inp[k] for k in _FLAGS[:-1] if flags[k]})
    return out, bool(flags["clip"])


def _ref(cfg, inp, clip=False, dtype=np.float64):
    return lr.control(_model(), cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=inp.get("forces"),
                      swing_ref=inp.get("swing_ref"), stance=inp.get("stance"), tau_bias=inp.get("tau_bias"), mass_matrix=inp.get("mass_matrix"),
                      acc_bias=inp.get("acc_bias"), arm_q_des=inp.get("arm_q_des"), tau_limit=inp.get("tau_limit"), clip=clip, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _case(n, combo):
    """(cfg, inputs, clip, fp64 reference), computed once and left unchanged."""
    cfg = _cfg()
    inp, clip = _select(_inputs(n), combo)
    return cfg, inp, clip, _ref(cfg, inp, clip)


def judge(cfg, ref, const=None):
    """From the fp64 reference alone: leg_ok [N, 4] and arm_ok [N], False where a bit of that leg (the arm) is thin."""
    const = CONST if const is None else const
    d = ref["diag"]
    n = d["w"].shape[0]
    leg_ok, arm_ok = np.ones((n, 4), dtype=bool), np.ones(n, dtype=bool)
    if d["edges"] is not None:
        fin, lim = d["edges"]["fin"], d["edges"]["lim"]
        tol = lambda x: const["leg_force"] * EPS * np.maximum(np.abs(x), 1e-30)        # noqa: E731
        for a in (0, 1):
            leg_ok &= (np.abs(fin[..., a] - lim) >= tol(lim)) & (np.abs(fin[..., a] + lim) >= tol(lim))
        for edge in (0.0, 1.0):                                                        # an input that IS 0 or 1 is exact in every precision: judged
            leg_ok &= (d["stance"] == edge) | (np.abs(d["stance"] - edge) >= EPS)
    if d["limits"] is not None:
        raw, lim = d["raw_tau"], d["limits"]
        near = np.abs(np.abs(raw) - lim) < const["tau"] * EPS * ref["mag"]["tau"]
        leg_ok &= ~near[:, d["dofs"]].any(-1)
        arm_ok &= ~near[:, d["arm"]].any(-1)
    return dict(leg_ok=leg_ok & ~d["failed"][:, None], arm_ok=arm_ok & ~d["failed"])


def _info_mask(j):
    bits = np.full(j["arm_ok"].shape[0], lr.INFO_FAILED, dtype=np.int64)
    per_leg = lr.INFO_FORCE_CLIPPED | lr.INFO_FF_SINGULAR | lr.INFO_SATURATED
    for i in range(4):
        bits |= np.where(j["leg_ok"][:, i], per_leg << i, 0)
    return bits | np.where(j["arm_ok"], lr.INFO_SATURATED << 4, 0)


def compare(got, ref, cfg, const=None, who=""):
    """Hold `got` (numpy, any float type) to the fp64 reference: the info bits exactly outside thin cases, every entry of the continuous
    outputs within the bound. Returns (the largest ratios, thin cases, cases)."""
    const = CONST if const is None else const
    j = judge(cfg, ref, const)
    bits = _info_mask(j)
    assert np.array_equal(np.asarray(got["info"]).astype(np.int64) & bits, ref["info"] & bits), who
    r = lr.ratios(got, ref)
    for k in lr.OUTPUTS:
        assert r[k] <= const[k], (who, k, r[k])
    fingers = ref["diag"]["fingers"]
    assert (np.asarray(got["tau"])[:, fingers] == 0).all(), who
    return r, int((~j["leg_ok"]).sum() + (~j["arm_ok"]).sum()), j["leg_ok"].size + j["arm_ok"].size


# ------------------------------------------------------------------------------------------------------------ CPU
_INPUTS = ("quat", "dof", "base_pos", "base_vel", "ang_vel", "forces", "swing_ref", "stance", "tau_bias", "mass_matrix", "acc_bias", "arm_q_des",
           "tau_limit")
_OUTS = ("tau", "leg_force", "foot", "info")
_NAMES = ("sim", "cfg", "quat", "dof", "base_pos", "base_vel", "ang_vel", "forces", "swing_ref", "stance", "tau_bias", "tau_bias_stride",
          "mass_matrix", "mass_matrix_stride", "acc_bias", "acc_bias_stride", "arm_q_des", "tau_limit", "flags") + _OUTS + ("stream",)


def _refusals(base):
    """[(arguments that differ from the good call `base`, a word of the message)]: every refusal of wbc_sim_leg_control but the NULL sim."""
    good = _cfg()
    mk = lambda **kw: _make_cfg(good, **kw)                                          # noqa: E731
    nan, inf = float("nan"), float("inf")
    out = [(dict(cfg=None), b"NULL"), (dict(flags=2), b"flag"), (dict(flags=-1), b"flag")]
    for field, count in (("kp", 3), ("kd", 3), ("kp_arm", 6), ("kd_arm", 6)):
        for i in range(count):
            vec = lambda bad: [bad if k == i else good[field][k] for k in range(count)]   # noqa: E731
            out += [(dict(cfg=mk(**{field: vec(bad)})), field.split("_")[0].encode()) for bad in (-1.0, nan, inf)]
    for i in range(6):
        vec = lambda bad: [bad if k == i else good["arm_q_default"][k] for k in range(6)]   # noqa: E731
        out += [(dict(cfg=mk(arm_q_default=vec(bad))), b"arm_q_default") for bad in (nan, inf, -inf)]
    out += [(dict(cfg=mk(**{field: bad})), field.encode()) for field in ("kd_stance", "damping", "fz_min", "mu") for bad in (-1e-3, nan, inf)]
    out += [(dict(cfg=mk(fz_max=bad)), b"fz_max") for bad in (nan, inf, -1.0)] + [(dict(cfg=mk(fz_min=10.0, fz_max=9.0)), b"fz_max")]
    out += [(dict(tau_bias_stride=bad), b"tau_bias_stride") for bad in (25, 0, -26)]
    out += [(dict(mass_matrix_stride=bad), b"mass_matrix_stride") for bad in (675, 0, -676)]
    out += [(dict(acc_bias_stride=bad), b"acc_bias_stride") for bad in (161, 0, -162)]
    out += [({k: base[k] + off}, b"aligned") for k in _INPUTS + _OUTS for off in (1, 2, 3)]
    out += [(dict(swing_ref=None), b"without swing_ref")]
    out += [(dict(tau=None, leg_force=None, foot=None, info=None), b"every output is NULL")]
    return out


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_leg_control(*[C.byref(args[k]) if isinstance(args[k], abi.WbcLegControlCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device():
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    import __graft_entry__ as g
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    assert "wbc_sim_leg_control" in EXPORTED_SYMBOLS and hasattr(L, "wbc_sim_leg_control")
    assert "wbc_legctl_kernel.hip" in g.SOURCES and "wbc_legctl.h" in g.HEADERS
    # the mirror against the header's struct: the same fields in the same order with the same counts, all floats
    header = open(g.ROOT + "/include/wbc_sim.h").read()
    body = re.search(r"typedef struct \{([^}]*)\} wbc_leg_control_cfg;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"float ([^;]*);", body):
        for name in decl.split(","):
            name = name.strip()
            count = int(re.search(r"\[(\d+)\]", name).group(1)) if "[" in name else 1
            fields.append((name.split("[")[0], count))
    assert [f for f, _ in fields] == list(lr.CFG_FIELDS) == [f for f, _ in abi.WbcLegControlCfg._fields_]
    assert [c for _, c in fields] == list(lr.CFG_COUNTS)
    assert C.sizeof(abi.WbcLegControlCfg) == 4 * sum(c for _, c in fields) == 4 * 29
    offsets, at = {}, 0
    for f, c in fields:
        offsets[f] = at
        at += 4 * c
    assert {f: getattr(abi.WbcLegControlCfg, f).offset for f, _ in fields} == offsets
    assert (abi.LEGCTL_CLIP, abi.LEGCTL_INFO_FAILED, abi.LEGCTL_INFO_FORCE_CLIPPED, abi.LEGCTL_INFO_FF_SINGULAR, abi.LEGCTL_INFO_SATURATED) == (
        lr.CLIP, lr.INFO_FAILED, lr.INFO_FORCE_CLIPPED, lr.INFO_FF_SINGULAR, lr.INFO_SATURATED)
    for name in ("CLIP", "INFO_FAILED", "INFO_FORCE_CLIPPED", "INFO_FF_SINGULAR", "INFO_SATURATED"):
        assert int(re.search(r"#define WBC_LEGCTL_%s (\d+)" % name, header).group(1)) == getattr(abi, "LEGCTL_" + name), name
    assert len(L.wbc_sim_leg_control.argtypes) == len(_NAMES)
    buf = (C.c_float * 16384)()
    p = C.addressof(buf)
    base = dict(sim=None, cfg=_make_cfg(_cfg()), flags=0, stream=None, tau_bias_stride=26, mass_matrix_stride=676, acc_bias_stride=162,
                **{k: p + 512 * (1 + i) for i, k in enumerate(_INPUTS + _OUTS)})
    refusals = _refusals(base)
    assert len(refusals) > 120
    zero = _make_cfg(_cfg(kp=(0, 0, 0), kd=(0, 0, 0), kd_stance=0.0, damping=0.0, fz_min=0.0, fz_max=0.0, mu=0.0, kp_arm=(0,) * 6, kd_arm=(0,) * 6))
    for kw, word in refusals + [(dict(), b"sim is NULL"), (dict(flags=abi.LEGCTL_CLIP), b"sim is NULL"), (dict(cfg=zero), b"sim is NULL"),
                                (dict(tau_bias_stride=52, mass_matrix_stride=1000, acc_bias_stride=200), b"sim is NULL"),
                                (dict(tau_bias=None, tau_bias_stride=0, mass_matrix=None, mass_matrix_stride=0, acc_bias=None, acc_bias_stride=0),
                                 b"sim is NULL"),                                      # a stride without its pointer is not looked at
                                (dict(mass_matrix=None, swing_ref=None), b"sim is NULL"),
                                (dict(tau=None, leg_force=None, foot=None), b"sim is NULL"),
                                ({k: None for k in _INPUTS}, b"sim is NULL")]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_leg_control: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def _regular(n, seed):
    """Inputs without the straight knees."""
    inp = {k: np.array(v, copy=True) for k, v in _inputs(n, seed).items()}
    m = _model()
    rng = np.random.default_rng(seed)
    dlo, dhi = np.asarray(m.dof_lower), np.asarray(m.dof_upper)
    inp["dof"][:, :, 0] = F32(dlo + (dhi - dlo) * rng.uniform(0.2, 0.8, (n, 20)))
    return inp


def test_feed_forward_is_the_operational_space_inertia_times_the_acceleration():
    """delta = 0 and a regular J_i: tau_ff = J_i^T (J_i M_i^-1 J_i^T)^-1 a to fp64 rounding, through control() with everything else off."""
    n = 40
    inp = _regular(n, 1)
    cfg = _cfg(damping=0.0, kp=(0, 0, 0), kd=(0, 0, 0), kd_stance=0.0, kp_arm=(0,) * 6, kd_arm=(0,) * 6)
    stance = np.zeros((n, 4))
    o = lr.control(_model(), cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], swing_ref=inp["swing_ref"], stance=stance,
                   mass_matrix=inp["mass_matrix"], acc_bias=inp["acc_bias"])
    d = o["diag"]
    J, dofs = d["jac"], d["dofs"]
    assert np.linalg.cond(J).max() < 1e4 and not d["singular"].any()
    idx = 6 + dofs
    Mi = inp["mass_matrix"][:, idx[:, :, None], idx[:, None, :]]
    a = inp["swing_ref"][:, :, 6:9] - inp["acc_bias"][:, d["feet_rb"], 0:3]
    Lam = np.linalg.inv(J @ np.linalg.inv(Mi) @ np.swapaxes(J, -1, -2))
    want = np.einsum("nfik,nfij,nfj->nfk", J, Lam, a)
    got = o["tau"][:, dofs]
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-9 * scale * np.linalg.cond(J).max(), np.abs(got - want).max()
    assert np.allclose(J @ d["qdd"][..., None], a[..., None], rtol=0, atol=1e-9 * np.abs(a).max() * np.linalg.cond(J).max())


def test_full_stance_satisfies_the_joint_rows_of_the_whole_body_equations():
    """w = 1, no swing inputs: tau_leg = bias - J_i^T f. With bias = M nudot + h (inverse_dynamics_reference) and f = lambda this is the
    joint rows of M nudot + h = S^T tau + sum J^T lambda with the whole-body Jacobian (whole_body_reference): tau_j = (M nudot + h)_j -
    (J^T lambda)_j for random nudot and lambda, which ties the leg Jacobians, their signs and the DoF rows to the whole-body model."""
    import inverse_dynamics_reference as idr
    import whole_body_reference as wb
    m = _model()
    n = 6
    inp = _inputs(n, 2)
    rng = np.random.default_rng(3)
    cfg = _cfg(kd_stance=0.0, kp_arm=(0,) * 6, kd_arm=(0,) * 6)
    legs, arm, fingers, feet_rb, _ = lr.dof_groups(m)
    lam = rng.uniform(-50, 50, (n, 4, 3))
    bias, want = np.zeros((n, 26)), np.zeros((n, 26))
    for e in range(n):
        quat = inp["quat"][e] / np.linalg.norm(inp["quat"][e])
        nu = np.r_[inp["base_vel"][e], inp["ang_vel"][e], inp["dof"][e, :, 1]]
        nudot = rng.uniform(-3, 3, 26)
        bias[e], _ = idr.inverse_dynamics(m, inp["base_pos"][e], quat, inp["dof"][e, :, 0], nu, nudot)
        Jw = wb.jacobian(m, inp["base_pos"][e], quat, inp["dof"][e, :, 0])[feet_rb, 0:3]            # [4, 3, 26]
        want[e] = bias[e] - np.einsum("fic,fi->c", Jw, lam[e])
    o = lr.control(m, cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=lam, tau_bias=bias)
    live = np.r_[legs.reshape(-1), arm]
    assert np.abs(o["tau"][:, live] - want[:, 6 + live]).max() <= 1e-10 * np.abs(want).max()
    assert (o["tau"][:, fingers] == 0).all() and np.array_equal(o["leg_force"], -lam) and (o["info"] == 0).all()


def test_swing_on_its_reference_at_rest_leaves_the_bias():
    """w = 0, the foot on its reference with the reference's velocity, a = 0: tau_leg = bias."""
    n = 20
    inp = _inputs(n, 3)
    cfg = _cfg(kp_arm=(0,) * 6, kd_arm=(0,) * 6)
    first = _ref(cfg, dict(inp, forces=None, swing_ref=None, stance=None, tau_bias=None, mass_matrix=None, acc_bias=None, tau_limit=None))
    ab = inp["acc_bias"]
    swing = np.concatenate([first["foot"], ab[:, first["diag"]["feet_rb"], 0:3]], axis=-1)          # acc_ref = acc_bias: a = 0
    o = lr.control(_model(), cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=inp["forces"], swing_ref=swing,
                   stance=np.zeros((n, 4)), tau_bias=inp["tau_bias"], mass_matrix=inp["mass_matrix"], acc_bias=ab)
    live = np.r_[first["diag"]["dofs"].reshape(-1), first["diag"]["arm"]]
    assert np.array_equal(o["tau"][:, live], inp["tau_bias"][:, 6 + live]) and (o["leg_force"] == 0).all()


def test_jacobian_and_foot_velocity_are_derivatives_of_the_foot_position():
    """J_i from central differences of the reference's own forward kinematics; pd_i from the time difference of p_i along a motion with
    the given v, angular velocity and joint rates."""
    n, h = 12, 1e-6
    inp = _inputs(n, 4)
    cfg = _cfg()
    m = _model()

    def foot(quat, dof, b):
        return lr.control(m, cfg, quat, dof, b, inp["base_vel"], inp["ang_vel"])["foot"][:, :, 0:3]
    base = lr.control(m, cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"])
    J, dofs = base["diag"]["jac"], base["diag"]["dofs"]
    for f in range(4):
        for k in range(3):
            dp, dm = np.array(inp["dof"]), np.array(inp["dof"])
            dp[:, dofs[f, k], 0] += h; dm[:, dofs[f, k], 0] -= h
            col = (foot(inp["quat"], dp, inp["base_pos"]) - foot(inp["quat"], dm, inp["base_pos"]))[:, f] / (2 * h)
            assert np.abs(col - J[:, f, :, k]).max() < 1e-8
    # the motion: b + h v, R <- exp(h [w]x) R, q + h qd
    qn = inp["quat"] / np.linalg.norm(inp["quat"], axis=1, keepdims=True)

    def moved(s):
        th = s * inp["ang_vel"]
        ang = np.linalg.norm(th, axis=1, keepdims=True)
        dq = np.concatenate([th / np.maximum(ang, 1e-300) * np.sin(ang / 2), np.cos(ang / 2)], axis=1)            # xyzw
        x1, y1, z1, w1 = dq.T
        x2, y2, z2, w2 = qn.T
        q = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                      w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], axis=1)
        dof = np.array(inp["dof"]); dof[:, :, 0] += s * dof[:, :, 1]
        return foot(q, dof, inp["base_pos"] + s * inp["base_vel"])
    pd = (moved(h) - moved(-h)) / (2 * h)
    assert np.abs(pd - base["foot"][:, :, 3:6]).max() < 1e-7


def test_clip_is_the_mpc_output_rule():
    """The identity inside the pyramid; f_z to [fz_min, fz_max] and then f_x, f_y to +-mu f_z; the bit exactly where a component changed
    and the weight is positive."""
    n = 64
    inp = _inputs(n, 5)
    cfg = _cfg()
    f = np.array(inp["forces"])
    f[:16, :, 2] = np.abs(f[:16, :, 2]).clip(1, 99); f[:16, :, 0:2] = f[:16, :, 0:2].clip(-0.4, 0.4) * f[:16, :, 2:3]     # inside
    stance = np.array(inp["stance"]); stance[16:24] = 0.0; stance[24:32] = -0.5
    o = lr.control(_model(), cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=f, stance=stance, clip=True)
    plain = lr.control(_model(), cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=f, stance=stance)
    w = np.clip(stance, 0, 1)
    fz = np.clip(f[..., 2], cfg["fz_min"], cfg["fz_max"])
    want = np.stack([np.clip(f[..., 0], -cfg["mu"] * fz, cfg["mu"] * fz), np.clip(f[..., 1], -cfg["mu"] * fz, cfg["mu"] * fz), fz], axis=-1)
    assert np.array_equal(o["leg_force"], -w[..., None] * want)
    assert np.array_equal(o["leg_force"][:16], plain["leg_force"][:16]) and (o["info"][:16] == 0).all()
    changed = (want != f).any(-1) & (w > 0)
    assert np.array_equal(o["info"], (changed * (lr.INFO_FORCE_CLIPPED << np.arange(4))).sum(-1))
    assert (o["info"][16:32] == 0).all() and changed[32:].any() and (plain["info"] == 0).all()
    assert (want[..., 2] >= 0).all() and (np.abs(want[..., 0:2]) <= cfg["mu"] * want[..., 2:3]).all()


def test_damped_feed_forward_stays_bounded_at_a_straight_knee():
    """delta > 0: |qdd| <= |a| / (2 delta), the knee exactly straight included; FF_SINGULAR from the factorisation alone."""
    n = 50
    inp = {k: np.array(v, copy=True) for k, v in _inputs(n, 6).items()}
    dofs = lr.dof_groups(_model())[0]
    inp["dof"][::2, dofs[:, 2], 0] = 0.0                                               # every leg of every second env exactly straight
    for delta in (0.02, 0.1, 1e-3):
        o = lr.control(_model(), _cfg(damping=delta), inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], swing_ref=inp["swing_ref"],
                       stance=np.zeros((n, 4)), mass_matrix=inp["mass_matrix"], acc_bias=inp["acc_bias"])
        a = inp["swing_ref"][:, :, 6:9] - inp["acc_bias"][:, o["diag"]["feet_rb"], 0:3]
        assert not o["diag"]["singular"].any()
        assert (np.linalg.norm(o["diag"]["qdd"], axis=-1) <= np.linalg.norm(a, axis=-1) / (2 * np.float32(delta)) * (1 + 1e-9)).all()
        assert np.linalg.svd(o["diag"]["jac"][::2], compute_uv=False)[..., 2].max() < 1e-6
    # the factorisation alone: a rank-deficient J at delta = 0 has a pivot that is not positive, and the feed-forward is then left out
    J = np.zeros((3, 3, 3)); J[0] = np.diag([1.0, 1.0, 0.0]); J[1] = np.eye(3); J[2] = np.array([[1.0, 2.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    M = np.broadcast_to(np.eye(3), (3, 3, 3))
    t, _, ok, mag = lr.feed_forward(J, M, np.ones((3, 3)), 0.0)
    assert ok.tolist() == [False, True, False] and (t[~ok] == 0).all() and (mag[~ok] == 0).all() and np.allclose(t[1], 1.0)
    t, _, ok, _ = lr.feed_forward(J, M, np.ones((3, 3)), 0.5)
    assert ok.all()
    with np.errstate(all="ignore"):
        t, _, ok, _ = lr.feed_forward(J * np.array([1.0, np.nan, np.inf])[:, None, None], M, np.ones((3, 3)), 0.5)
    assert ok.tolist() == [True, False, False]
    # and control() turns it into the bit: an exactly straight knee at delta = 0 in fp64 is singular or enormous, never silently wrong
    o = lr.control(_model(), _cfg(damping=0.0), inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], swing_ref=inp["swing_ref"],
                   stance=np.zeros((n, 4)), mass_matrix=inp["mass_matrix"])
    sing = o["diag"]["singular"]
    assert np.array_equal(o["info"], (sing * (lr.INFO_FF_SINGULAR << np.arange(4))).sum(-1)) and not sing[1::2].any()


def test_blend_is_linear_in_the_weight_and_the_stance_damping_acts_through_it():
    n = 30
    inp = _inputs(n, 7)
    cfg = _cfg(kp_arm=(0,) * 6, kd_arm=(0,) * 6)
    run = lambda w, c=cfg: lr.control(_model(), c, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=inp["forces"],   # noqa: E731
                                      swing_ref=inp["swing_ref"], stance=np.full((n, 4), w), tau_bias=inp["tau_bias"], mass_matrix=inp["mass_matrix"],
                                      acc_bias=inp["acc_bias"])
    t0, t1, th = run(0.0), run(1.0), run(0.3)
    scale = max(np.abs(t0["tau"]).max(), np.abs(t1["tau"]).max())
    assert np.abs(th["tau"] - (0.7 * t0["tau"] + 0.3 * t1["tau"])).max() <= 1e-12 * scale
    assert np.abs(th["leg_force"] - (0.7 * t0["leg_force"] + 0.3 * t1["leg_force"])).max() <= 1e-12 * np.abs(t0["leg_force"]).max()
    assert np.array_equal(run(-3.0)["tau"], t0["tau"]) and np.array_equal(run(7.0)["tau"], t1["tau"])            # clamped
    nod = _cfg(kd_stance=0.0, kp_arm=(0,) * 6, kd_arm=(0,) * 6)
    assert np.array_equal(run(0.0, nod)["tau"], t0["tau"])                              # no stance damping at w = 0
    dofs = t1["diag"]["dofs"]
    diff = (run(1.0, nod)["tau"] - t1["tau"])[:, dofs]
    assert np.abs(diff - cfg["kd_stance"] * inp["dof"][:, dofs, 1]).max() <= 1e-12 * scale


def test_arm_rows_are_the_joint_pd_and_limits_clamp():
    n = 40
    inp = _inputs(n, 8)
    cfg = _cfg()
    m = _model()
    o = lr.control(m, cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=inp["forces"], tau_bias=inp["tau_bias"],
                   arm_q_des=inp["arm_q_des"])
    arm = o["diag"]["arm"]
    assert arm.tolist() == sorted(arm.tolist()) and len(arm) == 6
    want = inp["tau_bias"][:, 6 + arm] + np.array(cfg["kp_arm"]) * (inp["arm_q_des"] - inp["dof"][:, arm, 0]) - np.array(cfg["kd_arm"]) * inp["dof"][:, arm, 1]
    assert np.abs(o["tau"][:, arm] - want).max() <= 1e-13 * np.abs(want).max()
    d = lr.control(m, cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=inp["forces"], tau_bias=inp["tau_bias"])
    want = inp["tau_bias"][:, 6 + arm] + np.array(cfg["kp_arm"]) * (np.array(cfg["arm_q_default"]) - inp["dof"][:, arm, 0]) - np.array(cfg["kd_arm"]) * inp["dof"][:, arm, 1]
    assert np.abs(d["tau"][:, arm] - want).max() <= 1e-13 * np.abs(want).max()
    # limits: |tau| <= limit, the bits exactly where a torque changed; the limit's column is the DoF's rank among the 18 revolute joints
    lim = inp["tau_limit"]
    c = lr.control(m, cfg, inp["quat"], inp["dof"], inp["base_pos"], inp["base_vel"], inp["ang_vel"], forces=inp["forces"], tau_bias=inp["tau_bias"],
                   arm_q_des=inp["arm_q_des"], tau_limit=lim)
    dofs = o["diag"]["dofs"]
    live = np.sort(np.r_[dofs.reshape(-1), arm])
    assert live.tolist() == list(range(18))
    assert (np.abs(c["tau"][:, live]) <= lim).all()
    changed = c["tau"] != o["tau"]
    assert np.array_equal(c["tau"][~changed], o["tau"][~changed]) and np.array_equal(np.abs(c["tau"][:, live])[changed[:, live]], lim[changed[:, live]])
    want_bits = (changed[:, dofs].any(-1) * (lr.INFO_SATURATED << np.arange(4))).sum(-1) + changed[:, arm].any(-1) * (lr.INFO_SATURATED << 4)
    assert np.array_equal(c["info"], want_bits) and changed[:, dofs].any() and changed[:, arm].any() and (~changed[:, live]).any()
    assert (c["tau"][:, o["diag"]["fingers"]] == 0).all()


def test_non_finite_inputs_fail_the_env_alone():
    n = 16
    cfg = _cfg()
    inp, clip = _select(_inputs(n, 9), 0)
    good = _ref(cfg, inp, clip)
    bad = {k: np.array(v, copy=True) for k, v in inp.items()}
    legs, arm, fingers, feet_rb, _ = lr.dof_groups(_model())
    bad["base_pos"][0, 1] = np.nan; bad["quat"][1, 3] = np.inf; bad["dof"][2, legs[1, 2], 0] = np.nan; bad["dof"][3, legs[0, 0], 1] = np.inf
    bad["base_vel"][4, 0] = np.nan; bad["ang_vel"][5, 2] = np.nan; bad["forces"][6, 2, 1] = np.inf; bad["swing_ref"][7, 3, 8] = np.nan
    bad["stance"][8, 0] = np.nan; bad["tau_bias"][9, 6 + arm[3]] = np.nan; bad["mass_matrix"][10, 6 + legs[2, 0], 6 + legs[2, 2]] = np.nan
    bad["acc_bias"][11, feet_rb[1], 2] = np.inf; bad["arm_q_des"][12, 5] = np.nan; bad["tau_limit"][13, 4] = -1.0
    # never read: a root row of the bias, a finger's row, a mass-matrix entry across two legs, an angular row of acc_bias, a finger's joint
    bad["tau_bias"][14, 2] = np.nan; bad["tau_bias"][14, 6 + fingers[0]] = np.nan; bad["mass_matrix"][14, 6 + legs[0, 0], 6 + legs[1, 0]] = np.nan
    bad["acc_bias"][15, feet_rb[0], 4] = np.nan; bad["acc_bias"][15, 0, 0] = np.nan; bad["dof"][15, fingers[1], :] = np.nan
    o = _ref(cfg, bad, clip)
    assert o["info"][:14].tolist() == [lr.INFO_FAILED] * 14 and np.array_equal(o["info"][14:], good["info"][14:])
    for k in lr.OUTPUTS:
        assert (o[k][:14] == 0).all() and np.array_equal(o[k][14:], good[k][14:]), k


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref per output over every judged case, the thin cases and how often each bit occurs, the fp32 reference's bits held to fp64 on the way."""
    worst = {k: 0.0 for k in lr.OUTPUTS}
    thin = [0, 0]
    seen = dict(clipped=0, saturated_leg=0, saturated_arm=0, straight=0)
    for n in SIZES:
        for combo in range(len(COMBOS)):
            cfg, inp, clip, ref = _case(n, combo)
            r32 = _ref(cfg, inp, clip, dtype=np.float32)
            j = judge(cfg, ref)
            bits = _info_mask(j)
            assert np.array_equal(r32["info"] & bits, ref["info"] & bits), (n, combo)
            assert not ref["diag"]["failed"].any() and not ref["diag"]["singular"].any()
            r = lr.ratios(r32, ref)
            worst = {k: max(worst[k], r[k]) for k in worst}
            thin[0] += int((~j["leg_ok"]).sum() + (~j["arm_ok"]).sum()); thin[1] += j["leg_ok"].size + j["arm_ok"].size
            seen["clipped"] += int(ref["diag"]["clipped"].sum()); seen["saturated_leg"] += int(ref["diag"]["sat_leg"].sum())
            seen["saturated_arm"] += int(ref["diag"]["sat_arm"].sum())
            if inp.get("mass_matrix") is not None:
                seen["straight"] += int((np.linalg.svd(ref["diag"]["jac"], compute_uv=False)[..., 2] < 0.01).sum())
    return worst, thin, seen


def test_fp32_yardstick_is_where_the_constants_came_from():
    worst, _, _ = _yardsticks()
    print("leg control yardsticks: " + ", ".join(f"{k} K_ref = {worst[k]:.3g} (C = {CONST[k]:g})" for k in worst))
    for k in K_REF:
        assert abs(worst[k] - K_REF[k]) <= 0.25 * K_REF[k], (k, worst[k])
        assert 4 * worst[k] <= CONST[k] and CONST[k] == _pow2(4 * K_REF[k])


def test_thin_cases_stay_under_the_cap():
    _, thin, seen = _yardsticks()
    print(f"leg control thin cases: {thin[0]} of {thin[1]}; bits and straight knees in the judged cases: {seen}")
    assert thin[0] <= THIN_CAP * thin[1], thin
    assert all(v > 0 for v in seen.values()), seen                                     # and the cases are not vacuous


@functools.lru_cache(maxsize=None)
def _kernel_assembly():
    """csrc/wbc_legctl_kernel.hip compiled to gfx950 assembly with the build's own flags."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    source = "wbc_legctl_kernel.hip"
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "legctl.s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        return open(out).read()


def test_leg_control_kernel_codegen():
    """From the compiler's metadata: one kernel, no scratch, no LDS, a single wavefront per workgroup, at most 128 VGPRs."""
    text = _kernel_assembly()
    entry = text[text.index("amdhsa.kernels:"):]
    assert re.findall(r"\.symbol:\s+(\S+)\n", entry) == ["wbc_leg_control_kernel.kd"] and re.search(r"\.name:\s+wbc_leg_control_kernel\n", entry)
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))          # noqa: E731
    print(f"wbc_leg_control_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('private_segment_fixed_size')} bytes of scratch, {meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("group_segment_fixed_size") == 0
    assert meta("max_flat_workgroup_size") == 64 and meta("vgpr_count") <= 128


# ------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _env(n, seed=5):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    return WidowGo1(cfg, sim_device="cuda:0", seed=seed)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


_SHAPES = {"tau": ((20,), torch.float32), "leg_force": ((4, 3), torch.float32), "foot": ((4, 6), torch.float32), "info": ((), torch.int32)}
_STRIDES = dict(tau_bias=26, mass_matrix=676, acc_bias=162)


def _load_sim(env, inp):
    """The sim's own root and joint state from the inputs."""
    root = env.sim.tensor("ROOT_STATES").clone()
    root[:, 0, 0:3] = _dev(inp["base_pos"]); root[:, 0, 3:7] = _dev(inp["quat"])
    root[:, 0, 7:10] = _dev(inp["base_vel"]); root[:, 0, 10:13] = _dev(inp["ang_vel"])
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(_dev(inp["dof"]))
    torch.cuda.synchronize()


def _call(env, cfg, inp, clip=False, which=_OUTS, null=(), tensors=None, strides=None):
    """A direct C-ABI call into sentinel-framed buffers; returns {name: [n, ...] tensor} of the outputs asked for. The inputs named in
    `null`, and those missing from inp, are handed over as NULL; `tensors` replaces device inputs (strided views), `strides` their strides."""
    n = env.num_envs
    size = {k: int(np.prod(s, dtype=np.int64)) for k, (s, _) in _SHAPES.items()}
    bufs = {}
    for name in which:
        dt = _SHAPES[name][1]
        bufs[name] = torch.full((n * size[name] + 16,), SENTINEL if dt == torch.float32 else ISENTINEL, dtype=dt, device="cuda")
    tens = {k: _dev(inp.get(k)) for k in _INPUTS if k not in null}
    tens.update(tensors or {})
    st = dict(_STRIDES, **(strides or {}))
    ptr = lambda d, k, off=0: d[k][off:].data_ptr() if d.get(k) is not None and d[k].numel() > 0 else None     # noqa: E731
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_leg_control(env.sim.h, C.byref(c), *[ptr(tens, k) for k in _INPUTS[:9]], st["tau_bias"], ptr(tens, "mass_matrix"),
                                       st["mass_matrix"], ptr(tens, "acc_bias"), st["acc_bias"], ptr(tens, "arm_q_des"), ptr(tens, "tau_limit"),
                                       abi.LEGCTL_CLIP if clip else 0, *[ptr(bufs, k, 8) for k in _OUTS], None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        sent = SENTINEL if _SHAPES[name][1] == torch.float32 else ISENTINEL
        assert bool((b[:8] == sent).all()) and bool((b[8 + n * size[name]:] == sent).all()), name
    return {name: b[8:8 + n * size[name]].view((n,) + _SHAPES[name][0]).clone() for name, b in bufs.items()}


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_entry_against_fp64(n):
    env = _env(n)
    worst = {k: 0.0 for k in lr.OUTPUTS}
    for combo in range(len(COMBOS)):
        cfg, inp, clip, ref = _case(n, combo)
        got = _np(_call(env, cfg, inp, clip))
        assert all(np.isfinite(got[k].astype(np.float64)).all() for k in got)
        r, _, _ = compare(got, ref, cfg, who=(n, COMBOS[combo]))
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"leg control n={n}: largest |kernel - ref| / (2^-24 mag): {worst}")


@pytest.mark.gpu
def test_outputs_one_at_a_time_two_runs_a_graph_and_the_sim_untouched():
    n, combo = 130, 0
    env = _env(n)
    cfg, inp, clip, _ = _case(n, combo)
    _load_sim(env, inp)
    names = ("ROOT_STATES", "DOF_STATE")
    before = [env.sim.tensor(k).clone() for k in names]
    full = _call(env, cfg, inp, clip)
    assert _same(full, _call(env, cfg, inp, clip))                                     # a second run
    for k in _OUTS:
        one = _call(env, cfg, inp, clip, which=(k,))
        assert torch.equal(one[k], full[k]), k
    # a graph replay of the Python entry point on caller-owned buffers
    c = _make_cfg(cfg)
    tens = {k: _dev(v) for k, v in inp.items()}
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _SHAPES.items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        env.sim.leg_control(c, clip=clip, **tens, **outs)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert _same(outs, full)
    for t in outs.values():
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.sim.leg_control(c, clip=clip, **tens, **outs)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(outs, full)
    assert all(torch.equal(a, env.sim.tensor(k)) for a, k in zip(before, names))       # no sim tensor changed


@pytest.mark.gpu
def test_null_inputs_and_strided_views_give_the_same_bits():
    n, combo = 17, 0
    env = _env(n)
    cfg, inp, clip, _ = _case(n, combo)
    _load_sim(env, inp)
    full = _call(env, cfg, inp, clip)
    # NULL quat / dof / base_* / ang_vel: the sim's own tensors, one at a time and all together
    for null in (("quat",), ("dof",), ("base_pos",), ("base_vel",), ("ang_vel",), ("quat", "dof", "base_pos", "base_vel", "ang_vel")):
        assert _same(_call(env, cfg, inp, clip, null=null), full), null
    # mass_matrix as env.mm_whole, acc_bias as the [N, 27, 6] tensor, both as they stand; tau_bias as a plane of a wider NaN-framed buffer
    mm = env.mm_whole
    mm.copy_(_dev(inp["mass_matrix"]))
    acc = env.rigid_body_accelerations()
    acc.copy_(_dev(inp["acc_bias"]))
    wide = torch.full((n, 3, 26), float("nan"), device="cuda")
    wide[:, 1] = _dev(inp["tau_bias"])
    mmw = torch.full((n, 700), float("nan"), device="cuda")
    mmw[:, :676] = _dev(inp["mass_matrix"]).reshape(n, 676)
    accw = torch.full((n, 170), float("nan"), device="cuda")
    accw[:, :162] = _dev(inp["acc_bias"]).reshape(n, 162)
    assert _same(_call(env, cfg, inp, clip, tensors=dict(mass_matrix=mm, acc_bias=acc)), full)
    assert _same(_call(env, cfg, inp, clip, tensors=dict(tau_bias=wide[:, 1], mass_matrix=mmw, acc_bias=accw),
                       strides=dict(tau_bias=78, mass_matrix=700, acc_bias=170)), full)
    # and through the Python entry point, which reads the strides off the views
    outs = {k: torch.zeros((n,) + s, dtype=dt, device="cuda") for k, (s, dt) in _SHAPES.items()}
    tens = {k: _dev(v) for k, v in inp.items()}
    tens.update(tau_bias=wide[:, 1], mass_matrix=mmw.as_strided((n, 26, 26), (700, 26, 1)),
                acc_bias=accw.as_strided((n, 27, 6), (170, 6, 1)))
    for k in ("quat", "dof", "base_pos", "base_vel", "ang_vel"):
        tens[k] = None
    env.sim.leg_control(_make_cfg(cfg), clip=clip, **tens, **outs)
    torch.cuda.synchronize()
    assert _same(outs, full)
    # entries that are never read may hold NaN
    nanny = {k: np.array(v, copy=True) for k, v in inp.items()}
    legs, arm, fingers, feet_rb, _ = lr.dof_groups(_model())
    nanny["tau_bias"][:, 0:6] = np.nan; nanny["tau_bias"][:, 6 + fingers] = np.nan; nanny["dof"][:, fingers, :] = np.nan
    keep = np.zeros((26, 26), dtype=bool)
    for leg in legs:
        keep[np.ix_(6 + leg, 6 + leg)] = True
    nanny["mass_matrix"][:, ~keep] = np.nan
    rows = np.zeros((27, 6), dtype=bool); rows[feet_rb, 0:3] = True
    nanny["acc_bias"][:, ~rows] = np.nan
    assert _same(_call(env, cfg, nanny, clip), full)


@pytest.mark.gpu
def test_failed_envs_write_zeros_and_their_neighbours_keep_their_bits():
    n, combo = 17, 0
    env = _env(n)
    cfg, inp, clip, _ = _case(n, combo)
    full = _call(env, cfg, inp, clip)
    bad = {k: np.array(v, copy=True) for k, v in inp.items()}
    legs, arm, fingers, feet_rb, _ = lr.dof_groups(_model())
    bad["base_pos"][0, 1] = np.nan; bad["quat"][2, 3] = np.inf; bad["dof"][4, legs[1, 2], 0] = np.nan; bad["forces"][6, 2, 1] = np.inf
    bad["swing_ref"][8, 3, 8] = np.nan; bad["stance"][10, 0] = np.nan; bad["tau_bias"][12, 6 + arm[3]] = np.nan
    bad["mass_matrix"][14, 6 + legs[2, 0], 6 + legs[2, 2]] = np.nan; bad["tau_limit"][16, 4] = -1.0
    got = _call(env, cfg, bad, clip)
    ref = _ref(cfg, bad, clip)
    failed = torch.tensor(ref["diag"]["failed"], device="cuda")
    assert failed.tolist() == [e % 2 == 0 for e in range(n)]
    assert bool((got["info"][failed] == lr.INFO_FAILED).all())
    for k in ("tau", "leg_force", "foot"):
        assert bool((got[k][failed] == 0).all()), k
    for k in _OUTS:
        assert torch.equal(got[k][~failed], full[k][~failed]), k


def _id_reference(env, nudot):
    """(M nudot + h [n, 26], its magnitude) of inverse_dynamics_reference at the sim's downloaded fp32 state."""
    import inverse_dynamics_reference as idr
    m = env.robot_model
    root = env.root_states.cpu().numpy().astype(np.float64)
    q, qd = env.dof_pos.cpu().numpy().astype(np.float64), env.dof_vel.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    g = [float(x) for x in env.tcfg.gravity]
    out = [idr.inverse_dynamics(m, root[e, :3], root[e, 3:7], q[e], np.r_[root[e, 7:13], qd[e]], nudot[e], bp[e], g) for e in range(env.num_envs)]
    return np.array([t for t, _ in out]), np.array([mg for _, mg in out])


@pytest.mark.gpu
def test_full_stance_on_the_simulator_reproduces_whole_body_inverse_dynamics():
    """8 envs standing on the plane: with forces = the lambda of env.whole_body_inverse_dynamics and tau_bias = env.inverse_dynamics(nudot)
    the kernel's tau is held to the fp64 reference on the logged inputs (the bound set the same way: the yardstick measured here from the
    reference's fp32 run), and agrees with that call's torques within the sum of that bound, the call's own bound on its joint dynamics
    rows (C_JOINT 2^-24 scale, tests/task_inverse_dynamics_reference.py) and inverse dynamics' own (C_ID 2^-24 mag)."""
    import constrained_dynamics_reference as cdr
    import task_inverse_dynamics_reference as tir
    n = 8
    env = _env(n, seed=11)
    env.reset()
    zero = torch.zeros(n, 18, device="cuda")
    for _ in range(25):
        env.step(zero)
    torch.cuda.synchronize()
    base_acc = torch.zeros(n, 6, device="cuda"); base_acc[:, 2] = 0.5; base_acc[:, 0] = 0.3
    torques, nudot, lam = env.whole_body_inverse_dynamics(base_acc=base_acc)
    bias = env.inverse_dynamics(nudot)
    env.refresh_mass_matrix_tensors()
    torch.cuda.synchronize()
    cfg = _cfg(kd_stance=0.0, kp_arm=(0,) * 6, kd_arm=(0,) * 6)
    root = env.root_states
    inp = {k: F32(v.cpu().numpy()) for k, v in dict(base_pos=root[:, 0:3], quat=root[:, 3:7], base_vel=root[:, 7:10], ang_vel=root[:, 10:13],
                                                    dof=env.sim.tensor("DOF_STATE"), forces=lam, tau_bias=bias).items()}
    got = _np(_call(env, cfg, inp, null=("quat", "dof", "base_pos", "base_vel", "ang_vel")))
    ref, r32 = _ref(cfg, inp), _ref(cfg, inp, dtype=np.float32)
    k_ref = lr.ratios(r32, ref)
    const = {k: _pow2(4 * max(v, 0.25)) for k, v in k_ref.items()}
    r, _, _ = compare(got, ref, cfg, const=const, who="simulator")
    print(f"leg control on the simulator: K_ref {k_ref}, C {const}, the kernel {r}")
    assert (got["info"] == 0).all() and np.abs(inp["forces"][:, :, 2]).min() > 1.0
    # against the call's own torques
    t_call = torques.cpu().numpy().astype(np.float64)
    nd, lm = nudot.cpu().numpy().astype(np.float64), lam.cpu().numpy().astype(np.float64)
    M = env.mm_whole.cpu().numpy().astype(np.float64)
    _, idmag = _id_reference(env, nd)
    J, dofs = ref["diag"]["jac"], ref["diag"]["dofs"]
    worst = 0.0
    for e in range(n):
        Jc = np.zeros((12, 26))
        for f in range(4):
            Jc[3 * f:3 * f + 3, 6 + dofs[f]] = J[e, f]
        _, scale = cdr.dynamics_residual_and_scale(M[e], np.zeros(26), np.r_[np.zeros(6), t_call[e]], Jc, nd[e], lm[e].reshape(-1))
        bound = EPS * (const["tau"] * ref["mag"]["tau"][e] + tir.C_JOINT * scale[6:] + cdr.C_ID * idmag[e, 6:])
        live = np.r_[dofs.reshape(-1), ref["diag"]["arm"]]
        worst = max(worst, float((np.abs(got["tau"][e].astype(np.float64) - t_call[e])[live] / bound[live]).max()))
    print(f"leg control on the simulator: largest |kernel tau - whole_body_inverse_dynamics' torques| / summed bound = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_twenty_control_steps_behind_the_estimator_planner_and_mpc():
    """The stand gait through LegController: every output finite and every status word one of its defined values. The trunk height is
    printed, not asserted: nothing here is tuned."""
    n = 8
    env = _env(n, seed=13)
    env.reset()
    env.reset_buf.zero_()
    est, planner, mpc, ctl = env.base_state_estimator(), env.gait_planner("stand", horizon=10), env.centroidal_mpc(horizon=10), env.leg_controller()
    assert abs(float(ctl.cfg.kp_arm[0]) - float(env.p_gains[ctl.arm_dofs[0]])) < 1e-6 and ctl.tau_limit.shape == (n, 18)
    assert [list(leg) for leg in ctl.leg_dofs] == lr.dof_groups(_model())[0].tolist() and list(ctl.arm_dofs) == lr.dof_groups(_model())[1].tolist()
    zero2, wz = torch.zeros(n, 2, device="cuda"), torch.zeros(n, device="cuda")
    live, fingers = sorted([d for leg in ctl.leg_dofs for d in leg] + list(ctl.arm_dofs)), lr.dof_groups(_model())[2].tolist()
    allowed = lr.INFO_FAILED | sum((lr.INFO_FORCE_CLIPPED | lr.INFO_FF_SINGULAR | lr.INFO_SATURATED) << i for i in range(4)) | (lr.INFO_SATURATED << 4)
    heights = []
    for k in range(20):
        est.update(contact=planner.contact)
        planner.update(zero2, wz, state=est)
        mpc.solve(planner.contact_schedule, zero2, wz, foot_positions=planner.foot_positions, state=est)
        tau = ctl.update(forces=mpc.forces, swing_ref=planner.swing_ref, stance=planner.contact, state=est, feedforward=(k % 2 == 0))
        assert tau is ctl.tau and tuple(tau.shape) == (n, 20)
        for t in (ctl.tau, ctl.leg_force, ctl.foot, mpc.forces):
            assert bool(torch.isfinite(t).all())
        assert bool(((ctl.info & ~allowed) == 0).all()) and bool((ctl.tau[:, fingers] == 0).all())
        assert bool((ctl.tau[:, live].abs() <= ctl.tau_limit).all())
        assert set(mpc.status.cpu().tolist()) <= {0, 1, 2} and set(est.status.cpu().tolist()) <= {0, 1, 2}
        env.sim.set_dof_forces(tau.contiguous())
        for _ in range(int(env.cfg.control.decimation)):
            env.sim.simulate()
        heights.append(round(float(env.root_states[:, 2].mean()), 4))
    assert bool((ctl.info & lr.INFO_FAILED == 0).all())
    print(f"leg control, 20 control steps of the stand gait: mean trunk height per step {heights}")
