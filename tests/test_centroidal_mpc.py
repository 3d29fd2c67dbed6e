"""wbc_sim_centroidal_mpc (include/wbc_sim.h) against tests/mpc_reference.py, the fp64 numpy restatement of the same fixed-iteration ADMM /
Riccati recursion.

CPU: the prototypes and every refusal without a device; the reference against the dense least-squares solution of the condensed problem
and against the QP's KKT conditions; properties of the equations; the fp32 yardstick; the code object's metadata.
GPU: every entry of every output against fp64 within C * 2^-24 * mag (magnitudes: mpc_reference's docstring), warm starts, partial outputs,
graph capture, refusals, the simulator untouched, and the env-level object on a standing robot.

The fp32 yardstick, by the project's rule: K_ref is the largest ratio |fp32 reference - fp64 reference| / (2^-24 mag) over the judged cases
(CASES below: n in {1, 3, 130} x H in {1, 2, 10, 16} x four settings, the four schedules dealt over the envs), C = 4 K_ref rounded up to a
power of two. No constant comes from the kernel.

| output   | K_ref | C    | the kernel's largest ratio on an MI355X |
|----------|-------|------|------------------------------------------|
| forces   | 154   | 1024 | 64.7                                     |
| u        | 154   | 1024 | 117                                      |
| x_pred   | 303   | 2048 | 285                                      |
| base_acc | 154   | 1024 | 65.0                                     |
| res      | 52.6  | 256  | 28.5                                     |
NULL x0 / foot_pos against the call on explicit tensors (test_null_inputs_mean_the_sims_state): 214 / 214 / 668 / 331 / 26.5.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arm_codegen
import mpc_reference as mr
from wbc_amd import abi

SIZES = (1, 3, 130)
HORIZONS = (1, 2, 10, 16)
GRAVITY = (0.0, 0.0, float(np.float32(-9.81)))
G = 9.81
EPS = 2.0 ** -24
OUTPUTS = ("forces", "u", "x_pred", "base_acc", "res")
F32 = lambda v: float(np.float32(v))
Q_DEFAULT = (25.0, 25.0, 10.0, 2.0, 2.0, 50.0, 0.0, 0.0, 0.3, 0.2, 0.2, 0.1)


def _cfg(**kw):
    c = dict(horizon=10, iters=40, dt=F32(0.03), rho=F32(1e-4), mu=F32(0.5), fz_min=0.0, fz_max=250.0, q=tuple(F32(v) for v in Q_DEFAULT),
             r=(F32(4e-5),) * 3, tol=F32(0.05))
    c.update(kw)
    return c


BINDING = dict(mu=F32(0.15), fz_max=30.0)
# (iters, binding limits, foot_pos_stages = H)
SETTINGS = ((1, False, False), (40, True, True), (40, False, False), (1, True, True))
CASES = [(n, H, s) for n in SIZES for H in HORIZONS for s in range(len(SETTINGS))]

# K_ref: measured by test_fp32_yardstick_is_where_the_constants_came_from on the CPU and asserted there
K_REF = {"forces": 154.0, "u": 154.0, "x_pred": 303.0, "base_acc": 154.0, "res": 52.6}
# the kernel's largest ratios on an MI355X over the same cases (printed by test_every_entry_against_fp64)
K_GPU = {"forces": 64.7, "u": 117.0, "x_pred": 285.0, "base_acc": 65.0, "res": 28.5}


def _pow2(v):
    return float(2.0 ** int(np.ceil(np.log2(4.0 * v))))


CONST = {k: _pow2(v) for k, v in K_REF.items()}
LDS_STATIC_BYTES = 4 * (5 * 12 * 13 + 16 + 4 * 12 + 24 + 2 * 64)               # one env's work matrices and vectors: 3984
LDS_STAGE_BYTES = 4 * (12 * 25 + 36 + 12 + 3 * 20 + 12 + 12 + 12 + 1)          # dynamic, per env and stage: 1780


def schedule(kind, H):
    """u8 [H, 4]: 0 full stance, 1 trot (the diagonals alternate every two stages), 2 one foot, 3 all swing."""
    c = np.zeros((H, 4), np.uint8)
    if kind == 0:
        c[:] = 1
    elif kind == 1:
        for k in range(H):
            c[k] = (1, 0, 0, 1) if (k // 2) % 2 == 0 else (0, 1, 1, 0)
    elif kind == 2:
        c[:, 0] = 1
    return c


@functools.lru_cache(maxsize=None)
def inputs(n, H, stages_h=False, seed=0, kinds=None):
    """Go1-like bodies near a stand, fp32-rounded: the four schedules dealt over the envs."""
    g = np.random.default_rng(1000 * n + 10 * H + seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    mass = f32(g.uniform(12.0, 17.0, n))
    Rr = np.linalg.qr(g.normal(size=(n, 3, 3)))[0]
    inertia = f32(Rr @ (np.eye(3) * g.uniform(0.08, 0.45, (n, 1, 3))) @ np.swapaxes(Rr, 1, 2))
    inertia = f32(0.5 * (inertia + np.swapaxes(inertia, 1, 2)))
    x0 = np.zeros((n, 12))
    x0[:, 0:3] = g.uniform(-0.15, 0.15, (n, 3))
    x0[:, 3:5] = g.uniform(-2.0, 2.0, (n, 2)); x0[:, 5] = g.uniform(0.25, 0.4, n)
    x0[:, 6:9] = g.uniform(-0.5, 0.5, (n, 3)); x0[:, 9:12] = g.uniform(-0.4, 0.4, (n, 3))
    x0 = f32(x0)
    S = H if stages_h else 1
    nominal = np.array([[0.19, 0.13, 0.0], [0.19, -0.13, 0.0], [-0.19, 0.13, 0.0], [-0.19, -0.13, 0.0]])
    vcmd = g.uniform(-0.6, 0.6, (n, 2))
    t = (np.arange(1, H + 1) * 0.03)[None, :, None]
    foot = np.zeros((n, S, 4, 3))
    foot[:, :, :, 0:2] = x0[:, None, None, 3:5] + nominal[None, None, :, 0:2] + g.uniform(-0.03, 0.03, (n, 1, 4, 2))
    foot[:, :, :, 2] = g.uniform(0.0, 0.02, (n, 1, 4))
    if stages_h:
        foot[:, :, :, 0:2] += (vcmd[:, None, :] * t)[:, :, None, :]
    x_ref = np.zeros((n, H, 12))
    x_ref[:, :, 3:5] = x0[:, None, 3:5] + vcmd[:, None, :] * t
    x_ref[:, :, 5] = 0.32
    x_ref[:, :, 9:11] = vcmd[:, None, :]
    x_ref[:, :, 2] = g.uniform(-0.5, 0.5, (n, 1)) * t[:, :, 0]
    kinds = [(e + H + seed) % 4 for e in range(n)] if kinds is None else list(kinds)
    contact = np.stack([schedule(kinds[e], H) for e in range(n)])
    return dict(x0=x0, mass=mass, inertia=inertia, foot_pos=f32(foot), contact=contact, x_ref=f32(x_ref))


# candidates for tol, nearest to 0.2 N first, from 0.0125 N (well above what fp32 resolves of a residual) to 819 N (above every residual)
TOLS = tuple(sorted((0.2 * 2.0 ** (j / 4) for j in range(-16, 49)), key=lambda t: abs(np.log(t / 0.2))))


def _base_cfg(H, s):
    iters, binding, _ = SETTINGS[s]
    return _cfg(horizon=H, iters=iters, **(BINDING if binding else {}))


@functools.lru_cache(maxsize=None)
def _solved(n, H, s, fp32=False):
    return mr.solve(_base_cfg(H, s), gravity=GRAVITY, dtype=np.float32 if fp32 else np.float64, **inputs(n, H, SETTINGS[s][2]))


@functools.lru_cache(maxsize=None)
def case_cfg(n, H, s):
    """The case's cfg: tol is the first of TOLS with none of the fp64 reference's residuals in [tol / 2, 2 tol] (tol decides the status alone)."""
    res = _solved(n, H, s)["res"]
    tol = next(t for t in TOLS if not ((res >= t / 2) & (res <= 2 * t)).any())
    return dict(_base_cfg(H, s), tol=F32(tol))


@functools.lru_cache(maxsize=None)
def reference(n, H, s, fp32=False):
    out = dict(_solved(n, H, s, fp32))
    tol = case_cfg(n, H, s)["tol"]
    status = np.where((out["res"] <= tol).all(-1), mr.STATUS_OK, mr.STATUS_ITERATIONS).astype(np.int32)
    out["status"] = np.where(out["status"] == mr.STATUS_FAILED, mr.STATUS_FAILED, status).astype(np.int32)
    return out


def ratios(got, ref, mag):
    """Per output the largest |got - ref| / (2^-24 mag)."""
    return {k: float((np.abs(np.asarray(got[k], np.float64) - ref[k]) / (EPS * mag[k])).max()) for k in OUTPUTS}


def _mag(n, H, s):
    return mr.magnitudes(case_cfg(n, H, s), reference(n, H, s), inputs(n, H, SETTINGS[s][2])["mass"].astype(np.float64), GRAVITY)


# ------------------------------------------------------------------------------------------------------------ CPU
_INPUTS = ("x0", "mass", "inertia", "foot_pos")
_NAMES = ("sim", "cfg") + _INPUTS + ("foot_pos_stages", "contact", "x_ref", "warm", "flags", "forces", "u", "x_pred", "base_acc", "res", "status",
                                     "workspace", "stream")
_POINTERS = _INPUTS + ("x_ref", "warm", "forces", "u", "x_pred", "base_acc", "res", "status", "workspace")


def _make_cfg(cfg=None, **kw):
    c = dict(_cfg() if cfg is None else cfg, **kw)
    return abi.WbcMpcCfg(int(c["horizon"]), int(c["iters"]), c["dt"], c["rho"], c["mu"], c["fz_min"], c["fz_max"], (C.c_float * 12)(*c["q"]),
                         (C.c_float * 3)(*c["r"]), c["tol"])


def _refusals(base):
    """[(arguments that differ from the good call `base`, a word of the message)]: every refusal of wbc_sim_centroidal_mpc but the NULL sim."""
    nan, inf = float("nan"), float("inf")
    out = [(dict(cfg=None), b"NULL"), (dict(contact=None), b"NULL"), (dict(x_ref=None), b"NULL"), (dict(flags=4), b"flag"), (dict(flags=-1), b"flag")]
    out += [(dict(cfg=_make_cfg(horizon=h), foot_pos_stages=1), b"horizon") for h in (0, -1, 17)]
    out += [(dict(cfg=_make_cfg(iters=i)), b"iters") for i in (0, -3, 1001)]
    for field in ("dt", "rho", "mu", "tol"):
        out += [(dict(cfg=_make_cfg(**{field: bad})), b"dt, rho, mu and tol") for bad in (0.0, -1.0, nan, inf)]
    for j in range(3):
        out += [(dict(cfg=_make_cfg(r=tuple(bad if i == j else 4e-5 for i in range(3)))), b"every r") for bad in (0.0, -1.0, nan, inf)]
    for j in range(12):
        out += [(dict(cfg=_make_cfg(q=tuple(bad if i == j else 1.0 for i in range(12)))), b"every q") for bad in (-1e-3, nan, inf)]
    out += [(dict(cfg=_make_cfg(fz_min=bad)), b"fz_min") for bad in (-1.0, nan, inf)]
    out += [(dict(cfg=_make_cfg(fz_min=10.0, fz_max=bad)), b"fz_max") for bad in (9.0, nan, inf)]
    out += [(dict(foot_pos_stages=s), b"foot_pos_stages") for s in (0, 2, 9, 11, -1)]
    out += [({k: base[k] + off}, b"aligned") for k in _POINTERS for off in (1, 2, 3)]
    out += [(dict(workspace=None, **{k: None}), b"workspace") for k in ("x0", "mass", "inertia")]
    return out


def _raw_call(L, base, **kw):
    args = dict(base, **kw)
    return L.wbc_sim_centroidal_mpc(*[C.byref(args[k]) if isinstance(args[k], abi.WbcMpcCfg) else args[k] for k in _NAMES])


def test_prototypes_and_refusals_without_a_device():
    """The argument checks come before the sim is looked at, so every refusal is met here, with host memory and no sim."""
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    for sym in ("wbc_sim_centroidal_mpc", "wbc_sim_centroidal_mpc_workspace_floats"):
        assert sym in EXPORTED_SYMBOLS and hasattr(L, sym)
    fields = [f for f, _ in abi.WbcMpcCfg._fields_]
    assert fields == ["horizon", "iters", "dt", "rho", "mu", "fz_min", "fz_max", "q", "r", "tol"]
    assert C.sizeof(abi.WbcMpcCfg) == 4 * (2 + 5 + 12 + 3 + 1) and abi.WbcMpcCfg.q.offset == 28 and abi.WbcMpcCfg.tol.offset == 88
    assert (abi.MPC_COLD, abi.MPC_SHIFT) == (mr.COLD, mr.SHIFT) == (1, 2)
    assert (abi.MPC_STATUS_OK, abi.MPC_STATUS_ITERATIONS, abi.MPC_STATUS_FAILED) == (mr.STATUS_OK, mr.STATUS_ITERATIONS, mr.STATUS_FAILED) == (0, 1, 2)
    assert (abi.MPC_NX, abi.MPC_NU, abi.MPC_NZ, abi.MPC_MAX_HORIZON) == (12, 12, 20, 16)
    assert [L.wbc_sim_centroidal_mpc_workspace_floats(n) for n in (0, 1, 130, 4096)] == [0, 16, 16 * 130, 16 * 4096]
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    base = dict(sim=None, cfg=_make_cfg(), foot_pos_stages=10, flags=0, stream=None, contact=p + 4000,
                **{k: p + 256 * (i + 1) for i, k in enumerate(_POINTERS)})
    good = [(dict(), b"sim is NULL"), (dict(flags=abi.MPC_COLD | abi.MPC_SHIFT), b"sim is NULL"), (dict(foot_pos_stages=1), b"sim is NULL"),
            (dict(contact=p + 4001), b"sim is NULL"), (dict(x0=None, mass=None, inertia=None, foot_pos=None, warm=None), b"sim is NULL"),
            (dict(cfg=_make_cfg(fz_min=5.0, fz_max=5.0, q=(0.0,) * 12)), b"sim is NULL")]
    for kw, word in _refusals(base) + good:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_centroidal_mpc: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    assert all(v == 0.0 for v in buf)


def _dense(cfg, inp, e, out):
    """The condensed problem of env e: (Hessian, gradient at u = 0, Su, c) over the stacked controls."""
    m = out["model"]
    H = cfg["horizon"]
    c, Su = mr.condense(m["A"], m["B"][e], m["d"], inp["x0"][e].astype(np.float64))
    Qb = np.tile(np.asarray(cfg["q"], np.float64), H)
    Rb = np.tile(np.asarray(cfg["r"], np.float64), 4 * H)
    Hs = Su.T @ (Qb[:, None] * Su) + np.diag(Rb)
    g0 = Su.T @ (Qb * (c - inp["x_ref"][e].astype(np.float64).reshape(-1)))
    return Hs, g0, Su, c


@pytest.mark.parametrize("H", (1, 2, 10))
def test_reference_equals_the_dense_least_squares_solution(H):
    """No row binds (wide limits): the fixed point of the iteration is the minimiser of the condensed quadratic over the stance feet's
    forces, which np.linalg.solve gives without ADMM or Riccati."""
    n = 4
    cfg = _cfg(horizon=H, iters=300, rho=1e-6, mu=3.0, fz_min=0.0, fz_max=1e6)
    inp = inputs(n, H, True, seed=3, kinds=(0, 1, 2, 0))
    inp = dict(inp, x_ref=inp["x_ref"].copy(), x0=inp["x0"].copy())
    inp["x0"][:, 0:3] *= np.float32(0.05); inp["x0"][:, 6:12] = 0                   # near rest, and asked to stay: every f_z stays well above 0
    inp["x_ref"][:] = 0
    inp["x_ref"][:, :, 3:6] = inp["x0"][:, None, 3:6]
    out = mr.solve(cfg, gravity=GRAVITY, **inp)
    for e in range(n):
        Hs, g0, Su, c = _dense(cfg, inp, e, out)
        free = np.repeat(inp["contact"][e].reshape(-1) != 0, 3)
        u = np.zeros(12 * H)
        u[free] = np.linalg.solve(Hs[np.ix_(free, free)], -g0[free])
        Cu = u.reshape(H, 12) @ out["model"]["C"].T
        assert (Cu[out["model"]["stance"][e]] > 0).all()                            # no row binds at the dense solution
        scale = np.abs(u).max()
        assert np.abs(out["u"][e].reshape(-1) - u).max() <= 1e-9 * scale, (e, np.abs(out["u"][e].reshape(-1) - u).max(), scale)
        assert np.abs(out["x_pred"][e].reshape(-1) - (c + Su @ u)).max() <= 1e-9 * max(1.0, np.abs(c).max())
        assert (out["u"][e].reshape(-1)[~free] == 0).all()


@functools.lru_cache(maxsize=None)
def _converged_binding():
    n, H = 4, 4
    cfg = _cfg(horizon=H, iters=1000, rho=F32(1e-3), **BINDING)
    inp = inputs(n, H, False, seed=7, kinds=(0, 1, 2, 0))
    warm, out = None, None
    for _ in range(40):
        out = mr.solve(cfg, gravity=GRAVITY, warm=warm, **inp)
        warm = out["warm"]
        if out["res"].max() < 1e-10:
            break
    return cfg, inp, out


def test_reference_satisfies_the_kkt_conditions_on_binding_cases():
    """mu = 0.15 and fz_max below the demand: run to residuals below 1e-10, the iterate satisfies the QP's KKT conditions with the
    multipliers rho y -- stationarity, sign and complementarity per row, feasibility. This pins the reference independently of ADMM."""
    cfg, inp, out = _converged_binding()
    assert out["res"].max() < 1e-10, out["res"]
    m = out["model"]
    Cm, lo, hi = m["C"], m["lo"], m["hi"]
    z, y = out["warm"][:, 0], out["warm"][:, 1]
    H = cfg["horizon"]
    binding_rows = 0
    for e in range(inp["x0"].shape[0]):
        Hs, g0, Su, c = _dense(cfg, inp, e, out)
        u = out["u"][e].reshape(-1)
        lam = float(cfg["rho"]) * y[e]                                              # [H, 20]
        grad = Hs @ u + g0 + (lam @ Cm).reshape(-1)
        free = np.repeat(inp["contact"][e].reshape(-1) != 0, 3)
        scale = max(np.abs(Hs @ u).max(), np.abs(g0).max())
        assert np.abs(grad[free]).max() <= 1e-8 * scale, (e, np.abs(grad[free]).max(), scale)
        assert (u[~free] == 0).all()
        Cu = out["u"][e] @ Cm.T
        st = m["stance"][e]
        fscale = np.abs(u).max()
        assert (Cu[st] >= np.broadcast_to(lo, Cu.shape)[st] - 1e-8 * fscale).all() and (Cu[st] <= np.broadcast_to(hi, Cu.shape)[st] + 1e-8 * fscale).all()
        at_lo = np.abs(Cu - lo) <= 1e-8 * fscale
        at_hi = np.abs(Cu - hi) <= 1e-8 * fscale
        lam_tol = 1e-8 * np.abs(lam).max()
        assert (lam[st & ~at_lo & ~at_hi] == 0).all() or np.abs(lam[st & ~at_lo & ~at_hi]).max() <= lam_tol        # complementarity
        assert (lam[st & at_lo & ~at_hi] <= lam_tol).all() and (lam[st & at_hi & ~at_lo] >= -lam_tol).all()        # signs
        assert (lam[~st] == 0).all()
        binding_rows += int((st & (at_lo | at_hi) & (np.abs(lam) > lam_tol)).sum())
    assert binding_rows >= 10, binding_rows


def test_all_swing_is_ballistic_and_swing_forces_are_zero():
    H = 10
    inp = inputs(4, H, False, seed=5, kinds=(3, 3, 1, 2))
    cfg = _cfg(horizon=H, iters=5)
    out = mr.solve(cfg, gravity=GRAVITY, **inp)
    assert (out["u"][:2] == 0).all() and (out["forces"][:2] == 0).all()
    dt, g = float(cfg["dt"]), np.asarray(GRAVITY)
    for k in range(1, H + 1):
        t = k * dt
        x0 = inp["x0"][:2].astype(np.float64)
        want = np.concatenate([x0[:, 0:3] + t * x0[:, 6:9], x0[:, 3:6] + t * x0[:, 9:12] + 0.5 * t * t * g, x0[:, 6:9], x0[:, 9:12] + t * g], -1)
        assert np.abs(out["x_pred"][:2, k - 1] - want).max() <= 1e-12
    np.testing.assert_allclose(out["base_acc"][:2, 0:3], np.broadcast_to(g, (2, 3)))
    assert (out["base_acc"][:2, 3:6] == 0).all()
    swing = np.repeat(inp["contact"] == 0, 3, axis=-1)
    assert (out["u"][swing] == 0).all()                                             # a swing foot's force is exactly 0 in every stage


def test_at_rest_the_forces_carry_the_weight():
    """Four feet under a level body at rest, x_ref the state itself, the default weights: the stage-0 forces sum to the weight within 1 %
    and their net moment about the centre of mass is below 1 % of m |g| x 1 m."""
    from wbc_amd.envs import CentroidalMPC
    n, H = 3, 10
    d = CentroidalMPC.DEFAULTS
    cfg = _cfg(horizon=H, iters=d["iters"], rho=F32(d["rho"]), mu=F32(d["mu"]), fz_min=d["fz_min"], fz_max=d["fz_max"],
               q=tuple(F32(v) for v in d["q"]), r=tuple(F32(v) for v in d["r"]), tol=F32(d["tol"]))
    mass = np.array([12.0, 15.0, 18.5], np.float32)
    inertia = np.broadcast_to(np.diag([0.1, 0.3, 0.35]).astype(np.float32), (n, 3, 3)).copy()
    x0 = np.zeros((n, 12), np.float32); x0[:, 5] = 0.3
    foot = np.array([[0.2, 0.13, 0.0], [0.2, -0.13, 0.0], [-0.17, 0.13, 0.0], [-0.17, -0.13, 0.0]], np.float32)
    inp = dict(x0=x0, mass=mass, inertia=inertia, foot_pos=np.broadcast_to(foot, (n, 1, 4, 3)).copy(), contact=np.ones((n, H, 4), np.uint8),
               x_ref=np.broadcast_to(x0[:, None], (n, H, 12)).copy())
    out = mr.solve(cfg, gravity=GRAVITY, **inp)
    w = mass.astype(np.float64) * G
    assert (np.abs(out["forces"][:, :, 2].sum(1) - w) <= 0.01 * w).all(), out["forces"][:, :, 2].sum(1) / w
    moment = np.cross(out["model"]["r"][:, 0], out["forces"]).sum(1)
    assert (np.abs(moment).max(-1) <= 0.01 * w).all(), moment
    assert (out["status"] == mr.STATUS_OK).all(), out["res"]


@functools.lru_cache(maxsize=None)
def _yardsticks():
    k = {name: 0.0 for name in OUTPUTS}
    for (n, H, s) in CASES:
        r = ratios(reference(n, H, s, True), reference(n, H, s), _mag(n, H, s))
        k = {name: max(k[name], r[name]) for name in k}
    return k


def test_fp32_yardstick_is_where_the_constants_came_from():
    k = _yardsticks()
    print("mpc yardsticks: " + ", ".join(f"{name} K_ref = {k[name]:.3g} (C = {CONST[name]:g})" for name in k))
    for name in OUTPUTS:
        assert abs(k[name] - K_REF[name]) <= 0.25 * K_REF[name], (name, k[name])     # a largest ratio moves with the summation order of the BLAS at hand
        assert 4 * k[name] <= CONST[name]
    for (n, H, s) in CASES:                                                         # finite, and the fp32 run fails no env that the fp64 run solves
        assert (reference(n, H, s)["status"] != mr.STATUS_FAILED).all() and (reference(n, H, s, True)["status"] != mr.STATUS_FAILED).all()


def test_no_reference_residual_lies_near_tol():
    """tol and the judged cases are such that no env's residual lies in [tol / 2, 2 tol]: the statuses are then compared exactly on the GPU."""
    seen = set()
    for (n, H, s) in CASES:
        ref = reference(n, H, s)
        tol = float(case_cfg(n, H, s)["tol"])
        near = (ref["res"] >= tol / 2) & (ref["res"] <= 2 * tol)
        assert not near.any(), ((n, H, s), ref["res"][near.any(-1)])
        seen |= set(ref["status"].tolist())
    assert seen == {mr.STATUS_OK, mr.STATUS_ITERATIONS}


@functools.lru_cache(maxsize=None)
def _kernel_metadata():
    """csrc/wbc_mpc_kernel.hip compiled to gfx950 assembly with the build's own flags: the metadata of its code object."""
    import os
    import subprocess
    import tempfile
    import __graft_entry__ as g
    if not os.path.exists(arm_codegen.HIPCC):
        pytest.skip("hipcc not installed")
    source = "wbc_mpc_kernel.hip"
    assert source in g.SOURCES and "wbc_mpc.h" in g.HEADERS
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(source, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "mpc.s")
        subprocess.check_call([arm_codegen.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(g.CSRC, source)], stderr=subprocess.DEVNULL)
        text = open(out).read()
    return text.count(".amdhsa_kernel "), text[text.index("amdhsa.kernels:"):]


def test_mpc_kernel_codegen():
    """One kernel, no scratch, a single wavefront per workgroup, the static LDS DESIGN.md states (the per-stage part is dynamic: MPC_STAGE_BYTES per env and stage), at most 128 VGPRs: from the metadata."""
    import os
    import re
    import __graft_entry__ as g
    kernels, entry = _kernel_metadata()
    assert kernels == 1
    meta = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))
    assert re.search(r"\.name:\s+wbc_centroidal_mpc_kernel\n", entry)
    print(f"wbc_centroidal_mpc_kernel: {meta('vgpr_count')} VGPRs, {meta('sgpr_count')} SGPRs, {meta('group_segment_fixed_size')} bytes of LDS, "
          f"{meta('kernarg_segment_size')} bytes of kernel arguments")
    assert meta("private_segment_fixed_size") == 0 and meta("max_flat_workgroup_size") == 64
    assert meta("group_segment_fixed_size") == LDS_STATIC_BYTES and meta("vgpr_count") <= 128
    header = open(os.path.join(g.CSRC, "wbc_mpc.h")).read()
    assert re.search(r"#define MPC_STAGE_BYTES %d\b" % LDS_STAGE_BYTES, header) and re.search(r"#define MPC_EPW 1\b", header)
    assert LDS_STATIC_BYTES + 16 * LDS_STAGE_BYTES == 32464                        # the largest workgroup, H = 16: five per CU


def test_trot_schedule():
    from wbc_amd.envs import trot_schedule
    phase = torch.tensor([0.0, 0.25, 0.5, 0.9])
    c = trot_schedule(phase, period=0.4, duty=0.5, horizon=10, dt=0.04)
    assert c.dtype == torch.uint8 and tuple(c.shape) == (4, 10, 4)
    assert torch.equal(c[..., 0], c[..., 3]) and torch.equal(c[..., 1], c[..., 2]) and bool((c[..., 0] + c[..., 1] == 1).all())
    assert c[0, :, 0].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0] and c[2, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]
    full = trot_schedule(phase, period=0.4, duty=1.0, horizon=3, dt=0.04)
    assert bool((full == 1).all())


# ------------------------------------------------------------------------------------------------------------ GPU
SENTINEL, ISENTINEL = -7.25, -77
_OUT_SHAPES = lambda H: {"forces": (4, 3), "u": (H, 12), "x_pred": (H, 12), "base_acc": (6,), "res": (2,), "status": ()}
ALL_OUT = ("forces", "u", "x_pred", "base_acc", "res", "status")


@functools.lru_cache(maxsize=None)
def _env(n, seed=5):
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    return WidowGo1(cfg, sim_device="cuda:0", seed=seed)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda").contiguous()


def _call(env, cfg, inp, which=ALL_OUT, warm=None, flags=0, workspace=True):
    """A direct C-ABI call into sentinel-framed buffers; returns {name: [n, ...] tensor} of the outputs asked for (and "warm" if given,
    updated in place in a framed copy). Inputs missing from inp, or None, are handed over as NULL."""
    n, H = env.num_envs, int(cfg["horizon"])
    shapes = _OUT_SHAPES(H)
    size = {k: int(np.prod(s, dtype=np.int64)) for k, s in shapes.items()}
    bufs = {}
    for name in which:
        bufs[name] = torch.full((n * size[name] + 8,), ISENTINEL if name == "status" else SENTINEL,
                                dtype=torch.int32 if name == "status" else torch.float32, device="cuda")
    wbuf = None
    if warm is not None:
        wbuf = torch.full((n * 2 * H * 20 + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        wbuf[:n * 2 * H * 20] = warm.reshape(-1)
    tens = {k: _dev(inp.get(k)) for k in _INPUTS + ("x_ref",)}
    tens["contact"] = _dev(inp["contact"], torch.uint8)
    ws = torch.full((16 * n + 8,), SENTINEL, dtype=torch.float32, device="cuda") if workspace else None
    ptr = lambda d, k: d[k].data_ptr() if d.get(k) is not None else None
    stages = int(inp["foot_pos"].shape[1]) if inp.get("foot_pos") is not None else 1
    c = _make_cfg(cfg)
    rc = env.sim.L.wbc_sim_centroidal_mpc(env.sim.h, C.byref(c), *[ptr(tens, k) for k in _INPUTS], stages, ptr(tens, "contact"), ptr(tens, "x_ref"),
                                          wbuf.data_ptr() if wbuf is not None else None, flags, *[ptr(bufs, k) for k in ALL_OUT],
                                          ws.data_ptr() if ws is not None else None, None)
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert bool((b[n * size[name]:] == (ISENTINEL if name == "status" else SENTINEL)).all()), name
    out = {name: b[:n * size[name]].view((n,) + shapes[name]).clone() for name, b in bufs.items()}
    if wbuf is not None:
        assert bool((wbuf[n * 2 * H * 20:] == SENTINEL).all())
        out["warm"] = wbuf[:n * 2 * H * 20].view(n, 2, H, 20).clone()
    if ws is not None:
        assert bool((ws[16 * n:] == SENTINEL).all())
    return out


def _same(a, b, keys=None):
    return all(torch.equal(a[k], b[k]) for k in (keys or a))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("H", HORIZONS)
def test_every_entry_against_fp64(n, H):
    """Every entry of forces, u, x_pred, base_acc and res within C 2^-24 mag of the fp64 reference, the statuses exactly, over the four
    settings of (iters, limits, foot_pos_stages) with the four schedules dealt over the envs."""
    env = _env(n)
    worst = {k: 0.0 for k in OUTPUTS}
    fails = []
    for s in range(len(SETTINGS)):
        cfg, inp, ref = case_cfg(n, H, s), inputs(n, H, SETTINGS[s][2]), reference(n, H, s)
        got = _call(env, cfg, inp, warm=torch.full((n, 2, H, 20), 3.0, device="cuda"), flags=abi.MPC_COLD)
        r = ratios({k: got[k].cpu().numpy() for k in OUTPUTS}, ref, _mag(n, H, s))
        worst = {k: max(worst[k], r[k]) for k in worst}
        if not np.array_equal(got["status"].cpu().numpy(), ref["status"]):
            fails.append((s, "status"))
        wmag = np.maximum(_mag(n, H, s)["res"][:, 0], np.abs(ref["warm"]).max((-1, -2, -3)))[:, None, None, None]     # z and y: rows of C u, sums of them
        wr = float((np.abs(got["warm"].cpu().numpy().astype(np.float64) - ref["warm"]) / (EPS * wmag)).max())
        if wr > CONST["u"]:
            fails.append((s, "warm", wr))
    print(f"mpc n={n} H={H}: the kernel's largest ratios " + ", ".join(f"{k} {worst[k]:.3g} (C = {CONST[k]:g})" for k in worst))
    assert not fails, fails
    for k in OUTPUTS:
        assert worst[k] <= CONST[k], (k, worst[k], CONST[k])


def _sim_state_inputs(env, H):
    """The explicit tensors that NULL inputs stand for, from env.sim.centroidal(), the root state and the feet's rigid-body state."""
    from wbc_amd.envs import CentroidalMPC
    com, _, _, inr = env.sim.centroidal()
    env.sim.refresh_rigid_body_state()
    root = env.root_states
    q = root[:, 3:7] / root[:, 3:7].norm(dim=-1, keepdim=True)
    theta = CentroidalMPC._heading_rotvec(q, CentroidalMPC._yaw(q))
    x0 = torch.cat([theta, root[:, 0:3] + com[:, 0:3], root[:, 10:13], com[:, 3:6]], dim=-1).contiguous()
    inertia = inr[:, [1, 4, 5, 4, 2, 6, 5, 6, 3]].view(-1, 3, 3).contiguous()
    feet = env.rigid_body_state[:, env.feet_indices, 0:3].reshape(-1, 1, 4, 3).contiguous()
    return dict(x0=x0, mass=inr[:, 0].contiguous(), inertia=inertia, foot_pos=feet)


@pytest.mark.gpu
def test_null_inputs_mean_the_sims_state():
    """mass and inertia NULL: the bits of the call given env.sim.centroidal()'s. x0 and foot_pos NULL: the centre of mass, its velocity and
    the angular velocity are the explicit tensors' bits (checked through an all-swing stage, where x_1 = A x_0 + d is a sum of two
    products); theta and the feet come from the kernel's own logarithm and leg walk, which torch's atan2 / acos and the step kernel's
    kinematics do not reproduce bit for bit, so the full result is held to the explicit call within the element-wise bound instead."""
    n, H = 130, 10
    env = _env(n)
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    for _ in range(4):
        env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.5)
    exp = {k: v.cpu().numpy() for k, v in _sim_state_inputs(env, H).items()}
    base = inputs(n, H, False, seed=2)
    x_ref = base["x_ref"].copy()
    x_ref[:, :, 3:5] += exp["x0"][:, None, 3:5] - base["x0"][:, None, 3:5]
    cfg = _cfg(horizon=H)
    full = dict(exp, contact=base["contact"], x_ref=x_ref)
    want = _call(env, cfg, full)
    got = _call(env, cfg, dict(full, mass=None, inertia=None))
    assert _same(got, want)
    got = _call(env, cfg, dict(full, mass=None))
    assert _same(got, want)
    got = _call(env, cfg, dict(full, x0=None, mass=None, inertia=None, foot_pos=None))
    ref = mr.solve(cfg, gravity=GRAVITY, **full)
    mag = mr.magnitudes(cfg, ref, exp["mass"].astype(np.float64), GRAVITY)
    r = ratios({k: got[k].cpu().numpy() for k in OUTPUTS}, ref, mag)
    print("mpc NULL inputs against the reference on the explicit tensors: " + ", ".join(f"{k} {r[k]:.3g}" for k in r))
    assert torch.equal(got["status"], want["status"])
    for k in OUTPUTS:
        assert r[k] <= CONST[k], (k, r[k])
    # p, omega and v of the NULL x0, bit for bit: one all-swing stage with theta handed over through x_ref's position only
    swing = dict(contact=np.zeros((n, 1, 4), np.uint8), x_ref=x_ref[:, :1].copy())
    c1 = _cfg(horizon=1, iters=1)
    a = _call(env, c1, dict(swing, x0=exp["x0"], foot_pos=exp["foot_pos"]))["x_pred"]
    b = _call(env, c1, swing)["x_pred"]
    assert torch.equal(a[:, :, 3:], b[:, :, 3:])
    assert float((a[:, :, :3] - b[:, :, :3]).abs().max()) <= 16 * EPS


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_warm_starts(n):
    """Two warm calls of 20 iterations have the bits of one cold call of 40; WBC_MPC_SHIFT equals the call on a buffer shifted by hand;
    WBC_MPC_COLD ignores the buffer's contents."""
    H = 10
    env = _env(n)
    inp = inputs(n, H, True)
    cfg40, cfg20 = _cfg(horizon=H, iters=40, **BINDING), _cfg(horizon=H, iters=20, **BINDING)
    junk = torch.full((n, 2, H, 20), 5.5, device="cuda")
    want = _call(env, cfg40, inp, warm=junk, flags=abi.MPC_COLD)
    assert _same(_call(env, cfg40, inp), want, ALL_OUT)                             # warm NULL implies cold
    first = _call(env, cfg20, inp, warm=torch.zeros(n, 2, H, 20, device="cuda"), flags=abi.MPC_COLD)
    second = _call(env, cfg20, inp, warm=first["warm"])
    assert _same(second, want)
    w = first["warm"]
    by_hand = torch.cat([w[:, :, 1:], w[:, :, -1:]], dim=2).contiguous()
    shifted = _call(env, cfg20, inp, warm=w, flags=abi.MPC_SHIFT)
    assert _same(shifted, _call(env, cfg20, inp, warm=by_hand))
    assert not torch.equal(shifted["warm"], second["warm"])                         # the shift is not a no-op on these inputs


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_partial_outputs_and_a_non_finite_env(n):
    H = 10
    env = _env(n)
    inp = inputs(n, H, True)
    cfg = _cfg(horizon=H, **BINDING)
    before = [env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")]
    want = _call(env, cfg, inp)
    for which in ((), ("forces",), ("base_acc",), ("status",), ("u", "res"), ("x_pred", "status"), ("forces", "base_acc")):
        got = _call(env, cfg, inp, which=which, workspace=False)
        assert set(got) == set(which) and _same(got, want, which), which
    outs = env.sim.centroidal_mpc(_make_cfg(cfg), _dev(inp["contact"], torch.uint8), _dev(inp["x_ref"]), x0=_dev(inp["x0"]), mass=_dev(inp["mass"]),
                                  inertia=_dev(inp["inertia"]), foot_pos=_dev(inp["foot_pos"]))
    assert len(outs) == 6 and all(torch.equal(a, want[k]) for a, k in zip(outs, ALL_OUT))
    # a non-finite input: status 2 and zeros for that env alone, warm included; its neighbours are unchanged
    e = n // 2
    for key, idx, val in (("x0", (e, 4), np.nan), ("mass", (e,), np.inf), ("inertia", (e, 1, 1), np.nan), ("foot_pos", (e, H - 1, 2, 0), -np.inf),
                          ("x_ref", (e, H - 1, 7), np.nan), ("mass", (e,), -1.0)):
        broken = dict(inp, **{key: inp[key].copy()})
        broken[key][idx] = val
        got = _call(env, cfg, broken, warm=torch.zeros(n, 2, H, 20, device="cuda"))
        full = _call(env, cfg, inp, warm=torch.zeros(n, 2, H, 20, device="cuda"))
        rest = torch.ones(n, dtype=torch.bool, device="cuda"); rest[e] = False
        assert int(got["status"][e]) == mr.STATUS_FAILED, key
        for k in OUTPUTS + ("warm",):
            assert bool((got[k][e] == 0).all()), (key, k)
        for k in ALL_OUT + ("warm",):
            assert torch.equal(got[k][rest], full[k][rest]), (key, k)
    torch.cuda.synchronize()
    for k, t in zip(("ROOT_STATES", "DOF_STATE", "BODY_PARAMS"), before):
        assert torch.equal(env.sim.tensor(k), t), k                                   # the sim's state is read, never written


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n, H = 3, 10
    env = _env(n)
    inp = inputs(n, H, False)
    cfg = _cfg(horizon=H)
    want = _call(env, cfg, dict(inp, mass=None, inertia=None))
    c = _make_cfg(cfg)
    t = {k: _dev(inp[k]) for k in ("x0", "foot_pos", "x_ref")}
    contact = _dev(inp["contact"], torch.uint8)
    outs = [torch.zeros_like(want[k]) for k in ALL_OUT]
    ws = torch.zeros(16 * n, device="cuda")
    warm = torch.zeros(n, 2, H, 20, device="cuda")
    call = lambda: env.sim.centroidal_mpc(c, contact, t["x_ref"], x0=t["x0"], foot_pos=t["foot_pos"], warm=warm, cold=True, forces=outs[0], u=outs[1],
                                          x_pred=outs[2], base_acc=outs[3], res=outs[4], status=outs[5], workspace=ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                     # warm-up off the default stream
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, want[k]) for a, k in zip(outs, ALL_OUT))


@pytest.mark.gpu
def test_every_refusal_leaves_the_buffers_untouched():
    n, H = 3, 10
    env = _env(n)
    L, h = env.sim.L, env.sim.h
    inp = inputs(n, H, True)
    size = dict(forces=12, u=H * 12, x_pred=H * 12, base_acc=6, res=2, warm=2 * H * 20, workspace=16)
    bufs = {k: torch.full((n * size[k] + 8,), SENTINEL, dtype=torch.float32, device="cuda") for k in size}
    bufs["status"] = torch.full((n + 8,), ISENTINEL, dtype=torch.int32, device="cuda")
    tens = {k: _dev(inp[k]) for k in _INPUTS + ("x_ref",)}
    tens["contact"] = _dev(inp["contact"], torch.uint8)
    base = dict(sim=h, cfg=_make_cfg(_cfg(horizon=H)), foot_pos_stages=H, flags=0, stream=None, **{k: t.data_ptr() for k, t in tens.items()},
                **{k: b.data_ptr() for k, b in bufs.items()})
    skip = lambda kw: "foot_pos_stages" in kw and kw.get("cfg") is None and kw["foot_pos_stages"] == 1
    for kw, word in [r for r in _refusals(base) if not skip(r[0])] + [(dict(sim=None), b"sim is NULL")]:
        assert _raw_call(L, base, **kw) == -1, kw
        assert L.wbc_last_error().startswith(b"wbc_sim_centroidal_mpc: ") and word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == (ISENTINEL if k == "status" else SENTINEL)).all()), k


@pytest.mark.gpu
def test_step_is_untouched_by_the_mpc():
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1, trot_schedule
    n = 64
    finals = []
    for use in (False, True):
        cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
        env = WidowGo1(cfg, sim_device="cuda:0", seed=6)
        mpc = env.centroidal_mpc(horizon=10) if use else None
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        for k in range(4):
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                before = [env.sim.tensor(t).clone() for t in ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")]
                sched = trot_schedule(torch.full((n,), 0.1 * k, device="cuda"), 0.5, 0.5, 10, mpc.cfg.dt)
                mpc.solve(sched, vel_cmd=torch.zeros(n, 2, device="cuda"), shift=True)
                torch.cuda.synchronize()
                assert all(torch.equal(env.sim.tensor(t), b) for t, b in zip(("ROOT_STATES", "DOF_STATE", "BODY_PARAMS"), before))
                assert bool(torch.isfinite(mpc.forces).all()) and bool((mpc.status != mr.STATUS_FAILED).all())
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for a, b_ in zip(*finals):
        assert torch.equal(a, b_)


@pytest.mark.gpu
def test_standing_robot_through_the_env():
    """env.centroidal_mpc on a standing robot: status 0, forces inside their cones, sum f_z within 2 % of the env's own m |g| (randomised
    mass included), and base_acc is accepted by env.whole_body_controller."""
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    n = 130
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = n; cfg.terrain.mesh_type = "plane"
    cfg.domain_rand.randomize_base_mass = True
    env = WidowGo1(cfg, sim_device="cuda:0", seed=4)
    rs, ds = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    rs[:, 0, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda"); rs[:, 0, 7:13] = 0.0
    ds[..., 0] = env.default_dof_pos.to(torch.float32); ds[..., 1] = 0.0
    env.sim.set_root_state(rs.contiguous()); env.sim.set_dof_state(ds.contiguous())
    mpc = env.centroidal_mpc(horizon=10)
    forces = mpc.solve(torch.ones(n, 10, 4, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    mass = env.centroidal_inertia()[0]
    assert bool((mpc.status == abi.MPC_STATUS_OK).all()), mpc.residuals.max(0)
    mu = float(mpc.cfg.mu)
    fz = forces[:, :, 2]
    assert bool((fz >= 0).all()) and bool((forces[:, :, 0].abs() <= mu * fz).all()) and bool((forces[:, :, 1].abs() <= mu * fz).all())
    w = mass * G
    print(f"standing: sum f_z / (m |g|) in [{float((fz.sum(1) / w).min()):.4f}, {float((fz.sum(1) / w).max()):.4f}], mass in "
          f"[{float(mass.min()):.2f}, {float(mass.max()):.2f}]")
    assert bool(((fz.sum(1) - w).abs() <= 0.02 * w).all())
    assert float(mass.max() - mass.min()) > 0.5
    tau, nudot, lam, info = env.whole_body_controller(base_acc=mpc.base_acc, stance=torch.ones(n, 4, dtype=torch.bool, device="cuda"))
    torch.cuda.synchronize()
    assert tuple(tau.shape) == (n, 20) and bool(torch.isfinite(tau).all()) and bool(torch.isfinite(lam).all())
