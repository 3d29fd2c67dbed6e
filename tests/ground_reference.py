"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the blind terrain estimate that wbc_sim_ground_estimate computes
(include/wbc_sim.h has the text; the step numbers below are its), batched over envs, in fp64 or -- the same text, `dtype=np.float32` -- in
fp32 as the yardstick of what single precision costs. Nothing here comes from the kernel: the leg kinematics are estimator_reference's walk
of widowgo1_model.json, the 2 x 2 factorisation is written out here.

estimate() also returns the MAGNITUDES an error is judged against (2^-24 mag): the summed sizes of the terms that make up each entry.
A foot origin p_i = b + R fk_i is made of terms of size P_i = |b| + reach_i (per coordinate |b_k| + reach_i); a contact point that is
latched in this call (a standing foot, a reset) carries that size, F_i = P_i, a stored one is an exact input, F_i = 0. From there, per
coordinate, everything ANCHORED is built from differences, not from |m_i|:
    e_i = m_i - m_0         E_i = |e_i| + F_i + F_0
    r = sum w e / W         Rm = sum w_i E_i / W
    d_i = e_i - r           D_i = E_i + Rm
    d_u d_v                 X_uv = |d_u| D_v + D_u |d_v| (what a rounding of each factor moves the product by)
    a = A^-1 rhs            Am = |A^-1| (sum w X_xy,z + lw |a_prev| + (sum w X_xy,xy + lw I) |a|), plus |a| where a was clamped
    a0 = m_0,z + r_z        A0 = |m_0,z| + F_0,z + Rm_z
    a point x -> g          G = |x - m_0| + (its own size: P_i for a foot origin, 0 for b_xy and the query points) + F_0 + Rm   (xy)
    z(x)                    Z = A0 + sum_k (Am_k |g_k| + |a_k| G_k)
    normal                  1 + Am_1 + Am_2 (every entry)
    ground_i                Z at p_i
    residual_i              D_i,z + sum_k (Am_k |d_i,k| + |a_k| D_i,k)
    trunk                   Z at b; |b_z| + Z + |b_z - z| (1 + Am_1 + Am_2); twice Am_1 + Am_2 + (|a_1| + |a_2|) / |(R_00, R_10)|; 1; 1
    theta_ref               tilt_gain (Am_1 + Am_2 + |a|) for the first two entries, 1 for the zero
    query_z                 Z at the query point
    state                   m_i: P_i where latched, |m_i| where kept; t_i: |t_i| + dt; reserved: 1; anchor: |m_0| + F_0 + Rm (xy): a world
                            coordinate, the one entry judged against |m|; a0: A0; a1, a2: Am
Magnitudes have a floor of 1e-30 so that an exact zero is judged as one. `diag` holds what thinness is judged from: |a| before
the clamp with Am_1 + Am_2, and the pivot d1 = A11 - l A10, l = A10 / A00, with the sizes of its terms' errors, X_yy + 2 |l| X_xy + l^2 X_xx
(sums over the feet, lw included)."""
import numpy as np

import estimator_reference as er

NS, NFEET = 32, 4
SERIES = 1e-4
INFO_RESET, INFO_FAILED, INFO_DEGENERATE, INFO_CLAMPED, INFO_LATCHED = 1, 2, 4, 8, 16
CFG_FIELDS = ("dt", "c_on", "tau_age", "lambda", "slope_max", "tilt_gain")
OUTPUTS = ("normal", "ground", "residual", "trunk", "theta_ref", "query_z", "state")      # the continuous ones
EPS = 2.0 ** -24


def sum4(v):
    """(s_0 + s_1) + (s_2 + s_3) over axis 1."""
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def chol2_solve(A00, A10, A11, b0, b1):
    """(a1, a2, ok): the 2 x 2 system by the written-out Cholesky factorisation of step 4; ok False where a pivot is not a positive finite
    number or the solution is not finite (a is then garbage)."""
    with np.errstate(all="ignore"):
        l00 = np.sqrt(A00); l10 = A10 / l00
        d1 = A11 - l10 * l10; l11 = np.sqrt(d1)
        z0 = b0 / l00; z1 = (b1 - l10 * z0) / l11
        y1 = z1 / l11; y0 = (z0 - l10 * y1) / l00
        ok = np.isfinite(A00) & (A00 > 0) & np.isfinite(d1) & (d1 > 0) & np.isfinite(y0) & np.isfinite(y1)
    return y0, y1, ok, d1


def foot_positions(model, quat, dof, base_pos, dtype=np.float64):
    """Step 1: p [N, 4, 3] the foot origins, R [N, 3, 3], the [4, 3] DoF indices of the legs."""
    D = dtype
    dof = np.asarray(dof, dtype=D)
    R = er.quat_to_mat(quat, D)
    fk, _, _, dofs = er.leg_kinematics(model, dof[:, :, 0], None, jac=True, dtype=D)
    p = np.asarray(base_pos, dtype=D)[:, None, :] + np.einsum("nij,nfj->nfi", R, fk)
    return p.astype(D), R, dofs


def tilt_factor(s, dtype=np.float64):
    """g(s) = atan(s) / s, its series 1 - s^2 / 3 below SERIES."""
    D = dtype
    s = np.asarray(s, dtype=D)
    with np.errstate(all="ignore"):
        return np.where(s < D(SERIES), D(1) - s * s / D(3), np.arctan(s) / s).astype(D)


def fit(m, t, a_prev, cfg, dtype=np.float64):
    """Steps 3 (the weights) and 4 on contact points m [N, 4, 3] with ages t [N, 4] and the previous slope a_prev [N, 2]. Returns a dict:
    w, W, m0, r, d, a (after DEGENERATE and the clamp), a_fit (before both), ok, clamped, the system (A00, A10, A11, b0, b1, d1)."""
    D = dtype
    m, t, ap = np.asarray(m, dtype=D), np.asarray(t, dtype=D), np.asarray(a_prev, dtype=D)
    with np.errstate(all="ignore"):
        tmin = t.min(axis=1, keepdims=True)
        w = np.exp(-(t - tmin) / D(cfg["tau_age"])).astype(D)
        W = sum4(w)
        m0 = m[:, 0]
        e = m - m0[:, None, :]
        r = np.stack([sum4(w * e[:, :, k]) / W for k in range(3)], axis=-1).astype(D)
        d = (e - r[:, None, :]).astype(D)
        S = lambda u, v: sum4((w * d[:, :, u]) * d[:, :, v])                            # noqa: E731
        lw = D(cfg["lambda"]) * W
        A00, A10, A11 = S(0, 0) + lw, S(0, 1), S(1, 1) + lw
        b0, b1 = S(0, 2) + lw * ap[:, 0], S(1, 2) + lw * ap[:, 1]
        y0, y1, ok, d1 = chol2_solve(A00, A10, A11, b0, b1)
        a_fit = np.stack([y0, y1], axis=-1)
        a = np.where(ok[:, None], a_fit, ap).astype(D)
        sl = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
        clamped = sl > D(cfg["slope_max"])
        k = np.where(clamped, D(cfg["slope_max"]) / sl, D(1)).astype(D)
        a = np.where(clamped[:, None], a * k[:, None], a).astype(D)
    return dict(w=w, W=W, m0=m0, r=r, d=d, a=a, a_fit=a_fit, ok=ok, clamped=clamped, slope_before_clamp=sl, lw=lw, A00=A00, A10=A10, A11=A11,
                b0=b0, b1=b1, d1=d1)


def estimate(model, cfg, state, quat, dof, base_pos, contact, reset=None, query_xy=None, dtype=np.float64):
    """One call of wbc_sim_ground_estimate for a batch. state [N, 32]; reset: None, True (every env) or a mask [N]; query_xy [N, Q, 2] or
    None. Returns a dict: the new `state`, every output, `mag` and `diag` (module docstring)."""
    D = dtype
    f = lambda v: np.asarray(v, dtype=D)                                               # noqa: E731
    c = {k: D(cfg[k]) for k in CFG_FIELDS}
    state0 = f(state)
    n = state0.shape[0]
    b, dof, con = f(base_pos), f(dof), f(contact)
    rs = np.zeros(n, dtype=bool) if reset is None else (np.ones(n, dtype=bool) if reset is True else np.asarray(reset) != 0)
    q = None if query_xy is None else f(query_xy)
    nq = 0 if q is None else q.shape[1]
    feet = state0[:, :20].reshape(n, NFEET, 5)

    with np.errstate(all="ignore"):
        # 1 kinematics
        p, R, dofs = foot_positions(model, quat, dof, b, D)
        finite = np.isfinite(p).all((1, 2)) & np.isfinite(con).all(1)
        finite &= np.where(rs, True, np.isfinite(feet[:, :, 0:4]).all((1, 2)) & np.isfinite(state0[:, 23:25]).all(1))
        if q is not None:
            finite &= np.isfinite(q).all((1, 2))
        # 2 reset, 3 latch
        stand = con >= c["c_on"]
        fresh = stand | rs[:, None]
        m = np.where(fresh[:, :, None], p, feet[:, :, 0:3]).astype(D)
        t = np.where(stand, D(0), np.where(rs[:, None], D(0), feet[:, :, 3]) + c["dt"]).astype(D)
        ap = np.where(rs[:, None], D(0), state0[:, 23:25]).astype(D)
        # 4 fit
        F = fit(m, t, ap, cfg, D)
        w, W, m0, r, d, a = F["w"], F["W"], F["m0"], F["r"], F["d"], F["a"]
        a0 = (m0[:, 2] + r[:, 2]).astype(D)
        anchor = (m0[:, 0:2] + r[:, 0:2]).astype(D)
        plane = lambda xy: (a0[:, None] + (a[:, None, 0] * ((xy[:, :, 0] - m0[:, None, 0]) - r[:, None, 0]) +       # noqa: E731
                                           a[:, None, 1] * ((xy[:, :, 1] - m0[:, None, 1]) - r[:, None, 1]))).astype(D)
        # 5 outputs
        s2 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        s = np.sqrt(s2)
        ninv = D(1) / np.sqrt(D(1) + s2)
        nrm = np.stack([-a[:, 0] * ninv, -a[:, 1] * ninv, ninv], axis=-1).astype(D)
        normal = np.repeat(nrm[:, None, :], NFEET, axis=1)
        ground = plane(p[:, :, 0:2])
        residual = (d[:, :, 2] - (a[:, None, 0] * d[:, :, 0] + a[:, None, 1] * d[:, :, 1])).astype(D)
        zb = plane(b[:, None, 0:2])[:, 0]
        hn = np.sqrt(R[:, 0, 0] * R[:, 0, 0] + R[:, 1, 0] * R[:, 1, 0])
        ch = np.where(hn > 0, R[:, 0, 0] / hn, D(1)); sh = np.where(hn > 0, R[:, 1, 0] / hn, D(0))
        zero = np.zeros(n, dtype=D)
        trunk = np.stack([zb, (b[:, 2] - zb) * ninv, a[:, 0] * ch + a[:, 1] * sh, a[:, 1] * ch - a[:, 0] * sh, zero, zero], axis=-1).astype(D)
        g = c["tilt_gain"] * tilt_factor(s, D)
        theta = np.stack([g * a[:, 1], D(0) - g * a[:, 0], zero], axis=-1).astype(D)
        query_z = plane(q) if q is not None else np.zeros((n, 0), dtype=D)
        new_feet = np.concatenate([m, t[:, :, None], np.zeros((n, NFEET, 1), dtype=D)], axis=-1).reshape(n, 20)
        new_state = np.concatenate([new_feet, anchor, a0[:, None], a, np.zeros((n, NS - 25), dtype=D)], axis=-1).astype(D)

        # magnitudes, fp64 throughout
        A_ = lambda v: np.abs(np.asarray(v, dtype=np.float64))                         # noqa: E731
        reach = er.reach(model)
        Pm = A_(b)[:, None, :] + reach[None, :, None]                                   # [N, 4, 3]
        Fm = np.where(fresh[:, :, None], Pm, 0.0)
        w64, W64 = w.astype(np.float64), W.astype(np.float64)
        Em = A_(m - m0[:, None, :]) + Fm + Fm[:, :1, :]
        Rm = (w64[:, :, None] * Em).sum(1) / W64[:, None]
        Dm = Em + Rm[:, None, :]
        lw = F["lw"].astype(np.float64)
        Aabs = np.zeros((n, 2, 2)); rhs = np.zeros((n, 2))
        d64 = A_(d)
        prod = lambda u, v: (w64 * (d64[:, :, u] * Dm[:, :, v] + Dm[:, :, u] * d64[:, :, v])).sum(1)   # noqa: E731  (the size of d_u d_v's error terms)
        for u in range(2):
            rhs[:, u] = prod(u, 2) + lw * A_(ap)[:, u]
            for v in range(2):
                Aabs[:, u, v] = prod(u, v) + (lw if u == v else 0.0)
        A64 = np.zeros((n, 2, 2))
        A64[:, 0, 0], A64[:, 0, 1], A64[:, 1, 0], A64[:, 1, 1] = F["A00"], F["A10"], F["A10"], F["A11"]
        A64 = np.where((F["ok"] & np.isfinite(A64).all((1, 2)))[:, None, None], A64, np.eye(2))
        Am = np.einsum("nuv,nv->nu", np.abs(np.linalg.inv(A64)), rhs + np.einsum("nuv,nv->nu", Aabs, A_(F["a_fit"])))
        Am = np.where(F["ok"][:, None], Am, A_(ap)) + np.where(F["clamped"][:, None], A_(a), 0.0)
        Am = np.maximum(np.nan_to_num(Am, nan=1.0, posinf=1e300), 1e-30)
        A0m = A_(m0[:, 2]) + Fm[:, 0, 2] + Rm[:, 2]

        def zmag(xy, own):                                                           # xy [N, K, 2], own [N, K, 2]
            gk = A_((xy - m0[:, None, 0:2]) - r[:, None, 0:2])
            Gk = A_(xy - m0[:, None, 0:2]) + own + Fm[:, :1, 0:2] + Rm[:, None, 0:2]
            return A0m[:, None] + (Am[:, None, :] * gk + A_(a)[:, None, :] * Gk).sum(-1)

        nmag = 1.0 + Am.sum(1)
        zbm = zmag(b[:, None, 0:2], np.zeros((n, 1, 2)))[:, 0]
        smag = Am.sum(1) + A_(a).sum(1) / np.maximum(hn.astype(np.float64), 1e-30)
        one = np.ones(n)
        tg = float(c["tilt_gain"])
        mag = dict(
            normal=np.repeat(np.repeat(nmag[:, None, None], NFEET, axis=1), 3, axis=2),
            ground=zmag(p[:, :, 0:2], Pm[:, :, 0:2]),
            residual=Dm[:, :, 2] + (Am[:, None, :] * A_(d[:, :, 0:2]) + A_(a)[:, None, :] * Dm[:, :, 0:2]).sum(-1),
            trunk=np.stack([zbm, A_(b[:, 2]) + zbm + A_(b[:, 2] - zb) * nmag, smag, smag, one, one], axis=-1),
            theta_ref=np.stack([tg * (Am.sum(1) + A_(s))] * 2 + [one], axis=-1),
            query_z=zmag(q, np.zeros((n, nq, 2))) if q is not None else np.zeros((n, 0)))
        feet_mag = np.concatenate([np.where(fresh[:, :, None], Pm, A_(m)), (A_(t) + float(c["dt"]))[:, :, None], np.ones((n, NFEET, 1))],
                                  axis=-1).reshape(n, 20)
        mag["state"] = np.concatenate([feet_mag, A_(m0[:, 0:2]) + Fm[:, 0, 0:2] + Rm[:, 0:2], A0m[:, None], Am, np.ones((n, NS - 25))], axis=-1)
        mag = {k: np.maximum(np.nan_to_num(v, nan=1.0, posinf=1e300), 1e-30) for k, v in mag.items()}

        lr = np.nan_to_num(np.abs(F["A10"].astype(np.float64) / F["A00"].astype(np.float64)), nan=1.0, posinf=1e300)   # d1 = A11 - (A10 / A00) A10
    failed = ~finite
    info = (np.where(rs, INFO_RESET, 0) + np.where(~F["ok"], INFO_DEGENERATE, 0) + np.where(F["clamped"], INFO_CLAMPED, 0) +
            (stand * (INFO_LATCHED << np.arange(NFEET))).sum(-1)).astype(np.int64)
    out = dict(state=new_state, normal=normal, ground=ground, residual=residual, trunk=trunk, theta_ref=theta, query_z=query_z, info=info)
    if failed.any():
        for k in ("normal", "ground", "residual", "trunk", "theta_ref", "query_z"):
            out[k][failed] = 0
        out["state"][failed] = state0[failed]
        out["info"][failed] = INFO_FAILED
    out["mag"] = mag
    out["diag"] = dict(failed=failed, foot_pos=p, dofs=dofs, stand=stand, contact=con.astype(np.float64), fit=F, a=a.astype(np.float64),
                       slope=F["slope_before_clamp"].astype(np.float64), slope_mag=Am.sum(1), pivot=F["d1"].astype(np.float64),
                       pivot_mag=Aabs[:, 1, 1] + 2 * lr * Aabs[:, 0, 1] + lr * lr * Aabs[:, 0, 0], w=w64, W=W64)
    return out


def ratios(got, ref, keep=None):
    """{output: the largest |got - ref| / (2^-24 mag)} over the entries kept (keep: bool mask [N] of envs, None: all)."""
    out = {}
    for k in OUTPUTS:
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)) / (EPS * ref["mag"][k])
        if keep is not None:
            err = err[keep]
        assert not np.isnan(err).any(), k
        out[k] = float(err.max()) if err.size else 0.0
    return out
