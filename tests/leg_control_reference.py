"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the leg controller that wbc_sim_leg_control computes (include/wbc_sim.h has the
text; the step numbers below are its), batched over envs, in fp64 or -- the same text, `dtype=np.float32` -- in fp32 as the yardstick of
what single precision costs. Nothing here comes from the kernel: the leg kinematics and Jacobians are estimator_reference's walk of
widowgo1_model.json (through contact_reference.leg_jacobians), the 3 x 3 factorisation is contact_reference.chol3_solve.

control() also returns the MAGNITUDES an error is judged against (2^-24 mag): per entry, the sum of the absolute sizes of the terms summed
into it, with the size of a term that is itself a sum carried along (|.| entrywise, reach_i the summed lengths of leg i's offsets):
    foot      p: |b| + reach_i;   pd: |v| + (sum |w_b| + sum of the leg's |qd|) reach_i            (estimator_reference's sizes)
    F_i       kp o (|pos_ref| + mag(p)) + kd o (|vel_ref| + mag(pd))
    leg_force (1 - w) mag(F) + w |f|           (G_i; f after the clip)
    tau_fb    |J_i^T| mag(G_i)
    tau_ff    (1 - w) |M_i| |A^-1| (|J_i^T| (|acc_ref| + |acc_bias|));  0 where FF_SINGULAR
    tau leg   mag(tau_fb) + mag(tau_ff) + |bias| + w kd_stance |qd|
    tau arm   |bias| + kp_arm (|q_des| + |q|) + kd_arm |qd|
A clamped torque keeps the size of what was clamped; a finger's entry is exact and is judged against 1e-30.
`diag` holds what thinness is judged from: the unclamped torques, the clip's edges, the weights."""
import numpy as np

import contact_reference as cr
import estimator_reference as er

NFEET, NDOF, NCOL, NRB = 4, 20, 26, 27
CLIP = 1
INFO_FAILED, INFO_FORCE_CLIPPED, INFO_FF_SINGULAR, INFO_SATURATED = 2, 16, 256, 4096
CFG_FIELDS = ("kp", "kd", "kd_stance", "damping", "fz_min", "fz_max", "mu", "kp_arm", "kd_arm", "arm_q_default")
CFG_COUNTS = (3, 3, 1, 1, 1, 1, 1, 6, 6, 6)
OUTPUTS = ("tau", "leg_force", "foot")                                                 # the continuous ones
EPS = 2.0 ** -24


def dof_groups(model):
    """(legs [4, 3], arm [6], fingers [2], feet_rb [4], limit_col {dof: column of tau_limit}) from the model alone."""
    _, _, _, legs = er.leg_kinematics(model, np.zeros((1, NDOF)), None, jac=True)
    driven = sorted({int(model.body_dof[b]) for b in range(1, len(model.parent))})
    in_leg = set(int(d) for d in legs.reshape(-1))
    arm = [d for d in driven if d not in in_leg]
    fingers = [d for d in range(NDOF) if d not in driven]
    feet_rb = [rb for rb, name in enumerate(model.rb_names) if "foot" in name]
    return legs, np.array(arm), np.array(fingers), np.array(feet_rb), {d: i for i, d in enumerate(driven)}


def clip_force(f, fz_min, fz_max, mu, dtype=np.float64):
    """Step 3's clip: the output rule of wbc_sim_centroidal_mpc. Returns (clipped, changed [..., 3])."""
    D = dtype
    f = np.asarray(f, dtype=D)
    fz = np.minimum(np.maximum(f[..., 2], D(fz_min)), D(fz_max))
    lim = (D(mu) * fz).astype(D)
    out = np.stack([np.minimum(np.maximum(f[..., 0], -lim), lim), np.minimum(np.maximum(f[..., 1], -lim), lim), fz], axis=-1).astype(D)
    return out, out != f


def feed_forward(J, M, a, damping, dtype=np.float64):
    """Step 6 without the weight: (M qdd [..., 3], qdd [..., 3], ok, mag [..., 3]) with qdd = (J^T J + damping^2 I)^-1 J^T a."""
    D = dtype
    J, M, a = np.asarray(J, dtype=D), np.asarray(M, dtype=D), np.asarray(a, dtype=D)
    A = np.einsum("...ik,...il->...kl", J, J) + (D(damping) * D(damping)) * np.eye(3, dtype=D)
    rhs = np.einsum("...ik,...i->...k", J, a)
    with np.errstate(all="ignore"):
        y, ok = cr.chol3_solve(A, rhs)
        ok = ok & np.isfinite(y).all(-1)
        t = ((M[..., :, 0] * y[..., 0:1] + M[..., :, 1] * y[..., 1:2]) + M[..., :, 2] * y[..., 2:3]).astype(D)
        A64 = np.where(ok[..., None, None], A.astype(np.float64), np.eye(3))
        ymag = np.einsum("...kl,...l->...k", np.abs(np.linalg.pinv(A64, hermitian=True)), np.einsum("...ik,...i->...k", np.abs(J.astype(np.float64)), np.abs(a.astype(np.float64))))
        mag = np.einsum("...kl,...l->...k", np.abs(M.astype(np.float64)), ymag)
    return np.where(ok[..., None], t, 0).astype(D), y, ok, np.where(ok[..., None], mag, 0.0)


def control(model, cfg, quat, dof, base_pos, base_vel, ang_vel, forces=None, swing_ref=None, stance=None, tau_bias=None, mass_matrix=None,
            acc_bias=None, arm_q_des=None, tau_limit=None, clip=False, dtype=np.float64):
    """One call of wbc_sim_leg_control for a batch. Returns a dict: every output, `mag` and `diag` (module docstring)."""
    D = dtype
    f = lambda a: np.asarray(a, dtype=D)                                               # noqa: E731
    assert mass_matrix is None or swing_ref is not None
    c = {k: (f(cfg[k]) if n > 1 else D(cfg[k])) for k, n in zip(CFG_FIELDS, CFG_COUNTS)}
    legs, arm, fingers, feet_rb, limit_col = dof_groups(model)
    b, v, ww, dof = f(base_pos), f(base_vel), f(ang_vel), f(dof)
    n = b.shape[0]
    lreach = er.reach(model)
    a64 = lambda a: np.abs(np.asarray(a, dtype=np.float64))                            # noqa: E731

    with np.errstate(all="ignore"):
        # 1 kinematics
        R = er.quat_to_mat(quat, D)
        P, J, dofs = cr.leg_jacobians(model, quat, dof, b, D)
        assert (dofs == legs).all()
        fk, vrel = er.leg_kinematics(model, dof[:, :, 0], dof[:, :, 1], dtype=D)
        wb = np.einsum("nji,nj->ni", R, ww)
        Pd = (v[:, None, :] + np.einsum("nij,nfj->nfi", R, np.cross(wb[:, None, :], fk) + vrel)).astype(D)
        qd = dof[:, dofs, 1]                                                           # [N, 4, 3]
        finite = np.isfinite(f(quat)).all(1) & np.isfinite(b).all(1) & np.isfinite(v).all(1) & np.isfinite(ww).all(1)
        finite &= np.isfinite(dof[:, dofs.reshape(-1)]).all((1, 2)) & np.isfinite(P).all((1, 2)) & np.isfinite(Pd).all((1, 2))
        pmag = a64(b)[:, None, :] + lreach[None, :, None]
        rate = a64(wb).sum(-1)[:, None] + a64(qd).sum(-1)
        pdmag = a64(v)[:, None, :] + (rate * lreach[None, :])[:, :, None]
        # 2 weight
        w = np.ones((n, NFEET), dtype=D)
        s_raw = np.ones((n, NFEET))
        if stance is not None:
            s = f(stance)
            s_raw = s.astype(np.float64)
            finite &= np.isfinite(s).all(1)
            w = np.minimum(np.maximum(s, D(0)), D(1)).astype(D)
        # 3 stance force
        fs = np.zeros((n, NFEET, 3), dtype=D)
        clipped = np.zeros((n, NFEET), dtype=bool)
        edges = None
        if forces is not None:
            fin = f(forces)
            finite &= np.isfinite(fin).all((1, 2))
            fs = fin
            if clip:
                fs, changed = clip_force(fin, c["fz_min"], c["fz_max"], c["mu"], D)
                clipped = changed.any(-1) & (w > 0)
                edges = dict(fin=fin.astype(np.float64), lim=float(c["mu"]) * fs[..., 2].astype(np.float64))
        # 4 swing force
        F = np.zeros((n, NFEET, 3), dtype=D)
        Fmag = np.zeros((n, NFEET, 3))
        aref = np.zeros((n, NFEET, 3), dtype=D)
        if swing_ref is not None:
            sr = f(swing_ref)
            rp, rv = sr[:, :, 0:3], sr[:, :, 3:6]
            finite &= np.isfinite(sr[:, :, 0:6]).all((1, 2))
            F = (c["kp"] * (rp - P) + c["kd"] * (rv - Pd)).astype(D)
            Fmag = c["kp"].astype(np.float64) * (a64(rp) + pmag) + c["kd"].astype(np.float64) * (a64(rv) + pdmag)
            if mass_matrix is not None:
                aref = sr[:, :, 6:9]
                finite &= np.isfinite(aref).all((1, 2))
        # 5 feedback torque
        sw = (D(1) - w).astype(D)
        G = (F * sw[..., None] - fs * w[..., None]).astype(D)
        Gmag = sw.astype(np.float64)[..., None] * Fmag + w.astype(np.float64)[..., None] * a64(fs)
        t = np.einsum("nfik,nfi->nfk", J, G).astype(D)
        tmag = np.einsum("nfik,nfi->nfk", a64(J), Gmag)
        # 6 feed-forward
        singular = np.zeros((n, NFEET), dtype=bool)
        qdd = np.zeros((n, NFEET, 3), dtype=D)
        if mass_matrix is not None:
            acc, accmag = aref, a64(aref)
            if acc_bias is not None:
                ab = f(acc_bias)[:, feet_rb, 0:3]
                finite &= np.isfinite(ab).all((1, 2))
                acc = (aref - ab).astype(D)
                accmag = a64(aref) + a64(ab)
            Mfull = f(mass_matrix)
            idx = 6 + dofs                                                             # [4, 3]
            Mi = Mfull[:, idx[:, :, None], idx[:, None, :]]                            # [N, 4, 3, 3]
            finite &= np.isfinite(Mi).all((1, 2, 3))
            # the magnitude is that of J^T acc with acc's own size: feed_forward takes |a|, so hand it accmag through a second call
            tff, qdd, ok, _ = feed_forward(J, Mi, acc, c["damping"], D)
            _, _, _, ffmag = feed_forward(J.astype(np.float64), Mi.astype(np.float64), accmag, float(c["damping"]))
            ffmag = np.where(ok[..., None], ffmag, 0.0)
            singular = ~ok
            t = (t + sw[..., None] * tff).astype(D)
            tmag = tmag + sw.astype(np.float64)[..., None] * ffmag
        # 7 leg joints
        if tau_bias is not None:
            tb = f(tau_bias)
            bl = tb[:, 6 + dofs]
            finite &= np.isfinite(bl).all((1, 2))
            t = (t + bl).astype(D)
            tmag = tmag + a64(bl)
        kds = (w * c["kd_stance"]).astype(D)
        t = (t - kds[..., None] * qd).astype(D)
        tmag = tmag + a64(kds)[..., None] * a64(qd)
        # 8 arm
        q_arm, qd_arm = dof[:, arm, 0], dof[:, arm, 1]
        qdes = np.broadcast_to(c["arm_q_default"], (n, 6)).astype(D) if arm_q_des is None else f(arm_q_des)
        ba = f(tau_bias)[:, 6 + arm] if tau_bias is not None else np.zeros((n, 6), dtype=D)
        finite &= np.isfinite(q_arm).all(1) & np.isfinite(qd_arm).all(1) & np.isfinite(qdes).all(1) & np.isfinite(ba).all(1)
        ta = ((ba + c["kp_arm"] * (qdes - q_arm)) - c["kd_arm"] * qd_arm).astype(D)
        tamag = a64(ba) + c["kp_arm"].astype(np.float64) * (a64(qdes) + a64(q_arm)) + c["kd_arm"].astype(np.float64) * a64(qd_arm)
        tau = np.zeros((n, NDOF), dtype=D)
        taumag = np.full((n, NDOF), 1e-30)
        tau[:, dofs.reshape(-1)] = t.reshape(n, 12)
        taumag[:, dofs.reshape(-1)] = tmag.reshape(n, 12)
        tau[:, arm] = ta
        taumag[:, arm] = tamag
        raw = tau.astype(np.float64).copy()
        # 9 limit
        sat_leg, sat_arm = np.zeros((n, NFEET), dtype=bool), np.zeros(n, dtype=bool)
        limits = None
        if tau_limit is not None:
            lim = f(tau_limit)
            finite &= (np.isfinite(lim) & (lim >= 0)).all(1)
            full = np.full((n, NDOF), np.inf, dtype=D)
            for d, col in limit_col.items():
                full[:, d] = lim[:, col]
            clamped = np.minimum(np.maximum(tau, -full), full).astype(D)
            changed = clamped != tau
            sat_leg = changed[:, dofs].any(-1)
            sat_arm = changed[:, arm].any(-1)
            tau = clamped
            limits = full.astype(np.float64)
        finite &= np.isfinite(tau).all(1) & np.isfinite(G).all((1, 2))
    failed = ~finite
    shift = np.arange(NFEET)
    bits = lambda m, base: (m * (base << shift)).sum(-1)                              # noqa: E731
    info = (bits(clipped, INFO_FORCE_CLIPPED) + bits(singular, INFO_FF_SINGULAR) + bits(sat_leg, INFO_SATURATED) +
            sat_arm * (INFO_SATURATED << 4)).astype(np.int64)
    foot = np.concatenate([P, Pd], axis=-1).astype(D)
    out = dict(tau=tau.astype(D), leg_force=G, foot=foot, info=info)
    if failed.any():
        for k in OUTPUTS:
            out[k] = out[k].copy()
            out[k][failed] = 0
        out["info"][failed] = INFO_FAILED
    out["mag"] = dict(tau=np.maximum(taumag, 1e-30), leg_force=np.maximum(Gmag, 1e-30), foot=np.concatenate([pmag, pdmag], axis=-1))
    out["diag"] = dict(failed=failed, jac=J, dofs=dofs, arm=arm, fingers=fingers, w=w.astype(np.float64), stance=s_raw, raw_tau=raw, limits=limits, edges=edges,
                       clipped=clipped, singular=singular, sat_leg=sat_leg, sat_arm=sat_arm, qdd=qdd, foot_pos=P, foot_vel=Pd, feet_rb=feet_rb)
    return out


def ratios(got, ref, keep=None):
    """{output: the largest |got - ref| / (2^-24 mag)} over the entries kept (keep: {output: bool mask shaped like it}, None: all)."""
    out = {}
    for k in OUTPUTS:
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)) / (EPS * ref["mag"][k])
        if keep is not None:
            err = np.where(keep[k], err, 0.0)
        assert not np.isnan(err).any(), k
        out[k] = float(err.max()) if err.size else 0.0
    return out
