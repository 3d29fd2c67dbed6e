"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the foot slip detector and friction estimate that wbc_sim_slip_detect computes
(include/wbc_sim.h has the text; the step numbers below are its), batched over envs, in fp64 or -- the same text, `dtype=np.float32` -- in
fp32 as the yardstick of what single precision costs. Nothing here comes from the kernel: the leg kinematics are estimator_reference's walk
of widowgo1_model.json, erf is the C library's (rounded to the working precision).

detect() also returns the MAGNITUDES an error is judged against (2^-24 mag), per foot unless said otherwise, each built from the sizes of
the terms that are summed into the entry, never from the result (|.|: the Euclidean length of a vector, reach_i: the summed lengths of leg
i's joint offsets and foot offset, estimator_reference.reach):
    foot_vel   U_i = |v| + (|w| + sum_k |qd_k|) reach_i, for each of the three coordinates
    speed      S_i = 2 G_i, G_i = U_i + common_mode (sum_j cw_j U_j) / (sum_j cw_j) (the second term only where the common mode is taken
               out): g_i and n_i (n_i . g_i) are of that size each
    prob       Pm_i = max(1, |p| + alpha (max(1, c_i pdf(x) (S_i + v_slip) / sigma_v) + |p|)), x = (s_i - v_slip) / sigma_v, p the stored value
    weight     Pm_i (c_i <= 1)
    distance   |d| + S_i dt where the flag is set, |d| elsewhere (d the value after a touchdown's zero)
    force      fn: Fn = sum_k |n_k| |f_k|;  ft: Ft = |(|f_k| + |n_k| Fn)_k|;  rho: Rho = (Ft + rho Fn) / |fn|
    mu_lower   gamma |m_i| + (Rho where the maximum was taken)
    w_i        Wm_i = gamma |w_i| + (Pm_i where it was added to)
    mu_i       Mm_i = |mu_i| + k (Rho + |mu_i|) + |rho - mu_i| (k + (Pm_i gamma w_i + p gamma |w_i|) / w_new^2), k = p / w_new, where the
               mean moved; |mu_i| elsewhere
    mu_env     ((sum_i (Wm_i |mu_i| + w_i Mm_i)) + |mu_env| sum_i Wm_i) / W where W >= w_min, 1 elsewhere; and sum_i Wm_i for W (per env)
    mu         mu_scale (Mm_i where w_i >= w_min, mu_env's elsewhere)
    state      (Pm_i, 1, |t| + dt, 1, distance's, Mm_i, Wm_i, mu_lower's)
Magnitudes have a floor of 1e-30 so that an exact zero is judged as one. `diag` holds what thinness is judged from (judge())."""
import math

import numpy as np

import estimator_reference as er

NS, NFEET = 8, 4
INFO_RESET, INFO_FAILED, INFO_NO_FORCE, INFO_START, INFO_END, INFO_SLIPPING, INFO_MU_VALID = 1, 2, 4, 16, 256, 4096, 65536
CFG_FIELDS = ("dt", "c_on", "v_slip", "sigma_v", "alpha", "p_on", "p_off", "t_dwell", "common_mode", "fn_min", "gamma", "w_min", "mu_prior",
              "mu_min", "mu_max", "mu_scale")
OUTPUTS = ("prob", "weight", "foot_vel", "speed", "distance", "mu", "mu_lower", "mu_env", "state")      # the continuous ones
EPS = 2.0 ** -24
_erf64 = np.vectorize(math.erf, otypes=[np.float64])


def erf(x, dtype=np.float64):
    return _erf64(np.asarray(x, dtype=np.float64)).astype(dtype)


def Phi(x, dtype=np.float64):
    """(1/2) (1 + erf(x / sqrt 2))."""
    D = dtype
    return (D(0.5) * (D(1) + erf(np.asarray(x, dtype=D) / D(np.sqrt(2.0)), D))).astype(D)


def pdf(x):
    return np.exp(-0.5 * np.asarray(x, dtype=np.float64) ** 2) / np.sqrt(2 * np.pi)


def sum4(v):
    """(x_0 + x_1) + (x_2 + x_3) over axis 1."""
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def foot_positions(model, quat, dof, base_pos, dtype=np.float64):
    """The foot origins p_i = b + R fk_i(q) [N, 4, 3]: what step 1's velocity is the time derivative of (the call itself never forms
    them: it has no position argument)."""
    D = dtype
    dof = np.asarray(dof, dtype=D)
    R = er.quat_to_mat(quat, D)
    fk, _ = er.leg_kinematics(model, dof[:, :, 0], None, dtype=D)
    return np.asarray(base_pos, dtype=D)[:, None, :] + np.einsum("nij,nfj->nfi", R, fk)


def lever_lengths(model, q):
    """(|fk_i| [N, 4], |fk_i - o_k| [N, 4, 3]) in fp64: the levers of the trunk's rotation and of each leg joint on the foot origin."""
    q = np.asarray(q, dtype=np.float64)
    n = q.shape[0]
    fkl, lev = np.zeros((n, NFEET)), np.zeros((n, NFEET, 3))
    for i, (chain, off) in enumerate(er.legs(model)):
        E = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
        p = np.zeros((n, 3))
        origins = []
        for axis, dof, xyz in chain:
            p = p + E @ xyz
            E = E @ er._axis_rot(axis, q[:, dof])
            origins.append(p)
        fk = p + E @ off
        fkl[:, i] = np.linalg.norm(fk, axis=1)
        for k, o in enumerate(origins):
            lev[:, i, k] = np.linalg.norm(fk - o, axis=1)
    return fkl, lev


def foot_velocity(model, quat, dof, base_vel, ang_vel, ang_world=False, dtype=np.float64):
    """Step 1: (u [N, 4, 3], R, fk [N, 4, 3], w [N, 3] in trunk axes, dofs [4, 3]). ang_world: ang_vel is in world axes (the sim's own)
    and is turned by R^T first."""
    D = dtype
    dof = np.asarray(dof, dtype=D)
    R = er.quat_to_mat(quat, D)
    w = np.asarray(ang_vel, dtype=D)
    if ang_world:
        w = np.einsum("nji,nj->ni", R, w).astype(D)
    fk, vrel, _, dofs = er.leg_kinematics(model, dof[:, :, 0], dof[:, :, 1], jac=True, dtype=D)
    u = np.asarray(base_vel, dtype=D)[:, None, :] + np.einsum("nij,nfj->nfi", R, np.cross(w[:, None, :], fk) + vrel)
    return u.astype(D), R, fk, w, dofs


def detect(model, cfg, state, quat, dof, base_vel, ang_vel, contact, foot_force=None, normal=None, reset=None, mu_init=None,
           ang_world=False, dtype=np.float64):
    """One call of wbc_sim_slip_detect for a batch. state [N, 4, 8]; reset: None, True (every env) or a mask [N]. Returns a dict: the new
    `state`, every output, `mag` and `diag` (module docstring)."""
    D = dtype
    f = lambda a: np.asarray(a, dtype=D)                                               # noqa: E731
    A = lambda a: np.abs(np.asarray(a, dtype=np.float64))                              # noqa: E731
    c = {k: D(cfg[k]) for k in CFG_FIELDS}
    cf = {k: float(cfg[k]) for k in CFG_FIELDS}
    state0 = f(state)
    n = state0.shape[0]
    st = state0.reshape(n, NFEET, NS)
    dof, v, con = f(dof), f(base_vel), f(contact)
    rs = np.zeros(n, dtype=bool) if reset is None else (np.ones(n, dtype=bool) if reset is True else np.asarray(reset) != 0)
    rs4 = rs[:, None]
    lreach = er.reach(model)

    with np.errstate(all="ignore"):
        # 1 kinematics
        u, R, fk, w, dofs = foot_velocity(model, quat, dof, v, ang_vel, ang_world, D)
        ld = dofs.reshape(-1)
        finite = np.isfinite(v).all(1) & np.isfinite(f(ang_vel)).all(1) & np.isfinite(dof[:, ld, 0]).all(1) & np.isfinite(dof[:, ld, 1]).all(1)
        finite &= np.isfinite(u).all((1, 2)) & np.isfinite(con).all(1)
        qd_sum = np.stack([A(dof[:, dofs[i], 1]).sum(-1) for i in range(NFEET)], axis=1)                       # [N, 4]
        Um = np.linalg.norm(A(v), axis=1)[:, None] + (np.linalg.norm(A(w), axis=1)[:, None] + qd_sum) * lreach[None, :]
        # 2 reset
        mu0 = np.full((n, NFEET), c["mu_prior"], dtype=D) if mu_init is None else f(mu_init)
        finite &= np.where(rs, np.isfinite(mu0).all(1), np.isfinite(st).all((1, 2)))
        p = np.where(rs4, D(0), st[:, :, 0]).astype(D)
        s = np.where(rs4, False, st[:, :, 1] != 0)
        t = np.where(rs4, c["t_dwell"], st[:, :, 2]).astype(D)
        cp = np.where(rs4, False, st[:, :, 3] != 0)
        d = np.where(rs4, D(0), st[:, :, 4]).astype(D)
        mu = np.where(rs4, mu0, st[:, :, 5]).astype(D)
        wi = np.where(rs4, D(0), st[:, :, 6]).astype(D)
        mi = np.where(rs4, D(0), st[:, :, 7]).astype(D)
        # 3 standing
        cc = np.minimum(np.maximum(con, D(0)), D(1)).astype(D)
        stand = cc >= c["c_on"]
        d = np.where(stand & ~cp, D(0), d).astype(D)
        # 4 common mode
        cw = np.where(stand, cc, D(0)).astype(D)
        S = sum4(cw)
        cnt = stand.sum(1)
        cm = (cnt >= 2) & (S > 0)
        ub = np.stack([np.where(cm, sum4(cw * u[:, :, k]) / S, D(0)) for k in range(3)], axis=-1).astype(D)
        g = (u - c["common_mode"] * ub[:, None, :]).astype(D)
        nrm = np.broadcast_to(np.array([0, 0, 1], dtype=D), (n, NFEET, 3))
        if normal is not None:
            nn = f(normal)
            nrm = (nn * (D(1) / np.sqrt((nn * nn).sum(-1, keepdims=True)))).astype(D)
            finite &= np.isfinite(nrm).all((1, 2))
        gt = (g - nrm * (nrm * g).sum(-1, keepdims=True)).astype(D)
        sp = np.sqrt((gt * gt).sum(-1)).astype(D)
        cw64 = cw.astype(np.float64)
        Ubar = np.where(cm, (cw64 * Um).sum(1) / np.where(cm, S.astype(np.float64), 1.0), 0.0)
        Sm = 2.0 * (Um + cf["common_mode"] * Ubar[:, None])
        # 5 evidence
        x = (sp - c["v_slip"]) / c["sigma_v"]
        P = np.where(stand, cc * Phi(x, D), D(0)).astype(D)
        mP = np.maximum(1.0, A(cc) * pdf(x) * (Sm + cf["v_slip"]) / cf["sigma_v"])
        Pm = np.maximum(1.0, A(p) + cf["alpha"] * (mP + A(p)))
        p = (p + c["alpha"] * (P - p)).astype(D)
        # 6 flag
        tm = A(t) + cf["dt"]
        t = (t + c["dt"]).astype(D)
        tc = t.astype(np.float64)                                                       # what is compared with t_dwell
        lift = ~stand & s
        start = ~lift & stand & ~s & (p >= c["p_on"]) & (t >= c["t_dwell"])
        stop = ~lift & ~start & s & (p <= c["p_off"]) & (t >= c["t_dwell"])
        end = lift | stop
        s_before = s
        s = np.where(start, True, np.where(end, False, s))
        t = np.where(start | end, D(0), t).astype(D)
        dm = A(d) + np.where(s, Sm * cf["dt"], 0.0)
        d = (d + np.where(s, sp * c["dt"], D(0))).astype(D)
        # 7 friction
        Mm, Wm, Lm = A(mu), A(wi), A(mi)
        fn = np.zeros((n, NFEET), dtype=D)
        Fnm = np.ones((n, NFEET))
        valid = np.zeros((n, NFEET), dtype=bool)
        if foot_force is not None:
            ff = f(foot_force)
            finite &= np.isfinite(ff).all((1, 2))
            fn = (nrm * ff).sum(-1).astype(D)
            fv = (ff - nrm * fn[:, :, None]).astype(D)
            ft = np.sqrt((fv * fv).sum(-1)).astype(D)
            valid = stand & (fn >= c["fn_min"])
            rho = (ft / fn).astype(D)
            Fnm = (A(nrm) * A(ff)).sum(-1)
            Ftm = np.linalg.norm(A(ff) + A(nrm) * Fnm[:, :, None], axis=-1)
            Rhom = (Ftm + A(rho) * Fnm) / np.maximum(A(fn), 1e-300)
            stick, slide = valid & ~s, valid & s & (p > 0)
            Lm = cf["gamma"] * A(mi) + np.where(stick, Rhom, 0.0)
            mi = (c["gamma"] * mi).astype(D)
            mi = np.where(stick, np.maximum(mi, rho), mi).astype(D)
            gw = (c["gamma"] * wi).astype(D)
            wn = np.where(slide, gw + p, gw).astype(D)
            Wm = cf["gamma"] * A(wi) + np.where(slide, Pm, 0.0)
            k = np.where(slide, p / wn, D(0)).astype(D)
            k64, wn64 = k.astype(np.float64), np.where(slide, wn.astype(np.float64), 1.0)
            Mm = np.where(slide, A(mu) + k64 * (Rhom + A(mu)) + A(rho - mu) * (k64 + (Pm * A(gw) + A(p) * cf["gamma"] * A(wi)) / wn64 ** 2), A(mu))
            mu = np.where(slide, mu + k * (rho - mu), mu).astype(D)
            wi = wn
        mu_valid = wi >= c["w_min"]
        finite &= np.isfinite(p).all(1) & np.isfinite(t).all(1) & np.isfinite(d).all(1) & np.isfinite(mu).all(1) & np.isfinite(wi).all(1) & np.isfinite(mi).all(1)
        # 8 fuse
        W = sum4(wi)
        have = W >= c["w_min"]
        mue = np.where(have, sum4(wi * mu) / W, c["mu_prior"]).astype(D)
        mraw = np.where(mu_valid, mu, mue[:, None]).astype(D)
        W64 = np.where(have, W.astype(np.float64), 1.0)
        WmS = Wm.sum(1)
        muem = np.where(have, ((Wm * A(mu) + A(wi) * Mm).sum(1) + A(mue) * WmS) / W64, 1.0)
        # 9 outputs
        mu_out = np.minimum(np.maximum(c["mu_scale"] * mraw, c["mu_min"]), c["mu_max"]).astype(D)
        weight = (cc * (D(1) - p)).astype(D)
    failed = ~finite
    shift = np.arange(NFEET)
    bits = lambda m, base: (m * (base << shift)).sum(-1)                              # noqa: E731
    info = (np.where(rs, INFO_RESET, 0) + (INFO_NO_FORCE if foot_force is None else 0) + bits(start, INFO_START) + bits(end, INFO_END) +
            bits(s, INFO_SLIPPING) + bits(mu_valid, INFO_MU_VALID)).astype(np.int64)
    new_state = np.stack([p, s.astype(D), t, stand.astype(D), d, mu, wi, mi], axis=-1).astype(D)
    out = dict(state=new_state, prob=p.copy(), slip=s.astype(np.uint8), weight=weight, foot_vel=u.copy(), speed=sp.copy(), distance=d.copy(),
               mu=mu_out, mu_lower=mi.copy(), mu_env=np.stack([mue, W], axis=-1).astype(D), info=info)
    if failed.any():
        for k in ("prob", "slip", "weight", "foot_vel", "speed", "distance", "mu", "mu_lower", "mu_env"):
            out[k][failed] = 0
        out["state"][failed] = st[failed]
        out["info"][failed] = INFO_FAILED
    one = np.ones((n, NFEET))
    mum = cf["mu_scale"] * np.where(mu_valid, Mm, muem[:, None])
    mag = dict(prob=Pm, weight=Pm, foot_vel=np.repeat(Um[:, :, None], 3, axis=2), speed=Sm, distance=dm, mu=mum, mu_lower=Lm,
               mu_env=np.stack([muem, WmS], axis=-1), state=np.stack([Pm, one, tm, one, dm, Mm, Wm, Lm], axis=-1))
    out["mag"] = {k: np.maximum(np.nan_to_num(m, nan=1.0, posinf=1e300), 1e-30) for k, m in mag.items()}
    out["diag"] = dict(failed=failed, stand=stand, contact=cc.astype(np.float64), p=p.astype(np.float64), pmag=Pm, t=t.astype(np.float64),
                       t_compared=tc, tmag=tm, fn=fn.astype(np.float64), fnmag=Fnm, valid=valid,
                       w=wi.astype(np.float64), wmag=Wm, W=W.astype(np.float64), Wmag=WmS, start=start, end=end, lift=lift, slip=s,
                       slip_before=s_before, speed=sp.astype(np.float64), P=P.astype(np.float64), common=cm, fk=fk, R=R, w_trunk=w, dofs=dofs,
                       have_force=foot_force is not None, umag=Um)
    return out


def judge(cfg, ref, const):
    """From the fp64 reference alone: env_ok [N], False for a failed env and for an env with a THIN foot-case: a value that a flag hangs
    on within its bound (C 2^-24 mag) of the threshold. const: {output: C}; p is judged with prob's constant (the state's where that is
    larger), everything else with the state's. A foot that neither stands nor slips has no flag that could switch on p or t."""
    d = ref["diag"]
    cs = const["state"] * EPS
    cp = max(const["prob"], const["state"]) * EPS
    thin = np.abs(d["contact"] - cfg["c_on"]) < EPS
    could = d["stand"] | d["slip_before"]
    thin |= could & ((np.abs(d["p"] - cfg["p_on"]) < cp * d["pmag"]) | (np.abs(d["p"] - cfg["p_off"]) < cp * d["pmag"]))
    thin |= could & (np.abs(d["t_compared"] - cfg["t_dwell"]) < cs * d["tmag"])
    if d["have_force"]:
        thin |= d["stand"] & (np.abs(d["fn"] - cfg["fn_min"]) < cs * d["fnmag"])
    thin |= np.abs(d["w"] - cfg["w_min"]) < cs * d["wmag"]
    thin_env = thin.any(1) | (np.abs(d["W"] - cfg["w_min"]) < cs * d["Wmag"])
    return ~thin_env & ~d["failed"]


def ratios(got, ref, keep=None):
    """{output: the largest |got - ref| / (2^-24 mag)} over the entries kept (keep: bool mask [N] of envs, None: all)."""
    out = {}
    for k in OUTPUTS:
        with np.errstate(all="ignore"):
            err = np.abs(np.asarray(got[k], dtype=np.float64).reshape(ref[k].shape) - np.asarray(ref[k], dtype=np.float64)) / (EPS * ref["mag"][k])
        if keep is not None:
            err = err[keep]
        assert not np.isnan(err).any(), k
        out[k] = float(err.max()) if err.size else 0.0
    return out
