"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the probabilistic contact detector that wbc_sim_contact_detect computes
(include/wbc_sim.h has the text; the step numbers below are its), batched over envs, in fp64 or -- the same text, `dtype=np.float32` -- in
fp32 as the yardstick of what single precision costs. Nothing here comes from the kernel: the leg kinematics and Jacobians are
estimator_reference's walk of widowgo1_model.json, the 3 x 3 factorisation is written out here, erf is the C library's (rounded to the
working precision).

detect() also returns the MAGNITUDES an error is judged against (2^-24 mag), per foot:
    force   sum_k |J_k| (|A^-1| |tau|)_k per axis: the sizes of the terms summed into f (|f| itself where foot_force is the input, 0 without a force)
    P_f     max(1, pdf(x_f) / sigma_f (sum_j |n_j| mag(f_j) + |mu_f|)): the force's size carried through Phi by its slope
    P_z     max(1, pdf(x_z) / sigma_z (|b_z| + reach_i + |ground_i| + |mu_z|))
    P_phi   max(1, slope(s) mag(s)), slope(s) = (exp(-s^2 / 2 sigma^2) + exp(-(1 - s)^2 / 2 sigma^2)) / (sigma sqrt(2 pi)),
            mag(s) = (|phase| + offset_i + 1) / duty in stance and (|phase| + offset_i + 1 + duty) / (1 - duty) in swing
    P       the inverse-variance mean of the present terms' magnitudes (an absent term is exactly 0 and is judged against 1)
    prob    max(1, |p| + alpha (mag(P) + |p|));   state: (prob, 1, |t| + dt, 1) per foot
and, in `diag`, what thinness is judged from: phi, s, the schedule, the filtered p and its magnitude."""
import math

import numpy as np

import estimator_reference as er

NS, NFEET = 16, 4
INFO_RESET, INFO_FAILED, INFO_TOUCHDOWN, INFO_LIFTOFF, INFO_EARLY, INFO_LATE, INFO_FORCE_SINGULAR = 1, 2, 16, 256, 4096, 65536, 1048576
CFG_FIELDS = ("dt", "duty", "offset", "sigma_phase", "mu_z", "sigma_z", "mu_f", "sigma_f", "var_phase", "var_z", "var_f", "alpha", "p_on", "p_off",
              "t_dwell", "early_min", "late_min", "damping")
OUTPUTS = ("prob", "terms", "force", "state")                                          # the continuous ones
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


def prior(phi, duty, sigma, dtype=np.float64):
    """(P_phi, scheduled stance, s) of foot phases phi: step 4's gait prior with wbc_sim_footstep_plan's stance rule."""
    D = dtype
    phi, duty, sigma = np.asarray(phi, dtype=D), D(duty), D(sigma)
    sched = np.ones(phi.shape, dtype=bool) if duty >= 1 else phi < duty
    with np.errstate(all="ignore"):
        s = np.where(sched, phi / duty, (phi - duty) / (D(1) - duty)).astype(D)
    k = sigma * D(np.sqrt(2.0))
    G = D(0.5) * (erf(s / k, D) + erf((D(1) - s) / k, D))
    return np.where(sched, G, D(1) - G).astype(D), sched, s


def chol3_solve(A, tau):
    """(y, ok): A y = tau for a batch [..., 3, 3] by the row-by-row Cholesky factorisation of step 3; ok False where a pivot is not a
    positive finite number (y is then garbage)."""
    with np.errstate(all="ignore"):
        a00, a10, a11, a20, a21, a22 = A[..., 0, 0], A[..., 1, 0], A[..., 1, 1], A[..., 2, 0], A[..., 2, 1], A[..., 2, 2]
        l00 = np.sqrt(a00); l10 = a10 / l00
        d1 = a11 - l10 * l10; l11 = np.sqrt(d1)
        l20 = a20 / l00; l21 = (a21 - l20 * l10) / l11
        d2 = a22 - l20 * l20 - l21 * l21; l22 = np.sqrt(d2)
        z0 = tau[..., 0] / l00; z1 = (tau[..., 1] - l10 * z0) / l11; z2 = (tau[..., 2] - l20 * z0 - l21 * z1) / l22
        y2 = z2 / l22; y1 = (z1 - l21 * y2) / l11; y0 = (z0 - l10 * y1 - l20 * y2) / l00
        ok = np.ones(a00.shape, dtype=bool)
        for d in (a00, d1, d2):
            ok &= np.isfinite(d) & (d > 0)
    return np.stack([y0, y1, y2], axis=-1), ok


def leg_jacobians(model, quat, dof, base_pos, dtype=np.float64):
    """Step 2: (P [N, 4, 3] the foot origins, J [N, 4, 3, 3] the leg Jacobians in world axes (column k: joint k), dofs [4, 3])."""
    D = dtype
    dof = np.asarray(dof, dtype=D)
    R = er.quat_to_mat(quat, D)
    fk, _, Jt, dofs = er.leg_kinematics(model, dof[:, :, 0], None, jac=True, dtype=D)
    P = np.asarray(base_pos, dtype=D)[:, None, :] + np.einsum("nij,nfj->nfi", R, fk)
    J = np.einsum("nij,nfjk->nfik", R, Jt)
    return P.astype(D), J.astype(D), dofs


def foot_force(J, tau, damping, dtype=np.float64):
    """Step 3: (f [..., 3], ok, mag [..., 3]) = J (J^T J + damping^2 I)^-1 tau."""
    D = dtype
    J, tau = np.asarray(J, dtype=D), np.asarray(tau, dtype=D)
    A = np.einsum("...ik,...il->...kl", J, J) + (D(damping) * D(damping)) * np.eye(3, dtype=D)
    y, ok = chol3_solve(A, tau)
    with np.errstate(all="ignore"):
        fs = (J[..., 0] * y[..., 0:1] + J[..., 1] * y[..., 1:2]) + J[..., 2] * y[..., 2:3]
        ok = ok & np.isfinite(fs).all(-1)
        f = np.where(ok[..., None], fs, 0).astype(D)
        A64 = np.where(ok[..., None, None], A.astype(np.float64), np.eye(3))
        ymag = np.einsum("...kl,...l->...k", np.abs(np.linalg.inv(A64)), np.abs(tau.astype(np.float64)))
        mag = np.einsum("...ik,...k->...i", np.abs(J.astype(np.float64)), ymag)
    return f, ok, np.where(ok[..., None], mag, 0.0)


def detect(model, cfg, state, quat, dof, base_pos, tau_ext=None, foot_force_in=None, normal=None, ground=None, phase=None, reset=None,
           p_init=None, dtype=np.float64):
    """One call of wbc_sim_contact_detect for a batch. state [N, 16]; reset: None, True (every env) or a mask [N]. Returns a dict: the new
    `state`, every output, `mag` and `diag` (module docstring)."""
    D = dtype
    f = lambda a: np.asarray(a, dtype=D)                                               # noqa: E731
    assert tau_ext is None or foot_force_in is None
    assert not (tau_ext is None and foot_force_in is None and ground is None and phase is None)
    c = {k: (f(cfg[k]) if k == "offset" else D(cfg[k])) for k in CFG_FIELDS}
    state0 = f(state)
    n = state0.shape[0]
    st = state0.reshape(n, NFEET, 4)
    b, dof = f(base_pos), f(dof)
    rs = np.zeros(n, dtype=bool) if reset is None else (np.ones(n, dtype=bool) if reset is True else np.asarray(reset) != 0)
    pin = np.ones((n, NFEET), dtype=D) if p_init is None else f(p_init)
    lreach = er.reach(model)

    with np.errstate(all="ignore"):
        # 1 reset
        p = np.where(rs[:, None], pin, st[:, :, 0]).astype(D)
        on = np.where(rs[:, None], pin >= D(0.5), st[:, :, 1] != 0)
        t = np.where(rs[:, None], c["t_dwell"], st[:, :, 2]).astype(D)
        finite = np.where(rs, np.isfinite(pin).all(1), np.isfinite(st[:, :, 0:3]).all((1, 2)))
        # 2 kinematics
        P, J, dofs = leg_jacobians(model, quat, dof, b, D)
        finite &= np.isfinite(f(quat)).all(1) & np.isfinite(b).all(1) & np.isfinite(dof[:, dofs.reshape(-1), 0]).all(1) & np.isfinite(P).all((1, 2))
        # 3 force
        force = np.zeros((n, NFEET, 3), dtype=D)
        fmag = np.zeros((n, NFEET, 3))
        singular = np.zeros((n, NFEET), dtype=bool)
        have_force = True
        if foot_force_in is not None:
            force = f(foot_force_in)
            fmag = np.abs(force.astype(np.float64))
            finite &= np.isfinite(force).all((1, 2))
        elif tau_ext is not None:
            tau = f(tau_ext)[:, 6 + dofs]                                              # [N, 4, 3]
            finite &= np.isfinite(tau).all((1, 2))
            force, ok, fmag = foot_force(J, tau, c["damping"], D)
            singular = ~ok
        else:
            have_force = False
        nrm = np.broadcast_to(np.array([0, 0, 1], dtype=D), (n, NFEET, 3))
        if normal is not None and have_force:
            nn = f(normal)
            nrm = (nn * (D(1) / np.sqrt((nn * nn).sum(-1, keepdims=True)))).astype(D)
            finite &= np.isfinite(nrm).all((1, 2))
        # 4 terms, 5 fusion
        zero = np.zeros((n, NFEET), dtype=D)
        Pphi, Pz, Pf = zero.copy(), zero.copy(), zero.copy()
        mphi, mz, mf = np.zeros((n, NFEET)), np.zeros((n, NFEET)), np.zeros((n, NFEET))
        num, den, mnum = zero.copy(), D(0), np.zeros((n, NFEET))
        phi, s, sched = zero.copy(), zero.copy(), np.ones((n, NFEET), dtype=bool)
        if phase is not None:
            ph = f(phase)
            finite &= np.isfinite(ph)
            x0 = ph[:, None] + c["offset"][None, :]
            phi = (x0 - np.floor(x0)).astype(D)
            Pphi, sched, s = prior(phi, c["duty"], c["sigma_phase"], D)
            sg, s64, duty = float(c["sigma_phase"]), s.astype(np.float64), float(c["duty"])
            slope = (np.exp(-s64 ** 2 / (2 * sg * sg)) + np.exp(-(1 - s64) ** 2 / (2 * sg * sg))) / (sg * np.sqrt(2 * np.pi))
            mphase = np.abs(ph.astype(np.float64))[:, None] + c["offset"].astype(np.float64)[None, :] + 1
            ms = np.where(sched, mphase / duty, (mphase + duty) / (1 - duty) if duty < 1 else 0.0)
            mphi = np.maximum(1.0, slope * ms)
            num = num + Pphi / c["var_phase"]; den = den + D(1) / c["var_phase"]; mnum += mphi / float(c["var_phase"])
        if ground is not None:
            g = f(ground)
            finite &= np.isfinite(g).all(1)
            xz = (c["mu_z"] - (P[:, :, 2] - g)) / c["sigma_z"]
            Pz = Phi(xz, D)
            mh = np.abs(b[:, 2].astype(np.float64))[:, None] + lreach[None, :] + np.abs(g.astype(np.float64)) + abs(float(c["mu_z"]))
            mz = np.maximum(1.0, pdf(xz) / float(c["sigma_z"]) * mh)
            num = num + Pz / c["var_z"]; den = den + D(1) / c["var_z"]; mnum += mz / float(c["var_z"])
        if have_force:
            fn = (force * nrm).sum(-1)
            xf = (fn - c["mu_f"]) / c["sigma_f"]
            Pf = Phi(xf, D)
            mfn = (np.abs(nrm.astype(np.float64)) * fmag).sum(-1) + abs(float(c["mu_f"]))
            mf = np.maximum(1.0, pdf(xf) / float(c["sigma_f"]) * mfn)
            num = num + Pf / c["var_f"]; den = den + D(1) / c["var_f"]; mnum += mf / float(c["var_f"])
        Pfused = (num / den).astype(D)
        mP = mnum / float(den)
        pmag = np.maximum(1.0, np.abs(p.astype(np.float64)) + float(c["alpha"]) * (mP + np.abs(p.astype(np.float64))))
        p = (p + c["alpha"] * (Pfused - p)).astype(D)
        # 6 flag
        tmag = np.abs(t.astype(np.float64)) + float(c["dt"])
        t = (t + c["dt"]).astype(D)
        td = ~on & (p >= c["p_on"]) & (t >= c["t_dwell"])
        lo = on & (p <= c["p_off"]) & (t >= c["t_dwell"])
        on = np.where(td, True, np.where(lo, False, on))
        t = np.where(td | lo, 0, t).astype(D)
        # 7 events
        early, late = np.zeros((n, NFEET), dtype=bool), np.zeros((n, NFEET), dtype=bool)
        stance = on.copy()
        if phase is not None:
            early = ~sched & (s >= c["early_min"]) & on
            late = sched & (s >= c["late_min"]) & ~on
            stance = (sched | early) & ~late
    failed = ~finite
    shift = np.arange(NFEET)
    bits = lambda m, base: (m * (base << shift)).sum(-1)                              # noqa: E731
    info = (np.where(rs, INFO_RESET, 0) + bits(td, INFO_TOUCHDOWN) + bits(lo, INFO_LIFTOFF) + bits(early, INFO_EARLY) + bits(late, INFO_LATE) +
            bits(singular, INFO_FORCE_SINGULAR)).astype(np.int64)
    new_state = np.stack([p, on.astype(D), t, np.zeros_like(p)], axis=-1).reshape(n, NS).astype(D)
    terms = np.stack([Pphi, Pz, Pf, Pfused], axis=-1).astype(D)
    out = dict(state=new_state, prob=p.copy(), contact=on.astype(np.uint8), stance=stance.astype(np.uint8), force=force.astype(D), terms=terms, info=info)
    if failed.any():
        for k in ("prob", "contact", "stance", "force", "terms"):
            out[k][failed] = 0
        out["state"][failed] = state0[failed]
        out["info"][failed] = INFO_FAILED
    one = np.ones((n, NFEET))
    out["mag"] = dict(prob=pmag, terms=np.maximum(np.stack([mphi, mz, mf, mP], axis=-1), 1.0), force=np.maximum(fmag, 1e-30),
                      state=np.stack([pmag, one, tmag, one], axis=-1).reshape(n, NS))
    out["diag"] = dict(phi=phi, s=s, sched=sched, p=p.astype(np.float64), pmag=pmag, failed=failed, foot_pos=P, jac=J, dofs=dofs, touchdown=td, liftoff=lo,
                       early=early, late=late, singular=singular, have_phase=phase is not None)
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
