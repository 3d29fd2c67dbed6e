"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the attitude filter that wbc_sim_attitude_filter computes (include/wbc_sim.h has
the text: a multiplicative extended Kalman filter on the unit quaternion and the gyro bias), batched over envs, in fp64 or -- the same
text, `dtype=np.float32` -- in fp32 as the yardstick of what single precision costs. Nothing here comes from the kernel.

update() also returns the MAGNITUDES an error is judged against (2^-24 mag): the summed sizes of the terms that make up an entry. With
|.| taken entry by entry, my_j the forward substitution of |m| + |mh| through |L| (the size of the terms of y_j, scaled by mag(q)) and
mdx_j = |W_j|^T my_j the size of correction j's terms:
    q             1 + (sum_i (|gyro_i| + |b_i|) dt + sum_j sum_{i<3} mdx_j,i) / 2, one number per env: a unit quaternion's entries are
                  sums of products of unit quaternions' entries, moved by half the rotation vectors composed onto it
    b             |b| + sum_j mdx_j[3:6]
    P             after the predict |A| |P_tt| |A|^T + dt (|G| + |G|^T) + dt^2 |P_bb| + dt sigma_g^2 I with |G| = |A| |P_tb|, |G| + dt |P_bb| and
                  |P_bb| + dt sigma_b^2 I for the three blocks; every correction adds |W_j|^T |W_j|
    gyro_out      |gyro| + mag(b)
    gravity_body  mag(q)
    nis_j         2 |y_j| . my_j
A reset env's magnitudes are those of what it is set to: 1 for q, its variances for P, 0 for b and nis, |gyro| for gyro_out.
`diag` holds what thinness is judged from: d = 1 + m . w_0 of a reset from the accelerometer (NaN elsewhere)."""
import numpy as np

MAX_AUX = 4
ANTIPARALLEL = 1e-6
SWITCH = 1e-4
STATUS_MASK, STATUS_OK, STATUS_RESET, STATUS_FAILED, STATUS_FAILED_PIVOT = 15, 0, 1, 2, 3
INFO_ZERO, INFO_PIVOT, INFO_HALF_TURN = 16, 512, 16384
CFG_FIELDS = ("dt", "sigma_g", "sigma_b", "sigma_a", "kappa_a", "p0_theta", "p0_b")
OUTPUTS = ("q", "b", "P", "gyro_out", "gravity_body", "nis")                          # the continuous ones
EPS = 2.0 ** -24


def _cfg(cfg, D):
    get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    return {k: D(get(k)) for k in CFG_FIELDS}


def quat_mul(a, b):
    """Hamilton product of xyzw quaternions [..., 4], wbc_device.h's quat_mul term by term."""
    x = a[..., 3] * b[..., 0] + a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    y = a[..., 3] * b[..., 1] - a[..., 0] * b[..., 2] + a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0]
    z = a[..., 3] * b[..., 2] + a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3]
    w = a[..., 3] * b[..., 3] - a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2]
    return np.stack([x, y, z, w], axis=-1)


def quat_to_mat(q):
    """R(q) [..., 3, 3], world <- trunk, of a unit xyzw quaternion (not normalised here)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def normalise(q):
    with np.errstate(all="ignore"):
        return q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))


def exp_closed(phi):
    """(phi / |phi| sin(|phi| / 2), cos(|phi| / 2)); NaN at phi = 0."""
    D = phi.dtype.type
    n = np.sqrt(np.sum(phi * phi, axis=-1, keepdims=True))
    with np.errstate(all="ignore"):
        return np.concatenate([phi * (np.sin(D(0.5) * n) / n), np.cos(D(0.5) * n)], axis=-1)


def exp_series(phi):
    """(phi / 2 (1 - |phi|^2 / 24), 1 - |phi|^2 / 8)."""
    D = phi.dtype.type
    n2 = np.sum(phi * phi, axis=-1, keepdims=True)
    return np.concatenate([phi * (D(0.5) * (D(1) - n2 / D(24))), D(1) - n2 / D(8)], axis=-1)


def exp_quat(phi):
    """The quaternion of the rotation vector phi [..., 3]: the series for |phi| < 1e-4, the closed form elsewhere."""
    D = phi.dtype.type
    n = np.sqrt(np.sum(phi * phi, axis=-1, keepdims=True))
    return np.where(n < D(SWITCH), exp_series(phi), exp_closed(phi)).astype(phi.dtype)


def log_mat(R):
    """The rotation vector of a rotation matrix [..., 3, 3] (for the tests' finite differences; fp64, angles well below pi)."""
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = np.linalg.norm(v, axis=-1, keepdims=True)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1)[..., None] - 1.0)
    ang = np.arctan2(s, c)
    with np.errstate(all="ignore"):
        return np.where(s > 1e-12, v * (ang / s), v)


def skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z], axis=-1).reshape(v.shape[:-1] + (3, 3))


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def sym_lower(P):
    """P as the kernel reads it: the lower triangle, mirrored."""
    L = np.tril(P)
    return L + np.swapaxes(np.tril(P, -1), -1, -2)


def up_vector(gravity, D):
    g = np.asarray(gravity, dtype=D)
    gn = np.sqrt(np.sum(g * g))
    return (-g / gn).astype(D), D(gn)


def half_axis(up):
    """The half turn's axis: normalise(c x up), c the world x axis where |up_x| <= 0.9 and the world y axis otherwise."""
    D = up.dtype.type
    z = D(0)
    h = np.array([z, -up[2], up[1]], dtype=up.dtype) if abs(up[0]) <= D(0.9) else np.array([up[2], z, -up[0]], dtype=up.dtype)
    return h / np.sqrt(np.sum(h * h))


def sim_gyro(quat, ang_vel, dtype=np.float64):
    """The entry point's rule for a NULL gyro: (R(q / |q|)^T omega, the summed sizes of its terms) from ROOT_STATES' quaternion and world
    angular velocity."""
    D = dtype
    q, w = np.asarray(quat, dtype=D), np.asarray(ang_vel, dtype=D)
    qu = q * (D(1) / np.sqrt(np.sum(q * q, axis=-1, keepdims=True)))
    R = quat_to_mat(qu.astype(D))
    return np.einsum("nji,nj->ni", R, w).astype(D), np.einsum("nji,nj->ni", np.abs(R), np.abs(w)).astype(np.float64)


def transition(dq, dt):
    """Phi [..., 6, 6] = [[R(dq)^T, -dt I], [0, I]]."""
    D = dq.dtype.type
    F = np.zeros(dq.shape[:-1] + (6, 6), dtype=dq.dtype)
    F[..., :3, :3] = np.swapaxes(quat_to_mat(dq), -1, -2)
    F[..., :3, 3:] = -D(dt) * np.eye(3, dtype=dq.dtype)
    F[..., 3:, 3:] = np.eye(3, dtype=dq.dtype)
    return F


def predict(c, q, b, P, gyro):
    """(q-, P-, dq, mag P-, sum |phi| terms) of the predict step; P symmetric."""
    D = q.dtype.type
    dt = c["dt"]
    dq = exp_quat((gyro - b) * dt)
    qm = normalise(quat_mul(q, dq))
    A = np.swapaxes(quat_to_mat(dq), -1, -2)
    tt, tb, bb = P[:, :3, :3], P[:, :3, 3:], P[:, 3:, 3:]
    I = np.eye(3, dtype=q.dtype)
    G = A @ tb
    Pm = np.empty_like(P)
    Pm[:, :3, :3] = (A @ tt) @ np.swapaxes(A, -1, -2) - dt * (G + np.swapaxes(G, -1, -2)) + dt * dt * bb + dt * (c["sigma_g"] * c["sigma_g"]) * I
    Pm[:, :3, 3:] = G - dt * bb
    Pm[:, 3:, :3] = np.swapaxes(Pm[:, :3, 3:], -1, -2)
    Pm[:, 3:, 3:] = bb + dt * (c["sigma_b"] * c["sigma_b"]) * I
    Pm = sym_lower(Pm)
    aA, aG = np.abs(A), np.abs(A) @ np.abs(tb)
    mag = np.empty_like(P)
    mag[:, :3, :3] = (aA @ np.abs(tt)) @ np.swapaxes(aA, -1, -2) + dt * (aG + np.swapaxes(aG, -1, -2)) + dt * dt * np.abs(bb) + dt * (c["sigma_g"] * c["sigma_g"]) * I
    mag[:, :3, 3:] = aG + dt * np.abs(bb)
    mag[:, 3:, :3] = np.swapaxes(mag[:, :3, 3:], -1, -2)
    mag[:, 3:, 3:] = np.abs(bb) + dt * (c["sigma_b"] * c["sigma_b"]) * I
    return qm.astype(q.dtype), Pm.astype(q.dtype), dq, mag, np.sum((np.abs(gyro) + np.abs(b)) * dt, axis=-1)


def measurement_jacobian(q, w):
    """(mh, H [..., 3, 6]) with mh = R(q)^T w and H = [[mh]x, 0]."""
    mh = np.einsum("...ji,...j->...i", quat_to_mat(q), w)
    H = np.zeros(q.shape[:-1] + (3, 6), dtype=q.dtype)
    H[..., :, :3] = skew(mh)
    return mh, H


def correct(q, b, P, w, u, r, magq=None):
    """One 3-row update for every env: dict with the new q, b, P, nis, `zero` (u . u = 0: skipped) and `pivot` (a failed pivot: skipped),
    W, y, and the magnitudes mdx [N, 6], mW = |W|^T |W|, mnis. Skipped envs keep q, b, P; their nis, mdx, mW and mnis are 0. P symmetric."""
    D = q.dtype.type
    n = q.shape[0]
    magq = np.ones(n, dtype=np.float64) if magq is None else magq
    with np.errstate(all="ignore"):
        u2 = np.sum(u * u, axis=-1)
        zero = u2 == 0
        m = u * (D(1) / np.sqrt(u2))[:, None]
        mh, H = measurement_jacobian(q, w)
        e = m - mh
        HP = H @ P
        S = HP @ np.swapaxes(H, -1, -2) + r[:, None, None] * np.eye(3, dtype=q.dtype)
        a00, a10, a11, a20, a21, a22 = S[:, 0, 0], S[:, 1, 0], S[:, 1, 1], S[:, 2, 0], S[:, 2, 1], S[:, 2, 2]
        l00 = np.sqrt(a00); l10 = a10 / l00
        d1 = a11 - l10 * l10; l11 = np.sqrt(d1)
        l20 = a20 / l00; l21 = (a21 - l20 * l10) / l11
        d2 = a22 - l20 * l20 - l21 * l21; l22 = np.sqrt(d2)
        ok = np.ones(n, dtype=bool)
        for d in (a00, d1, d2):
            ok &= np.isfinite(d) & (d > 0)

        w0 = HP[:, 0, :] / l00[:, None]
        w1 = (HP[:, 1, :] - l10[:, None] * w0) / l11[:, None]
        w2 = (HP[:, 2, :] - l20[:, None] * w0 - l21[:, None] * w1) / l22[:, None]
        W = np.stack([w0, w1, w2], axis=1)                                         # [N, 3, 6]
        y0 = e[:, 0] / l00
        y1 = (e[:, 1] - l10 * y0) / l11
        y2 = (e[:, 2] - l20 * y0 - l21 * y1) / l22
        y = np.stack([y0, y1, y2], axis=-1)
        dx = np.einsum("nrc,nr->nc", W, y)
        qn = normalise(quat_mul(q, exp_quat(dx[:, :3].astype(q.dtype))))
        bn = b + dx[:, 3:]
        Pn = sym_lower(P - np.einsum("nri,nrj->nij", W, W))
        nis = np.sum(y * y, axis=-1)
        me = (np.abs(m) + np.abs(mh)).astype(np.float64) * magq[:, None]
        l64 = [np.asarray(v, dtype=np.float64) for v in (l00, l10, l11, l20, l21, l22)]
        my0 = me[:, 0] / l64[0]
        my1 = (me[:, 1] + np.abs(l64[1]) * my0) / l64[2]
        my2 = (me[:, 2] + np.abs(l64[3]) * my0 + np.abs(l64[4]) * my1) / l64[5]
        my = np.stack([my0, my1, my2], axis=-1)
        aW = np.abs(W).astype(np.float64)
        mdx = np.einsum("nrc,nr->nc", aW, my)
        mW = np.einsum("nri,nrj->nij", aW, aW)
        mnis = 2 * np.sum(np.abs(y).astype(np.float64) * my, axis=-1)
    skip = zero | ~ok
    k1, k2 = skip[:, None], skip[:, None, None]
    return dict(q=np.where(k1, q, qn).astype(q.dtype), b=np.where(k1, b, bn).astype(q.dtype), P=np.where(k2, P, Pn).astype(q.dtype),
                nis=np.where(skip, D(0), nis).astype(q.dtype), zero=zero, pivot=~zero & ~ok, W=W, y=y, H=H, S=S, e=e,
                mdx=np.where(k1, 0.0, mdx), mW=np.where(k2, 0.0, mW), mnis=np.where(skip, 0.0, mnis))


def reset_quat(accel, up, q_init, n, D):
    """(q, bits, d) of a reset for n envs: from q_init, else from the accelerometer, else the identity."""
    A = np.float32 if D is np.float32 else np.float64
    bits = np.zeros(n, dtype=np.int64)
    d = np.full(n, np.nan)
    o = np.zeros((n, 4), dtype=A); o[:, 3] = 1
    if q_init is not None:
        o = np.asarray(q_init, dtype=A).copy()
    elif accel is not None:
        with np.errstate(all="ignore"):
            u2 = np.sum(accel * accel, axis=-1)
            zero = u2 == 0
            m = accel * (D(1) / np.sqrt(u2))[:, None]
            dd = D(1) + np.sum(m * up[None], axis=-1)
            flip = ~zero & (dd < D(ANTIPARALLEL))
            o = np.concatenate([cross(m, np.broadcast_to(up, m.shape)), dd[:, None]], axis=-1).astype(A)
        o[flip] = np.concatenate([half_axis(up), [D(0)]]).astype(A)
        o[zero] = np.array([0, 0, 0, 1], dtype=A)
        bits = np.where(zero, INFO_ZERO, np.where(flip, INFO_HALF_TURN, 0)).astype(np.int64)
        d = np.where(zero, np.nan, dd.astype(np.float64))
    return normalise(o).astype(A), bits, d


def update(cfg, q, b, P, gyro, accel=None, aux_body=None, aux_world=None, aux_sigma=None, reset_mask=None, q_init=None, reset=False,
           gravity=(0.0, 0.0, -9.81), gyro_mag=None, dtype=np.float64):
    """One call of wbc_sim_attitude_filter for every env. gyro is required here (the entry point's NULL rule is sim_gyro, whose second
    result goes in as gyro_mag: the size of the gyro's own terms, |gyro| where it is an input).
    Returns dict(q, b, P, gyro_out, gravity_body, nis [N, 1 + K], status, mag=dict of the OUTPUTS' magnitudes, diag=dict(d))."""
    D = dtype
    c = _cfg(cfg, D)
    arr = lambda v: None if v is None else np.asarray(v, dtype=D)
    q0, b0, P0, gyro, accel, aux_body, aux_world, aux_sigma, q_init = map(arr, (q, b, P, gyro, accel, aux_body, aux_world, aux_sigma, q_init))
    n = q0.shape[0]
    K = 0 if aux_sigma is None else aux_sigma.shape[1]
    assert K <= MAX_AUX
    up, gn = up_vector(gravity, D)
    rs = np.ones(n, dtype=bool) if reset else (np.zeros(n, dtype=bool) if reset_mask is None else np.asarray(reset_mask) != 0)
    fin = lambda v: np.isfinite(v).reshape(n, -1).all(axis=1)
    bad = ~fin(gyro)
    if accel is not None:
        bad |= ~fin(accel)
    low = np.tril(np.ones((6, 6), dtype=bool))
    bad |= ~rs & ~(fin(q0) & fin(b0) & np.isfinite(np.where(low, P0, D(0))).reshape(n, -1).all(axis=1))
    if q_init is not None:
        bad |= rs & ~fin(q_init)

    with np.errstate(all="ignore"):
        # the envs that run the filter (computed for every env, selected below)
        Ps = sym_lower(P0)
        qf, Pf, _, magP, mphi = predict(c, q0, b0, Ps, gyro)
        bf = b0.copy()
        nis = np.zeros((n, 1 + K), dtype=D)
        mnis = np.zeros((n, 1 + K))
        bits = np.zeros(n, dtype=np.int64)
        mrot = mphi.astype(np.float64) if gyro_mag is None else np.sum((gyro_mag + np.abs(b0)) * np.float64(c["dt"]), axis=-1)
        mb = np.abs(b0).astype(np.float64)
        magP = magP.astype(np.float64)
        meas = []
        if accel is not None:
            x = (np.sqrt(np.sum(accel * accel, axis=-1)) - gn) / gn
            meas.append((0, np.broadcast_to(up, (n, 3)), accel, c["sigma_a"] * c["sigma_a"] * (D(1) + c["kappa_a"] * (x * x)), np.ones(n, dtype=bool), np.zeros(n, dtype=bool)))
        for k in range(K):
            sg = aux_sigma[:, k]
            on = ~(sg <= 0)
            bad |= ~rs & on & ~(np.isfinite(sg) & fin(aux_body[:, k]) & fin(aux_world[:, k]))
            w2 = np.sum(np.where(on[:, None], aux_world[:, k], D(1)) ** 2, axis=-1)
            wz = on & (w2 == 0)
            wu = aux_world[:, k] * (D(1) / np.sqrt(w2))[:, None]
            meas.append((1 + k, wu, aux_body[:, k], sg * sg, on & ~wz, wz))
        for j, w, u, r, on, wzero in meas:
            magq = 1.0 + 0.5 * mrot
            use = on & ~bad & ~rs
            safe = lambda v, fill: np.where(use.reshape((n,) + (1,) * (v.ndim - 1)), v, D(fill))
            res = correct(qf, bf, Pf, safe(w, 1), safe(u, 1), safe(r, 1), magq)
            k1, k2 = use[:, None], use[:, None, None]
            qf, bf, Pf = np.where(k1, res["q"], qf), np.where(k1, res["b"], bf), np.where(k2, res["P"], Pf)
            nis[:, j] = np.where(use, res["nis"], D(0))
            mnis[:, j] = np.where(use, res["mnis"], 0.0)
            bits |= np.where(use & res["zero"], INFO_ZERO << j, 0) | np.where(use & res["pivot"], INFO_PIVOT << j, 0)
            bits |= np.where(wzero & ~bad & ~rs, INFO_ZERO << j, 0)
            mrot = mrot + np.where(use, res["mdx"][:, :3].sum(axis=1), 0.0)
            mb = mb + np.where(k1, res["mdx"][:, 3:], 0.0)
            magP = magP + np.where(k2, res["mW"], 0.0)
        code = np.where((bits & (INFO_PIVOT * 31)) != 0, STATUS_FAILED_PIVOT, STATUS_OK)

        # the envs that are reset
        qr, rbits, d = reset_quat(accel, up, q_init, n, D)
        Pr = np.zeros((6, 6), dtype=D)
        Pr[np.arange(3), np.arange(3)] = c["p0_theta"]; Pr[np.arange(3, 6), np.arange(3, 6)] = c["p0_b"]
        r1, r2 = rs[:, None], rs[:, None, None]
        qn, bn, Pn = np.where(r1, qr, qf).astype(D), np.where(r1, D(0), bf).astype(D), np.where(r2, Pr[None], Pf).astype(D)
        nis = np.where(r1, D(0), nis)
        status = np.where(rs, STATUS_RESET | rbits, code | bits)
        magq = np.where(rs, 1.0, 1.0 + 0.5 * mrot)
        mb = np.where(r1, 0.0, mb)
        magP = np.where(r2, np.abs(Pr)[None].astype(np.float64), magP)
        mnis = np.where(r1, 0.0, mnis)

        bad |= ~(fin(qn) & fin(bn) & fin(Pn))
        g1, g2 = bad[:, None], bad[:, None, None]
        out = dict(q=np.where(g1, q0, qn).astype(D), b=np.where(g1, b0, bn).astype(D), P=np.where(g2, P0, Pn).astype(D),
                   gyro_out=np.where(g1, D(0), gyro - bn).astype(D),
                   gravity_body=np.where(g1, D(0), -np.einsum("nji,j->ni", quat_to_mat(qn), up)).astype(D),
                   nis=np.where(g1, D(0), nis).astype(D), status=np.where(bad, STATUS_FAILED, status).astype(np.int32))
    mq4 = np.repeat(magq[:, None], 4, axis=1)
    out["mag"] = dict(q=mq4, b=mb, P=magP, gyro_out=(np.abs(np.nan_to_num(gyro)).astype(np.float64) if gyro_mag is None else gyro_mag) + mb, gravity_body=np.repeat(magq[:, None], 3, axis=1),
                      nis=mnis)
    out["diag"] = dict(d=np.where(rs & ~bad, d, np.nan))
    return out


def ratios(got, ref):
    """The largest |got - ref| / (2^-24 mag) per continuous output present in `got`, over the envs the reference did not fail."""
    live = (ref["status"] & STATUS_MASK) != STATUS_FAILED
    res = {}
    for k in OUTPUTS:
        if k not in got or got[k] is None:
            continue
        err = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64))[live]
        mag = ref["mag"][k][live]
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / (EPS * mag))
        res[k] = float(r.max()) if r.size else 0.0
    return res
