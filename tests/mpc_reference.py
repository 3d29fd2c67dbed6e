"""fp64 numpy restatement of wbc_sim_centroidal_mpc (include/wbc_sim.h): the convex MPC on the single-rigid-body model, solved by a fixed
number of ADMM iterations on z = C u around a Riccati solve of the equality-constrained subproblem. Batched over the envs; `dtype` runs
the same statements in fp32, which is what the tests' K_ref comes from. Nothing here knows the kernel.

Magnitudes the element-wise bounds use (per env, from the reference alone):
  forces, u     max(m |g|, max |u|)
  x_pred        per block (theta, p, omega, v) the largest entry over the horizon, floored at 1
  base_acc      linear max(|g|, max |u| / m); angular max(1, |I_G^-1| * max |r_0| * max |u|)
  res           (max(m |g|, max |u|) * (1 + mu), rho * the same)
"""
import numpy as np

COLD, SHIFT = 1, 2
STATUS_OK, STATUS_ITERATIONS, STATUS_FAILED = 0, 1, 2
NX, NU, NZ = 12, 12, 20


def cone_rows(mu, dtype=np.float64):
    """C [20, 12], lo [20], hi [20] of the four feet."""
    c5 = np.array([[-1, 0, mu], [1, 0, mu], [0, -1, mu], [0, 1, mu], [0, 0, 1]], dtype=dtype)
    C = np.zeros((NZ, NU), dtype=dtype)
    for f in range(4):
        C[5 * f:5 * f + 5, 3 * f:3 * f + 3] = c5
    return C


def skew(r):
    z = np.zeros_like(r[..., 0])
    return np.stack([np.stack([z, -r[..., 2], r[..., 1]], -1), np.stack([r[..., 2], z, -r[..., 0]], -1),
                     np.stack([-r[..., 1], r[..., 0], z], -1)], -2)


def inv3(I):
    """Adjugate over determinant, as the kernel forms it; the determinant as well."""
    a, b, c, d, e, f, g, h, i = [I[:, r, s] for r in range(3) for s in range(3)]
    A0, A1, A2 = e * i - f * h, c * h - b * i, b * f - c * e
    det = a * A0 + d * A1 + g * A2
    adj = np.stack([np.stack([A0, A1, A2], -1), np.stack([f * g - d * i, a * i - c * g, c * d - a * f], -1),
                    np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    with np.errstate(all="ignore"):
        return adj / det[:, None, None], det


def heading_rotvec(R):
    """theta = log(R Rz(psi)^T), psi the yaw of R's x axis. R [N, 3, 3]."""
    psi = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    c, s = np.cos(psi), np.sin(psi)
    z, o = np.zeros_like(c), np.ones_like(c)
    Rz = np.stack([np.stack([c, -s, z], -1), np.stack([s, c, z], -1), np.stack([z, z, o], -1)], -2)
    M = R @ np.swapaxes(Rz, 1, 2)
    ang = np.arccos(np.clip((M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2] - 1) / 2, -1, 1))
    with np.errstate(all="ignore"):
        k = np.where(ang > 1e-3, ang / (2 * np.sin(ang)), 0.5 * (1 + ang * ang / 6))
    return k[:, None] * np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], -1)


def model(cfg, x0, mass, inertia, foot_pos, contact, x_ref, gravity, dtype=np.float64):
    """A [12,12], B [N,H,12,12], d [12], W [N,H,4,3,3], r [N,H,4,3], I_G^-1 [N,3,3], det I_G [N]."""
    dt = dtype(cfg["dt"])
    N, H = contact.shape[0], contact.shape[1]
    A = np.eye(NX, dtype=dtype)
    A[0:3, 6:9] = dt * np.eye(3, dtype=dtype)
    A[3:6, 9:12] = dt * np.eye(3, dtype=dtype)
    g = np.asarray(gravity, dtype=dtype)
    half = dtype(0.5) * dt * dt
    d = np.concatenate([np.zeros(3, dtype), half * g, np.zeros(3, dtype), dt * g])
    Iinv, det = inv3(inertia.astype(dtype))
    pbar = np.concatenate([x0[:, None, 3:6], x_ref[:, :H - 1, 3:6]], axis=1).astype(dtype)          # [N,H,3]
    fp = foot_pos.astype(dtype)
    if fp.shape[1] == 1:
        fp = np.repeat(fp, H, axis=1)
    r = fp - pbar[:, :, None, :]
    W = Iinv[:, None, None] @ skew(r)                                                               # [N,H,4,3,3]
    im = (dtype(1) / mass.astype(dtype))[:, None, None, None, None] * np.eye(3, dtype=dtype)
    c = (contact != 0).astype(dtype)[..., None, None]
    blocks = np.concatenate([half * W, half * im + 0 * W, dt * W, dt * im + 0 * W], axis=-2) * c     # [N,H,4,12,3]
    B = np.concatenate([blocks[:, :, f] for f in range(4)], axis=-1)
    return A, B, d, W, r, Iinv, det


def _cholesky(G):
    """Left-looking, column by column; D = 1 / L_jj; bad [N] where a pivot's 1 / sqrt is not a positive finite number."""
    L = np.zeros_like(G)
    n = G.shape[-1]
    D = np.zeros(G.shape[:-1], G.dtype)
    bad = np.zeros(G.shape[0], bool)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = G[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(-1)
            idj = (1 / np.sqrt(dj)).astype(G.dtype)
            ok = (idj > 0) & np.isfinite(idj)
            bad |= ~ok
            idj = np.where(ok, idj, 1)
            D[:, j] = idj
            L[:, j, j] = 1 / idj
            L[:, j + 1:, j] = (G[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, j:j + 1, :j]).sum(-1)) * idj[:, None]
    return L, D, bad


def _solve(L, D, X):
    """L L^T Y = X, row by row."""
    Y = X.copy()
    n = L.shape[-1]
    for i in range(n):
        Y[:, i] = (Y[:, i] - (L[:, i, :i, None] * Y[:, :i]).sum(1)) * D[:, i, None]
    for i in range(n - 1, -1, -1):
        Y[:, i] = (Y[:, i] - (L[:, i + 1:, i, None] * Y[:, i + 1:]).sum(1)) * D[:, i, None]
    return Y


def solve(cfg, x0, mass, inertia, foot_pos, contact, x_ref, gravity, warm=None, flags=0, dtype=np.float64, iters=None):
    """One call. cfg: dict with horizon, iters, dt, rho, mu, fz_min, fz_max, q [12], r [3], tol. x0 [N,12], mass [N], inertia [N,3,3],
    foot_pos [N,S,4,3], contact u8 [N,H,4], x_ref [N,H,12], warm [N,2,H,20] or None. Returns a dict of forces, u, x_pred, base_acc, res,
    status and warm (the new z and y)."""
    with np.errstate(all="ignore"):
        return _solve_call(cfg, x0, mass, inertia, foot_pos, contact, x_ref, gravity, warm, flags, dtype, iters)


def _solve_call(cfg, x0, mass, inertia, foot_pos, contact, x_ref, gravity, warm, flags, dtype, iters):
    H = int(cfg["horizon"])
    iters = int(cfg["iters"] if iters is None else iters)
    N = contact.shape[0]
    rho, mu = dtype(cfg["rho"]), dtype(cfg["mu"])
    fz_min, fz_max = dtype(cfg["fz_min"]), dtype(cfg["fz_max"])
    q = np.asarray(cfg["q"], dtype=dtype)
    rr = np.asarray(cfg["r"], dtype=dtype)
    x0 = x0.astype(dtype)
    x_ref = x_ref.astype(dtype)
    finite = (np.isfinite(x0).all(-1) & np.isfinite(mass) & np.isfinite(inertia).all((-1, -2)) & np.isfinite(foot_pos).all((-1, -2, -3))
              & np.isfinite(x_ref).all((-1, -2)))
    A, B, d, W, r, Iinv, det = model(cfg, x0, mass, inertia, foot_pos, contact, x_ref, gravity, dtype)
    bad = ~finite | ~((det > 0) & np.isfinite(det)) | ~(mass > 0)
    C = cone_rows(mu, dtype)
    ctc = np.tile(np.array([2, 2, 4 * mu * mu + 1], dtype=dtype), 4)
    Rt = np.tile(rr, 4) + rho * ctc
    stance = np.repeat(contact != 0, 5, axis=-1)                                                   # [N,H,20]
    lo = np.tile(np.array([0, 0, 0, 0, fz_min], dtype=dtype), 4)
    hi = np.tile(np.array([np.inf, np.inf, np.inf, np.inf, fz_max], dtype=dtype), 4)

    # ---- factor ----
    Q = np.diag(q)
    P = np.broadcast_to(Q, (N, NX, NX)).copy()
    K = np.zeros((N, H, NU, NX), dtype)
    Gi = np.zeros((N, H, NU, NU), dtype)
    Pd = np.zeros((N, H, NX), dtype)                                                                # Pd[k] = P_{k+1} d
    eye = np.broadcast_to(np.eye(NU, dtype=dtype), (N, NU, NU))
    for k in range(H - 1, -1, -1):
        Bk = B[:, k]
        Pd[:, k] = P @ d
        PB = P @ Bk
        G = np.swapaxes(Bk, 1, 2) @ PB
        G[:, np.arange(NU), np.arange(NU)] += Rt
        L, D, fail = _cholesky(G)
        bad |= fail
        BtPA = np.swapaxes(PB, 1, 2) @ A
        sol = _solve(L, D, np.concatenate([BtPA, eye], axis=2))
        K[:, k], Gi[:, k] = sol[:, :, :NX], sol[:, :, NX:]
        M = A - Bk @ K[:, k]
        Pn = A.T @ (P @ M)
        if k > 0:
            Pn = Pn + Q
        P = (0.5 * (Pn + np.swapaxes(Pn, 1, 2))).astype(dtype)

    # ---- warm start ----
    z = np.zeros((N, H, NZ), dtype)
    y = np.zeros((N, H, NZ), dtype)
    if warm is not None and not (flags & COLD):
        z, y = warm[:, 0].astype(dtype), warm[:, 1].astype(dtype)
        if flags & SHIFT:
            z = np.concatenate([z[:, 1:], z[:, -1:]], axis=1)
            y = np.concatenate([y[:, 1:], y[:, -1:]], axis=1)
        bad |= ~(np.isfinite(z).all((-1, -2)) & np.isfinite(y).all((-1, -2)))
    z = np.where(stance, z, 0).astype(dtype)
    y = np.where(stance, y, 0).astype(dtype)

    qx = -q * x_ref                                                                                 # [N,H,12]: -Q x_ref_k at index k - 1
    u = np.zeros((N, H, NU), dtype)
    xs = np.zeros((N, H + 1, NX), dtype)
    xs[:, 0] = x0
    kap = np.zeros((N, H, NU), dtype)
    z_prev = z
    for _ in range(iters):
        rt = -rho * ((z - y) @ C)                                                                   # [N,H,12]
        p = qx[:, H - 1]
        for k in range(H - 1, -1, -1):
            s = p + Pd[:, k]
            v = np.einsum("nij,ni->nj", B[:, k], s) + rt[:, k]
            kap[:, k] = np.einsum("nij,nj->ni", Gi[:, k], v)
            p = s @ A - np.einsum("nji,nj->ni", K[:, k], v)
            if k > 0:
                p = p + qx[:, k - 1]
        for k in range(H):
            u[:, k] = -np.einsum("nij,nj->ni", K[:, k], xs[:, k]) - kap[:, k]
            xs[:, k + 1] = xs[:, k] @ A.T + np.einsum("nij,nj->ni", B[:, k], u[:, k]) + d
        Cu = u @ C.T
        z_prev = z
        z = np.where(stance, np.clip(Cu + y, lo, hi), 0).astype(dtype)
        y = np.where(stance, y + Cu - z, 0).astype(dtype)

    Cu = u @ C.T
    r_pri = np.where(stance, np.abs(Cu - z), 0).max((-1, -2))
    r_dual = rho * np.abs((z - z_prev) @ C).max((-1, -2))
    res = np.stack([r_pri, r_dual], -1).astype(dtype)
    f = u[:, 0].reshape(N, 4, 3).copy()
    f[:, :, 2] = np.clip(f[:, :, 2], fz_min, fz_max)
    lim = mu * f[:, :, 2]
    f[:, :, 0] = np.clip(f[:, :, 0], -lim, lim)
    f[:, :, 1] = np.clip(f[:, :, 1], -lim, lim)
    f = np.where((contact[:, 0] != 0)[..., None], f, 0).astype(dtype)
    g = np.asarray(gravity, dtype=dtype)
    lin = f.sum(1) / mass.astype(dtype)[:, None] + g
    ang = np.einsum("nij,nj->ni", Iinv, np.cross(r[:, 0], f).sum(1))
    base_acc = np.concatenate([lin, ang], -1).astype(dtype)
    tol = dtype(cfg["tol"])
    status = np.where((res[:, 0] <= tol) & (res[:, 1] <= tol), STATUS_OK, STATUS_ITERATIONS).astype(np.int32)
    bad |= ~(np.isfinite(u).all((-1, -2)) & np.isfinite(xs).all((-1, -2)) & np.isfinite(res).all(-1) & np.isfinite(base_acc).all(-1)
             & np.isfinite(z).all((-1, -2)) & np.isfinite(y).all((-1, -2)))
    out = dict(forces=f, u=u.copy(), x_pred=xs[:, 1:].copy(), base_acc=base_acc, res=res, status=status, warm=np.stack([z, y], 1))
    for name in ("forces", "u", "x_pred", "base_acc", "res", "warm"):
        out[name][bad] = 0
    out["status"][bad] = STATUS_FAILED
    out["model"] = dict(A=A, B=B, d=d, r=r, Iinv=Iinv, C=C, lo=lo, hi=hi, stance=stance)
    return out


def condense(A, B, d, x0):
    """x_{1..H} stacked = Sx x0 + Su u + Sd for ONE env: B [H,12,12], x0 [12]. Returns (c = Sx x0 + Sd [H*12], Su [H*12, H*12])."""
    H = B.shape[0]
    Su = np.zeros((H * NX, H * NU), B.dtype)
    c = np.zeros(H * NX, B.dtype)
    x = x0.copy()
    for k in range(H):
        x = A @ x + d
        c[k * NX:(k + 1) * NX] = x
        for j in range(k + 1):
            blk = B[j]
            for _ in range(k - j):
                blk = A @ blk
            Su[k * NX:(k + 1) * NX, j * NU:(j + 1) * NU] = blk
    return c, Su


def magnitudes(cfg, ref, mass, gravity):
    """Per-env magnitudes of the element-wise bounds, from the fp64 reference alone (module docstring)."""
    g = float(np.linalg.norm(gravity))
    umax = np.abs(ref["u"]).max((-1, -2))
    fmag = np.maximum(mass * g, umax)
    xp = np.abs(ref["x_pred"])
    xmag = np.repeat(np.maximum(1.0, np.stack([xp[:, :, 3 * b:3 * b + 3].max((-1, -2)) for b in range(4)], -1)), 3, axis=-1)   # [N,12]
    m = ref["model"]
    iinv = np.abs(m["Iinv"]).max((-1, -2))
    rmax = np.abs(m["r"][:, 0]).max((-1, -2))
    lin = np.maximum(g, umax / mass)
    ang = np.maximum(1.0, iinv * rmax * umax)
    amag = np.concatenate([np.repeat(lin[:, None], 3, 1), np.repeat(ang[:, None], 3, 1)], -1)
    rmag = np.stack([fmag * (1 + cfg["mu"]), cfg["rho"] * fmag * (1 + cfg["mu"])], -1)
    return dict(forces=fmag[:, None, None], u=fmag[:, None, None], x_pred=xmag[:, None, :], base_acc=amag, res=rmag)
