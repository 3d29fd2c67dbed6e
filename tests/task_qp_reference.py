"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) references for wbc_sim_task_inverse_dynamics_qp (wbc_taskqp_solve_kernel in
csrc/wbc_arm_kernel.hip; definition in include/wbc_sim.h): tests/task_inverse_dynamics_reference.py's problem with a torque box and five
contact rows per active stance body.

  * Rows: an fp64 restatement of the inequalities, all written n . x >= b in the 18 joint torques x through
    lambda = lambda_0 + G_lambda x, with the header's tangent rule. Row i has the kernel's bit: j: tau_j <= lim_j; 18 + j:
    tau_j >= -lim_j; 36 + 5 k + {0: n . lam >= fn_min, 1: +t1, 2: -t1, 3: +t2, 4: -t2 (+-t . lam <= mu n . lam)}.
  * reference: the reduced problem from tir.null_space and tir._hessian (H_r = Z^T H Z = R^T R by Cholesky, c = R^-T g_r) and
    active_set_solve in fp64: a dual active-set method (Goldfarb and Idnani) on min 1/2 |R x + c|^2.
  * certificate: at a candidate (tau, nudot, lam, reported set) in fp64
      feasibility   every contact row at lambda(tau) = lambda_0 + G_lambda tau_j and at the returned lam: -slack over the sum of
                    the absolute terms of the row, sum_c |a_c| (|lambda_0c| + sum_j |G_cj tau_j|) + |b|;
      box           |tau_j| <= lim_j exactly;
      stationarity  min over y >= 0 of |Z^T grad f - sum_{i in set} y_i n_i| (a 25-line Lawson-Hanson NNLS on the components divided by
                    their scale), per component over tir's reduced-gradient scale + sum_i y_i |n_i|;
      set           every reported contact row's |slack| over the same scale as feasibility; reported torque bits exact; no bit of
                    an inactive body or beyond the stance list.
    Feasibility and stationarity over the reported set prove optimality of this convex problem.
  * yardstick_f32: the kernel's chain in numpy float32, never the kernel: tir.yardstick_f32's steps up to the reflected stack (R, c
    and the unscaled [G_lambda | lambda_0]), active_set_solve in float32 with the kernel's tolerances, the final clamp, and
    (nudot, lam) from constrained_dynamics_reference.yardstick_f32.
Bounds: ratio <= C 2^-24; C_F, C_S follow the project's rule (K_ref over the 180 problems of tests/test_task_qp.py, asserted <= C / 16
there, C the smallest power of two >= 16 K_ref), capped at 16384 and 32768.
"""
import numpy as np

import constrained_dynamics_reference as cdr
import mass_solve_reference as msr
import task_inverse_dynamics_reference as tir

NCOL, LIVE, JOINTS, NJ, NL, EPS = tir.NCOL, tir.LIVE, tir.JOINTS, tir.NJ, tir.NL, tir.EPS
LIMIT_SETS = {"nominal": (0.6, 2.0, 1.0), "tight": (0.4, 5.0, 0.5), "loose": (1.0, 0.0, 1.0)}     # mu, fn_min, torque-limit scale
BOX = 2 * NJ                                           # first contact bit
TOL32, DEP32, ITER32 = 256.0 * EPS, 1e-8, 100            # the kernel's TQ_TOL, TQ_DEP2 and default max_iter
# Measured by tests/test_task_qp.py::test_fp32_yardstick_sits_well_inside_the_bounds (table in that module's docstring)
C_F = 8192.0                                           # feasibility and reported-set rows
C_S = 16384.0                                          # stationarity
assert C_F <= 16384 and C_S <= 32768


def tangents(normal):
    """(n, t1, t2) of include/wbc_sim.h: None: (z, x, y); else n normalised, t1 = normalise(n x e), e = world x (world y where
    |n_x| > 0.9), t2 = n x t1."""
    if normal is None:
        return np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    t1 = np.cross(n, [0.0, 1.0, 0.0] if abs(n[0]) > 0.9 else [1.0, 0.0, 0.0])
    t1 = t1 / np.linalg.norm(t1)
    return n, t1, np.cross(n, t1)


class Rows:
    """The rows n . x >= b of one env. G [3K, 18], l0 [3K] (zeros on inactive rows): lambda = l0 + G x; on_bodies [K] bool; lim [18];
    mu [K] or a scalar; normals [K, 3] or None. bits [nc], N [nc, 18], b [nc]; contact rows also as A [ncontact, 3K] . lambda >= bf."""

    def __init__(self, G, l0, on_bodies, lim, mu, fn_min, normals=None):
        K = len(on_bodies)
        self.G, self.l0, self.lim = np.asarray(G, dtype=np.float64), np.asarray(l0, dtype=np.float64), np.asarray(lim, dtype=np.float64)
        mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (K,))
        bits, A, bf = [], [], []
        for k in range(K):
            if not on_bodies[k]:
                continue
            n, t1, t2 = tangents(None if normals is None else normals[k])
            for t, a in enumerate((n, mu[k] * n - t1, mu[k] * n + t1, mu[k] * n - t2, mu[k] * n + t2)):
                row = np.zeros(3 * K)
                row[3 * k:3 * k + 3] = a
                bits.append(BOX + 5 * k + t); A.append(row); bf.append(fn_min if t == 0 else 0.0)
        self.A, self.bf = np.array(A).reshape(len(A), 3 * K), np.array(bf)
        self.bits = np.r_[np.arange(BOX), np.array(bits, dtype=np.int64)].astype(np.int64)
        self.N = np.concatenate([-np.eye(NJ), np.eye(NJ), self.A @ self.G])
        self.b = np.r_[-self.lim, -self.lim, self.bf - self.A @ self.l0]

    def slack_and_scale(self, x, f=np.float64):
        """(slack, scale) [nc] at x, evaluated in dtype f the way the kernel does: lambda(x) and the sum of its absolute terms first."""
        x = np.asarray(x, dtype=f)
        G, l0, lim, A, bf = (np.asarray(v, dtype=f) for v in (self.G, self.l0, self.lim, self.A, self.bf))
        lam = (l0 + G @ x).astype(f)
        mag = (np.abs(l0) + np.abs(G) @ np.abs(x)).astype(f)
        s = np.r_[lim - x, lim + x, A @ lam - bf].astype(f)
        sc = np.r_[lim + np.abs(x), lim + np.abs(x), np.abs(A) @ mag + np.abs(bf)].astype(f)
        return s, sc


def _gram_schmidt(D, f):
    """Q [18, q], T [q, q] with D^T = Q T, column by column, Gram-Schmidt applied twice, in dtype f."""
    q = D.shape[0]
    Q, T = np.zeros((NJ, q), dtype=f), np.zeros((q, q), dtype=f)
    for j in range(q):
        w1 = Q[:, :j].T @ D[j]
        z = D[j] - Q[:, :j] @ w1
        w2 = Q[:, :j].T @ z
        z = z - Q[:, :j] @ w2
        rho = f(np.sqrt(max(float(z @ z), 1e-30 * float(D[j] @ D[j]))))
        Q[:, j], T[:j, j], T[j, j] = z / rho, w1 + w2, rho
    return Q, T


def _tri(T, v, lower, f):
    """Solve with the upper triangle T (lower: with T^T) in dtype f."""
    q = len(v)
    x = np.zeros(q, dtype=f)
    order = range(q) if lower else range(q - 1, -1, -1)
    for i in order:
        s = f(v[i])
        for k in (range(i) if lower else range(i + 1, q)):
            s = f(s - f((T[k, i] if lower else T[i, k]) * x[k]))
        x[i] = f(s / T[i, i])
    return x


def active_set_solve(R, c, rows, f=np.float64, tol=1e-12, dep2=1e-22, max_iter=1000):
    """min 1/2 |R x + c|^2 s.t. rows, R [18, 18] upper triangular: the method of wbc_taskqp_solve_kernel in dtype f. In y = R x + c row i is
    d_i . y >= beta_i, d_i = R^-T n_i. W is held as D_W^T = Q T (rebuilt from the d_i whenever it changes); after every accepted row
    x and the multipliers u are rebuilt from W. Returns (x, W as a list of row positions, status 0 / 1 / 2, iterations, u)."""
    R, c = np.asarray(R, dtype=f), np.asarray(c, dtype=f)
    N, b = rows.N.astype(f), rows.b.astype(f)
    D = np.stack([_tri(R, N[i], True, f) for i in range(len(N))])
    beta = (b + D @ c).astype(f)
    inv_d = (1.0 / np.sqrt(np.sum(D * D, axis=1))).astype(f)
    x0 = _tri(R, -c, False, f)
    x, W, u, p, sp = x0.copy(), [], np.zeros(0, dtype=f), -1, f(0)
    skip = []                                                                     # rows that W implies, until W changes
    for it in range(max_iter + 1):
        if p < 0:
            s, sc = rows.slack_and_scale(x, f)
            viol = s < np.r_[np.zeros(BOX, dtype=f), -f(tol) * sc[BOX:]]          # a box row has no tolerance
            viol[W + skip] = False
            if not viol.any():
                return x, W, 0, it, u
            p = int(np.argmax(np.where(viol, -s * inv_d, 0)))
            sp = s[p]
        if it >= max_iter:
            return x0, [], 1, it, u
        Q, T = _gram_schmidt(D[W], f)
        q = len(W)
        w1 = Q.T @ D[p]
        z = D[p] - Q @ w1
        w2 = Q.T @ z
        z = z - Q @ w2
        zz, dd = f(z @ z), f(D[p] @ D[p])
        dep = q >= NJ or not zz > f(dep2) * dd
        r = _tri(T, (w1 + w2).astype(f), False, f)
        t1, l = np.inf, -1
        for j in range(q):
            if r[j] > 0 and max(u[j], 0) / r[j] < t1:
                t1, l = max(u[j], f(0)) / r[j], j
        if dep and q > 0:
            # n_p = sum_j r_j n_j, so with W's rows tight the slack of p is sum_j r_j b_j - b_p whatever x is: the rounding of x says
            # nothing about it. Where that is no violation (the fourth and fifth row at a pyramid's apex) p is set aside, not swapped in
            simp = f(np.sum((r * b[W]).astype(f)) - b[p])
            if simp >= -f(tol) * f(np.sum(np.abs(r * b[W])) + abs(b[p]) + sc[p]):
                skip, p = skip + [p], -1
                continue
        if not dep and not (l >= 0 and t1 * zz < -sp):
            W = W + [p]
            p, skip = -1, []
            Q, T = _gram_schmidt(D[W], f)
            v = _tri(T, beta[W], True, f)
            u = _tri(T, v, False, f)
            x = _tri(R, ((Q @ v).astype(f) - c).astype(f), False, f)
            continue
        if l < 0:
            return x0, [], 2, it + 1, u
        if not dep:
            sp = f(sp + t1 * zz)
        u = np.delete((u - f(t1) * r).astype(f), l)
        W = W[:l] + W[l + 1:]
        skip = []
    raise AssertionError("unreachable")


def finish(x, W, status, rows, f=np.float64):
    """The returned torques: a joint whose limit row is in W on the limit exactly and every joint inside the box (status 0); the
    unconstrained optimum clamped (status 1, 2). (tau_j [18], reported set as a Python int)."""
    lim = rows.lim.astype(f)
    x = np.asarray(x, dtype=f).copy()
    bits = 0
    if status == 0:
        for i in W:
            bits |= 1 << int(rows.bits[i])
            if i < NJ:
                x[i] = lim[i]
            elif i < BOX:
                x[i - NJ] = -lim[i - NJ]
    return np.clip(x, -lim, lim), bits


def reduced(P):
    """(Z, x0, m, R, c, G [3K, 18], l0 [3K]) of the reduced problem in fp64: f = 1/2 |R x + c|^2 + const, lambda = l0 + G x."""
    Z, x0, m = tir.null_space(P)
    H, g = tir._hessian(P, m)
    R = np.linalg.cholesky(Z.T @ H @ Z).T
    c = np.linalg.solve(R.T, Z.T @ (H @ x0 + g))
    G, l0 = np.zeros((len(P.on), NJ)), np.zeros(len(P.on))
    G[P.on], l0[P.on] = Z[NL:NL + m], x0[NL:NL + m]
    return Z, x0, m, R, c, G, l0


def rows_of(P, lim, mu, fn_min, normals=None):
    """The fp64 rows of problem P (stance bodies: P.on in threes)."""
    _, _, _, _, _, G, l0 = reduced(P)
    return Rows(G, l0, P.on[::3], lim, mu, fn_min, normals)


def reference(P, lim, mu, fn_min, normals=None):
    """(tau [26], nudot [26], lam [3K], reported set, status, iterations, multipliers by bit) of the fp64 optimum."""
    Z, x0, m, R, c, G, l0 = reduced(P)
    rows = Rows(G, l0, P.on[::3], lim, mu, fn_min, normals)
    x, W, status, it, u = active_set_solve(R, c, rows)
    xj, bits = finish(x, W, status, rows)
    tau, nudot, lam = tir._unpack(P, x0 + Z @ xj, m)
    return tau, nudot, lam, bits, status, it, {int(rows.bits[i]): float(v) for i, v in zip(W, u)}


def nnls(A, b, iters=200):
    """min |A y - b| over y >= 0 (Lawson and Hanson)."""
    n = A.shape[1]
    y, P = np.zeros(n), np.zeros(n, dtype=bool)
    for _ in range(iters):
        w = A.T @ (b - A @ y)
        w[P] = -np.inf
        if n == 0 or w.max() <= 1e-14 * max(1.0, np.abs(A.T @ b).max()):
            break
        P[int(np.argmax(w))] = True
        for _ in range(iters):
            s = np.zeros(n)
            s[P] = np.linalg.lstsq(A[:, P], b, rcond=None)[0]
            if s[P].min() > 0:
                break
            neg = P & (s <= 0)
            alpha = np.min(y[neg] / (y[neg] - s[neg]))
            y = y + alpha * (s - y)
            P &= y > 1e-300
        y = s
    return y


def certificate(P, rows, tau, nudot, lam, bits):
    """Ratios (residual / (2^-24 scale)) of a status-0 candidate: 'feas' (contact rows at lambda(tau) and at lam), 'stat', 'set';
    booleans 'box' (inside, exactly), 'bits' (reported torque bits exact, no bit without a row)."""
    x = np.asarray(tau, dtype=np.float64)[JOINTS]
    s, sc = rows.slack_and_scale(x)
    s_ret = rows.A @ lam - rows.bf
    feas = max(float(np.max(-s[BOX:] / (EPS * sc[BOX:]), initial=0.0)), float(np.max(-s_ret / (EPS * sc[BOX:]), initial=0.0)))
    rep = [i for i in range(len(rows.bits)) if (bits >> int(rows.bits[i])) & 1]
    known = sum(1 << int(v) for v in rows.bits)
    bits_ok = (bits & ~known) == 0 and all(x[i] == rows.lim[i] for i in rep if i < NJ) and all(x[i - NJ] == -rows.lim[i - NJ] for i in rep if NJ <= i < BOX)
    crep = [i for i in rep if i >= BOX]
    on_set = max(float(np.max(np.abs(s[crep]) / (EPS * sc[crep]), initial=0.0)),
                 float(np.max(np.abs(s_ret[[i - BOX for i in crep]]) / (EPS * sc[crep]), initial=0.0)))
    # stationarity: Z^T grad f = sum y_i n_i, y >= 0, over the reported rows
    Z, _, _ = tir.null_space(P)
    JL, a, ref = P.Jt[:, LIVE], nudot[LIVE], P.ref[LIVE]
    grad = np.r_[JL.T @ (P.w * (JL @ a + P.gt - P.acc)) + P.wp * (a - ref), P.wf * lam[P.on], P.wt * tau[JOINTS]]
    _, sg = tir.reduced_gradient_and_scale(P, tau, nudot, lam)
    r = Z.T @ grad
    Nw = rows.N[rep].T
    y = nnls(Nw / sg[:, None], r / sg)
    stat = float(np.max(np.abs(r - Nw @ y) / (EPS * (sg + np.abs(Nw) @ y))))
    return {"feas": feas, "stat": stat, "set": on_set, "box": bool(np.all(np.abs(x) <= rows.lim)), "bits": bool(bits_ok)}


def chain_f32(P):
    """(R [18, 18] upper, c [18], G [3K, 18], l0 [3K]) of tir.yardstick_f32's chain in numpy float32: the reflected stack and the
    unscaled [G_lambda | lambda_0]. The steps are that function's, restated because it returns the torques alone."""
    f = np.float32
    on = P.on
    m = len(on)
    ST = np.zeros((NJ, NCOL))
    ST[np.arange(NJ), JOINTS] = 1.0
    J32 = P.Jc.astype(f)
    rhs = np.concatenate([J32.astype(np.float64), -P.h.astype(f).astype(np.float64)[None], ST])
    Y = msr.ldlt_solve_f32(P.M, rhs).astype(f)
    Yc, yh, Ys = Y[:m], Y[m], Y[m + 1:]
    damping, sp, sf, st = f(P.damping), f(np.sqrt(f(P.wp))), f(np.sqrt(f(P.wf))), f(np.sqrt(f(P.wt)))
    both = on[:, None] & on[None, :]
    A = np.where(both, tir._dots_f32(J32, Yc) + np.where(np.eye(m, dtype=bool), damping, f(0)), np.eye(m, dtype=f)).astype(f)
    c0 = ((P.a_stance.astype(f) - P.gamma.astype(f)).astype(f) - tir._dots_f32(J32, yh[None])[:, 0]).astype(f)
    C = np.concatenate([(f(0) - tir._dots_f32(J32, Ys)).astype(f), c0[:, None]], axis=1)
    C[~on] = 0
    L = np.zeros((m, m), dtype=f)                                                 # row-order Cholesky, every operation rounded
    for j in range(m):
        d = A[j, j]
        for k in range(j):
            d = f(d - f(L[j, k] * L[j, k]))
        L[j, j] = f(np.sqrt(d))
        for i in range(j + 1, m):
            s = A[i, j]
            for k in range(j):
                s = f(s - f(L[i, k] * L[j, k]))
            L[i, j] = f(s / L[j, j])
    G = C.copy()
    for j in range(NJ + 1):                                                       # L L^T g = column j, rounded to float32 per substitution
        y = _tri(L.T.copy(), C[:, j], True, f)
        G[:, j] = _tri(L.T.copy(), y, False, f)
    base = np.concatenate([Ys.T, yh[:, None]], axis=1)[LIVE]
    Ga = base.copy()
    for k in range(m):
        Ga = (Ga + (Yc[k][LIVE][:, None] * G[k][None, :]).astype(f)).astype(f)
    T = P.Jt.shape[0]
    JL = P.Jt.astype(f)[:, LIVE]
    Tr = np.zeros((T, NJ + 1), dtype=f)
    for s in range(NL):
        Tr = (Tr + (JL[:, s, None] * Ga[None, s, :]).astype(f)).astype(f)
    Tr[:, NJ] = (Tr[:, NJ] + (P.gt.astype(f) - P.acc.astype(f)).astype(f)).astype(f)
    Tr = np.where(P.w[:, None] > 0, (np.sqrt(P.w.astype(f)).astype(f)[:, None] * Tr).astype(f), f(0)).astype(f)
    post = Ga.copy()
    post[:, NJ] = (post[:, NJ] - P.ref.astype(f)[LIVE]).astype(f)
    post = (sp * post).astype(f)
    S = np.concatenate([post, (G * sf).astype(f), Tr, (st * np.eye(NJ, NJ + 1, dtype=f)).astype(f)]).astype(f)
    nrow = S.shape[0]
    for k in range(NJ):
        dots = np.zeros(NJ + 1, dtype=f)
        for r in range(k, nrow):
            dots = (dots + (S[r, k] * S[r]).astype(f)).astype(f)
        akk = S[k, k]
        nrm = f(np.sqrt(dots[k]))
        alpha = f(-nrm) if akk >= 0 else nrm
        vk = f(akk - alpha)
        t = ((dots - (alpha * S[k]).astype(f)).astype(f) * f(f(-1) / f(alpha * vk))).astype(f)
        v = S[:, k].copy()
        v[k] = vk
        for r in range(k, nrow):
            S[r, k + 1:] = (S[r, k + 1:] - (t[k + 1:] * v[r]).astype(f)).astype(f)
        S[k, k] = alpha
        S[k + 1:, k] = 0
    return np.triu(S[:NJ, :NJ]), S[:NJ, NJ].copy(), G[:, :NJ].copy(), G[:, NJ].copy()


def yardstick_f32(P, lim, mu, fn_min, normals=None, max_iter=ITER32):
    """(tau [26], nudot [26], lam [3K], reported set, status, iterations) of the kernel's chain in numpy float32."""
    f = np.float32
    R, c, G, l0 = chain_f32(P)
    rows = Rows(G, l0, P.on[::3], np.asarray(lim, dtype=f), np.asarray(mu, dtype=f), f(fn_min), normals)
    x, W, status, it, _ = active_set_solve(R, c, rows, f, TOL32, DEP32, max_iter)
    xj, bits = finish(x, W, status, rows, f)
    tau = np.zeros(NCOL)
    tau[JOINTS] = xj.astype(np.float64)
    nudot, lam = cdr.yardstick_f32(P.M, P.h, tau, P.Jc, P.gamma, P.a_stance.astype(f).astype(np.float64), P.damping, P.on)
    return tau, nudot, lam, bits, status, it
