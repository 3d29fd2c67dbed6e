"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) references for wbc_sim_task_inverse_dynamics (csrc/wbc_arm_kernel.hip; definition in
include/wbc_sim.h).

  * kkt_reference: a dense fp64 solve of the FULL Karush-Kuhn-Tucker system of the equality-constrained quadratic programme in
    x = (nudot [24 live], lambda [m active rows], tau_j [18]) and the multipliers of its 24 + m equality rows,
        [ H  E^T ] [ x  ]   [ -g ]        H = blkdiag(J_t^T W J_t + w_posture I, w_force I, w_torque I),
        [ E  0   ] [ mu ] = [  d ]        E = [ M  -Jc^T  -S^T ; Jc  damping I  0 ],   d = (-h ; a_stance - gamma).
    The kernel eliminates (nudot, lambda) through constrained forward dynamics and solves a least-squares problem in tau_j alone by
    Householder reflections: another algorithm, so agreement means something.
  * four tiers of residuals at a candidate (tau, nudot, lambda), each with the scale an fp32 evaluation's error is proportional to:
      1. dynamics rows: constrained_dynamics_reference.dynamics_residual_and_scale with tau = S^T tau_j (root rows reported apart);
      2. stance rows: constrained_dynamics_reference.constraint_residual_and_scale;
      3. structure (exact zeros): the tests assert these directly;
      4. reduced gradient r = Z^T grad f, Z = [G_a; G_lambda; I] the fp64 null-space basis of E (columns = unit joint torques),
         scale |Z|^T (sum of the absolute terms of grad f): first-order optimality, insensitive to the problem's conditioning.
  * yardstick_f32: the kernel's chain in numpy float32 (never the kernel): mass_solve_reference.ldlt_solve_f32 for
    Y = (M^-1 [Jc^T | -h | S^T])^T, the Delassus matrix and its row-order Cholesky, [G_lambda | lambda_0], [G_a | a_0], the stacked
    sqrt(weight)-scaled rows, 18 Householder reflections with the dot products split over three row groups, back-substitution, then
    (nudot, lambda) recomputed from tau_j by constrained_dynamics_reference.yardstick_f32's chain. Sums run in the kernel's order with
    every operation rounded (vectorised over independent entries only).
Bounds: C 2^-24 scale, plus C_ID 2^-24 mag(h) on the dynamics rows and C_A 2^-24 mag(gamma) on the stance rows (restated from
constrained_dynamics_reference.py). The constants follow the project's rule: K_ref the yardstick's largest ratio over the families of
tests/test_task_inverse_dynamics.py (measured there on the CPU, asserted <= C / 16), C the smallest power of two >= 16 K_ref.
"""
import numpy as np

import constrained_dynamics_reference as cdr
import mass_solve_reference as msr
import whole_body_reference as wb

NCOL, FINGERS, LIVE, EPS = cdr.NCOL, cdr.FINGERS, cdr.LIVE, cdr.EPS
JOINTS = [c for c in LIVE if c >= 6]                   # the 18 columns that carry a joint torque, DoF order
NJ, NL = len(JOINTS), len(LIVE)
assert NJ == 18 and list(LIVE[:6]) == [0, 1, 2, 3, 4, 5]
C_S, C_ID, C_A = cdr.C_S, cdr.C_ID, cdr.C_A            # 128, 4096, 64: restated
# Measured by tests/test_task_inverse_dynamics.py::test_fp32_yardsticks_sit_well_inside_the_bounds (table in that module's docstring)
C_ROOT = 128.0                                         # dynamics rows 0:6
C_JOINT = 256.0                                        # dynamics rows 6:
C_STANCE = 1024.0                                       # stance rows
C_GRAD = 8192.0                                        # reduced gradient
assert C_GRAD <= 16384


class Problem:
    """One env's problem in fp64. Jc [3K, 26], gamma, a_stance [3K] (zero on inactive rows), on [3K] bool; Jt [6T, 26], gt, acc, w [6T]
    (acc is ignored where w = 0); ref [26]; weights = (posture, force, torque, damping)."""

    def __init__(self, M, h, Jc, gamma, a_stance, on, Jt, gt, acc, w, ref, weights):
        self.M, self.h = M, h
        self.on = np.asarray(on, dtype=bool)
        self.Jc, self.gamma = Jc * self.on[:, None], gamma * self.on
        self.a_stance = np.where(self.on, np.asarray(a_stance, dtype=np.float64), 0.0)
        self.Jt, self.gt = Jt, gt
        self.w = np.asarray(w, dtype=np.float64)
        self.acc = np.where(self.w > 0, np.asarray(acc, dtype=np.float64), 0.0)
        self.ref = np.zeros(NCOL) if ref is None else np.asarray(ref, dtype=np.float64)
        self.wp, self.wf, self.wt, self.damping = [float(x) for x in weights]


def task_rows(J, acc, mag, bodies):
    """(Jt [6T, 26], gt [6T], mag [6T]) of the listed rigid bodies from whole_body_reference.jacobian's J [27, 6, 26] and
    constrained_dynamics_reference.body_accelerations' (Jdot nu, mag) [27, 6]."""
    if len(bodies) == 0:
        return np.zeros((0, NCOL)), np.zeros(0), np.zeros(0)
    return np.concatenate([J[r] for r in bodies]), np.concatenate([acc[r] for r in bodies]), np.concatenate([mag[r] for r in bodies])


def _equality(P):
    """E [24 + m, 24 + m + 18] and d of the active rows."""
    on = P.on
    m = int(on.sum())
    E = np.zeros((NL + m, NL + m + NJ))
    E[:NL, :NL] = P.M[np.ix_(LIVE, LIVE)]
    E[:NL, NL:NL + m] = -P.Jc[on][:, LIVE].T
    for j, c in enumerate(JOINTS):
        E[LIVE.index(c) if isinstance(LIVE, list) else int(np.nonzero(np.asarray(LIVE) == c)[0][0]), NL + m + j] = -1.0
    E[NL:, :NL] = P.Jc[on][:, LIVE]
    E[NL:, NL:NL + m] = P.damping * np.eye(m)
    d = np.r_[-P.h[LIVE], (P.a_stance - P.gamma)[on]]
    return E, d, m


def _hessian(P, m):
    JL = P.Jt[:, LIVE]
    H = np.zeros((NL + m + NJ, NL + m + NJ))
    H[:NL, :NL] = JL.T @ (P.w[:, None] * JL) + P.wp * np.eye(NL)
    H[NL:NL + m, NL:NL + m] = P.wf * np.eye(m)
    H[NL + m:, NL + m:] = P.wt * np.eye(NJ)
    g = np.zeros(NL + m + NJ)
    g[:NL] = JL.T @ (P.w * (P.gt - P.acc)) - P.wp * P.ref[LIVE]
    return H, g


def _unpack(P, x, m):
    nudot, lam, tau = np.zeros(NCOL), np.zeros(len(P.on)), np.zeros(NCOL)
    nudot[LIVE] = x[:NL]
    lam[P.on] = x[NL:NL + m]
    tau[JOINTS] = x[NL + m:NL + m + NJ]
    return tau, nudot, lam


def kkt_reference(P):
    """(tau [26], nudot [26], lam [3K]) of the optimum; tau rows 0:6 and fingers 0, lam 0 on inactive rows."""
    E, d, m = _equality(P)
    H, g = _hessian(P, m)
    nx, ne = H.shape[0], E.shape[0]
    K = np.zeros((nx + ne, nx + ne))
    K[:nx, :nx], K[:nx, nx:], K[nx:, :nx] = H, E.T, E
    x = np.linalg.solve(K, np.r_[-g, d])
    return _unpack(P, x[:nx], m)


def objective(P, tau, nudot, lam):
    r = P.Jt @ nudot + P.gt - P.acc
    return 0.5 * (P.w @ (r * r)) + 0.5 * P.wp * np.sum((nudot - P.ref)[LIVE] ** 2) + 0.5 * P.wf * np.sum(lam[P.on] ** 2) \
        + 0.5 * P.wt * np.sum(tau[JOINTS] ** 2)


def null_space(P):
    """Z [24 + m + 18, 18] = [G_a; G_lambda; I] and the particular solution x0 (tau_j = 0) of E x = d, in fp64."""
    E, d, m = _equality(P)
    A = E[:, :NL + m]
    G = np.linalg.solve(A, -E[:, NL + m:])
    x0 = np.linalg.solve(A, d)
    return np.vstack([G, np.eye(NJ)]), np.r_[x0, np.zeros(NJ)], m


def reduced_gradient_and_scale(P, tau, nudot, lam):
    """(|Z^T grad f| [18], scale [18]) at (tau, nudot, lam)."""
    Z, _, m = null_space(P)
    JL, a, ref = P.Jt[:, LIVE], nudot[LIVE], P.ref[LIVE]
    grad = np.r_[JL.T @ (P.w * (JL @ a + P.gt - P.acc)) + P.wp * (a - ref), P.wf * lam[P.on], P.wt * tau[JOINTS]]
    mag = np.r_[np.abs(JL).T @ (P.w * (np.abs(JL) @ np.abs(a) + np.abs(P.gt) + np.abs(P.acc))) + P.wp * (np.abs(a) + np.abs(ref)),
                P.wf * np.abs(lam[P.on]), P.wt * np.abs(tau[JOINTS])]
    return np.abs(Z.T @ grad), np.abs(Z).T @ mag


def tiers(P, tau, nudot, lam):
    """dict of (residual, scale) arrays: 'root' [6], 'joint' [18], 'stance' [active rows], 'grad' [18]."""
    r, s = cdr.dynamics_residual_and_scale(P.M, P.h, tau, P.Jc, nudot, lam)
    rc, sc = cdr.constraint_residual_and_scale(P.M, P.Jc, P.gamma, P.a_stance, P.damping, nudot, lam)
    rg, sg = reduced_gradient_and_scale(P, tau, nudot, lam)
    return {"root": (r[:6], s[:6]), "joint": (r[JOINTS], s[JOINTS]), "stance": (rc[P.on], sc[P.on]), "grad": (rg, sg)}


def ratios(P, tau, nudot, lam):
    """Largest residual / (2^-24 scale) of each tier (0 for an empty tier)."""
    out = {}
    for k, (r, s) in tiers(P, tau, nudot, lam).items():
        assert np.all(s > 0), k
        out[k] = float((r / (EPS * s)).max()) if len(r) else 0.0
    return out


def _dots_f32(A, B):
    """[a, b]: sum_c A[a, c] B[b, c] in float32, c in order, every product and sum rounded."""
    f = np.float32
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=f)
    for c in range(A.shape[1]):
        acc = (acc + (A[:, c, None] * B[None, :, c]).astype(f)).astype(f)
    return acc


def yardstick_f32(P):
    """(tau [26], nudot [26], lam [3K]) of the kernel's chain in numpy float32."""
    f = np.float32
    on = P.on
    m = len(on)
    ST = np.zeros((NJ, NCOL))
    ST[np.arange(NJ), JOINTS] = 1.0
    J32 = P.Jc.astype(f)
    rhs = np.concatenate([J32.astype(np.float64), -P.h.astype(f).astype(np.float64)[None], ST])
    Y = msr.ldlt_solve_f32(P.M, rhs).astype(f)                                   # [m + 1 + 18, 26]
    Yc, yh, Ys = Y[:m], Y[m], Y[m + 1:]
    damping, sp, sf, st = f(P.damping), f(np.sqrt(f(P.wp))), f(np.sqrt(f(P.wf))), f(np.sqrt(f(P.wt)))
    both = on[:, None] & on[None, :]
    A = np.where(both, _dots_f32(J32, Yc) + np.where(np.eye(m, dtype=bool), damping, f(0)), np.eye(m, dtype=f)).astype(f)
    c0 = ((P.a_stance.astype(f) - P.gamma.astype(f)).astype(f) - _dots_f32(J32, yh[None])[:, 0]).astype(f)
    C = np.concatenate([(f(0) - _dots_f32(J32, Ys)).astype(f), c0[:, None]], axis=1)                              # [m, 19]
    C[~on] = 0
    L = np.zeros((m, m), dtype=f)
    D = np.zeros(m, dtype=f)
    for j in range(m):
        d = A[j, j]
        for k in range(j):
            d = f(d - f(L[j, k] * L[j, k]))
        D[j] = f(f(1) / f(np.sqrt(d)))
        for i in range(j + 1, m):
            s = A[i, j]
            for k in range(j):
                s = f(s - f(L[i, k] * L[j, k]))
            L[i, j] = f(s * D[j])

    def chol_solve(X):                                                           # columns of X [m, k] in place
        X = X.copy()
        for i in range(m):
            s = X[i]
            for k in range(i):
                s = (s - (L[i, k] * X[k]).astype(f)).astype(f)
            X[i] = (s * D[i]).astype(f)
        for i in range(m - 1, -1, -1):
            s = X[i]
            for k in range(i + 1, m):
                s = (s - (L[k, i] * X[k]).astype(f)).astype(f)
            X[i] = (s * D[i]).astype(f)
        return X

    G = chol_solve(C)                                                            # [G_lambda | lambda_0]
    base = np.concatenate([Ys.T, yh[:, None]], axis=1)[LIVE]                     # [24, 19]
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
    diag = np.zeros(NJ, dtype=f)
    for k in range(NJ):
        part = np.zeros((3, NJ + 1), dtype=f)
        for g in range(3):
            for r in range(k + g, nrow, 3):
                part[g] = (part[g] + (S[r, k] * S[r]).astype(f)).astype(f)
        dots = ((part[0] + part[1]).astype(f) + part[2]).astype(f)
        akk = S[k, k]
        nrm = f(np.sqrt(dots[k]))
        alpha = f(-nrm) if akk >= 0 else nrm
        vk = f(akk - alpha)
        t = ((dots - (alpha * S[k]).astype(f)).astype(f) * f(f(-1) / f(alpha * vk))).astype(f)
        v = S[:, k].copy()
        v[k] = vk
        for r in range(k, nrow):
            S[r, k + 1:] = (S[r, k + 1:] - (t[k + 1:] * v[r]).astype(f)).astype(f)
        diag[k] = alpha
    tj = np.zeros(NJ, dtype=f)
    for k in range(NJ - 1, -1, -1):
        x = f(f(0) - S[k, NJ])
        for j in range(k + 1, NJ):
            x = f(x - f(S[k, j] * tj[j]))
        tj[k] = f(x / diag[k])
    tau = np.zeros(NCOL)
    tau[JOINTS] = tj.astype(np.float64)
    nudot, lam = cdr.yardstick_f32(P.M, P.h, tau, P.Jc, P.gamma, P.a_stance.astype(f).astype(np.float64), P.damping, on)
    return tau, nudot, lam
