"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) references for wbc_sim_mass_solve / wbc_sim_forward_dynamics (csrc/wbc_arm_kernel.hip;
definitions in include/wbc_sim.h).

  * M_ref = whole_body_reference.mass_matrix in fp64 (centre-of-mass Jacobians, no factorisation over the tree), plus the
    implicit-PD armature on the joint diagonal when asked; h_ref = inverse_dynamics_reference.bias_forces. Solves are dense
    numpy.linalg.solve on the 24 live coordinates.
  * ldlt_solve_f32: a plain row-order L D L^T in numpy float32, one rounded operation at a time, on M_ref rounded to fp32. It is the
    rounding YARDSTICK (what an fp32 solve that knows nothing of the tree loses on this matrix) and is never the kernel.
  * the row scale of the tests' bound. With d_k = sqrt(M_kk) an L D L^T solve in any elimination order satisfies
        |M x - b|_k <= (3 n + 1) u (|L| |D| |L^T| |x|)_k        (Higham, Accuracy and Stability of Numerical Algorithms, ch. 10)
    and (|L| |D| |L^T|)_kj <= d_k d_j by Cauchy-Schwarz, so
        |M_ref x - b|_k <= C_S 2^-24 (d_k sum_j d_j |x_j| + |b_k|),   C_S = 128:
    3 * 24 + 1 = 73 for the solve, 55 * 2^-24 d_k d_j for forming M_kj in fp32, rounded up to a power of two. The scale is
    invariant under diagonal scaling (cond M reaches 3e5, after scaling by d it is about 40); |M| |x| + |b| is NOT the scale of
    this problem (the yardstick itself reaches 183 against it) and is not used.
"""
import numpy as np

import inverse_dynamics_reference as idr
import whole_body_reference as wb

NCOL = wb.NCOL
FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(NCOL) if c not in FINGERS]
EPS = 2.0 ** -24
C_S = 128.0


def armature_vector(tcfg):
    """[26]: 0 for the root coordinates, wbc_task_cfg.joint_armature for the actuated joints, 0 for the fingers."""
    a = np.zeros(NCOL)
    a[6:6 + len(tcfg.joint_armature)] = [float(x) for x in tcfg.joint_armature]
    return a


def mass_matrix(model, root_pos, root_quat, q, body_params=None, armature=None):
    """M_ref [26, 26] (+ diag(armature))."""
    M = wb.mass_matrix(model, root_pos, root_quat, q, body_params)
    return M if armature is None else M + np.diag(armature)


def solve(M, b):
    """M^-1 b on the live coordinates in fp64, fingers 0; b [26] or [K, 26]."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    x[..., LIVE] = np.linalg.solve(M[np.ix_(LIVE, LIVE)], b[..., LIVE].T if b.ndim == 2 else b[LIVE]).T
    return x


def forward_dynamics(model, root_pos, root_quat, q, nu, tau=None, body_params=None, gravity=idr.GRAVITY, armature=None):
    """(nudot [26], M, h, mag): (M_ref + A) nudot = tau - h_ref, with mag the magnitude vector of h_ref."""
    M = mass_matrix(model, root_pos, root_quat, q, body_params, armature)
    h, mag = idr.bias_forces(model, root_pos, root_quat, q, nu, body_params, gravity)
    b = (np.zeros(NCOL) if tau is None else np.asarray(tau, dtype=np.float64)) - h
    return solve(M, b), M, h, mag


def row_scale(M, x, b):
    """d_k sum_j d_j |x_j| + |b_k| over the live coordinates (0 on the fingers); x, b [26] or [K, 26]."""
    d = np.zeros(NCOL)
    d[LIVE] = np.sqrt(np.diag(M)[LIVE])
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = d * (np.abs(x) @ d)[..., None] + np.abs(b)
    s[..., FINGERS] = 0.0
    return s


def residual(M, x, b):
    """|M x - b| on the live coordinates, 0 on the fingers."""
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    r = np.abs(x @ M.T - b)
    r[..., FINGERS] = 0.0
    return r


def largest_ratio(M, x, b):
    """max over right-hand sides and live rows of |M x - b|_k / (2^-24 scale_k)."""
    r, s = residual(M, x, b)[..., LIVE], row_scale(M, x, b)[..., LIVE]
    assert np.all(s > 0)
    return float((r / (EPS * s)).max())


def ldlt_solve_f32(M, b):
    """x [K, 26] (float32 values) of a row-order L D L^T solve carried out in float32 on fl32(M) restricted to the live
    coordinates, every operation rounded; b [26] or [K, 26]."""
    f = np.float32
    A = M[np.ix_(LIVE, LIVE)].astype(f)
    n = len(LIVE)
    L = np.zeros((n, n), dtype=f)
    D = np.zeros(n, dtype=f)
    for j in range(n):
        acc = A[j, j]
        for k in range(j):
            acc = f(acc - f(f(L[j, k] * L[j, k]) * D[k]))
        D[j] = acc
        for i in range(j + 1, n):
            acc = A[i, j]
            for k in range(j):
                acc = f(acc - f(f(L[i, k] * L[j, k]) * D[k]))
            L[i, j] = f(acc / D[j])
    b2 = np.atleast_2d(np.asarray(b, dtype=np.float64))
    out = np.zeros(b2.shape, dtype=np.float64)
    for r in range(b2.shape[0]):
        z = b2[r, LIVE].astype(f)
        for i in range(n):
            acc = z[i]
            for k in range(i):
                acc = f(acc - f(L[i, k] * z[k]))
            z[i] = acc
        for i in range(n):
            z[i] = f(z[i] / D[i])
        for i in range(n - 1, -1, -1):
            acc = z[i]
            for k in range(i + 1, n):
                acc = f(acc - f(L[k, i] * z[k]))
            z[i] = acc
        out[r, LIVE] = z.astype(np.float64)
    return out if np.ndim(b) == 2 else out[0]


# ---- the right-hand-side families of the GPU tests (the CPU test measures the yardstick on the same ones) -------------------------
def force_rhs(rng, shape):
    """Generalised forces [..., 26]: force rows uniform +-100 N, moment rows +-20 N m, joint rows +-10 N m."""
    b = rng.uniform(-1.0, 1.0, tuple(shape) + (NCOL,))
    b[..., 0:3] *= 100.0
    b[..., 3:6] *= 20.0
    b[..., 6:] *= 10.0
    return b


def jacobian_rows(model, root_pos, root_quat, q, rigid_body):
    """[6, 26]: the six Jacobian rows of one rigid body's origin (whole_body_reference.point_jacobian)."""
    import arm_osc_oracle as ao
    R, p = ao.fk(model, root_pos, root_quat, np.asarray(q, dtype=np.float64))
    b = model.rb_body[rigid_body]
    return wb.point_jacobian(model, R, p, b, p[b] + R[b] @ model.rb_offset[rigid_body])


def lambda_inverse(M, J):
    """(J M^-1 J^T [6, 6], bound [6, 6]): the tests' bound 2 C_S 2^-24 |d o x_a|_1 |d o x_b|_1 with x = M^-1 J^T columns -- the
    residual bound pushed through x^T r, once for each factor."""
    X = solve(M, J)                                        # [6, 26]: row a = (M^-1 J_a^T)^T
    d = np.zeros(NCOL)
    d[LIVE] = np.sqrt(np.diag(M)[LIVE])
    w = np.abs(X) @ d
    return X @ J.T, 2.0 * C_S * EPS * np.outer(w, w)
