"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) references for wbc_sim_body_accelerations / wbc_sim_constrained_dynamics
(csrc/wbc_arm_kernel.hip; definitions in include/wbc_sim.h).

  * body_accelerations: the world-frame classical recursion of inverse_dynamics_reference.py (omega, alpha, acceleration of every
    moving body's origin, propagated down the tree), carried to each rigid body's origin. The kernel works with spatial vectors about
    the base origin in base axes instead, so agreement means something. With dtype = float32 the same recursion runs in numpy
    float32 on positions relative to the root (the kernel never sees the root position): the rounding YARDSTICK, never the kernel.
    mag [27, 6] is the sum of the sizes of the terms the recursion adds (Euclidean norms: the world rotation mixes the components,
    so all three rows of a block share one figure): |a_root| + sum over the path of (|alpha_parent| |r| + |omega_parent|^2 |r|) for
    the linear rows, |alpha_root| + sum of (|qdd| + |omega_parent| |qd|) for the angular rows -- the scale that an fp32 evaluation's
    error is proportional to.
  * kkt_solve: a dense fp64 solve of the saddle-point system
        [ M   -Jc^T     ] [ nudot  ]   [ tau - h       ]
        [ Jc  damping I ] [ lambda ] = [ a_des - gamma ]
    on the 24 live coordinates.
  * row scales of the tests' bounds, d = sqrt(diag M), w_i = sum_j |Jc_ij| / d_j:
        dynamics row k:    d_k sum_j d_j |nudot_j| + |tau_k| + (|Jc|^T |lambda|)_k       bound C_S 2^-24 scale + C_ID 2^-24 mag_k(h)
        constraint row i:  w_i sum_j d_j |nudot_j| + damping |lambda_i| + |a_des_i|      bound C_K 2^-24 scale + C_A 2^-24 mag_i(gamma)
    C_S = 128 and C_ID = 4096 are the constants tests/test_mass_solve.py uses for forward dynamics, restated. C_A and C_K are the
    smallest powers of two >= 16 K_ref (C_K at least 32, C_A at most 1024), K_ref the fp32 yardstick's largest ratio over the
    families of tests/test_constrained_dynamics.py, measured there on the CPU and asserted <= C / 16.
  * yardstick_f32: M_ref, Jc_ref, gamma_ref and h_ref rounded to fp32, then mass_solve_reference.ldlt_solve_f32 for
    Y = (M^-1 [Jc^T | tau - h])^T, A = Jc Y^T + damping I and a row-order Cholesky of it in numpy float32, lambda, nudot.
"""
import numpy as np

import arm_osc_oracle as ao
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import whole_body_reference as wb

NCOL, FINGERS, LIVE, EPS, C_S = msr.NCOL, msr.FINGERS, msr.LIVE, msr.EPS, msr.C_S
C_ID = 4096.0
# Measured by tests/test_constrained_dynamics.py::test_fp32_yardsticks_sit_well_inside_the_bounds (its table is in that module's
# docstring): K_ref 3.49 for the accelerations and 0.457 for the constraint rows.
C_A = 64.0
C_K = 32.0
assert C_A <= 1024 and C_K >= 32


def _fk(model, root_pos, root_quat, q, dt):
    nb = model.nb
    R, p = np.zeros((nb, 3, 3), dtype=dt), np.zeros((nb, 3), dtype=dt)
    R[0], p[0] = ao.quat_to_mat(np.asarray(root_quat, dtype=np.float64)).astype(dt), np.asarray(root_pos, dtype=dt)
    for i in range(1, nb):
        par = model.parent[i]
        p[i] = p[par] + R[par] @ np.asarray(model.joint_xyz[i], dtype=dt)
        R[i] = R[par] @ ao.rot_axis(model.axis[i], dt(q[model.body_dof[i]])).astype(dt)
    return R, p


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=a.dtype)


def body_accelerations(model, root_pos, root_quat, q, nu, nudot=None, dtype=np.float64):
    """(acc [27, 6], mag [27, 6]): classical world-frame linear acceleration of every rigid body's origin and its angular
    acceleration, J nudot + Jdot nu. dtype = numpy.float32: the yardstick (root at the origin, every operation rounded)."""
    dt = dtype
    q, nu = np.asarray(q, dtype=dt), np.asarray(nu, dtype=dt)
    nudot = np.zeros(NCOL, dtype=dt) if nudot is None else np.asarray(nudot, dtype=dt)
    R, p = _fk(model, root_pos if dt == np.float64 else np.zeros(3), root_quat, q, dt)
    nb = model.nb
    om, al, acc = np.zeros((nb, 3), dtype=dt), np.zeros((nb, 3), dtype=dt), np.zeros((nb, 3), dtype=dt)
    ml, ma = np.zeros(nb), np.zeros(nb)
    om[0], al[0], acc[0] = nu[3:6], nudot[3:6], nudot[0:3]
    nrm = lambda v: float(np.linalg.norm(np.asarray(v, dtype=np.float64)))
    ml[0], ma[0] = nrm(acc[0]), nrm(al[0])
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        ax = R[b][:, model.axis[b]]
        r = p[b] - p[par]
        om[b] = om[par] + ax * nu[6 + d]
        al[b] = al[par] + ax * nudot[6 + d] + _cross(om[par], ax * nu[6 + d])
        acc[b] = acc[par] + _cross(al[par], r) + _cross(om[par], _cross(om[par], r))
        ml[b] = ml[par] + (nrm(al[par]) + nrm(om[par]) ** 2) * nrm(r)
        ma[b] = ma[par] + abs(float(nudot[6 + d])) + nrm(om[par]) * abs(float(nu[6 + d]))
    out, mag = np.zeros((len(model.rb_body), 6), dtype=dt), np.zeros((len(model.rb_body), 6))
    for r_, b in enumerate(model.rb_body):
        rc = R[b] @ np.asarray(model.rb_offset[r_], dtype=dt)
        out[r_, 0:3] = acc[b] + _cross(al[b], rc) + _cross(om[b], _cross(om[b], rc))
        out[r_, 3:6] = al[b]
        mag[r_, 0:3] = ml[b] + (nrm(al[b]) + nrm(om[b]) ** 2) * nrm(rc)
        mag[r_, 3:6] = ma[b]
    return out.astype(np.float64), mag


def constraint_rows(model, root_pos, root_quat, q, nu, bodies, active=None):
    """(Jc [3K, 26], gamma [3K], mag [3K]) of the listed rigid bodies' origins: linear Jacobian rows, Jdot nu and its magnitude;
    the rows of an inactive body are zero."""
    J = wb.jacobian(model, root_pos, root_quat, q)
    acc, mag = body_accelerations(model, root_pos, root_quat, q, nu)
    on = np.repeat(np.ones(len(bodies), dtype=bool) if active is None else np.asarray(active, dtype=bool), 3)
    rows = lambda a: np.concatenate([a[r][0:3] for r in bodies])
    return rows(J) * on[:, None], rows(acc) * on, rows(mag) * on


def kkt_solve(M, h, tau, Jc, gamma, a_des, damping=0.0):
    """(nudot [26], lam [m]) of the saddle-point system on the live coordinates; Jc [m, 26] holds the ACTIVE rows only (m may be 0)."""
    m, nl = Jc.shape[0], len(LIVE)
    K = np.zeros((nl + m, nl + m))
    K[:nl, :nl] = M[np.ix_(LIVE, LIVE)]
    K[:nl, nl:] = -Jc[:, LIVE].T
    K[nl:, :nl] = Jc[:, LIVE]
    K[nl:, nl:] = damping * np.eye(m)
    b = np.r_[(np.zeros(NCOL) if tau is None else np.asarray(tau, dtype=np.float64))[LIVE] - h[LIVE], np.asarray(a_des, dtype=np.float64) - gamma]
    x = np.linalg.solve(K, b)
    nudot = np.zeros(NCOL)
    nudot[LIVE] = x[:nl]
    return nudot, x[nl:]


def solve_with_mask(M, h, tau, Jc, gamma, a_des, damping, on):
    """kkt_solve on the rows where `on` [m] holds; lam comes back full, zeros elsewhere."""
    on = np.asarray(on, dtype=bool)
    nudot, lam_on = kkt_solve(M, h, tau, Jc[on], gamma[on], np.asarray(a_des, dtype=np.float64)[on], damping)
    lam = np.zeros(len(on))
    lam[on] = lam_on
    return nudot, lam


def _d(M):
    d = np.zeros(NCOL)
    d[LIVE] = np.sqrt(np.diag(M)[LIVE])
    return d


def dynamics_residual_and_scale(M, h, tau, Jc, nudot, lam):
    """(|M nudot + h - tau - Jc^T lam| [26], scale [26]), fingers 0."""
    tau = np.zeros(NCOL) if tau is None else np.asarray(tau, dtype=np.float64)
    d = _d(M)
    res = np.abs(M @ nudot + h - tau - Jc.T @ lam)
    scale = d * (d @ np.abs(nudot)) + np.abs(tau) + np.abs(Jc).T @ np.abs(lam)
    res[FINGERS], scale[FINGERS] = 0.0, 0.0
    return res, scale


def constraint_residual_and_scale(M, Jc, gamma, a_des, damping, nudot, lam):
    """(|Jc nudot + gamma - a_des + damping lam| [m], scale [m]); Jc, gamma, a_des are zero on inactive rows by the caller."""
    d = _d(M)
    w = np.abs(Jc[:, LIVE]) @ (1.0 / d[LIVE])
    a_des = np.asarray(a_des, dtype=np.float64)
    res = np.abs(Jc @ nudot + gamma - a_des + damping * lam)
    return res, w * (d @ np.abs(nudot)) + damping * np.abs(lam) + np.abs(a_des)


def delassus_condition(M, Jc, damping, on):
    """Condition number of the diagonally scaled Delassus matrix A_ii^-1/2 A A_ii^-1/2 over the active rows (1 if none)."""
    on = np.asarray(on, dtype=bool)
    if not on.any():
        return 1.0
    J = Jc[on][:, LIVE]
    A = J @ np.linalg.solve(M[np.ix_(LIVE, LIVE)], J.T) + damping * np.eye(J.shape[0])
    s = 1.0 / np.sqrt(np.diag(A))
    return float(np.linalg.cond(A * s[:, None] * s[None, :]))


def yardstick_f32(M, h, tau, Jc, gamma, a_des, damping, on):
    """(nudot [26], lam [m]) of the chain in numpy float32: ldlt_solve_f32 on fl(M) with the right-hand sides [fl(Jc); fl(tau) - fl(h)],
    A from its lower triangle, a row-order Cholesky, the two triangular solves, nudot = a_free + Y^T lam. Inactive rows: identity."""
    f = np.float32
    on = np.asarray(on, dtype=bool)
    m = Jc.shape[0]
    J = Jc.astype(f)
    tau = np.zeros(NCOL) if tau is None else np.asarray(tau, dtype=np.float64)
    b = (tau.astype(f) - h.astype(f)).astype(f)
    Y = msr.ldlt_solve_f32(M, np.concatenate([J.astype(np.float64), b.astype(np.float64)[None]])).astype(f)      # [m + 1, 26]
    A = np.zeros((m, m), dtype=f)
    c = np.zeros(m, dtype=f)
    for i in range(m):
        for j in range(i + 1):
            acc = f(0)
            for k in LIVE:
                acc = f(acc + f(J[i, k] * Y[j, k]))
            A[i, j] = (f(acc + f(damping)) if i == j else acc) if on[i] and on[j] else f(i == j)
        if on[i]:
            acc = f(0)
            for k in LIVE:
                acc = f(acc + f(J[i, k] * Y[m, k]))
            c[i] = f(f(f(a_des[i]) - f(gamma[i])) - acc)
    L = np.zeros((m, m), dtype=f)
    for i in range(m):
        for j in range(i + 1):
            acc = A[i, j]
            for k in range(j):
                acc = f(acc - f(L[i, k] * L[j, k]))
            L[i, j] = f(np.sqrt(acc)) if i == j else f(acc / L[j, j])
    y = c.copy()
    for i in range(m):
        acc = y[i]
        for k in range(i):
            acc = f(acc - f(L[i, k] * y[k]))
        y[i] = f(acc / L[i, i])
    for i in range(m - 1, -1, -1):
        acc = y[i]
        for k in range(i + 1, m):
            acc = f(acc - f(L[k, i] * y[k]))
        y[i] = f(acc / L[i, i])
    nudot = np.zeros(NCOL)
    for k in LIVE:
        acc = Y[m, k]
        for i in range(m):
            acc = f(acc + f(Y[i, k] * y[i]))
        nudot[k] = float(acc)
    return nudot, np.where(on, y.astype(np.float64), 0.0)
