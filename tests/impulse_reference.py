"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) references for wbc_sim_impulse_dynamics (csrc/wbc_arm_kernel.hip; definitions in
include/wbc_sim.h): what a set of contacts that closes does to the generalised velocity,

    M (nu+ - nu) = iota + Jc^T lam ,     Jc nu+ + damping lam = t ,     t = vdes - e (u - vdes) ,   u = Jc nu .

  * solve_with_mask: a dense fp64 solve of the saddle-point system on the 24 live coordinates and the active rows
        [ M   -Jc^T     ] [ nu+ ]   [ M nu + iota ]
        [ Jc  damping I ] [ lam ] = [ t           ]
  * impact_map: P = 1 - M^-1 Jc^T (A + damping)^-1 diag(1 + e) Jc, A = Jc M^-1 Jc^T, finger rows and columns 0.
  * delta_energy: T(nu+) - T(nu), T = nu^T M nu / 2; energy_identity: (1 - e) lam^T u / 2 - damping |lam|^2 / 2, which equals it for
    iota = 0, vdes = 0 and one e for all rows.
  * contact_velocities: u by the world-frame recursion (omega, and the velocity of every moving body's origin relative to the root's
    linear motion, carried down the tree). With dtype = float32 the recursion runs in numpy float32 with the root at the origin: the
    yardstick of a velocity walk. product_f32 is the other form, the 24-term sum fl(Jc) fl(nu) in column order: the YARDSTICK of what
    the kernel does (never the kernel). tests/test_impulse_dynamics.py compares the two.
  * row scales of the tests' bounds, d = sqrt(diag M):
        momentum row k:   d_k sum_j d_j (|nu_j| + |nu+_j|) + |iota_k| + (|Jc|^T |lam|)_k                              bound C_P 2^-24 scale
        contact row i:    sum_c |Jc_ic| (|nu_c| + |nu+_c|) + damping |lam_i| + |t_i| + e_i sum_c |Jc_ic| |nu_c|        bound C_V 2^-24 scale
        energy:           [(sum d_j |nu_j|)^2 + (sum d_j |nu+_j|)^2 + (sum_j |iota_j| / d_j)^2] / 2                   bound C_E 2^-24 scale
        map row i:        (sum_j d_j (|nu_j| + |nu+_j|)) / d_i   for |(P nu)_i - nu+_i| (iota = 0, vdes = 0)          bound C_M 2^-24 scale
        (Jc P)_ic:        (|Jc| (1 + |M^-1 Jc^T| |A^-1 Jc|))_ic   for e = 0, damping = 0, active rows                  bound C_J 2^-24 scale
    The map row's scale is the momentum row's first term divided by d_i^2: a velocity. The (Jc P) scale carries the terms of P = 1 -
    Y^T X through |Jc| and not |P| itself: P's entries are what is left of those terms after they cancel, and with |P| alone the
    yardstick's ratio is 459 over the family (the Delassus matrix' conditioning, up to 85 there), against 49.5 with this one. The
    iota term of the energy scale is the kinetic energy an impulse iota can add at most, in the same form as the two velocity terms.
    Every C is the smallest power of two >= 16 K_ref, not below 32; K_ref is the fp32 yardstick's largest ratio over the family of
    tests/test_impulse_dynamics.py, measured there on the CPU and asserted <= C / 16.
  * yardstick_f32: M_ref, Jc_ref rounded to fp32, mass_solve_reference.ldlt_solve_f32 for Y = (M^-1 [Jc^T | iota])^T, A = Jc Y^T +
    damping I from its lower triangle and a row-order Cholesky of it in numpy float32, lam, nu+ = nu + (Y_iota + Y^T lam), the energy
    sum_c g_c (nu_c + dnu_c / 2) with g = iota + Jc^T lam, and P = 1 - Y^T X with X the column solves of diag(1 + e) Jc.
"""
import numpy as np

import constrained_dynamics_reference as cdr
import mass_solve_reference as msr

NCOL, FINGERS, LIVE, EPS = msr.NCOL, msr.FINGERS, msr.LIVE, msr.EPS
# Measured by tests/test_impulse_dynamics.py::test_fp32_yardsticks_sit_well_inside_the_bounds (the table is in that module's docstring).
C_P = 32.0
C_V = 256.0
C_E = 32.0
C_M = 32.0
C_J = 1024.0
CONSTANTS = {"momentum": C_P, "contact": C_V, "energy": C_E, "map": C_M, "jp": C_J}


def constant_for(k_ref):
    """The project's rule: the smallest power of two >= 16 K_ref, not below 32."""
    return max(32.0, 2.0 ** np.ceil(np.log2(16.0 * k_ref)))


def _d(M):
    d = np.zeros(NCOL)
    d[LIVE] = np.sqrt(np.diag(M)[LIVE])
    return d


def _vec(x):
    return np.zeros(NCOL) if x is None else np.asarray(x, dtype=np.float64)


# ---- kinematics ---------------------------------------------------------------------------------------------------------------------
def contact_velocities(model, root_quat, q, nu, bodies, dtype=np.float64):
    """u [3K]: the world-frame velocity of the listed rigid bodies' origins. dtype = numpy.float32: the yardstick of the walk."""
    dt = dtype
    q, nu = np.asarray(q, dtype=dt), np.asarray(nu, dtype=dt)
    R, p = cdr._fk(model, np.zeros(3), root_quat, q, dt)
    nb = model.nb
    om, vel = np.zeros((nb, 3), dtype=dt), np.zeros((nb, 3), dtype=dt)
    om[0] = nu[3:6]
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        om[b] = om[par] + R[b][:, model.axis[b]] * nu[6 + d]
        vel[b] = vel[par] + cdr._cross(om[par], p[b] - p[par])
    out = np.zeros(3 * len(bodies), dtype=dt)
    for k, r in enumerate(bodies):
        b = model.rb_body[r]
        rc = R[b] @ np.asarray(model.rb_offset[r], dtype=dt)
        out[3 * k:3 * k + 3] = nu[0:3] + (vel[b] + cdr._cross(om[b], rc))
    return out.astype(np.float64)


def product_f32(Jc, nu):
    """u [m] as the sum over the live columns of fl(Jc) fl(nu) in numpy float32, every operation rounded."""
    f = np.float32
    J, v = Jc.astype(f), np.asarray(nu).astype(f)
    out = np.zeros(Jc.shape[0])
    for i in range(Jc.shape[0]):
        acc = f(0)
        for c in LIVE:
            acc = f(acc + f(J[i, c] * v[c]))
        out[i] = float(acc)
    return out


def velocity_magnitude(Jc, nu):
    """sum_c |Jc_ic| |nu_c|: what an fp32 evaluation of u = Jc nu errs in proportion to."""
    return np.abs(Jc) @ np.abs(np.asarray(nu, dtype=np.float64))


def contact_rows(model, root_pos, root_quat, q, nu, bodies, active=None):
    """(Jc [3K, 26], u [3K]): constrained_dynamics_reference.constraint_rows' Jacobian rows (zero where inactive) and Jc nu of the
    UNMASKED rows, fp64."""
    Jall, _, _ = cdr.constraint_rows(model, root_pos, root_quat, q, nu, bodies, None)
    on = np.repeat(np.ones(len(bodies), dtype=bool) if active is None else np.asarray(active, dtype=bool), 3)
    return Jall * on[:, None], Jall @ np.asarray(nu, dtype=np.float64)


# ---- the fp64 solve -----------------------------------------------------------------------------------------------------------------
def target(u, e, vdes):
    """t = vdes - e (u - vdes); e and vdes [m] (one entry per row), vdes None: zeros."""
    vdes = np.zeros_like(u) if vdes is None else np.asarray(vdes, dtype=np.float64)
    return vdes - np.asarray(e, dtype=np.float64) * (u - vdes)


def solve_with_mask(M, Jc, nu, t, iota, damping, on):
    """(nu+ [26], lam [m]) of the saddle-point system on the live coordinates and the rows where `on` holds; lam 0 elsewhere."""
    on = np.asarray(on, dtype=bool)
    nu, iota = np.asarray(nu, dtype=np.float64), _vec(iota)
    J = Jc[on][:, LIVE]
    m, nl = J.shape[0], len(LIVE)
    K = np.zeros((nl + m, nl + m))
    K[:nl, :nl] = M[np.ix_(LIVE, LIVE)]
    K[:nl, nl:] = -J.T
    K[nl:, :nl] = J
    K[nl:, nl:] = damping * np.eye(m)
    x = np.linalg.solve(K, np.r_[M[np.ix_(LIVE, LIVE)] @ nu[LIVE] + iota[LIVE], np.asarray(t, dtype=np.float64)[on]])
    nu_plus, lam = np.zeros(NCOL), np.zeros(len(on))
    nu_plus[LIVE], lam[on] = x[:nl], x[nl:]
    return nu_plus, lam


def impact_map(M, Jc, e, damping, on):
    """P [26, 26] = d nu+ / d nu: 1 - M^-1 Jc^T (A + damping)^-1 diag(1 + e) Jc on the live coordinates, fingers 0."""
    on = np.asarray(on, dtype=bool)
    P = np.zeros((NCOL, NCOL))
    J = Jc[on][:, LIVE]
    Pl = np.eye(len(LIVE))
    if on.any():
        MiJt = np.linalg.solve(M[np.ix_(LIVE, LIVE)], J.T)
        A = J @ MiJt + damping * np.eye(J.shape[0])
        Pl = Pl - MiJt @ np.linalg.solve(A, (1.0 + np.asarray(e, dtype=np.float64)[on])[:, None] * J)
    P[np.ix_(LIVE, LIVE)] = Pl
    return P


def kinetic_energy(M, nu):
    v = np.asarray(nu, dtype=np.float64)[LIVE]
    return 0.5 * float(v @ M[np.ix_(LIVE, LIVE)] @ v)


def delta_energy(M, nu, nu_plus):
    return kinetic_energy(M, nu_plus) - kinetic_energy(M, nu)


def energy_identity(lam, u, e, damping):
    """T(nu+) - T(nu) for iota = 0, vdes = 0 and the scalar restitution e."""
    return 0.5 * (1.0 - e) * float(lam @ u) - 0.5 * damping * float(lam @ lam)


# ---- residuals and scales -------------------------------------------------------------------------------------------------------------
def momentum_residual_and_scale(M, nu, nu_plus, iota, Jc, lam):
    """(|M (nu+ - nu) - iota - Jc^T lam| [26], scale [26]), fingers 0."""
    nu, nu_plus, iota = np.asarray(nu, dtype=np.float64), np.asarray(nu_plus, dtype=np.float64), _vec(iota)
    d = _d(M)
    res = np.abs(M @ (nu_plus - nu) - iota - Jc.T @ lam)
    scale = d * (d @ (np.abs(nu) + np.abs(nu_plus))) + np.abs(iota) + np.abs(Jc).T @ np.abs(lam)
    res[FINGERS], scale[FINGERS] = 0.0, 0.0
    return res, scale


def contact_residual_and_scale(Jc, nu, nu_plus, lam, t, e, damping):
    """(|Jc nu+ + damping lam - t| [m], scale [m]); Jc and t are zero on inactive rows by the caller."""
    nu, nu_plus = np.asarray(nu, dtype=np.float64), np.asarray(nu_plus, dtype=np.float64)
    res = np.abs(Jc @ nu_plus + damping * lam - t)
    aJ = np.abs(Jc)
    return res, aJ @ (np.abs(nu) + np.abs(nu_plus)) + damping * np.abs(lam) + np.abs(t) + np.asarray(e, dtype=np.float64) * (aJ @ np.abs(nu))


def energy_scale(M, nu, nu_plus, iota=None):
    d = _d(M)
    iota = _vec(iota)
    return 0.5 * (float(d @ np.abs(nu)) ** 2 + float(d @ np.abs(nu_plus)) ** 2 + float(np.abs(iota[LIVE]) @ (1.0 / d[LIVE])) ** 2)


def map_residual_and_scale(M, P, nu, nu_plus):
    """(|P nu - nu+| [26], scale [26]) for a call without iota and vel_des; the product in fp64; fingers 0."""
    nu, nu_plus = np.asarray(nu, dtype=np.float64), np.asarray(nu_plus, dtype=np.float64)
    d = _d(M)
    res = np.abs(P @ nu - nu_plus)
    scale = np.zeros(NCOL)
    scale[LIVE] = (d @ (np.abs(nu) + np.abs(nu_plus))) / d[LIVE]
    res[FINGERS] = 0.0
    return res, scale


def jp_residual_and_scale(M, Jc, P, on):
    """(|Jc P| [m, 26], scale [m, 26]) for e = 0, damping = 0: a plastic impact leaves no velocity along an active row. The scale sums
    the sizes of the terms that cancel, P's own included: |Jc| (1 + |M^-1 Jc^T| |A^-1 Jc|), fp64, inactive rows and fingers 0."""
    on = np.asarray(on, dtype=bool)
    scale = np.zeros((len(on), NCOL))
    if on.any():
        J = Jc[on][:, LIVE]
        MiJt = np.linalg.solve(M[np.ix_(LIVE, LIVE)], J.T)
        terms = np.eye(len(LIVE)) + np.abs(MiJt) @ np.abs(np.linalg.solve(J @ MiJt, J))
        scale[np.ix_(on, LIVE)] = np.abs(J) @ terms
    return np.abs(Jc @ P), scale


def delassus_condition(M, Jc, damping, on):
    """Condition number of the diagonally scaled Delassus matrix over the active rows (1 if none)."""
    return cdr.delassus_condition(M, Jc, damping, on)


# ---- the fp32 yardstick ---------------------------------------------------------------------------------------------------------------
def yardstick_f32(M, Jc, u, nu, e, vdes, iota, damping, on, want_map=True):
    """(nu+ [26], lam [m], denergy, P [26, 26] or None) of the chain in numpy float32 on fl(M), fl(Jc); u [m] is handed in (the walk's or
    the product's float32 values). Inactive rows: identity in A, lam 0."""
    f = np.float32
    on = np.asarray(on, dtype=bool)
    m = Jc.shape[0]
    J = Jc.astype(f)
    v = np.asarray(nu, dtype=np.float64).astype(f)
    io = _vec(iota).astype(f)
    e = np.asarray(e, dtype=np.float64).astype(f)
    vd = (np.zeros(m) if vdes is None else np.asarray(vdes, dtype=np.float64)).astype(f)
    u = np.asarray(u, dtype=np.float64).astype(f)
    Y = msr.ldlt_solve_f32(M, np.concatenate([J.astype(np.float64), io.astype(np.float64)[None]])).astype(f)      # [m + 1, 26]
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
            t = f(vd[i] - f(e[i] * f(u[i] - vd[i])))
            c[i] = f(f(t - u[i]) - acc)
    L = np.zeros((m, m), dtype=f)
    for i in range(m):
        for j in range(i + 1):
            acc = A[i, j]
            for k in range(j):
                acc = f(acc - f(L[i, k] * L[j, k]))
            L[i, j] = f(np.sqrt(acc)) if i == j else f(acc / L[j, j])

    def chol_solve(b):
        y = b.copy()
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
        return y

    lam = chol_solve(c)
    nu_plus = np.zeros(NCOL)
    den = f(0)
    for k in LIVE:
        dv, g = Y[m, k], io[k]
        for i in range(m):
            dv = f(dv + f(Y[i, k] * lam[i]))
            g = f(g + f(J[i, k] * lam[i]))
        nu_plus[k] = float(f(v[k] + dv))
        den = f(den + f(g * f(v[k] + f(f(0.5) * dv))))
    P = None
    if want_map:
        X = np.zeros((m, NCOL), dtype=f)
        for k in LIVE:
            X[:, k] = chol_solve(np.array([f(f(f(1) + e[i]) * J[i, k]) if on[i] else f(0) for i in range(m)], dtype=f))
        P = np.zeros((NCOL, NCOL))
        for i in LIVE:
            for j in LIVE:
                acc = f(0)
                for k in range(m):
                    acc = f(acc + f(Y[k, i] * X[k, j]))
                P[i, j] = float(f(f(i == j) - acc))
    return nu_plus, np.where(on, lam.astype(np.float64), 0.0), float(den), P
