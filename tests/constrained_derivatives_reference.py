"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) reference for wbc_sim_constrained_dynamics_derivatives (csrc/wbc_arm_kernel.hip; definitions
and the tangent convention in include/wbc_sim.h).

The solution (nudot, lambda) of constrained_dynamics_reference.solve_with_mask satisfies
    r1 = ID(q, nu, nudot) [+ armature nudot] - Jc^T lambda - tau = 0,    r2 = Jc nudot + gamma - a_des + damping lambda = 0,
so its partial derivatives solve the same saddle-point matrix against -dr1/dx, -dr2/dx:
    dr1/dq = dtau_ID/dq - d(Jc^T lambda)/dq,  dr1/dnu = dtau_ID/dnu,  dr1/dtau = -1,  dr2/dq, dr2/dnu = below,  dr2/dtau = 0.
  * dtau_ID comes from dynamics_derivatives_reference.inverse_dynamics_derivatives at the solution's nudot.
  * constraint_partials: the analytic DIRECTIONAL DERIVATIVE, in forward mode along all 52 directions at once, of the world-frame classical
    recursion of constrained_dynamics_reference.body_accelerations carried to the listed origins (dr2), and of
    whole_body_reference.jacobian's linear rows against a fixed lambda (d(Jc^T lambda)/dq). The kernel walks in the root's axes, one
    (body, direction) pair per lane, and takes d(Jc^T lambda) in closed form from triple products, so agreement means something.
    mag of dr2 [m, 52] is the sum of the sizes of the terms the recursion adds (Euclidean norms; the three rows of a body share one figure,
    as in body_accelerations): per joint |d alpha_par| |r| + |alpha_par| |dr| + 2 |d omega_par| |omega_par| |r| + |omega_par|^2 |dr|, and
    the same at the body's offset. mag of d(Jc^T lambda) [26, 52] is sum_k (|d a x l| + |a x d l|)^T |lambda_k|, component-wise, with
    a, l the column's axis and lever. dtype = numpy.float32 is the rounding YARDSTICK (root at the origin, every array operation
    rounded), never the kernel.
  * constrained_dynamics_derivatives: the assembly by a dense fp64 solve of the KKT matrix on the live coordinates and active rows.
  * yardstick_f32: the kernel's chain in numpy float32: the fp32 recursions for the residual partials, mass_solve_reference.ldlt_solve_f32
    for X = -M^-1 dr1 and Y, a row-order fp32 Cholesky of A + damping I, the column solves, dnudot = X + Y dlambda.
  * column_bounds: the residual-form bounds of tests/test_constrained_dynamics_derivatives.py for one env.
"""
import numpy as np

import arm_osc_oracle as ao
import constrained_dynamics_reference as cdr
import dynamics_derivatives_reference as ddr
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import whole_body_reference as wb

NCOL, EPS, K = ddr.NCOL, ddr.EPS, ddr.K
FINGERS, LIVE = msr.FINGERS, msr.LIVE
C_S, C_K, C_D = 128.0, 32.0, {"dq": 32768.0, "dnu": 524288.0}
assert C_S == msr.C_S == cdr.C_S and C_K == cdr.C_K and C_D == ddr.C
# Measured by tests/test_constrained_dynamics_derivatives.py::test_fp32_yardsticks_sit_well_inside_the_bounds (the table is in that
# module's docstring): the smallest power of two >= 16 K_ref.
C_J = 16384.0
C_R = 128.0
GROUPS = ("q", "nu", "tau")
_cx = ddr._cx


def constraint_partials(model, root_pos, root_quat, q, nu, nudot, lam, bodies, on, dtype=np.float64):
    """(dr2 [m, 52], mag_r2 [m, 52], dJl [26, 52], mag_J [26, 52]): columns 0:26 the directions of q, 26:52 those of nu; the rows of an
    inactive body (and its lambda) are zero. dJl = d(Jc^T lambda) along the direction with lambda held."""
    dt = dtype
    q, nu, nudot = (np.asarray(x, dtype=dt) for x in (q, nu, nudot))
    on = np.asarray(on, dtype=bool)
    lam = np.where(on, np.asarray(lam, dtype=np.float64), 0.0).astype(dt)
    R, p = cdr._fk(model, root_pos if dt == np.float64 else np.zeros(3), root_quat, q, dt)
    nb = model.nb
    eye = np.eye(3, dtype=dt)
    seed = np.eye(K, dtype=dt)
    sq, sv = seed[0:NCOL], seed[NCOL:K]
    dR, dp = np.zeros((nb, K, 3, 3), dtype=dt), np.zeros((nb, K, 3), dtype=dt)
    for j in range(3):
        dp[0] += sq[j][:, None] * eye[j]
        dR[0] += sq[3 + j][:, None, None] * (ddr._skew(eye[j]).astype(dt) @ R[0])
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        rot = ao.rot_axis(model.axis[b], dt(q[d])).astype(dt)
        drot = (rot @ ddr._skew(np.eye(3)[model.axis[b]])).astype(dt)
        dp[b] = dp[par] + dR[par] @ np.asarray(model.joint_xyz[b], dtype=dt)
        dR[b] = dR[par] @ rot + sq[6 + d][:, None, None] * (R[par] @ drot)
    om, al, acc = (np.zeros((nb, 3), dtype=dt) for _ in range(3))
    dom, dal, dacc = (np.zeros((nb, K, 3), dtype=dt) for _ in range(3))
    mg = np.zeros((nb, K))
    nrm = lambda v: np.linalg.norm(np.asarray(v, dtype=np.float64), axis=-1)
    om[0], al[0], acc[0] = nu[3:6], nudot[3:6], nudot[0:3]
    for j in range(3):
        dom[0] += sv[3 + j][:, None] * eye[j]

    def carried(a, da, w, dw, r, dr):
        """alpha x r + omega x (omega x r), its tangent and the sizes of the tangent's terms."""
        wr, dwr = _cx(w, r), _cx(dw, r) + _cx(w, dr)
        val = _cx(a, r) + _cx(w, wr)
        dval = _cx(da, r) + _cx(a, dr) + _cx(dw, wr) + _cx(w, dwr)
        size = nrm(da) * nrm(r) + nrm(a) * nrm(dr) + 2 * nrm(dw) * nrm(w) * nrm(r) + nrm(w) ** 2 * nrm(dr)
        return val, dval, size
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        ax, dax = R[b][:, model.axis[b]], dR[b][:, :, model.axis[b]]
        r, dr = p[b] - p[par], dp[b] - dp[par]
        jv, djv = ax * nu[6 + d], dax * nu[6 + d] + sv[6 + d][:, None] * ax
        om[b], dom[b] = om[par] + jv, dom[par] + djv
        al[b] = al[par] + ax * nudot[6 + d] + _cx(om[par], jv)
        dal[b] = dal[par] + dax * nudot[6 + d] + _cx(dom[par], jv) + _cx(om[par], djv)
        val, dval, size = carried(al[par], dal[par], om[par], dom[par], r, dr)
        acc[b], dacc[b], mg[b] = acc[par] + val, dacc[par] + dval, mg[par] + size
    m = 3 * len(bodies)
    dr2, mag2 = np.zeros((m, K), dtype=dt), np.zeros((m, K))
    dJl, magJ = np.zeros((NCOL, K), dtype=dt), np.zeros((NCOL, K))
    a64 = lambda x: np.abs(np.asarray(x, dtype=np.float64))
    for k, rb in enumerate(bodies):
        if not on[3 * k]:
            continue
        b = model.rb_body[rb]
        off = np.asarray(model.rb_offset[rb], dtype=dt)
        rc, drc = R[b] @ off, dR[b] @ off
        _, dval, size = carried(al[b], dal[b], om[b], dom[b], rc, drc)
        dr2[3 * k:3 * k + 3] = (dacc[b] + dval).T
        mag2[3 * k:3 * k + 3] = mg[b] + size
        lk = lam[3 * k:3 * k + 3]
        pt, dpt = p[b] + rc, dp[b] + drc
        lever, dlever = pt - p[0], dpt - dp[0]
        for j in range(3):
            t = _cx(eye[j], dlever)                              # [K, 3]: the root's angular columns, e_j fixed in the world
            dJl[3 + j] += t @ lk
            magJ[3 + j] += a64(t) @ a64(lk)
        a = b
        while a > 0:
            ax, dax = R[a][:, model.axis[a]], dR[a][:, :, model.axis[a]]
            lever, dlever = pt - p[a], dpt - dp[a]
            t1, t2 = _cx(dax, lever), _cx(ax, dlever)
            col = 6 + model.body_dof[a]
            dJl[col] += (t1 + t2) @ lk
            magJ[col] += (a64(t1) + a64(t2)) @ a64(lk)
            a = model.parent[a]
    return dr2.astype(np.float64), mag2, dJl.astype(np.float64), magJ


def residual_partials(model, state, bodies, on, nudot, lam, gravity=idr.GRAVITY, dtype=np.float64):
    """The partials of (r1, r2) at (nudot, lam): {"r1": {g: [26, 26]}, "r2": {g: [m, 26]}, "mag_D", "mag_J", "mag_R": {g: ...}} with
    [i, j] = d r_i / d x_j, g in GROUPS; the fingers' rows and columns of r1 are zero (tau's entry there is ignored)."""
    pos, quat, q, nu, bp = state
    Dq, Dnu, mq, mn = ddr.inverse_dynamics_derivatives(model, pos, quat, q, nu, nudot, bp, gravity, dtype=dtype)
    dr2, mag2, dJl, magJ = constraint_partials(model, pos, quat, q, nu, nudot, lam, bodies, on, dtype=dtype)
    m = len(on)
    eye = np.eye(NCOL)
    eye[FINGERS, FINGERS] = 0.0
    z26, zm = np.zeros((NCOL, NCOL)), np.zeros((m, NCOL))
    return {"r1": {"q": Dq - dJl[:, :NCOL], "nu": Dnu, "tau": -eye}, "r2": {"q": dr2[:, :NCOL], "nu": dr2[:, NCOL:], "tau": zm},
            "mag_D": {"q": mq, "nu": mn, "tau": z26}, "mag_J": {"q": magJ[:, :NCOL], "nu": z26, "tau": z26},
            "mag_R": {"q": mag2[:, :NCOL], "nu": mag2[:, NCOL:], "tau": zm}, "dJl": dJl[:, :NCOL], "dr2": dr2}


def system(model, state, bodies, on, armature=None, gravity=idr.GRAVITY):
    """(M, h, Jc, gamma): the fp64 system of constrained_dynamics_reference; inactive rows zero."""
    pos, quat, q, nu, bp = state
    M = msr.mass_matrix(model, pos, quat, q, bp, armature)
    h, _ = idr.bias_forces(model, pos, quat, q, nu, bp, gravity)
    Jc, gamma, _ = cdr.constraint_rows(model, pos, quat, q, nu, bodies, np.asarray(on, dtype=bool)[::3])
    return M, h, Jc, gamma


def kkt_columns(M, Jc, damping, on, dr1, dr2):
    """(D [26, 26], Lam [m, 26]): the saddle-point matrix against -dr1, -dr2 column by column; fingers and inactive rows zero."""
    on = np.asarray(on, dtype=bool)
    mo, nl = int(on.sum()), len(LIVE)
    Kk = np.zeros((nl + mo, nl + mo))
    Kk[:nl, :nl] = M[np.ix_(LIVE, LIVE)]
    Kk[:nl, nl:] = -Jc[on][:, LIVE].T
    Kk[nl:, :nl] = Jc[on][:, LIVE]
    Kk[nl:, nl:] = damping * np.eye(mo)
    x = np.linalg.solve(Kk, -np.concatenate([dr1[LIVE], dr2[on]]))
    D, Lam = np.zeros((NCOL, NCOL)), np.zeros((len(on), NCOL))
    D[LIVE] = x[:nl]
    Lam[on] = x[nl:]
    return D, Lam


def constrained_dynamics_derivatives(model, state, bodies, on, tau, a_des, damping=0.0, armature=None, gravity=idr.GRAVITY):
    """{"nudot", "lambda", "dnudot": {g: [26, 26]}, "dlambda": {g: [m, 26]}, "parts": residual_partials, "M", "Jc"} in fp64."""
    M, h, Jc, gamma = system(model, state, bodies, on, armature, gravity)
    nudot, lam = cdr.solve_with_mask(M, h, tau, Jc, gamma, a_des, damping, on)
    parts = residual_partials(model, state, bodies, on, nudot, lam, gravity)
    out = {"nudot": nudot, "lambda": lam, "dnudot": {}, "dlambda": {}, "parts": parts, "M": M, "Jc": Jc}
    for g in GROUPS:
        out["dnudot"][g], out["dlambda"][g] = kkt_columns(M, Jc, damping, on, parts["r1"][g], parts["r2"][g])
    return out


def yardstick_f32(model, state, bodies, on, nudot, lam, M, Jc, damping, gravity=idr.GRAVITY):
    """({g: D [26, 26]}, {g: Lam [m, 26]}) of the kernel's chain in numpy float32 at the given (nudot, lam)."""
    f = np.float32
    on = np.asarray(on, dtype=bool)
    m = len(on)
    parts = residual_partials(model, state, bodies, on, nudot, lam, gravity, dtype=f)
    J = Jc.astype(f)
    Y = msr.ldlt_solve_f32(M, J.astype(np.float64)).astype(f) if m else np.zeros((0, NCOL), dtype=f)
    A = np.zeros((m, m), dtype=f)
    for i in range(m):
        for j in range(i + 1):
            acc = f(0)
            for k in LIVE:
                acc = f(acc + f(J[i, k] * Y[j, k]))
            A[i, j] = (f(acc + f(damping)) if i == j else acc) if on[i] and on[j] else f(i == j)
    L = np.zeros((m, m), dtype=f)
    for i in range(m):
        for j in range(i + 1):
            acc = A[i, j]
            for k in range(j):
                acc = f(acc - f(L[i, k] * L[j, k]))
            L[i, j] = f(np.sqrt(acc)) if i == j else f(acc / L[j, j])
    Ds, Ls = {}, {}
    for g in GROUPS:
        X = msr.ldlt_solve_f32(M, (-parts["r1"][g]).astype(f).astype(np.float64).T).astype(f)          # [direction, 26]
        r2 = parts["r2"][g].astype(f)
        D, Lam = np.zeros((NCOL, NCOL)), np.zeros((m, NCOL))
        for x in range(NCOL):
            z = np.zeros(m, dtype=f)
            for i in range(m):
                if on[i]:
                    acc = Y[i, x] if g == "tau" else r2[i, x]
                    if g != "tau":
                        for c in LIVE:
                            acc = f(acc + f(J[i, c] * X[x, c]))
                    z[i] = acc
            for i in range(m):
                acc = z[i]
                for k in range(i):
                    acc = f(acc - f(L[i, k] * z[k]))
                z[i] = f(acc / L[i, i])
            for i in range(m - 1, -1, -1):
                acc = z[i]
                for k in range(i + 1, m):
                    acc = f(acc - f(L[k, i] * z[k]))
                z[i] = f(acc / L[i, i])
            z = -z
            for c in LIVE:
                acc = X[x, c]
                for i in range(m):
                    acc = f(acc + f(Y[i, c] * z[i]))
                D[c, x] = float(acc)
            Lam[:, x] = np.where(on, z.astype(np.float64), 0.0)
        Ds[g], Ls[g] = D, Lam
    return Ds, Ls


def column_bounds(M, Jc, damping, on, parts, g, D, Lam):
    """The two residuals of group g's columns and their allowances, each [rows, 26] with column j the direction j:
    (res_dyn [26, 26], allow_dyn, res_con [m, 26], allow_con). parts: residual_partials at the (nudot, lambda) the columns belong to."""
    on = np.asarray(on, dtype=bool)
    m = len(on)
    res_d, all_d = np.zeros((NCOL, NCOL)), np.zeros((NCOL, NCOL))
    res_c, all_c = np.zeros((m, NCOL)), np.zeros((m, NCOL))
    z26, zero = np.zeros(NCOL), np.zeros(m)
    for j in range(NCOL):
        # M D + dr1 - Jc^T Lam: dynamics_residual_and_scale with h = 0 and tau = -dr1's column (the right-hand side, whose size it counts)
        r, s = cdr.dynamics_residual_and_scale(M, z26, -parts["r1"][g][:, j], Jc, D[:, j], Lam[:, j])
        res_d[:, j], all_d[:, j] = r, C_S * EPS * s
        # Jc D + dr2 + damping Lam: constraint_residual_and_scale with gamma = 0 and a_des = -dr2's column
        r, s = cdr.constraint_residual_and_scale(M, Jc, zero, -parts["r2"][g][:, j], damping, D[:, j], Lam[:, j])
        res_c[:, j], all_c[:, j] = np.where(on, r, 0.0), np.where(on, C_K * EPS * s, 0.0)
    all_d += (C_D["dnu" if g == "nu" else "dq"] * EPS * parts["mag_D"][g] + C_J * EPS * parts["mag_J"][g])
    all_c += C_R * EPS * parts["mag_R"][g]
    return res_d, all_d, res_c, all_c
