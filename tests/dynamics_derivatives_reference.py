"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) reference for wbc_sim_inverse_dynamics_derivatives and
wbc_sim_forward_dynamics_derivatives (csrc/wbc_arm_kernel.hip; definitions and the tangent convention in include/wbc_sim.h).

The analytic DIRECTIONAL DERIVATIVE of the world-frame classical recursion of inverse_dynamics_reference.inverse_dynamics, line by
line in forward mode: every quantity of that recursion (the frames R_b, p_b of the forward kinematics, omega, alpha, the acceleration
of the origin, then of the centre of mass, the world inertia, F, T, the centre-of-mass Jacobian J) is carried with its derivative along
all 52 directions at once -- 26 of the configuration tangent dq (root translation, WORLD rotation vector, joint increments; the world
components of nu and nudot held fixed) and 26 of nu -- and
    d tau = sum over bodies of  dJ_v^T F + J_v^T dF + dJ_w^T T + J_w^T dT.
The kernel instead carries the tangent of a root-frame SPATIAL recursion about the base origin, one (body, direction) pair per lane,
takes dS_c in closed form and never reads v_root or the root position, so agreement means something.

mag is the same sum with every factor replaced by its component-wise absolute value,
    mag = sum |J_v|^T |dF| + |J_w|^T |dT| + |dJ_v|^T |F| + |dJ_w|^T |T|,
the derivative of the sum that defines inverse_dynamics_reference's mag: the scale an fp32 evaluation's error is proportional to.
dtype = numpy.float32 is the rounding YARDSTICK (the same recursion in numpy float32 with the root at the origin, every array operation
rounded), never the kernel.

Exact structure of the reference (asserted by the tests), in value and in magnitude: the columns of v_root are exactly 0 (nu[0:3] is
never read), the translation columns too (every d p_b is the same unit vector, so each lever's tangent is an exact 0), and so are the
rows and columns of the locked fingers and the joint-row x joint-column entries across chains (no body carries both tangents).

Forward dynamics: nudot = M^-1 (tau - h), d nudot = -M^-1 (d tau at that nudot), d nudot / d tau = M^-1, with M of
whole_body_reference.mass_matrix (+ the armature on the joint diagonal) and dense fp64 solves on the 24 live coordinates.
"""
import numpy as np

import arm_osc_oracle as ao
import constrained_dynamics_reference as cdr
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import whole_body_reference as wb

NCOL, EPS = wb.NCOL, 2.0 ** -24
FINGERS, LIVE = msr.FINGERS, msr.LIVE
K = 2 * NCOL                       # directions carried at once: dq 0..25, dnu 26..51
# Measured by tests/test_dynamics_derivatives.py::test_fp32_yardsticks_sit_well_inside_the_bounds (the table is in that module's
# docstring): the smallest power of two >= 16 K_ref per output.
C = {"dq": 32768.0, "dnu": 524288.0}


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _cx(a, b):
    """a x b along the last axis, broadcasting, in the operands' dtype."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def inverse_dynamics_derivatives(model, root_pos, root_quat, q, nu, nudot=None, body_params=None, gravity=idr.GRAVITY,
                                 dtype=np.float64):
    """(D_q, D_nu, mag_q, mag_nu), each [26, 26] with [i, j] = d tau_i / d x_j."""
    dt = dtype
    q, nu = np.asarray(q, dtype=dt), np.asarray(nu, dtype=dt)
    nudot = np.zeros(NCOL, dtype=dt) if nudot is None else np.asarray(nudot, dtype=dt)
    g = np.asarray(gravity, dtype=dt)
    R, p = cdr._fk(model, root_pos if dt == np.float64 else np.zeros(3), root_quat, q, dt)
    nb = model.nb
    eye = np.eye(3, dtype=dt)
    seed = np.eye(K, dtype=dt)                                  # seed[x]: the direction vector of coordinate x
    sq, sv = seed[0:NCOL], seed[NCOL:K]                         # sq[c] [K]: d(configuration coordinate c), sv[c]: d(nu_c)
    # ---- forward kinematics and its tangent: p_b = p_par + R_par xyz_b, R_b = R_par Rot(axis_b, q_b)
    dR, dp = np.zeros((nb, K, 3, 3), dtype=dt), np.zeros((nb, K, 3), dtype=dt)
    for j in range(3):
        dp[0] += sq[j][:, None] * eye[j]                                                  # translation of the root origin
        dR[0] += sq[3 + j][:, None, None] * (_skew(eye[j]).astype(dt) @ R[0])              # R <- exp([dtheta]x) R
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        rot = ao.rot_axis(model.axis[b], dt(q[d])).astype(dt)
        drot = (rot @ _skew(np.eye(3)[model.axis[b]])).astype(dt)
        dp[b] = dp[par] + dR[par] @ np.asarray(model.joint_xyz[b], dtype=dt)
        dR[b] = dR[par] @ rot + sq[6 + d][:, None, None] * (R[par] @ drot)
    # ---- classical kinematics down the tree (inverse_dynamics_reference), each line with its tangent [K, 3]
    om, al, acc = (np.zeros((nb, 3), dtype=dt) for _ in range(3))
    dom, dal, dacc = (np.zeros((nb, K, 3), dtype=dt) for _ in range(3))
    om[0], al[0], acc[0] = nu[3:6], nudot[3:6], nudot[0:3]
    for j in range(3):
        dom[0] += sv[3 + j][:, None] * eye[j]                   # nudot is a parameter: no tangent; nu[0:3] is never read
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        ax, dax = R[b][:, model.axis[b]], dR[b][:, :, model.axis[b]]
        r, dr = p[b] - p[par], dp[b] - dp[par]
        jv, djv = ax * nu[6 + d], dax * nu[6 + d] + sv[6 + d][:, None] * ax
        om[b], dom[b] = om[par] + jv, dom[par] + djv
        al[b] = al[par] + ax * nudot[6 + d] + _cx(om[par], jv)
        dal[b] = dal[par] + dax * nudot[6 + d] + _cx(dom[par], jv) + _cx(om[par], djv)
        wr, dwr = _cx(om[par], r), _cx(dom[par], r) + _cx(om[par], dr)
        acc[b] = acc[par] + _cx(al[par], r) + _cx(om[par], wr)
        dacc[b] = dacc[par] + _cx(dal[par], r) + _cx(al[par], dr) + _cx(dom[par], wr) + _cx(om[par], dwr)
    # ---- forces, Jacobians, projection
    D, mag = np.zeros((NCOL, K), dtype=dt), np.zeros((NCOL, K))
    a64 = lambda x: np.abs(np.asarray(x, dtype=np.float64))
    for b, (m, com, I6) in enumerate(wb.body_inertias(model, body_params)):
        m, com, Ib = dt(m), np.asarray(com, dtype=dt), wb._sym(I6).astype(dt)
        rc, drc = R[b] @ com, dR[b] @ com
        wrc, dwrc = _cx(om[b], rc), _cx(dom[b], rc) + _cx(om[b], drc)
        a_com = acc[b] + _cx(al[b], rc) + _cx(om[b], wrc)
        da_com = dacc[b] + _cx(dal[b], rc) + _cx(al[b], drc) + _cx(dom[b], wrc) + _cx(om[b], dwrc)
        Iw = R[b] @ Ib @ R[b].T
        dIw = dR[b] @ Ib @ R[b].T + R[b] @ Ib @ dR[b].transpose(0, 2, 1)
        F, dF = m * (a_com - g), m * da_com
        Iom, dIom = Iw @ om[b], dIw @ om[b] + dom[b] @ Iw.T
        T = Iw @ al[b] + _cx(om[b], Iom)
        dT = dIw @ al[b] + dal[b] @ Iw.T + _cx(dom[b], Iom) + _cx(om[b], dIom)
        # J of whole_body_reference.point_jacobian at the centre of mass, and its tangent
        Jv, Jw = np.zeros((3, NCOL), dtype=dt), np.zeros((3, NCOL), dtype=dt)
        dJv, dJw = np.zeros((K, 3, NCOL), dtype=dt), np.zeros((K, 3, NCOL), dtype=dt)
        pt, dpt = p[b] + rc, dp[b] + drc
        Jv[:, 0:3] = eye
        Jw[:, 3:6] = eye
        lever, dlever = pt - p[0], dpt - dp[0]
        for j in range(3):
            Jv[:, 3 + j], dJv[:, :, 3 + j] = _cx(eye[j], lever), _cx(eye[j], dlever)
        a = b
        while a > 0:
            ax, dax = R[a][:, model.axis[a]], dR[a][:, :, model.axis[a]]
            col = 6 + model.body_dof[a]
            lever, dlever = pt - p[a], dpt - dp[a]
            Jv[:, col], dJv[:, :, col] = _cx(ax, lever), _cx(dax, lever) + _cx(ax, dlever)
            Jw[:, col], dJw[:, :, col] = ax, dax
            a = model.parent[a]
        D += (Jv.T @ dF.T + Jw.T @ dT.T + (dJv.transpose(0, 2, 1) @ F).T + (dJw.transpose(0, 2, 1) @ T).T).astype(dt)
        mag += a64(Jv).T @ a64(dF).T + a64(Jw).T @ a64(dT).T + (a64(dJv).transpose(0, 2, 1) @ a64(F)).T + (a64(dJw).transpose(0, 2, 1) @ a64(T)).T
    D = D.astype(np.float64)
    return D[:, 0:NCOL], D[:, NCOL:K], mag[:, 0:NCOL], mag[:, NCOL:K]


def forward_dynamics_derivatives(model, root_pos, root_quat, q, nu, tau=None, body_params=None, gravity=idr.GRAVITY, armature=None):
    """(nudot, X_q, X_nu, Minv, M, (D_q, D_nu, mag_q, mag_nu)): nudot = M^-1 (tau - h), X = -M^-1 D at that nudot, fingers exactly 0."""
    nudot, M, _h, _mag = msr.forward_dynamics(model, root_pos, root_quat, q, nu, tau, body_params, gravity, armature)
    parts = inverse_dynamics_derivatives(model, root_pos, root_quat, q, nu, nudot, body_params, gravity)
    Xq, Xn = -msr.solve(M, parts[0].T).T, -msr.solve(M, parts[1].T).T
    Minv = msr.solve(M, np.eye(NCOL))
    Minv[FINGERS] = 0.0
    return nudot, Xq, Xn, Minv, M, parts


def largest_ratio(got, ref, mag):
    """Largest |got - ref| / (2^-24 mag); where the magnitude is 0 both must be exactly 0."""
    got, ref, mag = (np.asarray(x, dtype=np.float64) for x in (got, ref, mag))
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    return float((np.abs(got - ref)[~zero] / (EPS * mag[~zero])).max())
