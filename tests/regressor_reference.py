"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the body-parameter regressor of whole-body inverse dynamics that
csrc/wbc_arm_kernel.hip (wbc_sim_inverse_dynamics_regressor) computes; the definition is the one in include/wbc_sim.h:

    tau = sum_b Y[:, b, :] pi_b,    pi_b = (m, m c, Ibar xx yy zz xy xz yz),  Ibar = I_c + m (|c|^2 1 - c c^T) about the body ORIGIN,

and with `native` the columns d tau / d (m, c, I_c) at the body's own (m, c).

Written from the world-frame classical recursion of inverse_dynamics_reference.py, not from the kernel: every body's angular velocity,
angular acceleration and the classical acceleration of its own origin are propagated down the tree in WORLD axes, the wrench one unit
of each parameter contributes at the body origin is formed there (h -> R_b e_k, Ibar -> R_b S R_b^T), and projected with the origin's
Jacobian (the kernel: body axes, levers between two origins of one chain). Positions are carried relative to the root origin: the
root position is not an argument.

mag: next to every entry, the sum of the absolute values of the terms that make it up, carried through the same recursion (sums become
sums of absolute values, cross products their absolute counterparts): the scale an fp32 evaluation's rounding error is proportional to.

dtype=np.float32 runs the same chain in numpy float32: the yardstick an fp32 kernel is measured against."""
import numpy as np

NCOL, NP = 26, 10
GRAVITY = (0.0, 0.0, -9.81)
SYM = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]           # (xx yy zz xy xz yz)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=a.dtype)


def _acr(a, b):
    """|a x b| term by term for component-wise magnitudes a, b."""
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]], dtype=a.dtype)


def _quat_to_mat(q):             # xyzw
    x, y, z, w = q
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=q.dtype)


def _rot_axis(ax, angle):
    c, s = np.cos(angle), np.sin(angle)
    R = np.eye(3, dtype=angle.dtype)
    a1, a2 = (ax + 1) % 3, (ax + 2) % 3
    R[a1, a1], R[a1, a2], R[a2, a1], R[a2, a2] = c, -s, s, c
    return R


def world_magnitude(v):
    """The magnitude of a vector that is GIVEN in world axes (gravity, the root's nu and nudot): its Euclidean norm in every component.
    An evaluation is free to hold such a vector in the root's axes, where each component is a sum of three products bounded by the norm;
    the component-wise absolute value would make an entry's magnitude exactly 0 where the vector happens to lie along a world axis
    (untilted gravity against the root's z moment), which holds for the world-frame chain alone."""
    return np.full(3, np.sqrt((v * v).sum()), dtype=v.dtype)


def kinematics(model, root_quat, q, nu, nudot, dtype):
    """World rotation R, origin p RELATIVE to the root origin, angular velocity, angular acceleration and classical origin acceleration
    of every moving body, and the magnitudes (sums of the absolute values of their terms) of the last three."""
    f = lambda x: np.asarray(x, dtype=dtype)
    quat, q, nu, nudot = f(root_quat), f(q), f(nu), f(nudot)
    nb = model.nb
    R, p, pg = np.zeros((nb, 3, 3), dtype), np.zeros((nb, 3), dtype), np.zeros((nb, 3), dtype)
    om, al, acc = np.zeros((nb, 3), dtype), np.zeros((nb, 3), dtype), np.zeros((nb, 3), dtype)
    R[0] = _quat_to_mat(quat)
    om[0], al[0], acc[0] = nu[3:6], nudot[3:6], nudot[0:3]
    omg, alg, accg = np.abs(om), np.abs(al), np.abs(acc)
    for x, xg in ((om, omg), (al, alg), (acc, accg)):                # the root's vectors: world_magnitude()
        xg[0] = world_magnitude(x[0])
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        r, rg = R[par] @ f(model.joint_xyz[b]), np.abs(R[par]) @ np.abs(f(model.joint_xyz[b]))   # rg: the terms of each rotated component
        p[b], pg[b] = p[par] + r, pg[par] + rg
        R[b] = R[par] @ _rot_axis(model.axis[b], q[d])
        ax = R[b][:, model.axis[b]]
        om[b] = om[par] + ax * nu[6 + d]
        al[b] = al[par] + ax * nudot[6 + d] + _cross(om[par], ax * nu[6 + d])
        acc[b] = acc[par] + _cross(al[par], r) + _cross(om[par], _cross(om[par], r))
        omg[b] = omg[par] + np.abs(ax * nu[6 + d])
        alg[b] = alg[par] + np.abs(ax * nudot[6 + d]) + _acr(omg[par], np.abs(ax * nu[6 + d]))
        accg[b] = accg[par] + _acr(alg[par], rg) + _acr(omg[par], _acr(omg[par], rg))
    return R, p, om, al, acc, omg, alg, accg, pg


def origin_jacobian(model, R, p, pg, b):
    """(J, Jg): the [6, 26] Jacobian of body b's own origin (rows linear, angular; world axes) from positions relative to the root
    origin, and its magnitude: a lever is the sum of the link offsets between the two origins (pg: the running sum of their absolute
    values), a linear entry the two products of a cross product -- an axis parallel to its lever gives 0 with a magnitude that is not."""
    J, Jg = np.zeros((6, NCOL), R.dtype), np.zeros((6, NCOL), R.dtype)
    J[0:3, 0:3] = Jg[0:3, 0:3] = np.eye(3)
    J[3:6, 3:6] = Jg[3:6, 3:6] = np.eye(3)
    eye = np.eye(3, dtype=R.dtype)
    for j in range(3):
        J[0:3, 3 + j], Jg[0:3, 3 + j] = _cross(eye[j], p[b]), _acr(eye[j], pg[b])
    a = b
    while a > 0:
        axis = R[a][:, model.axis[a]]
        dof = model.body_dof[a]
        J[0:3, 6 + dof], Jg[0:3, 6 + dof] = _cross(axis, p[b] - p[a]), _acr(np.abs(axis), pg[b] - pg[a])
        J[3:6, 6 + dof] = axis
        Jg[3:6, 6 + dof] = np.abs(axis)
        a = model.parent[a]
    return J, Jg


def regressor(model, root_quat, q, nu, nudot=None, gravity=GRAVITY, dtype=np.float64):
    """(Y [26, nb, 10], mag [26, nb, 10]) in the linear parameters."""
    nudot = np.zeros(NCOL) if nudot is None else nudot
    R, p, om, al, acc, omg, alg, accg, pg = kinematics(model, root_quat, q, nu, nudot, dtype)
    g = np.asarray(gravity, dtype=dtype)
    nb = model.nb
    Y, mag = np.zeros((NCOL, nb, NP), dtype), np.zeros((NCOL, nb, NP), dtype)
    for b in range(nb):
        F, N = np.zeros((3, NP), dtype), np.zeros((3, NP), dtype)             # wrench at the body origin per unit parameter
        Fg, Ng = np.zeros((3, NP), dtype), np.zeros((3, NP), dtype)
        dd, ddg = acc[b] - g, accg[b] + world_magnitude(g)
        F[:, 0], Fg[:, 0] = dd, ddg                                             # m
        for k in range(3):                                                      # h = m c: one unit along body axis k
            r = R[b][:, k]
            F[:, 1 + k] = _cross(al[b], r) + _cross(om[b], _cross(om[b], r))
            N[:, 1 + k] = _cross(r, dd)
            Fg[:, 1 + k] = _acr(alg[b], np.abs(r)) + _acr(omg[b], _acr(omg[b], np.abs(r)))
            Ng[:, 1 + k] = _acr(np.abs(r), ddg)
        for k, (i, j) in enumerate(SYM):                                        # Ibar: one unit of the symmetric entry (i, j)
            S = np.zeros((3, 3), dtype)
            S[i, j] = S[j, i] = 1
            Iw = R[b] @ S @ R[b].T
            N[:, 4 + k] = Iw @ al[b] + _cross(om[b], Iw @ om[b])
            Iwg = np.abs(R[b]) @ S @ np.abs(R[b]).T
            Ng[:, 4 + k] = Iwg @ alg[b] + _acr(omg[b], Iwg @ omg[b])
        J, Jg = origin_jacobian(model, R, p, pg, b)
        Y[:, b] = J[0:3].T @ F + J[3:6].T @ N
        mag[:, b] = Jg[0:3].T @ Fg + Jg[3:6].T @ Ng
    return Y, mag


def theta_of(model, body_params=None):
    """theta [nb, 10] float64: (m, c, I_c xx yy zz xy xz yz) of every moving body, the root composite and the gripper body from
    body_params [20] where given (the parametrisation of WBC_T_BODY_PARAMS and of wbc_model)."""
    nb = model.nb
    th = np.concatenate([np.asarray(model.mass, dtype=np.float64).reshape(nb, 1), np.asarray(model.com, dtype=np.float64).reshape(nb, 3),
                         np.asarray(model.inertia, dtype=np.float64).reshape(nb, 6)], axis=1)
    if body_params is not None:
        bp = np.asarray(body_params, dtype=np.float64)
        th[0], th[model.gripper_piece["body"]] = bp[0:10], bp[10:20]
    return th


def _shift(c):
    """vec(|c|^2 1 - c c^T) [..., 6]."""
    cc = (c * c).sum(-1)
    return np.stack([cc - c[..., 0] ** 2, cc - c[..., 1] ** 2, cc - c[..., 2] ** 2,
                     -c[..., 0] * c[..., 1], -c[..., 0] * c[..., 2], -c[..., 1] * c[..., 2]], axis=-1)


def pi_from_theta(theta):
    """The linear parameters [..., 10] of theta [..., 10]."""
    theta = np.asarray(theta)
    m, c, I = theta[..., 0:1], theta[..., 1:4], theta[..., 4:10]
    return np.concatenate([m, m * c, I + m * _shift(c)], axis=-1)


def theta_from_pi(pi):
    """The inverse map (m != 0)."""
    pi = np.asarray(pi)
    m, c = pi[..., 0:1], pi[..., 1:4] / pi[..., 0:1]
    return np.concatenate([m, c, pi[..., 4:10] - m * _shift(c)], axis=-1)


def native(Y, mag, theta):
    """(d tau / d theta [26, nb, 10], its magnitude) from the linear-parameter regressor by the chain rule at theta [nb, 10]."""
    theta = np.asarray(theta, dtype=Y.dtype)
    out, outg = Y.copy(), mag.copy()
    for b in range(Y.shape[1]):
        m, c = theta[b, 0], theta[b, 1:4]
        P = _shift(c)
        out[:, b, 0] = Y[:, b, 0] + Y[:, b, 1:4] @ c + Y[:, b, 4:10] @ P
        outg[:, b, 0] = mag[:, b, 0] + mag[:, b, 1:4] @ np.abs(c) + mag[:, b, 4:10] @ np.abs(P)
        for k in range(3):
            D = np.zeros(6, Y.dtype)                                           # vec(2 c_k 1 - e_k c^T - c e_k^T)
            for n, (i, j) in enumerate(SYM):
                D[n] = (2 * c[k] if i == j else 0) - (c[j] if i == k else 0) - (c[i] if j == k else 0)
            out[:, b, 1 + k] = m * (Y[:, b, 1 + k] + Y[:, b, 4:10] @ D)
            outg[:, b, 1 + k] = abs(m) * (mag[:, b, 1 + k] + mag[:, b, 4:10] @ np.abs(D))
    return out, outg


def inverse_dynamics_yardstick(model, root_quat, q, nu, nudot, theta, gravity=GRAVITY, dtype=np.float32):
    """tau [26] of inverse_dynamics_reference's chain (centre-of-mass forces and torques, world axes) evaluated in `dtype` with positions
    relative to the root origin: the fp32 yardstick of wbc_sim_inverse_dynamics for the identification test."""
    nudot = np.zeros(NCOL) if nudot is None else nudot
    R, p, om, al, acc, _, _, _, pg = kinematics(model, root_quat, q, nu, nudot, dtype)
    g, theta = np.asarray(gravity, dtype=dtype), np.asarray(theta, dtype=dtype)
    tau = np.zeros(NCOL, dtype)
    for b in range(model.nb):
        m, com, I6 = theta[b, 0], theta[b, 1:4], theta[b, 4:10]
        rc = R[b] @ com
        a_com = acc[b] + _cross(al[b], rc) + _cross(om[b], _cross(om[b], rc))
        Ib = np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]], dtype=dtype)
        Iw = R[b] @ Ib @ R[b].T
        F = m * (a_com - g)
        T = Iw @ al[b] + _cross(om[b], Iw @ om[b])
        J, _ = origin_jacobian(model, R, p, pg, b)
        tau += J[0:3].T @ F + J[3:6].T @ (T + _cross(rc, F))
    return tau


def subtree_mask(model):
    """[26, nb] bool: row c can hold a non-zero entry for body b (b in the subtree coordinate c moves; the locked fingers move none)."""
    mask = np.zeros((NCOL, model.nb), bool)
    mask[0:6] = True
    for b in range(model.nb):
        a = b
        while a > 0:
            mask[6 + model.body_dof[a], b] = True
            a = model.parent[a]
    return mask
