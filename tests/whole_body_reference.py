"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) restatement of the whole-body Jacobian [27, 6, 26] and mass matrix [26, 26]
that csrc/wbc_arm_kernel.hip (wbc_sim_body_dynamics) computes; the definition is the one in include/wbc_sim.h:
coordinates nu = (v_root, omega_root, qd[0..19]), world frame, rigid-body ORIGINS, locked fingers (DoFs 18, 19) zero.

Built with different algebra than the kernel so that agreement means something:
  * everything in world coordinates straight from the forward kinematics of oracle/arm_osc_oracle.py (the kernel: levers in the
    base frame, rotated at the end);
  * M = sum over moving bodies of  m Jv^T Jv + Jw^T (R I R^T) Jw  with centre-of-mass Jacobians (the kernel: composite spatial
    inertias about the base origin, M_ij = S_i^T Ic S_j);
  * body velocities for the kinetic-energy check by recursion over the tree (no Jacobian at all).
"""
import numpy as np

import arm_osc_oracle as ao

NCOL = 26


def _sym(I6):
    return np.array([[I6[0], I6[3], I6[4]], [I6[3], I6[1], I6[5]], [I6[4], I6[5], I6[2]]])


def body_inertias(model, body_params=None):
    """(mass, com [3], I6 [6]) of every moving body; body_params (the [20] row of WBC_T_BODY_PARAMS) replaces the root
    composite and the gripper body, as the step kernel integrates with them."""
    out = [(float(model.mass[b]), np.asarray(model.com[b], dtype=np.float64), np.asarray(model.inertia[b], dtype=np.float64))
           for b in range(model.nb)]
    if body_params is not None:
        bp = np.asarray(body_params, dtype=np.float64)
        out[0] = (bp[0], bp[1:4], bp[4:10])
        out[model.gripper_piece["body"]] = (bp[10], bp[11:14], bp[14:20])
    return out


def ancestors(model, b):
    """Moving bodies on the path root..b, b included."""
    path = [b]
    while b > 0:
        b = model.parent[b]
        path.append(b)
    return set(path)


def dof_body(model):
    """Moving body driven by each DoF, -1 for the DoFs no joint drives (the locked fingers)."""
    out = [-1] * len(model.dof_names)
    for b in range(1, model.nb):
        out[model.body_dof[b]] = b
    return out


def cross3(a, b):
    """a x b of two 3-vectors (np.cross spends most of its time on axis bookkeeping; the references call this a few hundred times
    per state)."""
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def point_jacobian(model, R, p, body, point):
    """[6, 26] Jacobian (linear velocity of the world point `point` riding on moving body `body`; the body's angular velocity)."""
    J = np.zeros((6, NCOL))
    J[0:3, 0:3] = np.eye(3)
    d = point - p[0]
    J[0:3, 3:6] = [[0.0, d[2], -d[1]], [-d[2], 0.0, d[0]], [d[1], -d[0], 0.0]]        # column j: e_j x d
    J[3:6, 3:6] = np.eye(3)
    b = body
    while b > 0:                                                                       # the joints on the path root..body
        a = R[b][:, model.axis[b]]
        dof = model.body_dof[b]
        J[0:3, 6 + dof] = cross3(a, point - p[b])
        J[3:6, 6 + dof] = a
        b = model.parent[b]
    return J


def rigid_body_poses(model, root_pos, root_quat, q):
    """World origin [27, 3] and rotation [27, 3, 3] of every rigid body."""
    R, p = ao.fk(model, root_pos, root_quat, np.asarray(q, dtype=np.float64))
    pos = np.array([p[b] + R[b] @ model.rb_offset[r] for r, b in enumerate(model.rb_body)])
    rot = np.array([R[b] for b in model.rb_body])
    return pos, rot


def jacobian(model, root_pos, root_quat, q):
    """[27, 6, 26]."""
    R, p = ao.fk(model, root_pos, root_quat, np.asarray(q, dtype=np.float64))
    return np.array([point_jacobian(model, R, p, b, p[b] + R[b] @ model.rb_offset[r]) for r, b in enumerate(model.rb_body)])


def mass_matrix(model, root_pos, root_quat, q, body_params=None):
    """[26, 26] from centre-of-mass Jacobians."""
    R, p = ao.fk(model, root_pos, root_quat, np.asarray(q, dtype=np.float64))
    M = np.zeros((NCOL, NCOL))
    for b, (m, com, I6) in enumerate(body_inertias(model, body_params)):
        J = point_jacobian(model, R, p, b, p[b] + R[b] @ com)
        Iw = R[b] @ _sym(I6) @ R[b].T
        M += m * J[0:3].T @ J[0:3] + J[3:6].T @ Iw @ J[3:6]
    return M


def kinetic_energy(model, root_pos, root_quat, q, v_root, w_root, qd, body_params=None):
    """sum over moving bodies of 1/2 (m |v_com|^2 + w^T I_world w), body velocities propagated down the tree."""
    R, p = ao.fk(model, root_pos, root_quat, np.asarray(q, dtype=np.float64))
    w = np.zeros((model.nb, 3)); v = np.zeros((model.nb, 3))          # angular velocity, velocity of the body origin
    w[0], v[0] = w_root, v_root
    for b in range(1, model.nb):
        par = model.parent[b]
        w[b] = w[par] + R[b][:, model.axis[b]] * qd[model.body_dof[b]]
        v[b] = v[par] + np.cross(w[par], p[b] - p[par])
    ke = 0.0
    for b, (m, com, I6) in enumerate(body_inertias(model, body_params)):
        vc = v[b] + np.cross(w[b], R[b] @ com)
        ke += 0.5 * (m * vc @ vc + w[b] @ (R[b] @ _sym(I6) @ R[b].T) @ w[b])
    return ke
