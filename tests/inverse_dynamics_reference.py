"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) restatement of the whole-body inverse dynamics that csrc/wbc_arm_kernel.hip
(wbc_sim_inverse_dynamics) computes; the definition is the one in include/wbc_sim.h:

    tau = M(q) nudot + C(q, nu) nu + g(q),     nu = (v_root, omega_root, qd[0..19]),  nudot = d/dt of nu's WORLD components,

rows 0:3 the net external force (world axes), rows 3:6 the net external moment about the ROOT ORIGIN (world axes), rows 6: the
joint torques; locked fingers (DoFs 18, 19) zero.

Built with different algebra than the kernel so that agreement means something: the kernel runs recursive Newton-Euler with
spatial vectors about the base origin in base axes and sums subtree forces; here every body's classical kinematics (omega,
alpha, acceleration of its origin, then of its centre of mass) is propagated down the tree in WORLD coordinates, the body's
inertia force F = m (a_com - g) and torque T = I_w alpha + omega x I_w omega are formed there, and both are projected on the
generalised coordinates with the centre-of-mass Jacobians of whole_body_reference.point_jacobian.
"""
import numpy as np

import arm_osc_oracle as ao
import whole_body_reference as wb

NCOL = wb.NCOL
GRAVITY = (0.0, 0.0, -9.81)


def inverse_dynamics(model, root_pos, root_quat, q, nu, nudot=None, body_params=None, gravity=GRAVITY, forces=None):
    """(tau [26], mag [26]). mag = sum over bodies of |J_v|^T |F| + |J_w|^T |T|, the component-wise absolute values of the sum
    that gives tau: the scale the rounding error of an fp32 evaluation is proportional to. forces: a list that receives every
    body's inertia force F (world axes, at its centre of mass)."""
    q, nu = np.asarray(q, dtype=np.float64), np.asarray(nu, dtype=np.float64)
    nudot = np.zeros(NCOL) if nudot is None else np.asarray(nudot, dtype=np.float64)
    g = np.asarray(gravity, dtype=np.float64)
    R, p = ao.fk(model, root_pos, root_quat, q)
    nb = model.nb
    om, al, acc = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3))     # angular velocity / acceleration, origin acceleration
    om[0], al[0], acc[0] = nu[3:6], nudot[3:6], nudot[0:3]
    for b in range(1, nb):
        par, d = model.parent[b], model.body_dof[b]
        ax = R[b][:, model.axis[b]]
        r = p[b] - p[par]
        om[b] = om[par] + ax * nu[6 + d]
        al[b] = al[par] + ax * nudot[6 + d] + wb.cross3(om[par], ax * nu[6 + d])
        acc[b] = acc[par] + wb.cross3(al[par], r) + wb.cross3(om[par], wb.cross3(om[par], r))
    tau, mag = np.zeros(NCOL), np.zeros(NCOL)
    for b, (m, com, I6) in enumerate(wb.body_inertias(model, body_params)):
        rc = R[b] @ com
        a_com = acc[b] + wb.cross3(al[b], rc) + wb.cross3(om[b], wb.cross3(om[b], rc))
        Iw = R[b] @ wb._sym(I6) @ R[b].T
        F = m * (a_com - g)
        T = Iw @ al[b] + wb.cross3(om[b], Iw @ om[b])
        if forces is not None:
            forces.append(F)
        J = wb.point_jacobian(model, R, p, b, p[b] + rc)
        tau += J[0:3].T @ F + J[3:6].T @ T
        mag += np.abs(J[0:3]).T @ np.abs(F) + np.abs(J[3:6]).T @ np.abs(T)
    return tau, mag


def bias_forces(model, root_pos, root_quat, q, nu, body_params=None, gravity=GRAVITY):
    """h = C nu + g and its magnitude vector."""
    return inverse_dynamics(model, root_pos, root_quat, q, nu, None, body_params, gravity)


def gravity_forces(model, root_pos, root_quat, q, body_params=None, gravity=GRAVITY):
    """g(q) and its magnitude vector."""
    return inverse_dynamics(model, root_pos, root_quat, q, np.zeros(NCOL), None, body_params, gravity)


def potential_energy(model, root_pos, root_quat, q, body_params=None, gravity=GRAVITY):
    """-sum over bodies of m g . c_world."""
    R, p = ao.fk(model, root_pos, root_quat, np.asarray(q, dtype=np.float64))
    g = np.asarray(gravity, dtype=np.float64)
    return -sum(m * g @ (p[b] + R[b] @ com) for b, (m, com, _) in enumerate(wb.body_inertias(model, body_params)))
