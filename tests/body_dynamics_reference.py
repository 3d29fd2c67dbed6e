"""TEST INFRASTRUCTURE ONLY -- per-entry magnitudes and fp32 yardsticks for the whole-body Jacobian J [27, 6, 26] and mass matrix
M [26, 26] of wbc_sim_body_dynamics and for the arm's mm [6, 6], ee_j_eef [6, 6] and g_torque [6] of wbc_sim_arm_dynamics
(csrc/wbc_arm_kernel.hip). The fp64 VALUES stay those of tests/whole_body_reference.py (centre-of-mass Jacobians, world coordinates);
this module adds what the siblings' convention needs: |kernel - ref| <= C 2^-24 mag for every entry.

Magnitudes (rotation invariant: Euclidean norms, as centroidal_reference._nrm; the world-axes sum of |terms| is exactly 0 on entries
such as M[0, 1], where an evaluation in the base frame legitimately rounds m (R^T e_0).(R^T e_1)):
    J, angular rows   1 on the columns that move the rigid body
    J, linear rows    the length of the tree path from the joint's origin (the root's origin for the omega_root columns) to the rigid
                      body's origin: the sum of |joint_xyz| and |rb_offset| along it
    M[i, j]           sum over the moving bodies k of  n_i^T N_k n_j,  n_c = (|angular half|, |linear half|) of column c of the spatial
                      Jacobian J_k about the root origin, N_k the 2 x 2 matrix of the Frobenius norms of the 3 x 3 blocks of I_k
    mm, ee_j_eef      the same magnitudes on their slices M[-8:-2, -8:-2], J[gripper, :, -8:-2]
    g_torque[c]       sum over the 9 links of link_mass 9.81 mag_J[link, z, c]
Where the magnitude is 0 the entry is fixed by the tree's structure (the masks of test_whole_body_dynamics._structure, the finger
columns, the identity parts of the root columns, a joint's lever to a rigid body at its own origin): value and reference must be EQUAL.

Yardsticks (numpy.float32, the root at the origin, never the kernel), two formulations:
    world   the per-body sum  M = sum_k J_k^T I_k J_k  of coriolis_reference.Terms in world axes about the root origin; J from
            whole_body_reference.point_jacobian on fp32 forward kinematics
    base    forward kinematics in the base frame, spatial inertias about its origin summed into subtree composites, M_ij = S_i . (Ic S_j)
            with the root columns R^T e_j; J's levers formed in the base frame and rotated to the world afterwards
K_ref of an output is the larger of the two largest ratios; tests/test_whole_body_dynamics.py measures and asserts it.
"""
import numpy as np

import arm_osc_oracle as ao
import constrained_dynamics_reference as cdr
import coriolis_reference as cor
import whole_body_reference as wb

NCOL, EPS = wb.NCOL, 2.0 ** -24
OUTPUTS = ("J", "M", "mm", "ee", "g")
ARM = slice(NCOL - 8, NCOL - 2)                 # the arm's six joints among the 26 coordinates (WG:557-558)
GRAVITY = 9.81
EE_NAME = "wx250s/ee_gripper_link"


def _nrm(v, axis=None):
    return np.linalg.norm(np.asarray(v, dtype=np.float64), axis=axis)


def arm_links(model):
    """(rigid body of the end effector, the 9 rigid bodies whose weight the arm compensates)."""
    return model.rb_names.index(EE_NAME), list(range(model.num_rigid_bodies - 9, model.num_rigid_bodies))


def lever_paths(model):
    """[27, 26]: the tree path length from column c's joint origin (root origin for columns 3..5) to rigid body r's origin; 0 where
    the column does not move the body (and on the v_root columns, which have no lever)."""
    L = np.zeros((model.num_rigid_bodies, NCOL))
    for r, b in enumerate(model.rb_body):
        length = float(_nrm(model.rb_offset[r]))
        while b > 0:
            L[r, 6 + model.body_dof[b]] = length
            length += float(_nrm(model.joint_xyz[b]))
            b = model.parent[b]
        L[r, 3:6] = length
    return L


def jacobian_magnitude(model):
    """[27, 6, 26]; depends on the model alone."""
    L = lever_paths(model)
    mag = np.zeros((model.num_rigid_bodies, 6, NCOL))
    for r, b in enumerate(model.rb_body):
        while b > 0:
            c = 6 + model.body_dof[b]
            mag[r, 0:3, c], mag[r, 3:6, c] = L[r, c], 1.0
            b = model.parent[b]
        for j in range(3):
            for k in range(3):
                if k != j:
                    mag[r, k, 3 + j] = L[r, 3 + j]              # (e_j x d)_k; k == j and the identities are structure
    return mag


def mass_matrix_magnitude(terms):
    """[26, 26] from the fp64 coriolis_reference.Terms of the state."""
    mag = np.zeros((NCOL, NCOL))
    for k in range(terms.nb):
        J, I = terms.J[k], terms.I[k]
        n = np.stack([_nrm(J[0:3], axis=0), _nrm(J[3:6], axis=0)])                                        # [2, 26]
        N = np.array([[_nrm(I[3 * a:3 * a + 3, 3 * b:3 * b + 3]) for b in range(2)] for a in range(2)])  # [2, 2]
        mag += n.T @ N @ n
    return 0.5 * (mag + mag.T)                   # N_k is symmetric; this takes the last bit of the products' order out


def _arm_outputs(model, J, M, link_mass):
    ee, links = arm_links(model)
    g = sum(float(mk) * GRAVITY * J[rb, 2, ARM] for rb, mk in zip(links, link_mass))
    return {"J": J, "M": M, "mm": M[ARM, ARM], "ee": J[ee][:, ARM], "g": g}


def reference(model, root_pos, root_quat, q, body_params=None, link_mass=None):
    """(out, mag): dicts over OUTPUTS of the fp64 values and their magnitudes. link_mass [9]: the masses g_torque weighs the arm's
    links with (default: the model's)."""
    link_mass = np.asarray(model.rb_mass[-9:] if link_mass is None else link_mass, dtype=np.float64)
    J = wb.jacobian(model, root_pos, root_quat, q)
    M = wb.mass_matrix(model, root_pos, root_quat, q, body_params)
    T = cor.Terms(model, root_pos, root_quat, q, np.zeros(NCOL), body_params)
    return _arm_outputs(model, J, M, link_mass), _arm_outputs(model, jacobian_magnitude(model), mass_matrix_magnitude(T), link_mass)


def _rigid_body_jacobians(model, R, p, dt):
    return np.array([wb.point_jacobian(model, R, p, b, p[b] + R[b] @ np.asarray(model.rb_offset[r], dtype=dt))
                     for r, b in enumerate(model.rb_body)])


def yardstick_world(model, root_quat, q, body_params=None, link_mass=None, dtype=np.float32):
    """The per-body world-axes sum about the root origin, every operation in dtype."""
    dt = dtype
    link_mass = np.asarray(model.rb_mass[-9:] if link_mass is None else link_mass, dtype=dt)
    T = cor.Terms(model, np.zeros(3), root_quat, q, np.zeros(NCOL), body_params, dtype=dt)
    M = np.zeros((NCOL, NCOL), dtype=dt)
    for k in range(T.nb):
        M = (M + T.J[k].T @ (T.I[k] @ T.J[k]).astype(dt)).astype(dt)
    R, p = cdr._fk(model, np.zeros(3), root_quat, np.asarray(q, dtype=dt), dt)
    J = _rigid_body_jacobians(model, R, p, dt)
    ee, links = arm_links(model)
    g = np.zeros(6, dtype=dt)
    for rb, mk in zip(links, link_mass):
        g = (g + mk * dt(GRAVITY) * J[rb, 2, ARM].astype(dt)).astype(dt)
    out = {"J": J, "M": M, "mm": M[ARM, ARM], "ee": J[ee][:, ARM], "g": g}
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def _spatial_inertia(m, c, Irot, dt):
    """6 x 6 (angular; linear) about the origin of the frame c and Irot are given in."""
    cx = cor._skew(c)
    I = np.zeros((6, 6), dtype=dt)
    I[0:3, 0:3] = Irot + m * ((c @ c) * np.eye(3, dtype=dt) - np.outer(c, c))
    I[0:3, 3:6], I[3:6, 0:3], I[3:6, 3:6] = m * cx, -m * cx, m * np.eye(3, dtype=dt)
    return I.astype(dt)


def yardstick_base(model, root_quat, q, body_params=None, link_mass=None, dtype=np.float32):
    """Composite inertias in the base frame about the root origin; the world enters through the root columns R^T e_j (M) and one
    rotation of every finished lever (J). Every operation in dtype."""
    dt = dtype
    nb = model.nb
    link_mass = np.asarray(model.rb_mass[-9:] if link_mass is None else link_mass, dtype=dt)
    Rw = ao.quat_to_mat(np.asarray(root_quat, dtype=np.float64)).astype(dt)
    E, P = cdr._fk(model, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), np.asarray(q, dtype=dt), dt)        # base frame
    Ic = []
    for b, (m, com, I6) in enumerate(wb.body_inertias(model, body_params)):
        c = (P[b] + E[b] @ np.asarray(com, dtype=dt)).astype(dt)
        Ic.append(_spatial_inertia(dt(m), c, (E[b] @ wb._sym(I6).astype(dt) @ E[b].T).astype(dt), dt))
    for b in range(nb - 1, 0, -1):                                   # children carry larger indices than their parents
        assert model.parent[b] < b
        Ic[model.parent[b]] = (Ic[model.parent[b]] + Ic[b]).astype(dt)
    S, body = np.zeros((NCOL, 6), dtype=dt), [0] * 6 + wb.dof_body(model)
    for j in range(3):
        S[j, 3:6] = Rw.T[:, j]                                       # v_F = R^T v_root
        S[3 + j, 0:3] = Rw.T[:, j]
    axF = {}
    for b in range(1, nb):
        a = axF[b] = E[b][:, model.axis[b]]
        S[6 + model.body_dof[b]] = np.r_[a, cdr._cross(P[b], a)]
    F = np.array([Ic[body[c]] @ S[c] if body[c] >= 0 else np.zeros(6, dtype=dt) for c in range(NCOL)], dtype=dt)
    M = np.zeros((NCOL, NCOL), dtype=dt)
    for i in range(NCOL):
        for j in range(NCOL):
            if body[i] < 0 or body[j] < 0:
                continue
            if body[i] in wb.ancestors(model, body[j]):
                M[i, j] = S[i] @ F[j]
            elif body[j] in wb.ancestors(model, body[i]):
                M[i, j] = S[j] @ F[i]
    J = np.zeros((model.num_rigid_bodies, 6, NCOL), dtype=dt)
    for r, b in enumerate(model.rb_body):
        pF = (P[b] + E[b] @ np.asarray(model.rb_offset[r], dtype=dt)).astype(dt)
        d = (Rw @ pF).astype(dt)
        J[r, 0:3, 0:3] = J[r, 3:6, 3:6] = np.eye(3, dtype=dt)
        for j in range(3):
            J[r, 0:3, 3 + j] = cdr._cross(np.eye(3, dtype=dt)[j], d)
        while b > 0:
            c = 6 + model.body_dof[b]
            J[r, 0:3, c], J[r, 3:6, c] = Rw @ cdr._cross(axF[b], (pF - P[b]).astype(dt)), Rw @ axF[b]
            b = model.parent[b]
    ee, links = arm_links(model)
    g = np.zeros(6, dtype=dt)
    for rb, mk in zip(links, link_mass):
        g = (g + mk * dt(GRAVITY) * J[rb, 2, ARM]).astype(dt)
    out = {"J": J, "M": M, "mm": M[ARM, ARM], "ee": J[ee][:, ARM], "g": g}
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def ratio(got, ref, mag):
    """(largest |got - ref| / (2^-24 mag), its index); where the magnitude is 0, got must EQUAL ref."""
    got, ref, mag = (np.asarray(x, dtype=np.float64) for x in (got, ref, mag))
    assert got.shape == ref.shape == mag.shape and np.isfinite(got).all()
    zero = mag == 0
    bad = zero & (got != ref)
    assert not bad.any(), ("a structural entry differs", tuple(int(i) for i in np.argwhere(bad)[0]), float(got[bad][0]), float(ref[bad][0]))
    r = np.where(zero, 0.0, np.abs(got - ref) / np.where(zero, 1.0, EPS * mag))
    at = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    return (float(r[at]) if r.size else 0.0), tuple(int(i) for i in at)
