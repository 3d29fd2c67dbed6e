"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) reference for wbc_sim_coriolis and wbc_sim_momentum_observer (csrc/wbc_arm_kernel.hip;
definitions in include/wbc_sim.h): the Coriolis matrix C(q, nu) of M nudot + C nu + g = tau in the factorisation with C + C^T = Mdot,
Mdot itself, the generalised momentum p = M nu, C^T nu, and the momentum observer's recursion.

Built with different algebra than the kernel so that agreement means something. The kernel walks the tree in the base frame about the
root origin, sums subtree composites of I_k and B_k through the ancestor masks and forms each entry from one or two six-term products.
Here every body contributes its own term of the brute-force sum

    C = sum_k J_k^T (I_k Jdot_k + B_k J_k),     B_k = 1/2 [crf(v_k) I_k + crfbar(I_k v_k) - I_k crm(v_k)],

in WORLD axes about one inertial point `origin`, with dense 6 x 6 matrices, the spatial Jacobians J_k from
whole_body_reference.point_jacobian (the point `origin` riding on body k) and v_k = J_k nu. Spatial vectors are (angular; linear).
Jdot_k's columns: 0 for the root's linear coordinates, (0; v_root x e_j) for its angular ones, crm(v_parent) S_c for a joint.
The vectors do not go through the matrix: p = sum_k J_k^T (I_k v_k), C^T nu = sum_k Jdot_k^T (I_k v_k)  (B_k^T v_k = 0).

The VALUES do not depend on `origin`; the magnitudes (the sums of the absolute values of the terms of each entry, which the rounding
error of an fp32 evaluation is proportional to) do. By default origin is the root's own position, so that no magnitude grows with the
robot's place in the world; tests/test_coriolis.py evaluates other points to show the independence.

Bounds of tests/test_coriolis.py: |got - ref| <= C 2^-24 mag for every entry, the constants in that module's docstring.
"""
import numpy as np

import constrained_dynamics_reference as cdr
import whole_body_reference as wb

NCOL, EPS = wb.NCOL, 2.0 ** -24
FAMILIES = ("cmat", "mdot", "p", "ctnu")


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=a.dtype)


def crm(v):
    """Motion cross-product matrix of v = (w; u)."""
    X = np.zeros((6, 6), dtype=v.dtype)
    X[0:3, 0:3] = X[3:6, 3:6] = _skew(v[0:3])
    X[3:6, 0:3] = _skew(v[3:6])
    return X


def crf(v):
    return -crm(v).T


def crfbar(f):
    """crfbar(f) v == crf(v) f."""
    X = np.zeros((6, 6), dtype=f.dtype)
    X[0:3, 0:3] = -_skew(f[0:3])
    X[0:3, 3:6] = X[3:6, 0:3] = -_skew(f[3:6])
    return X


class Terms:
    """Per moving body k: J_k, Jdot_k [6, 26], I_k [6, 6], v_k [6] about `origin` in world axes, every operation in `dtype`."""

    def __init__(self, model, root_pos, root_quat, q, nu, body_params=None, dtype=np.float64, origin=None):
        dt = self.dt = dtype
        nb = self.nb = model.nb
        root_pos = np.asarray(root_pos, dtype=np.float64)
        o = root_pos if origin is None else np.asarray(origin, dtype=np.float64)
        # positions relative to the point the moments are taken about, formed before any rounding to dtype
        R, p = cdr._fk(model, (root_pos - o).astype(dt), root_quat, np.asarray(q, dtype=dt), dt)
        nu = self.nu = np.asarray(nu, dtype=dt)
        zero = np.zeros(3, dtype=dt)
        self.J, self.Jd, self.I, self.v = [], [], [], []
        for k in range(nb):
            Jp = wb.point_jacobian(model, R, p, k, zero).astype(dt)
            self.J.append(np.concatenate([Jp[3:6], Jp[0:3]]))
            self.v.append((self.J[k] @ nu).astype(dt))
        for k, (m, com, I6) in enumerate(wb.body_inertias(model, body_params)):
            Jd = np.zeros((6, NCOL), dtype=dt)
            for j in range(3):
                Jd[3:6, 3 + j] = cdr._cross(nu[0:3], np.eye(3, dtype=dt)[j])
            b = k
            while b > 0:
                c = 6 + model.body_dof[b]
                Jd[:, c] = crm(self.v[model.parent[b]]) @ self.J[k][:, c]
                b = model.parent[b]
            self.Jd.append(Jd)
            m = dt(m)
            cw = (p[k] + R[k] @ np.asarray(com, dtype=dt)).astype(dt)
            Ib = R[k] @ wb._sym(I6).astype(dt) @ R[k].T + m * ((cw @ cw) * np.eye(3, dtype=dt) - np.outer(cw, cw))
            I = np.zeros((6, 6), dtype=dt)
            I[0:3, 0:3], I[0:3, 3:6], I[3:6, 0:3], I[3:6, 3:6] = Ib, m * _skew(cw), -m * _skew(cw), m * np.eye(3, dtype=dt)
            self.I.append(I)


def coriolis(model, root_pos, root_quat, q, nu, body_params=None, dtype=np.float64, origin=None, matrices=True):
    """(out, mag): dicts of cmat [26, 26], mdot [26, 26] (None unless matrices), p [26] and ctnu [26], float64 arrays of values
    computed in dtype. dtype = numpy.float32: the yardstick."""
    T = Terms(model, root_pos, root_quat, q, nu, body_params, dtype, origin)
    dt = dtype
    A = np.abs
    out = {"cmat": None, "mdot": None, "p": np.zeros(NCOL, dtype=dt), "ctnu": np.zeros(NCOL, dtype=dt)}
    mag = {"cmat": None, "mdot": None, "p": np.zeros(NCOL), "ctnu": np.zeros(NCOL)}
    if matrices:
        out["cmat"], mag["cmat"] = np.zeros((NCOL, NCOL), dtype=dt), np.zeros((NCOL, NCOL))
    for k in range(T.nb):
        J, Jd, I, v = T.J[k], T.Jd[k], T.I[k], T.v[k]
        h = (I @ v).astype(dt)
        out["p"] = (out["p"] + J.T @ h).astype(dt)
        out["ctnu"] = (out["ctnu"] + Jd.T @ h).astype(dt)
        hm = A(I).astype(np.float64) @ A(v)
        mag["p"] += A(J).T @ hm
        mag["ctnu"] += A(Jd).T @ hm
        if matrices:
            t1, t2, t3 = crf(v) @ I, crfbar(h), I @ crm(v)
            B = (dt(0.5) * (t1 + t2 - t3)).astype(dt)
            out["cmat"] = (out["cmat"] + J.T @ (I @ Jd + B @ J)).astype(dt)
            Bm = 0.5 * (A(crf(v)) @ A(I) + A(crfbar(hm.astype(dt))) + A(I) @ A(crm(v))).astype(np.float64)
            mag["cmat"] += A(J).T @ (A(I) @ A(Jd) + Bm @ A(J))
    out = {k: None if x is None else x.astype(np.float64) for k, x in out.items()}
    if matrices:
        out["mdot"] = (out["cmat"].astype(dt) + out["cmat"].astype(dt).T).astype(np.float64)
        mag["mdot"] = mag["cmat"] + mag["cmat"].T
    return out, mag


def observer_step(state, p, ctnu, grav, tau, gain, dt, reset=False):
    """One update of the momentum observer. state: (integral [26], residual [26]) or None with reset; returns the new pair.
        reset:      integral = p,                                             residual = 0
        otherwise:  integral += dt (tau + C^T nu - g + residual_old),         residual = gain (p - integral)."""
    if reset:
        return np.array(p, dtype=np.float64), np.zeros(NCOL)
    integral = state[0] + dt * (tau + ctnu - grav + state[1])
    return integral, gain * (p - integral)


def observer_magnitude(state, mag_p, mag_ctnu, mag_grav, tau, gain, dt):
    """(integral, residual) magnitudes of one update from the magnitudes of its inputs: the sizes of the terms added."""
    mi = np.abs(state[0]) + dt * (np.abs(tau) + mag_ctnu + mag_grav + np.abs(state[1]))
    return mi, gain * (mag_p + mi)


def largest_ratio(got, ref, mag):
    """Largest |got - ref| / (2^-24 mag); where the magnitude is 0 both must be exactly 0."""
    got, ref, mag = (np.asarray(x, dtype=np.float64) for x in (got, ref, mag))
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    return float((np.abs(got - ref)[~zero] / (EPS * mag[~zero])).max()) if (~zero).any() else 0.0
