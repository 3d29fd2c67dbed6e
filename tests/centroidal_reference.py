"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) reference for wbc_sim_centroidal (csrc/wbc_arm_kernel.hip; definition in include/wbc_sim.h):
centre of mass, centroidal momentum h_G, its rate, the centroidal momentum matrix A_G and the locked centroidal inertia I_G.

A DIRECT SUM over the moving bodies in world coordinates: forward kinematics of oracle/arm_osc_oracle.py, inertias of
whole_body_reference.body_inertias, the velocity recursion of whole_body_reference.kinetic_energy and the classical acceleration recursion
of constrained_dynamics_reference.body_accelerations carried to every body's centre of mass c_b:

    m = sum m_b,   c = sum m_b c_b / m,   h_G = sum (m_b v_cb ; I_b w_b + m_b (c_b - c) x v_cb),
    hdot_G = sum (m_b a_cb ; I_b al_b + w_b x I_b w_b + m_b (c_b - c) x a_cb),   I_G = sum I_b + m_b (|d|^2 1 - d d^T), d = c_b - c,

and A_G column by column from unit nu. The kernel instead walks in registers, takes every joint column of A_G from the subtree's composite
about the joint's own origin and moves it to the centre of mass, so agreement means something.

In fp64 the angular sums use the bodies' ABSOLUTE velocities and accelerations, as written above. sum m_b (c_b - c) x X vanishes for any
X common to all bodies, so v_root and nudot[0:3] drop out of every angular row; with dtype = numpy.float32 (the rounding YARDSTICK, never
the kernel: the same sums in numpy float32 with the root at the origin) and for the columns of A_G the velocities and accelerations are
taken relative to the root origin's linear motion and the linear part m v_root is added afterwards. The columns of v_root are then
exactly (m 1 ; 0).

mag, per the siblings' convention, is the sum of the sizes of the terms added (Euclidean norms: the three components of a block share one
figure), the scale an fp32 evaluation's error is proportional to:
    c - p_root        sum m_b |c_b - p_root| / m
    v_com, a_com      |v_root| + sum m_b |v_cb - v_root| / m                      (likewise with a)
    h_G               linear m |v_root| + sum m_b |v_cb - v_root|;  angular sum |I_b w_b| + m_b |c_b - c| |v_cb - v_root|
    hdot_G            linear likewise with a;  angular sum |I_b al_b| + |w_b x I_b w_b| + m_b |c_b - c| |a_cb - a_root|
    A_G               h_G's with unit nu, column by column
    I_G               sum |I_b|_F + m_b |c_b - c|^2                                (mass: m itself)
No term is proportional to |v_root| or |nudot[0:3]| in an angular row.

Bounds of tests/test_centroidal.py: |got - ref| <= C 2^-24 mag for every entry, C the smallest power of two >= 16 K_ref per output
family, K_ref the yardstick's largest ratio over that module's two state families (measured there on the CPU, asserted <= C / 16).
"""
import numpy as np

import constrained_dynamics_reference as cdr
import whole_body_reference as wb

NCOL, EPS = wb.NCOL, 2.0 ** -24
FAMILIES = ("com", "mom", "momdot", "cmm", "inertia")
# Measured by tests/test_centroidal.py::test_fp32_yardsticks_sit_well_inside_the_bounds (the table is in that module's docstring).
C = {"com": 64.0, "mom": 64.0, "momdot": 64.0, "cmm": 256.0, "inertia": 64.0}

_cross = cdr._cross


def _nrm(v):
    return float(np.linalg.norm(np.asarray(v, dtype=np.float64)))


class Kinematics:
    """Everything that depends on the pose alone: frames, centres of mass relative to the root origin, world inertias. The root position
    enters nothing (every output is relative to it), so the kinematics run with the root at the origin."""

    def __init__(self, model, root_pos, root_quat, q, body_params=None, dtype=np.float64):
        dt = self.dt = dtype
        self.model = model
        self.R, p = cdr._fk(model, np.zeros(3), root_quat, np.asarray(q, dtype=dt), dt)       # the root at the origin
        self.p = p
        # the step from the parent's origin to the body's, from the model's offset (p[b] - p[parent] would cancel at the far links)
        self.r = np.array([np.zeros(3, dtype=dt) if b == 0 else self.R[model.parent[b]] @ np.asarray(model.joint_xyz[b], dtype=dt)
                           for b in range(model.nb)], dtype=dt)
        inert = wb.body_inertias(model, body_params)
        self.m = np.array([m for m, _, _ in inert], dtype=dt)
        self.rc = np.array([self.R[b] @ np.asarray(com, dtype=dt) for b, (_, com, _) in enumerate(inert)], dtype=dt)
        self.cb = (p + self.rc).astype(dt)
        self.Iw = np.array([self.R[b] @ wb._sym(I6).astype(dt) @ self.R[b].T for b, (_, _, I6) in enumerate(inert)], dtype=dt)
        mt, mc = dt(0), np.zeros(3, dtype=dt)
        for b in range(model.nb):
            mt = dt(mt + self.m[b])
            mc = (mc + self.m[b] * self.cb[b]).astype(dt)
        self.mass, self.c = mt, (mc / mt).astype(dt)
        self.d = (self.cb - self.c).astype(dt)

    def velocities(self, nu):
        """(w [nb, 3], vr [nb, 3]): angular velocity and the centre of mass's velocity RELATIVE to v_root."""
        m, dt = self.model, self.dt
        nu = np.asarray(nu, dtype=dt)
        w, v = np.zeros((m.nb, 3), dtype=dt), np.zeros((m.nb, 3), dtype=dt)
        w[0] = nu[3:6]
        for b in range(1, m.nb):
            par = m.parent[b]
            w[b] = w[par] + self.R[b][:, m.axis[b]] * nu[6 + m.body_dof[b]]
            v[b] = v[par] + _cross(w[par], self.r[b])
        return w, np.array([v[b] + _cross(w[b], self.rc[b]) for b in range(m.nb)], dtype=dt)

    def accelerations(self, nu, nudot):
        """(w, al, ar): angular velocity and acceleration, the centre of mass's classical acceleration RELATIVE to nudot[0:3]."""
        m, dt = self.model, self.dt
        nu, nudot = np.asarray(nu, dtype=dt), np.asarray(nudot, dtype=dt)
        w, al, a = (np.zeros((m.nb, 3), dtype=dt) for _ in range(3))
        w[0], al[0] = nu[3:6], nudot[3:6]
        for b in range(1, m.nb):
            par, d = m.parent[b], m.body_dof[b]
            ax, r = self.R[b][:, m.axis[b]], self.r[b]
            w[b] = w[par] + ax * nu[6 + d]
            al[b] = al[par] + ax * nudot[6 + d] + _cross(w[par], ax * nu[6 + d])
            a[b] = a[par] + _cross(al[par], r) + _cross(w[par], _cross(w[par], r))
        ar = np.array([a[b] + _cross(al[b], self.rc[b]) + _cross(w[b], _cross(w[b], self.rc[b])) for b in range(m.nb)], dtype=dt)
        return w, al, ar

    def momentum(self, nu, relative):
        """(h_G [6], mag [6]) of the velocity nu. relative: the angular sum takes the velocities relative to v_root."""
        dt, nb = self.dt, self.model.nb
        v0 = np.asarray(nu, dtype=dt)[0:3]
        w, vr = self.velocities(nu)
        lin, ang, ml, ma = np.zeros(3, dtype=dt), np.zeros(3, dtype=dt), 0.0, 0.0
        for b in range(nb):
            Lw = self.Iw[b] @ w[b]
            lin = lin + self.m[b] * vr[b]
            ang = ang + Lw + self.m[b] * _cross(self.d[b], vr[b] if relative else vr[b] + v0)
            ml += float(self.m[b]) * _nrm(vr[b])
            ma += _nrm(Lw) + float(self.m[b]) * _nrm(self.d[b]) * _nrm(vr[b])
        lin = self.mass * v0 + lin
        ml += float(self.mass) * _nrm(v0)
        return np.r_[lin, ang].astype(np.float64), np.r_[[ml] * 3, [ma] * 3]

    def momentum_rate(self, nu, nudot, relative):
        dt, nb = self.dt, self.model.nb
        a0 = np.asarray(nudot, dtype=dt)[0:3]
        w, al, ar = self.accelerations(nu, nudot)
        lin, ang, ml, ma = np.zeros(3, dtype=dt), np.zeros(3, dtype=dt), 0.0, 0.0
        for b in range(nb):
            Ia, Lw = self.Iw[b] @ al[b], self.Iw[b] @ w[b]
            gy = _cross(w[b], Lw)
            lin = lin + self.m[b] * ar[b]
            ang = ang + Ia + gy + self.m[b] * _cross(self.d[b], ar[b] if relative else ar[b] + a0)
            ml += float(self.m[b]) * _nrm(ar[b])
            ma += _nrm(Ia) + _nrm(gy) + float(self.m[b]) * _nrm(self.d[b]) * _nrm(ar[b])
        lin = self.mass * a0 + lin
        ml += float(self.mass) * _nrm(a0)
        return np.r_[lin, ang].astype(np.float64), np.r_[[ml] * 3, [ma] * 3]

    def inertia(self):
        """(mass, I_G as xx yy zz xy xz yz) [7] and its magnitude."""
        dt = self.dt
        I, mag = np.zeros((3, 3), dtype=dt), 0.0
        for b in range(self.model.nb):
            d = self.d[b]
            I = I + self.Iw[b] + self.m[b] * ((d @ d) * np.eye(3, dtype=dt) - np.outer(d, d))
            mag += _nrm(self.Iw[b]) + float(self.m[b]) * _nrm(d) ** 2
        six = [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
        return np.r_[self.mass, six].astype(np.float64), np.r_[float(self.mass), [mag] * 6]


def centroidal(model, root_pos, root_quat, q, nu, nudot=None, body_params=None, dtype=np.float64, cmm=True):
    """(out, mag): dicts of com [9], mom [6] (h_G), momdot [6], cmm [6, 26] (None unless cmm) and inertia [7], in the layout of
    wbc_sim_centroidal; nudot None: zeros, i.e. the bias parts. dtype = numpy.float32: the yardstick."""
    dt = dtype
    K = Kinematics(model, root_pos, root_quat, q, body_params, dt)
    rel = dt != np.float64
    nu = np.asarray(nu, dtype=np.float64)
    nudot = np.zeros(NCOL) if nudot is None else np.asarray(nudot, dtype=np.float64)
    out, mag = {}, {}
    h, hm = K.momentum(nu, rel)
    hd, hdm = K.momentum_rate(nu, nudot, rel)
    mt = float(K.mass)
    cm = sum(float(K.m[b]) * _nrm(K.cb[b]) for b in range(model.nb)) / mt
    if rel:                                             # v_com = v_root + (sum m_b vr_b) / m, every operation rounded
        v0, a0 = nu[0:3].astype(dt), nudot[0:3].astype(dt)
        vc = (v0 + (h[0:3].astype(dt) - K.mass * v0) / K.mass).astype(np.float64)
        ac = (a0 + (hd[0:3].astype(dt) - K.mass * a0) / K.mass).astype(np.float64)
    else:
        vc, ac = h[0:3] / mt, hd[0:3] / mt
    out["com"], mag["com"] = np.r_[K.c.astype(np.float64), vc, ac], np.r_[[cm] * 3, hm[0:3] / mt, hdm[0:3] / mt]
    out["mom"], mag["mom"], out["momdot"], mag["momdot"] = h, hm, hd, hdm
    out["inertia"], mag["inertia"] = K.inertia()
    out["cmm"] = mag["cmm"] = None
    if cmm:
        cols = [K.momentum(np.eye(NCOL)[c], True) for c in range(NCOL)]
        out["cmm"], mag["cmm"] = np.array([a for a, _ in cols]).T, np.array([g for _, g in cols]).T
    return out, mag


def shift_to_com(rows, c):
    """[6, ...] rows about the root origin (linear; angular) -> about the point c relative to it: angular - c x linear."""
    rows = np.asarray(rows, dtype=np.float64)
    lin, ang = rows[0:3], rows[3:6]
    return np.concatenate([lin, ang - np.cross(np.asarray(c, dtype=np.float64), lin, axisa=0, axisb=0, axisc=0)])


def largest_ratio(got, ref, mag):
    """Largest |got - ref| / (2^-24 mag); where the magnitude is 0 both must be exactly 0."""
    got, ref, mag = (np.asarray(x, dtype=np.float64) for x in (got, ref, mag))
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.all(got[zero] == 0) and np.all(ref[zero] == 0)
    return float((np.abs(got - ref)[~zero] / (EPS * mag[~zero])).max()) if (~zero).any() else 0.0
