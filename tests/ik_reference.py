"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) statement of the whole-body inverse kinematics problem of include/wbc_sim.h
(wbc_sim_inverse_kinematics; the kernel is wbc_ik_kernel of csrc/wbc_arm_kernel.hip):

    f(x) = 1/2 sum_k sum_i w_pos[k,i] (t_k,i - x_k(q)_i)^2 + 1/2 sum_k w_ori[k] |log(R_t,k R_k(q)^T)|^2 + 1/2 posture |q_j - q_ref|^2
    subject to the joint limits, over the 24 live coordinates: root translation (world axes), a WORLD rotation vector
    (R <- exp([dtheta]x) R) and the 18 revolute joints.

Stated here: the objective, its exact gradient, the Gauss-Newton matrix, the active-set rule, the damped projected step, and the
projected Levenberg-Marquardt loop itself. Poses and Jacobians are those of whole_body_reference (world coordinates straight from the
forward kinematics), and the orientation error is the logarithm of a rotation MATRIX (the kernel: an error quaternion), so agreement
with the kernel means something. `solve(..., dtype=np.float32)` rounds the state, the residuals, J, H, g and the step to fp32 in every
iteration: the same text is the fp32 yardstick the tests' constants are measured with.

The GPU tests never replay the kernel's path: they judge the point it returned with projected_step, objective, residuals and their
scales below.
"""
import numpy as np

import arm_osc_oracle as ao
import whole_body_reference as wbr

EPS = 2.0 ** -24
NLIVE = 24
LAMBDA_UP, LAMBDA_MIN, LAMBDA_MAX, FLOOR, MAX_ITER = 8.0, 1e-9, 1e8, 1e-9, 64   # the kernel's constants (csrc/wbc_arm_kernel.hip, IK_*)
GRIPPER = "wx250s/ee_gripper_link"


def bodies(model):
    """(feet [4], gripper) rigid-body indices."""
    feet = [i for i, name in enumerate(model.rb_names) if "foot" in name]
    assert len(feet) == 4
    return feet, model.rb_names.index(GRIPPER)


def live_dofs(model):
    """The 18 DoFs a joint drives, in DoF order: coordinate 6 + j is DoF live_dofs[j]."""
    return [d for d, b in enumerate(wbr.dof_body(model)) if b >= 0]


def limits(model):
    """(lower [20], upper [20], limited [20]); lower == upper == 0 means unlimited."""
    lo, hi = np.asarray(model.dof_lower, dtype=np.float64), np.asarray(model.dof_upper, dtype=np.float64)
    return lo, hi, ~((lo == 0) & (hi == 0))


# ------------------------------------------------------------------------------------------------ rotations (xyzw quaternions)
def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def quat_unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.sqrt(q @ q)


def quat_from_rotvec(v):
    v = np.asarray(v, dtype=np.float64)
    a = np.sqrt(v @ v)
    k = np.sin(0.5 * a) / a if a > 1e-12 else 0.5
    return np.r_[v * k, np.cos(0.5 * a)]


def rot_log(R):
    """The rotation vector of a rotation matrix, |phi| <= pi."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.sqrt(v @ v), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if s > 1e-9:
        return v * (th / s)
    if c > 0:
        return v
    a = np.sqrt(np.maximum((np.diag(R) - c) / (1.0 - c), 0.0))                     # |phi| = pi: the axis from the symmetric part
    i = int(np.argmax(a))
    sg = np.sign(R[i] + R[:, i]); sg[i] = 1.0
    return th * a * sg


class Problem:
    """One env's problem. tquat None: no orientation rows; wpos / wori None: ones."""

    def __init__(self, model, rbs, tpos, tquat=None, wpos=None, wori=None, q_ref=None, posture=1e-2):
        self.model, self.rbs, self.K = model, [int(r) for r in rbs], len(rbs)
        self.tpos = np.asarray(tpos, dtype=np.float64).reshape(self.K, 3)
        self.wpos = np.ones((self.K, 3)) if wpos is None else np.asarray(wpos, dtype=np.float64).reshape(self.K, 3)
        if tquat is None:
            assert wori is None
            self.wori, self.trot, self.tquat = np.zeros(self.K), [np.eye(3)] * self.K, None
        else:
            self.wori = np.ones(self.K) if wori is None else np.asarray(wori, dtype=np.float64).reshape(self.K)
            tq = self.tquat = np.asarray(tquat, dtype=np.float64).reshape(self.K, 4)
            self.trot = [ao.quat_to_mat(quat_unit(tq[k])) if self.wori[k] != 0 else np.eye(3) for k in range(self.K)]
        self.q_ref = None if q_ref is None else np.asarray(q_ref, dtype=np.float64)
        self.posture = float(posture)
        self.live = live_dofs(model)
        self.lo, self.hi, self.limited = limits(model)
        self.lo32, self.hi32 = f32(self.lo), f32(self.hi)                          # the limits as the kernel holds them
        self.cols = [0, 1, 2, 3, 4, 5] + [6 + d for d in self.live]


def clamp_start(P, state):
    """The start with its limited joints clamped; q_ref None becomes the clamped start joints."""
    pos, quat, q = [np.array(a, dtype=np.float64) for a in state]
    for d in P.live:
        if P.limited[d]:
            q[d] = min(max(q[d], P.lo32[d]), P.hi32[d])
    if P.q_ref is None:
        P.q_ref = q.copy()
    return pos, quat_unit(quat), q


def kinematics(P, state, jac=True):
    """Residuals [K, 6] (target - x; phi = log(R_target R^T); exactly 0 on a skipped row), their Jacobian [K, 6, 24] in the tangent and
    the scales [K, 3] of the position rows: the sum of the magnitudes x_k,i is formed from (the root's offset from `origin`, every
    joint offset and the body's own offset, each rotated into the world) plus |t - origin|, with origin the start root position."""
    m = P.model
    pos, quat, q = state
    R, p = ao.fk(m, pos, quat_unit(quat), np.asarray(q, dtype=np.float64))
    r = np.zeros((P.K, 6))
    J = np.zeros((P.K, 6, NLIVE))
    for k, rb in enumerate(P.rbs):
        b = m.rb_body[rb]
        x = p[b] + R[b] @ m.rb_offset[rb]
        r[k, 0:3] = np.where(P.wpos[k] != 0, np.where(P.wpos[k] != 0, P.tpos[k], 0.0) - x, 0.0)
        if P.wori[k] != 0:
            r[k, 3:6] = rot_log(P.trot[k] @ R[b].T)
        if jac:
            J[k] = wbr.point_jacobian(m, R, p, b, x)[:, P.cols]
    return r, J


def position_scales(P, state, origin):
    m = P.model
    pos, quat, q = state
    R, p = ao.fk(m, pos, quat_unit(quat), np.asarray(q, dtype=np.float64))
    s = np.zeros((P.K, 3))
    for k, rb in enumerate(P.rbs):
        b = m.rb_body[rb]
        acc = np.abs(np.where(P.wpos[k] != 0, P.tpos[k], 0.0) - origin) * (P.wpos[k] != 0) + np.abs(pos - origin) + np.abs(R[b]) @ np.abs(m.rb_offset[rb])
        while b > 0:
            acc = acc + np.abs(R[m.parent[b]]) @ np.abs(m.joint_xyz[b])
            b = m.parent[b]
        s[k] = acc
    return s


def weights(P):
    return np.concatenate([P.wpos, np.repeat(P.wori[:, None], 3, 1)], 1)           # [K, 6]


def objective_terms(P, state, r=None):
    """Every term of f, each >= 0: the weighted squared residuals [6 K] and the posture squares [18]."""
    r = kinematics(P, state, jac=False)[0] if r is None else r
    w = weights(P)
    dq = state[2][P.live] - P.q_ref[P.live]
    return np.concatenate([(0.5 * np.where(w != 0, w * r * r, 0.0)).ravel(), 0.5 * P.posture * dq * dq])


def objective(P, state, r=None):
    return float(objective_terms(P, state, r).sum())


def gradient_hessian(P, state, rnd=lambda a: a):
    """(g [24], H [24, 24], r [K, 6]): the exact gradient -J^T W r + posture S^T (q - q_ref) in the tangent (for the scalar w_ori the
    orientation term's is -w_ori J_ang^T phi) and the Gauss-Newton matrix J^T W J + posture S^T S."""
    r, J = kinematics(P, state)
    r, J = rnd(r), rnd(J)
    w = weights(P)
    Jf, wf, rf = J.reshape(-1, NLIVE), w.ravel(), r.ravel()
    g = -(Jf.T @ (wf * rf))
    H = Jf.T @ (wf[:, None] * Jf)
    g[6:] += P.posture * (state[2][P.live] - P.q_ref[P.live])
    H[np.arange(6, NLIVE), np.arange(6, NLIVE)] += P.posture
    return rnd(g), rnd(H), r


def active_set(P, state, g):
    """bool [24]: a limited joint that sits on a limit with the descent direction -g pushing outward."""
    fixed = np.zeros(NLIVE, dtype=bool)
    q = state[2]
    for j, d in enumerate(P.live):
        if P.limited[d]:
            fixed[6 + j] = (q[d] <= P.lo32[d] and g[6 + j] > 0) or (q[d] >= P.hi32[d] and g[6 + j] < 0)
    return fixed


def _identity_solve(A, held, rhs):
    A = A.copy()
    A[held, :] = 0.0; A[:, held] = 0.0
    A[held, held] = 1.0
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return np.full(NLIVE, np.nan)
    return np.linalg.solve(L.T, np.linalg.solve(L, rhs))


def damped_step(P, state, H, g, fixed, lam, rnd=lambda a: a):
    """(d [24], snap [24]): (H + lam diag H + floor) d = -g with the identity's rows and columns on the fixed coordinates. Then one
    second pass: a free joint whose step would leave its limits goes ONTO the limit (snap: that limit, NaN elsewhere), and the other
    coordinates solve again with those steps held, so that the projected step stays a descent step of the model."""
    A = H + np.diag(lam * np.diag(H) + FLOOR)
    d = rnd(_identity_solve(A, fixed, np.where(fixed, 0.0, -g)))
    snap = np.full(NLIVE, np.nan)
    q = state[2]
    for j, dof in enumerate(P.live):
        if P.limited[dof] and not fixed[6 + j]:
            v = rnd(q[dof] + d[6 + j])
            if v < P.lo32[dof] or v > P.hi32[dof]:
                snap[6 + j] = P.lo32[dof] if v < P.lo32[dof] else P.hi32[dof]
    hit = ~np.isnan(snap)
    if hit.any():
        dc = np.where(hit, rnd(np.where(hit, snap, 0.0) - np.r_[np.zeros(6), q[P.live]]), 0.0)
        rhs = np.where(fixed, 0.0, np.where(hit, dc, rnd(-g - H[:, hit] @ dc[hit])))
        d = rnd(_identity_solve(A, fixed | hit, rhs))
    return d, snap


def retract(P, state, d, clamp=True, snap=None):
    """(the state moved by the tangent step d, the projected step [24] actually taken); snap: damped_step's."""
    pos, quat, q = state
    qn = np.array(q, dtype=np.float64)
    s = np.array(d, dtype=np.float64)
    for j, dof in enumerate(P.live):
        v = q[dof] + d[6 + j]
        if clamp and P.limited[dof]:
            v = min(max(v, P.lo32[dof]), P.hi32[dof])
        if snap is not None and not np.isnan(snap[6 + j]):
            v = snap[6 + j]
        qn[dof] = v
        s[6 + j] = v - q[dof]
    return (pos + d[0:3], quat_unit(quat_mul(quat_from_rotvec(d[3:6]), quat_unit(quat))), qn), s


def projected_step(P, state, lam):
    """Infinity norm of the projected damped step the fp64 statement proposes from `state` at damping lam."""
    g, H, _ = gradient_hessian(P, state)
    d, snap = damped_step(P, state, H, g, active_set(P, state, g), lam)
    return float(np.abs(retract(P, state, d, snap=snap)[1]).max())


def solve(P, start, lam0=1e-3, step_tol=1e-4, max_iter=0, dtype=np.float64):
    """The projected Levenberg-Marquardt loop of include/wbc_sim.h. Returns a dict: state, status, iterations, cost0, cost."""
    rnd = (lambda a: a) if dtype == np.float64 else (lambda a: np.asarray(a, dtype=dtype).astype(np.float64))
    rs = lambda s: (rnd(s[0]), rnd(s[1]), rnd(s[2]))                              # noqa: E731
    cap = max_iter if max_iter > 0 else MAX_ITER
    state = rs(clamp_start(P, rs(start)))
    g, H, r = gradient_hessian(P, state, rnd)
    cost0 = cost = float(rnd(objective(P, state, r)))
    out = dict(state=state, status=1, iterations=0, cost0=cost0, cost=cost0)
    if not np.isfinite(cost0):
        out["status"] = 3
        return out
    lam, fixed = lam0, active_set(P, state, g)
    for trip in range(cap + 1):
        d, snap = damped_step(P, state, H, g, fixed, lam, rnd)
        cand, s = retract(P, state, d, snap=snap)
        cand = rs(cand)
        if np.all(np.isfinite(d)) and np.abs(s).max() <= step_tol and lam <= lam0:
            out["status"] = 0
            break
        if trip == cap:
            break
        out["iterations"] += 1
        rc = rnd(kinematics(P, cand, jac=False)[0])
        cc = float(rnd(objective(P, cand, rc)))
        if cc <= cost:
            state, cost, lam = cand, cc, max(lam / LAMBDA_UP, LAMBDA_MIN)
            g, H, r = gradient_hessian(P, state, rnd)
            fixed = active_set(P, state, g)
        else:
            lam *= LAMBDA_UP
            if lam > LAMBDA_MAX:
                out["status"] = 2
                break
    out.update(state=state, cost=cost)
    return out


# ------------------------------------------------------------------------------------------------ the family of the tests
def random_configuration(model, rng, spread=1.0):
    """(pos, quat, q): joints uniform inside `spread` of their limits' range about its middle (the unlimited waist within +-1.5 rad),
    fingers 0, a random root pose within +-2 m and +-0.5 rad of upright with any yaw."""
    lo, hi, limited = limits(model)
    q = np.zeros(len(lo))
    for d in live_dofs(model):
        a, b = (lo[d], hi[d]) if limited[d] else (-1.5, 1.5)
        q[d] = 0.5 * (a + b) + spread * 0.5 * (b - a) * rng.uniform(-1, 1)
    yaw = quat_from_rotvec([0, 0, rng.uniform(-np.pi, np.pi)])
    tilt = quat_from_rotvec(np.r_[rng.uniform(-0.5, 0.5, 2), 0.0])
    return rng.uniform(-2, 2, 3), quat_unit(quat_mul(yaw, tilt)), q


def perturbed(P_or_model, conf, rng, size):
    """conf moved by +-size rad on every joint (clamped), +-size rad about a random axis and +-size / 4 m on the root."""
    model = getattr(P_or_model, "model", P_or_model)
    lo, hi, limited = limits(model)
    pos, quat, q = conf
    qn = np.array(q)
    for d in live_dofs(model):
        qn[d] = q[d] + size * rng.choice([-1.0, 1.0])
        if limited[d]:
            qn[d] = min(max(qn[d], lo[d]), hi[d])
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    return pos + 0.25 * size * rng.choice([-1.0, 1.0], 3), quat_unit(quat_mul(quat_from_rotvec(size * ax), quat)), qn


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def member(model, seed, variant="reach", posture=1e-2):
    """One member of the family: the feet (position rows) and the gripper (position and orientation) at the fp64 poses of a
    configuration q* drawn inside the limits, from a start that is q* perturbed by +-0.1 rad (even seeds) or +-0.3 rad (odd seeds).
    variant "reach": q_ref = q*, the minimum is residual 0; "tradeoff": q_ref = the start. Every input is an fp32 value.
    Returns (Problem, start, q*)."""
    rng = np.random.default_rng(9000 + seed)
    feet, grip = bodies(model)
    rbs = feet + [grip]
    star = random_configuration(model, rng, spread=0.9)
    star = (f32(star[0]), f32(star[1]), f32(star[2]))
    pos, rot = wbr.rigid_body_poses(model, star[0], quat_unit(star[1]), star[2])
    tq = np.tile([0.0, 0.0, 0.0, 1.0], (5, 1))
    tq[4] = mat_to_quat(rot[grip])
    wori = np.array([0.0, 0.0, 0.0, 0.0, 1.0])
    start = perturbed(model, star, rng, 0.1 if seed % 2 == 0 else 0.3)
    start = (f32(start[0]), f32(start[1]), f32(start[2]))
    P = Problem(model, rbs, f32(pos[rbs]), f32(tq), None, wori, q_ref=(star[2] if variant == "reach" else None), posture=posture)
    return P, start, star


def mat_to_quat(R):
    """xyzw quaternion of a rotation matrix (the branch with the largest pivot)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R))); j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return quat_unit(np.array(q))
