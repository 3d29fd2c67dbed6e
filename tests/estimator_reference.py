"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the leg-odometry Kalman filter that wbc_sim_leg_odometry computes
(include/wbc_sim.h has the definition), batched over envs, in fp64 or -- the same text, `dtype=np.float32` -- in fp32 as the yardstick of
what single precision costs. Nothing here comes from the kernels: the leg kinematics are read from widowgo1_model.json through
abi.load_default_model() and walked in trunk axes, S is factorised and W = L^-1 C P- formed by loops written here.

update() also returns, per output entry, the SIZE OF THE TERMS summed into it (`mag`): the scale an error is judged against is
2^-24 mag. The sizes, with |.| entrywise and K = W^T L^-1 the gain:
    x-    |p| + |v| dt + a_mag dt^2 / 2, |v| + a_mag dt (a_mag = |R| |accel| + |g|), |p_i|
    e     position rows reach_i + mag(p-) + |p_i|; velocity rows (|w_b| + sum over the leg's joints |qd|) reach_i + mag(v-); height rows |h_i| + |p_i,z|
          (reach_i: the summed lengths of leg i's joint offsets and foot offset)
    x+    mag(x-) + |K| mag(e)
    P-    A |P| A^T + Q;      P+   mag(P-) + |W|^T |W|
    nis   sum_k (|L^-1| mag(e))_k^2;      vel_body   |R|^T mag(v+)
    reset p_i: |p_init| + reach_i
An env whose factorisation fails, or that is reset, has the sizes of what it returns."""
import numpy as np

NX, NFEET = 18, 4
STATUS_OK, STATUS_RESET, STATUS_FAILED = 0, 1, 2
CFG_FIELDS = ("dt", "sigma_p", "sigma_v", "sigma_f", "sigma_r", "sigma_rdot", "sigma_z", "kappa", "p0_p", "p0_v", "p0_f")
EPS = 2.0 ** -24


def legs(model, foot_name="foot"):
    """Per foot, in rigid-body order (FL, FR, RL, RR): ([(axis, dof, joint offset)] from the trunk down, the foot's offset in its body)."""
    out = []
    for rb, name in enumerate(model.rb_names):
        if foot_name not in name:
            continue
        b, chain = int(model.rb_body[rb]), []
        while b > 0:
            chain.append((int(model.axis[b]), int(model.body_dof[b]), np.asarray(model.joint_xyz[b], dtype=np.float64)))
            b = int(model.parent[b])
        out.append((chain[::-1], np.asarray(model.rb_offset[rb], dtype=np.float64)))
    assert len(out) == NFEET
    return out


def reach(model):
    """[4]: the summed lengths of each leg's joint offsets and foot offset."""
    return np.array([sum(np.linalg.norm(xyz) for _, _, xyz in chain) + np.linalg.norm(off) for chain, off in legs(model)])


def _axis_rot(axis, ang):
    """[N, 3, 3] rotations about coordinate axis `axis`."""
    c, s = np.cos(ang), np.sin(ang)
    R = np.zeros(ang.shape + (3, 3), dtype=ang.dtype)
    i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
    R[..., i, i] = 1
    R[..., j, j] = c; R[..., j, k] = -s
    R[..., k, j] = s; R[..., k, k] = c
    return R


def leg_kinematics(model, q, qd=None, jac=False, dtype=np.float64):
    """fk [N, 4, 3]: the foot origins relative to the trunk's origin in trunk axes; vrel [N, 4, 3] = J(q) qd (None without qd); with jac the
    [N, 4, 3, 3] Jacobians against each leg's own three joints, and the [4, 3] DoF indices."""
    q = np.asarray(q, dtype=dtype)
    n = q.shape[0]
    fk = np.zeros((n, NFEET, 3), dtype=dtype)
    vrel = None if qd is None else np.zeros((n, NFEET, 3), dtype=dtype)
    J = np.zeros((n, NFEET, 3, 3), dtype=dtype) if jac else None
    dofs = np.zeros((NFEET, 3), dtype=np.int64)
    for f, (chain, off) in enumerate(legs(model)):
        E = np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3)).copy()
        p = np.zeros((n, 3), dtype=dtype)
        origins, axes = [], []
        for axis, dof, xyz in chain:
            p = p + E @ xyz.astype(dtype)
            E = E @ _axis_rot(axis, q[:, dof])
            origins.append(p); axes.append(E[:, :, axis])
        fk[:, f] = p + E @ off.astype(dtype)
        for k, (axis, dof, xyz) in enumerate(chain):
            col = np.cross(axes[k], fk[:, f] - origins[k])
            if vrel is not None:
                vrel[:, f] += col * np.asarray(qd, dtype=dtype)[:, dof, None]
            if jac:
                J[:, f, :, k] = col
            dofs[f, k] = dof
    return (fk, vrel, J, dofs) if jac else (fk, vrel)


def quat_to_mat(quat, dtype=np.float64):
    """[N, 3, 3] from xyzw quaternions [N, 4], normalised first."""
    q = np.asarray(quat, dtype=dtype)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), dtype=dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def rows(m):
    """(c1 [m], c2 [m] (-1: none), foot [m], group [m]) of the correction's rows: C has +1 at c1 and -1 at c2."""
    c1, c2, foot, group = [], [], [], []
    for f in range(NFEET):
        for a in range(3):
            c1.append(a); c2.append(6 + 3 * f + a); foot.append(f); group.append(0)
    for f in range(NFEET):
        for a in range(3):
            c1.append(3 + a); c2.append(-1); foot.append(f); group.append(1)
    for f in range(NFEET):
        c1.append(6 + 3 * f + 2); c2.append(-1); foot.append(f); group.append(2)
    return tuple(np.array(v[:m]) for v in (c1, c2, foot, group))


def selection(m, dtype=np.float64):
    """C [m, 18] written out (the kernel never forms it)."""
    c1, c2, _, _ = rows(m)
    C = np.zeros((m, NX), dtype=dtype)
    C[np.arange(m), c1] = 1
    C[np.arange(m)[c2 >= 0], c2[c2 >= 0]] = -1
    return C


def cholesky(S):
    """S = L L^T for a batch [N, m, m], column by column; ok [N] False where a pivot is not a positive finite number (L is then garbage)."""
    n, m, _ = S.shape
    L = np.zeros_like(S)
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(m):
            d = S[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(-1)
            ok &= np.isfinite(d) & (d > 0)
            dj = np.sqrt(np.where(ok, d, 1)).astype(S.dtype)
            L[:, j, j] = dj
            L[:, j + 1:, j] = (S[:, j + 1:, j] - np.einsum("nik,nk->ni", L[:, j + 1:, :j], L[:, j, :j])) / dj[:, None]
    return L, ok


def forward(L, B):
    """L^-1 B for a batch: L [N, m, m] lower, B [N, m, c]."""
    Y = np.zeros_like(B)
    with np.errstate(all="ignore"):
        for i in range(L.shape[1]):
            Y[:, i] = (B[:, i] - np.einsum("nk,nkc->nc", L[:, i, :i], Y[:, :i])) / L[:, i, i, None]
    return Y


def measurement(model, quat, gyro, dof, dtype=np.float64):
    """R [N, 3, 3], r [N, 4, 3], rdot [N, 4, 3] in world axes, and rate [N, 4] = |w_b| + the sum of leg i's |qd|: rate_i reach_i is the
    size of rdot_i's terms."""
    R = quat_to_mat(quat, dtype)
    dof = np.asarray(dof, dtype=dtype)
    wb = np.asarray(gyro, dtype=dtype)
    fk, vrel = leg_kinematics(model, dof[:, :, 0], dof[:, :, 1], dtype=dtype)
    r = np.einsum("nij,nfj->nfi", R, fk)
    rdot = np.einsum("nij,nfj->nfi", R, np.cross(wb[:, None, :], fk) + vrel)
    joint_rates = np.stack([sum(np.abs(dof[:, d, 1]) for _, d, _ in chain) for chain, _ in legs(model)], axis=1)     # [N, 4]
    rate = np.abs(wb).sum(-1)[:, None] + joint_rates
    return R, r, rdot, rate.astype(np.float64)


def update(model, cfg, x, P, quat, gyro, dof, contact, accel=None, foot_height=None, gravity=(0.0, 0.0, -9.81), reset=None, p_init=None,
           dtype=np.float64):
    """One wbc_sim_leg_odometry call on a batch, every input given (quat [N, 4], gyro [N, 3], dof [N, 20, 2]; accel / foot_height / p_init
    may be None; reset: None, True or a boolean / integer mask [N]). Returns a dict: x, P, vel_body, nis, status as the call leaves them,
    x_pred / P_pred (the prediction), S, W, y, K and `mag`, a dict of the term sizes of x, P, vel_body, nis (fp64 whatever dtype is)."""
    c = {k: dtype(cfg[k]) for k in CFG_FIELDS}
    x = np.array(x, dtype=dtype); P = np.array(P, dtype=dtype)
    n = x.shape[0]
    dt = c["dt"]
    R, r, rdot, rate = measurement(model, quat, gyro, dof, dtype)
    lreach = reach(model)
    cc = np.clip(np.nan_to_num(np.asarray(contact, dtype=dtype), nan=0.0), 0, 1)
    s = 1 + c["kappa"] * (1 - cc)                                                    # [N, 4]
    g = np.asarray(gravity, dtype=dtype)
    a = np.zeros((n, 3), dtype=dtype)
    a_mag = np.zeros((n, 3))
    if accel is not None:
        acc = np.asarray(accel, dtype=dtype)
        a = np.einsum("nij,nj->ni", R, acc) + g
        a_mag = np.einsum("nij,nj->ni", np.abs(R), np.abs(acc)).astype(np.float64) + np.abs(g).astype(np.float64)
    # predict
    xm = x.copy()
    xm[:, 0:3] = x[:, 0:3] + x[:, 3:6] * dt + dtype(0.5) * a * dt * dt
    xm[:, 3:6] = x[:, 3:6] + a * dt
    ax = np.abs(x).astype(np.float64)
    mag_xm = ax.copy()
    mag_xm[:, 0:3] = ax[:, 0:3] + ax[:, 3:6] * float(dt) + 0.5 * a_mag * float(dt) ** 2
    mag_xm[:, 3:6] = ax[:, 3:6] + a_mag * float(dt)
    A = np.eye(NX, dtype=dtype)
    A[0:3, 3:6] = dt * np.eye(3, dtype=dtype)
    qd = np.empty((n, NX), dtype=dtype)
    qd[:, 0:3] = dt * c["sigma_p"] ** 2; qd[:, 3:6] = dt * c["sigma_v"] ** 2
    qd[:, 6:] = np.repeat(dt * c["sigma_f"] ** 2 * s, 3, axis=1)
    Pm = A @ P @ A.T
    Pm[:, np.arange(NX), np.arange(NX)] += qd
    mag_Pm = A.astype(np.float64) @ np.abs(P).astype(np.float64) @ A.T.astype(np.float64)
    mag_Pm[:, np.arange(NX), np.arange(NX)] += qd.astype(np.float64)
    # correct
    m = 28 if foot_height is not None else 24
    c1, c2, foot, group = rows(m)
    C = selection(m, dtype)
    e = np.empty((n, m), dtype=dtype)
    e[:, 0:12] = (-r - (xm[:, None, 0:3] - xm[:, 6:].reshape(n, 4, 3))).reshape(n, 12)
    e[:, 12:24] = (-rdot - xm[:, None, 3:6]).reshape(n, 12)
    mag_e = np.empty((n, m))
    mag_e[:, 0:12] = (lreach[None, :, None] + mag_xm[:, None, 0:3] + mag_xm[:, 6:].reshape(n, 4, 3)).reshape(n, 12)
    mag_e[:, 12:24] = ((rate * lreach[None, :])[:, :, None] + mag_xm[:, None, 3:6]).reshape(n, 12)
    if m == 28:
        h = np.asarray(foot_height, dtype=dtype)
        e[:, 24:28] = h - xm[:, 8::3]
        mag_e[:, 24:28] = np.abs(h) + mag_xm[:, 8::3]
    sig2 = np.array([c["sigma_r"] ** 2, c["sigma_rdot"] ** 2, c["sigma_z"] ** 2], dtype=dtype)
    Rm = sig2[group][None, :] * s[:, foot]                                           # [N, m]
    CP = C @ Pm                                                                      # (written as a product here; entries are sums of <= 2 entries)
    S = CP @ C.T
    S[:, np.arange(m), np.arange(m)] += Rm
    L, ok = cholesky(S)
    Wy = forward(L, np.concatenate([CP, e[:, :, None]], axis=2))
    W, y = Wy[:, :, :NX], Wy[:, :, NX]
    with np.errstate(all="ignore"):
        xp = xm + np.einsum("nkj,nk->nj", W, y)
        Pp = Pm - np.einsum("nki,nkj->nij", W, W)
        Pp = np.tril(Pp) + np.transpose(np.tril(Pp, -1), (0, 2, 1))                  # one triangle, mirrored
        nis = (y * y).sum(-1)
        # the gain and L^-1 for the term sizes, in fp64
        L64 = np.where(ok[:, None, None], L, np.eye(m, dtype=dtype)).astype(np.float64)
        Linv = forward(L64, np.broadcast_to(np.eye(m), (n, m, m)).copy())
        W64 = np.where(ok[:, None, None], W, 0).astype(np.float64)
        K = np.einsum("nkj,nkl->njl", W64, Linv)                                     # [N, 18, m]
        mag_xp = mag_xm + np.einsum("njl,nl->nj", np.abs(K), mag_e)
        mag_Pp = mag_Pm + np.einsum("nki,nkj->nij", np.abs(W64), np.abs(W64))
        mag_nis = (np.einsum("nkl,nl->nk", np.abs(Linv), mag_e) ** 2).sum(-1)
    bad = ~ok
    status = np.where(bad, STATUS_FAILED, STATUS_OK).astype(np.int32)
    xo = np.where(bad[:, None], xm, xp); Po = np.where(bad[:, None, None], Pm, Pp)
    mag_x = np.where(bad[:, None], mag_xm, mag_xp); mag_P = np.where(bad[:, None, None], mag_Pm, mag_Pp)
    nis = np.where(bad, 0, nis).astype(dtype); mag_nis = np.where(bad, 0.0, mag_nis)
    if reset is not None:
        rs = np.ones(n, dtype=bool) if reset is True else (np.asarray(reset) != 0)
        p0 = np.zeros((n, 3), dtype=dtype) if p_init is None else np.asarray(p_init, dtype=dtype)
        xr = np.concatenate([p0, np.zeros((n, 3), dtype=dtype), (p0[:, None, :] + r).reshape(n, 12)], axis=1)
        mag_xr = np.concatenate([np.abs(p0), np.zeros((n, 3)), (np.abs(p0)[:, None, :] + lreach[None, :, None]).reshape(n, 12)], axis=1)
        Pr = np.diag(np.concatenate([np.full(3, c["p0_p"]), np.full(3, c["p0_v"]), np.full(12, c["p0_f"])]).astype(dtype))
        xo = np.where(rs[:, None], xr, xo); Po = np.where(rs[:, None, None], Pr[None], Po)
        mag_x = np.where(rs[:, None], mag_xr, mag_x); mag_P = np.where(rs[:, None, None], np.abs(Pr)[None].astype(np.float64), mag_P)
        nis = np.where(rs, 0, nis).astype(dtype); mag_nis = np.where(rs, 0.0, mag_nis)
        status = np.where(rs, STATUS_RESET, status).astype(np.int32)
    vel = np.einsum("nji,nj->ni", R, xo[:, 3:6])
    mag_vel = np.einsum("nji,nj->ni", np.abs(R).astype(np.float64), mag_x[:, 3:6])
    return dict(x=xo, P=Po, vel_body=vel, nis=nis, status=status, x_pred=xm, P_pred=Pm, S=S, L=L, W=W, y=y, K=K, e=e, Rm=Rm, R=R, r=r, rdot=rdot,
                mag=dict(x=mag_x, P=mag_P, vel_body=mag_vel, nis=mag_nis))


OUTPUTS = ("x", "P", "vel_body", "nis")


def ratios(got, ref):
    """{output: largest |got - ref| / (2^-24 mag)} over every entry; an entry of size 0 must be met exactly (ratio inf otherwise)."""
    out = {}
    for k in OUTPUTS:
        d = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64))
        mag = ref["mag"][k]
        with np.errstate(all="ignore"):
            q = np.where(mag > 0, d / (EPS * mag), np.where(d == 0, 0.0, np.inf))
        out[k] = float(np.max(q)) if q.size else 0.0
    return out


STAND = (0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 0.8, -1.5, -0.1, 0.8, -1.5) + (0.0,) * 8      # the task's default joint angles


# ---- a consistent log: a base motion over fixed footholds, a trot, legs solved onto their foot targets ----------------------------------
def _euler_quat(roll, pitch, yaw):
    """xyzw of Rz(yaw) Ry(pitch) Rx(roll), batched."""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def consistent_log(model, n, steps, dt, seed=0, gravity=(0.0, 0.0, -9.81), q_stand=STAND):
    """fp64 inputs of `steps` updates for n envs whose base follows a piecewise-constant world acceleration (constant over each update's
    interval) and a smooth orientation history over fixed footholds on the ground z = 0: a trot alternates the diagonal pairs every ten
    updates, swing feet follow arcs to their next footholds, each leg's q comes from Newton's method on its 3 x 3 foot-position
    problem, qd from the same Jacobian, the gyro from the orientation history's derivative; accelerometer and heights are exact.
    Returns a dict of arrays with a leading [steps] axis (the sample at the END of update k's interval) and `p0`, `v0`, `start`:
    the true state and the inputs at time 0 for the reset."""
    rng = np.random.default_rng(seed)
    g = np.asarray(gravity, dtype=np.float64)
    q0 = np.asarray(q_stand, dtype=np.float64)                                        # a stance with bent knees
    fk0 = leg_kinematics(model, q0[None])[0][0]                                        # nominal foot offsets, trunk axes
    # base translation
    seg, pattern = 35, np.array([1.0, -1.0, -1.0, 1.0])                              # the velocity returns to its start every four segments
    amp_a = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([0.7, 0.4, 0.1])
    acc = np.repeat(pattern[np.arange(steps // seg + 1) % 4][:, None, None] * amp_a[None], seg, axis=0)[:steps]
    p = np.zeros((steps + 1, n, 3)); v = np.zeros((steps + 1, n, 3))                  # at rest at time 0: a reset at p0 is the truth
    p[0] = rng.uniform(-1, 1, (n, 3)) * np.array([2.0, 2.0, 0.0]) + np.array([0.0, 0.0, -fk0[:, 2].mean() - 0.03])
    for k in range(steps):
        p[k + 1] = p[k] + v[k] * dt + 0.5 * acc[k] * dt * dt
        v[k + 1] = v[k] + acc[k] * dt
    # orientation: Euler angles as sums of sinusoids, their rates analytic
    t = np.arange(steps + 1)[:, None] * dt
    amp, om, ph = rng.uniform(0.03, 0.12, (3, n)), rng.uniform(0.5, 2.5, (3, n)), rng.uniform(0, 6.28, (3, n))
    amp[2] *= 3
    ang = [amp[i] * np.sin(om[i] * t + ph[i]) for i in range(3)]
    dang = [amp[i] * om[i] * np.cos(om[i] * t + ph[i]) for i in range(3)]
    roll, pitch, yaw = ang
    quat = _euler_quat(roll, pitch, yaw)                                               # [steps + 1, n, 4]
    gyro = np.stack([dang[0] - dang[2] * np.sin(pitch),
                     dang[1] * np.cos(roll) + dang[2] * np.cos(pitch) * np.sin(roll),
                     -dang[1] * np.sin(roll) + dang[2] * np.cos(pitch) * np.cos(roll)], axis=-1)
    R = quat_to_mat(quat.reshape(-1, 4)).reshape(steps + 1, n, 3, 3)
    # feet: world positions and velocities
    half = 10
    foot = np.zeros((steps + 1, n, 4, 3)); fvel = np.zeros((steps + 1, n, 4, 3)); contact = np.ones((steps + 1, n, 4))
    yaw_R = quat_to_mat(_euler_quat(0 * yaw, 0 * yaw, yaw).reshape(-1, 4)).reshape(steps + 1, n, 3, 3)
    nominal = lambda k: p[k][:, None, :] * np.array([1.0, 1.0, 0.0]) + np.einsum("nij,fj->nfi", yaw_R[k], fk0 * np.array([1.0, 1.0, 0.0]))
    hold = nominal(0)
    foot[0] = hold
    pairs = (np.array([0, 3]), np.array([1, 2]))
    for k0 in range(0, steps, half):
        k1 = min(k0 + half, steps)
        sw = pairs[(k0 // half) % 2]
        target = nominal(min(k0 + half + half // 2, steps))                            # where the trunk will be mid-way through the next stance
        for k in range(k0 + 1, k1 + 1):
            foot[k] = hold
            if k0 > 0:                                                                 # the first phase stands on all four
                tau = (k - k0) / half
                foot[k][:, sw] = hold[:, sw] + tau * (target[:, sw] - hold[:, sw])
                foot[k][:, sw, 2] += 0.05 * np.sin(np.pi * tau)
                fvel[k][:, sw] = (target[:, sw] - hold[:, sw]) / (half * dt)
                fvel[k][:, sw, 2] += 0.05 * np.pi * np.cos(np.pi * tau) / (half * dt)
                if k < k0 + half:
                    contact[k][:, sw] = 0.0
                else:
                    fvel[k][:, sw] = 0.0                                               # touches down at the phase's last sample
        if k0 > 0:
            hold = hold.copy(); hold[:, sw] = target[:, sw]
    # legs: fk(q) = R^T (foot - p), Newton from the previous sample's solution
    q = np.zeros((steps + 1, n, 20)); qd = np.zeros((steps + 1, n, 20))
    guess = np.broadcast_to(q0, (n, 20)).copy()
    for k in range(steps + 1):
        want = np.einsum("nji,nfj->nfi", R[k], foot[k] - p[k][:, None, :])
        for _ in range(30):
            fk, _, J, dofs = leg_kinematics(model, guess, jac=True)
            step = np.linalg.solve(J, (want - fk)[..., None])[..., 0]
            for f in range(4):
                guess[:, dofs[f]] += step[:, f]
            if np.abs(step).max() < 1e-15:
                break
        fk, _, J, dofs = leg_kinematics(model, guess, jac=True)
        assert np.abs(fk - want).max() < 1e-13, "a leg did not reach its foot target"
        # R (w_b x fk + J qd) = fvel - v
        rel = np.einsum("nji,nfj->nfi", R[k], fvel[k] - v[k][:, None, :]) - np.cross(gyro[k][:, None, :], fk)
        rate = np.linalg.solve(J, rel[..., None])[..., 0]
        q[k] = guess
        for f in range(4):
            qd[k][:, dofs[f]] = rate[:, f]
    dof = np.stack([q, qd], axis=-1)                                                   # [steps + 1, n, 20, 2]
    accel = np.einsum("knji,knj->kni", R[1:], acc - g)                                 # specific force in the trunk axes at the interval's end
    return dict(quat=quat[1:], gyro=gyro[1:], dof=dof[1:], accel=accel, contact=contact[1:], foot_height=np.zeros((steps, n, 4)),
                p=p[1:], v=v[1:], foot=foot[1:], p0=p[0], v0=v[0], start=dict(quat=quat[0], gyro=gyro[0], dof=dof[0], contact=contact[0]))


def run_log(model, cfg, log, steps, heights=True, gravity=(0.0, 0.0, -9.81), dtype=np.float64, cast=None, each=None):
    """Reset at the true position of time 0 (the log starts at rest), then `steps` updates of the log; `cast` rounds every input (e.g. to fp32) before use. Returns the last update's dict; each(k, out) is called after every update."""
    c = (lambda a: a) if cast is None else cast
    s = log["start"]
    n = log["p0"].shape[0]
    out = update(model, cfg, np.zeros((n, NX)), np.zeros((n, NX, NX)), c(s["quat"]), c(s["gyro"]), c(s["dof"]), c(s["contact"]), gravity=gravity,
                 reset=True, p_init=c(log["p0"]), dtype=dtype)
    x, P = out["x"], out["P"]
    for k in range(steps):
        out = update(model, cfg, x, P, c(log["quat"][k]), c(log["gyro"][k]), c(log["dof"][k]), c(log["contact"][k]), accel=c(log["accel"][k]),
                     foot_height=c(log["foot_height"][k]) if heights else None, gravity=gravity, dtype=dtype)
        x, P = out["x"], out["P"]
        if each is not None:
            each(k, out)
    return out
