"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) statement of what ONE physics substep (physics_substep of
csrc/wbc_step_kernel.hip, shared by wbc_step_kernel and wbc_simulate_kernel; the spec is DESIGN.md section 3) has to satisfy:
the equations of motion, row by row, evaluated at the state the sim stored before and after the substep.

    a   = (nu1 - nu0) / dt,          nu = (v_root, omega_root, qd) in world components (include/wbc_sim.h)
    res = ID_ref(q0, nu0, a) + armature * a - (0_6, tau + t_limit) - sum over feet of J_foot^T (R_b f, R_b t)

ID_ref = tests/inverse_dynamics_reference.py (M a + C nu + g with the env's BODY_PARAMS), J_foot = whole_body_reference.point_jacobian
at the foot sphere's centre, (f, t) the FORCE_SENSOR row, t_limit the joint-limit stop -kappa D/dt^2 viol - [qd viol > 0] delta D/dt qd
with D = 1 / (A^-1)_jj, A = M[6:, 6:] + diag(armature) restricted to the DoFs of joint j's subtree: no articulated-body recursion
anywhere. What is left of res is the rounding of the fp32 evaluation, which is proportional to

    scale = mag + |armature a| + (0_6, |tau| + |t_limit|) + (|M| + diag(armature)) (|nu0| + |nu1|) / dt + sum |J_foot|^T |wrench|
            + (0_6, base_origin_levers),

mag the magnitude vector of ID_ref; the (|nu0| + |nu1|) / dt term is the rounding of the two stored velocities, amplified by the
difference quotient; base_origin_levers is the cancellation of a recursion that takes its moments about the base origin (see
there: found on the forearm-roll row of the step tier, where the base accelerates at 190 rad/s^2). The tests assert |res_k| <= C 2^-24 scale_k.

The file also holds the integrator's restatement, the eligibility mask (which envs the equations above describe), the seeded
states of the case families and the loop that runs them through a sim, so that tests/test_forward_dynamics.py (the C oracle in
both precisions: pins this checker, measures K_ref) and tests/test_gpu_forward_dynamics.py (the HIP kernels) evaluate exactly the
same states. Nothing under wbc_amd imports this file.

K_REF: the fp32 oracle's largest |res| / (2^-24 scale) on exactly the states of each family (measured and asserted by
tests/test_forward_dynamics.py; never taken from the kernel). The kernels' bound is C = 4 x K_ref rounded up to a power of two
(the kernel orders its sums differently and uses the hardware reciprocal), at most 1024."""
import numpy as np

import arm_osc_oracle as ao
import inverse_dynamics_reference as idr
import whole_body_reference as wb

EPS = 2.0 ** -24
NCOL = wb.NCOL
FINGERS = [6 + 18, 6 + 19]
LIVE = [c for c in range(NCOL) if c not in FINGERS]
C_CAP = 1024.0
TILTED_GRAVITY = (0.7, -1.3, -9.5)

# family -> K_ref (fp32 oracle, largest ratio over every eligible env and live row of the family's cases)
K_REF = {"airborne": 6.62, "contact": 9.52, "limit": 5.01, "step": 14.07, "integrator": 3.82}


def bound(family):
    """C of a family: 4 x K_ref rounded up to a power of two."""
    c = 2.0 ** np.ceil(np.log2(4.0 * K_REF[family]))
    assert c <= C_CAP, (family, c)
    return float(c)


# ---------------------------------------------------------------------------------------------------------------- model tables
def tables(wmodel, tcfg):
    """The float32 tables of the wbc_model / wbc_task_cfg the kernel reads, as doubles."""
    arm = np.zeros(NCOL)
    arm[6:6 + len(tcfg.joint_armature)] = [float(x) for x in tcfg.joint_armature]
    return dict(dt=float(tcfg.sim_dt), gravity=[float(x) for x in tcfg.gravity], armature=arm,
                kappa=float(tcfg.limit_kappa), delta=float(tcfg.limit_delta),
                lo=np.array([float(x) for x in wmodel.q_lower]), hi=np.array([float(x) for x in wmodel.q_upper]),
                qd_limit=np.array([float(x) for x in wmodel.qd_limit]), feet_rb=[int(x) for x in wmodel.feet_rb])


def subtree_dofs(model, dof):
    """DoFs of the joints in the subtree of the body that `dof` drives, `dof` included."""
    b = wb.dof_body(model)[dof]
    return sorted(model.body_dof[c] for c in range(1, model.nb) if b in wb.ancestors(model, c))


def joint_inertia(model, M, armature, dof, with_armature=True):
    """D of joint `dof`: the inertia the joint feels with its parent held and its descendants free, from the joint-space inertia of
    its subtree alone (the (j, j) entry of the inverse is 1 / D)."""
    A = M[6:, 6:] + (np.diag(armature[6:]) if with_armature else 0.0)
    idx = subtree_dofs(model, dof)
    return 1.0 / np.linalg.inv(A[np.ix_(idx, idx)])[idx.index(dof), idx.index(dof)]


def limit_torque(model, tb, M, q0, qd0, with_armature=True):
    """t_limit [20] of DESIGN.md section 3, violations against the float32 limits."""
    t = np.zeros(len(q0))
    for d, b in enumerate(wb.dof_body(model)):
        if b < 0 or not tb["lo"][d] < tb["hi"][d]:
            continue
        viol = q0[d] - tb["hi"][d] if q0[d] > tb["hi"][d] else (q0[d] - tb["lo"][d] if q0[d] < tb["lo"][d] else 0.0)
        if viol == 0.0:
            continue
        D = joint_inertia(model, M, tb["armature"], d, with_armature)
        t[d] = -tb["kappa"] * D / tb["dt"] ** 2 * viol
        if qd0[d] * viol > 0:
            t[d] -= tb["delta"] * D / tb["dt"] * qd0[d]
    return t


def _robot_row(root):
    root = np.asarray(root, dtype=np.float64)
    return root[0] if root.ndim == 2 else root


# -------------------------------------------------------------------------------------------------------- equations of motion
def substep_residual(model, wmodel, tcfg, root0, dof0, tau, body_params, root1, dof1, force_sensor, limit_with_armature=True):
    """(res [26], scale [26]) of one env's downloaded fp32 state before (root0 [13] or [2, 13], dof0 [20, 2]) and after one
    substep under the joint torques tau [20]. The locked fingers (rows 24, 25) carry their acceleration, which has to be exactly
    0, over a scale of 0."""
    tb = tables(wmodel, tcfg)
    dt, arm = tb["dt"], tb["armature"]
    r0, r1 = _robot_row(root0), _robot_row(root1)
    dof0, dof1 = np.asarray(dof0, dtype=np.float64), np.asarray(dof1, dtype=np.float64)
    bp = np.asarray(body_params, dtype=np.float64)
    q0 = dof0[:, 0]
    nu0, nu1 = np.r_[r0[7:13], dof0[:, 1]], np.r_[r1[7:13], dof1[:, 1]]
    a = (nu1 - nu0) / dt
    tau = np.asarray(tau, dtype=np.float64).copy()
    tau[[c - 6 for c in FINGERS]] = 0.0
    F = []
    idt, mag = idr.inverse_dynamics(model, r0[0:3], r0[3:7], q0, nu0, a, bp, tb["gravity"], forces=F)
    M = wb.mass_matrix(model, r0[0:3], r0[3:7], q0, bp)
    t_lim = limit_torque(model, tb, M, q0, dof0[:, 1], limit_with_armature)
    res = idt + arm * a - np.r_[np.zeros(6), tau + t_lim]
    scale = mag + np.abs(arm * a) + np.r_[np.zeros(6), np.abs(tau) + np.abs(t_lim)] \
        + (np.abs(M) + np.diag(arm)) @ (np.abs(nu0) + np.abs(nu1)) / dt
    R, p = ao.fk(model, r0[0:3], r0[3:7], q0)
    scale[6:] += base_origin_levers(model, R, p, F)
    fs = np.asarray(force_sensor, dtype=np.float64).reshape(len(tb["feet_rb"]), 6)
    if np.any(fs != 0):
        for ft, rb in enumerate(tb["feet_rb"]):
            if not np.any(fs[ft] != 0):
                continue
            b = model.rb_body[rb]
            J = wb.point_jacobian(model, R, p, b, p[b] + R[b] @ np.asarray(model.rb_offset[rb], dtype=np.float64))
            w = np.r_[R[b] @ fs[ft, 0:3], R[b] @ fs[ft, 3:6]]
            res -= J.T @ w
            scale += np.abs(J).T @ np.abs(w)
    res[FINGERS], scale[FINGERS] = a[FINGERS], 0.0
    return res, scale


def base_origin_levers(model, R, p, F):
    """[20] What taking moments about the BASE origin costs a joint row. An articulated-body recursion that carries its spatial
    vectors about the base origin (the kernel's and the oracle's frame F) forms joint j's torque as axis . (moment of its subtree's
    forces about the base origin) - axis . ((p_j - p_0) x force of the subtree): two terms of size |p_j - p_0| |F| that cancel down
    to the lever about the joint itself, which is all that mag contains. Returned: sum over the bodies c of joint j's subtree of
    |axis_j| . (|p_j - p_0| x |F_c|) with the products of the cross product added, F_c the body's inertia force from ID_ref."""
    out = np.zeros(len(model.dof_names))
    for b in range(1, model.nb):
        ax, d = np.abs(R[b][:, model.axis[b]]), np.abs(p[b] - p[0])
        Fs = sum(np.abs(F[c]) for c in range(1, model.nb) if b in wb.ancestors(model, c))
        out[model.body_dof[b]] = ax @ np.array([d[1] * Fs[2] + d[2] * Fs[1], d[2] * Fs[0] + d[0] * Fs[2], d[0] * Fs[1] + d[1] * Fs[0]])
    return out


def forward_dynamics(model, wmodel, tcfg, root0, dof0, tau, body_params):
    """a_ref [26] of a contact-free substep without the velocity clamp: (M + diag(armature)) a = (0_6, tau + t_limit) - h."""
    tb = tables(wmodel, tcfg)
    r0, dof0 = _robot_row(root0), np.asarray(dof0, dtype=np.float64)
    bp = np.asarray(body_params, dtype=np.float64)
    q0, nu0 = dof0[:, 0], np.r_[r0[7:13], dof0[:, 1]]
    h, _ = idr.bias_forces(model, r0[0:3], r0[3:7], q0, nu0, bp, tb["gravity"])
    M = wb.mass_matrix(model, r0[0:3], r0[3:7], q0, bp)
    tau = np.asarray(tau, dtype=np.float64).copy()
    tau[[c - 6 for c in FINGERS]] = 0.0
    rhs = np.r_[np.zeros(6), tau + limit_torque(model, tb, M, q0, dof0[:, 1])] - h
    a = np.zeros(NCOL)
    a[LIVE] = np.linalg.solve((M + np.diag(tb["armature"]))[np.ix_(LIVE, LIVE)], rhs[LIVE])
    return a


# ------------------------------------------------------------------------------------------------------------------ integrator
def _ratio(err, scale):
    """err / (2^-24 scale); an entry whose scale is 0 has to be exactly 0."""
    out = np.where(err == 0, 0.0, np.inf)
    nz = scale > 0
    out[nz] = err[nz] / (EPS * scale[nz])
    return out


def integrator_errors(tcfg, root0, dof0, root1, dof1):
    """Semi-implicit Euler restated in fp64 from the velocities the sim STORED: q1 = q0 + dt qd1, pos1 = pos0 + dt v1,
    quat1 = normalize(quat0 + dt/2 (omega1, 0) (x) quat0) (xyzw). Returns the three error vectors ([20], [3], [4]), each over
    2^-24 (|x0| + dt |xdot1|)."""
    dt = float(tcfg.sim_dt)
    r0, r1 = _robot_row(root0), _robot_row(root1)
    dof0, dof1 = np.asarray(dof0, dtype=np.float64), np.asarray(dof1, dtype=np.float64)
    eq = _ratio(np.abs(dof1[:, 0] - (dof0[:, 0] + dt * dof1[:, 1])), np.abs(dof0[:, 0]) + dt * np.abs(dof1[:, 1]))
    ep = _ratio(np.abs(r1[0:3] - (r0[0:3] + dt * r1[7:10])), np.abs(r0[0:3]) + dt * np.abs(r1[7:10]))
    wx, wy, wz = r1[10:13]
    x, y, z, w = r0[3:7]
    qdot = 0.5 * np.array([wx * w + wy * z - wz * y, wy * w + wz * x - wx * z, wz * w + wx * y - wy * x, -wx * x - wy * y - wz * z])
    want = r0[3:7] + dt * qdot
    want /= np.linalg.norm(want)
    et = _ratio(np.abs(r1[3:7] - want), np.abs(r0[3:7]) + dt * np.abs(qdot))
    return eq, ep, et


# ----------------------------------------------------------------------------------------------------------------- eligibility
def eligible(wmodel, tcfg, dof0, dof1, net_contact_force, force_sensor, kind):
    """Mask [n] of the envs whose substep the equations above describe. kind: "airborne" (no contact at all: a random pose can
    collide with itself), "limit" (airborne, joints may start outside their limits), "contact" (feet only)."""
    tb = tables(wmodel, tcfg)
    dof0, dof1 = np.asarray(dof0, dtype=np.float64), np.asarray(dof1, dtype=np.float64)
    ncf = np.asarray(net_contact_force, dtype=np.float64)
    fs = np.asarray(force_sensor, dtype=np.float64)
    n = dof0.shape[0]
    clamped = tb["qd_limit"] > 0
    ok = (np.abs(dof1[:, clamped, 1]) < tb["qd_limit"][clamped]).all(1)          # the velocity clamp did not act
    if kind != "limit":
        lim = (tb["lo"] < tb["hi"]) & (np.arange(len(tb["lo"])) < 18)                # (the locked fingers have no stop)
        ok &= ((dof0[:, lim, 0] >= tb["lo"][lim]) & (dof0[:, lim, 0] <= tb["hi"][lim])).all(1)
    other = [rb for rb in range(27) if rb not in tb["feet_rb"]]                     # rows >= 27: the box
    ok &= (ncf[:, other] == 0).reshape(n, -1).all(1)
    if kind != "contact":
        ok &= (ncf == 0).reshape(n, -1).all(1) & (fs == 0).reshape(n, -1).all(1)
    return ok


# ----------------------------------------------------------------------------------------------------------------------- cases
def _park_box(root, z):
    root[:, 1] = 0
    root[:, 1, 0:3] = root[:, 0, 0:3] + np.array([50.0, 0.0, 0.0])
    root[:, 1, 2] = z
    root[:, 1, 6] = 1


def airborne_states(wmodel, tcfg, n, seed, arm_tau=0.3):
    """(root [n, 2, 13], dof [n, 20, 2], tau [n, 20]) float32: 5 m up, random attitude, q = default +- 0.6 clipped 0.05 rad inside
    the limits, |qd| <= 2 (legs) / 1 (arm), |v| <= 1, |omega| <= 2, |tau| <= 10 (legs) / arm_tau (arm); the box 50 m away."""
    rng = np.random.default_rng(seed)
    tb = tables(wmodel, tcfg)
    root = np.zeros((n, 2, 13), dtype=np.float32)
    root[:, 0, 0:2] = rng.uniform(-1, 1, (n, 2))
    root[:, 0, 2] = 5.0
    quat = rng.normal(size=(n, 4))
    root[:, 0, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    root[:, 0, 7:10] = rng.uniform(-1, 1, (n, 3))
    root[:, 0, 10:13] = rng.uniform(-2, 2, (n, 3))
    _park_box(root, 5.0)
    q = np.array([float(x) for x in tcfg.default_dof_pos])[None] + rng.uniform(-0.6, 0.6, (n, 20))
    lim = tb["lo"] < tb["hi"]
    q[:, lim] = np.clip(q[:, lim], tb["lo"][lim] + 0.05, tb["hi"][lim] - 0.05)
    dof = np.zeros((n, 20, 2), dtype=np.float32)
    dof[:, :, 0] = q
    dof[:, :12, 1] = rng.uniform(-2, 2, (n, 12))
    dof[:, 12:18, 1] = rng.uniform(-1, 1, (n, 6))
    dof[:, 18:] = 0
    tau = np.zeros((n, 20), dtype=np.float32)
    tau[:, :12] = rng.uniform(-10, 10, (n, 12))
    tau[:, 12:18] = rng.uniform(-arm_tau, arm_tau, (n, 6))
    return root, dof, tau


def limit_states(wmodel, tcfg, n, seed):
    """The airborne draws with two limited joints per env 0.005 to 0.05 rad beyond a limit (either one)."""
    root, dof, tau = airborne_states(wmodel, tcfg, n, seed)
    rng = np.random.default_rng(seed + 1000)
    tb = tables(wmodel, tcfg)
    limited = np.flatnonzero((tb["lo"] < tb["hi"])[:18])
    for e in range(n):
        for d in rng.choice(limited, 2, replace=False):
            over = rng.uniform(0.005, 0.05)
            dof[e, d, 0] = tb["hi"][d] + over if rng.random() < 0.5 else tb["lo"][d] - over
    return root, dof, tau


def contact_states(tcfg, n, seed):
    """Poses around the stance with the feet at the ground (helpers.random_standing_state: |qd| <= 2), |tau| <= 8 (legs) / 0.3 (arm:
    from 2 rad/s a few N m take the wrist to its pi rad/s clamp within the three substeps), the box 50 m away."""
    import helpers
    rng = np.random.default_rng(seed)
    root, dof = helpers.random_standing_state(n, tcfg, rng, height=(0.28, 0.36))
    _park_box(root, 0.05)
    tau = np.zeros((n, 20), dtype=np.float32)
    tau[:, :12] = rng.uniform(-8, 8, (n, 12))
    tau[:, 12:18] = rng.uniform(-0.3, 0.3, (n, 6))
    return root, dof, tau


# (family, case name, n, seed, gravity, substeps)
SUBSTEP_CASES = [("airborne", "airborne-1", 1, 101, None, 1), ("airborne", "airborne-13", 13, 102, TILTED_GRAVITY, 1),
                 ("airborne", "airborne-256", 256, 103, None, 1), ("contact", "contact-256", 256, 104, None, 3),
                 ("limit", "limit-128", 128, 105, None, 1)]
CLAMP_CASE = dict(n=64, seed=106, arm_tau=10.0)
STEP_CASES = [(13, 107), (2560, 108)]
STEP_COUNT, STEP_SIGMA, STEP_COUNTER = 5, 0.6, 1
MIN_ELIGIBLE = {"airborne": 0.90, "contact": 0.90, "limit": 0.75, "step": 0.90}


def case_states(family, wmodel, tcfg, n, seed):
    if family == "airborne":
        return airborne_states(wmodel, tcfg, n, seed)
    if family == "limit":
        return limit_states(wmodel, tcfg, n, seed)
    return contact_states(tcfg, n, seed)


def with_cfg(tcfg, gravity=None, decimation=None):
    tc = type(tcfg).from_buffer_copy(tcfg)
    if gravity is not None:
        for k in range(3):
            tc.gravity[k] = gravity[k]
    if decimation is not None:
        tc.decimation = decimation
    return tc


def step_envs(n):
    """Every env up to 256 of them; beyond that every tenth plus the last."""
    return list(range(n)) if n <= 256 else sorted(set(range(0, n, 10)) | {n - 1})


def step_actions(n, seed):
    rng = np.random.default_rng(seed)
    return [(STEP_SIGMA * rng.normal(size=(n, 18))).astype(np.float32) for _ in range(STEP_COUNT)]


# -------------------------------------------------------------------------------------------------------- running a sim through
def evaluate(model, wmodel, tcfg, kind, root0, dof0, tau, body_params, root1, dof1, force_sensor, net_contact_force, envs=None,
             skip=None, **kw):
    """One substep of a batch: dict(elig [n], ratio [n, 26] (nan where not evaluated; rows of scale 0: 0 if res is 0, else inf),
    scale [n, 26], integ [n, 27], contacts). envs: the envs to evaluate (default all); skip: mask of envs to leave out."""
    n = np.asarray(dof0).shape[0]
    elig = eligible(wmodel, tcfg, dof0, dof1, net_contact_force, force_sensor, kind)
    if skip is not None:
        elig &= ~np.asarray(skip, dtype=bool)
    ratio, scale, integ = np.full((n, NCOL), np.nan), np.full((n, NCOL), np.nan), np.full((n, 27), np.nan)
    for e in (range(n) if envs is None else envs):
        integ[e] = np.concatenate(integrator_errors(tcfg, root0[e], dof0[e], root1[e], dof1[e]))
        if elig[e]:
            res, scale[e] = substep_residual(model, wmodel, tcfg, root0[e], dof0[e], tau[e], body_params[e], root1[e], dof1[e],
                                             force_sensor[e], **kw)
            ratio[e] = _ratio(np.abs(res), scale[e])
    fs = np.asarray(force_sensor).reshape(n, 4, 6)
    return dict(elig=elig, ratio=ratio, scale=scale, integ=integ, contacts=int((np.abs(fs).sum(-1) > 0)[elig].sum()))


def run_substeps(sim, model, wmodel, tcfg, kind, root, dof, tau, substeps=1):
    """Load the state and the torques into `sim` (an adapter with load / simulate / get) and check every substep from the sim's
    own previous state."""
    sim.load(root, dof, tau)
    bp = sim.get("BODY_PARAMS")
    out = []
    for _ in range(substeps):
        r0, d0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
        sim.simulate()
        out.append(evaluate(model, wmodel, tcfg, kind, r0, d0, tau, bp, sim.get("ROOT_STATES"), sim.get("DOF_STATE"),
                            sim.get("FORCE_SENSOR"), sim.get("NET_CONTACT_FORCE")))
    return out


def run_steps(sim, model, wmodel, tcfg, actions, envs):
    """reset_all, then env steps of ONE substep each (tcfg.decimation == 1): the torques are the TORQUES tensor after the step,
    envs that reset in the step are left out."""
    assert tcfg.decimation == 1
    sim.reset_all()
    sim.set_step_counter(STEP_COUNTER)
    assert tcfg.push_interval == 0 or STEP_COUNTER + len(actions) < tcfg.push_interval            # no push fires
    bp = sim.get("BODY_PARAMS")
    out = []
    for a in actions:
        r0, d0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
        sim.step(a)
        out.append(evaluate(model, wmodel, tcfg, "contact", r0, d0, sim.get("TORQUES"), bp, sim.get("ROOT_STATES"),
                            sim.get("DOF_STATE"), sim.get("FORCE_SENSOR"), sim.get("NET_CONTACT_FORCE"), envs=envs,
                            skip=sim.get("RESET_BUF") != 0))
    return out


def clamp_check(sim, model, wmodel, tcfg):
    """The velocity clamp: airborne states under arm torques of CLAMP_CASE["arm_tau"]. Returns (clamped, free, stored, limit, integ):
    masks [n, 20] of the joints whose fp64 unclamped prediction qd0 + dt a_ref is beyond the limit by more than 1 % / inside it by
    more than 1 %, the stored velocities, the float32 limits with the prediction's sign, and the integrator ratios [n, 27]."""
    n = CLAMP_CASE["n"]
    root, dof, tau = airborne_states(wmodel, tcfg, n, CLAMP_CASE["seed"], CLAMP_CASE["arm_tau"])
    tb = tables(wmodel, tcfg)
    sim.load(root, dof, tau)
    bp = sim.get("BODY_PARAMS")
    r0, d0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
    sim.simulate()
    r1, d1 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
    assert not np.any(sim.get("NET_CONTACT_FORCE")[:, :27] != 0)
    lim = tb["qd_limit"]
    pred = np.array([d0[e, :, 1] + tb["dt"] * forward_dynamics(model, wmodel, tcfg, r0[e], d0[e], tau[e], bp[e])[6:] for e in range(n)])
    has = lim > 0
    clamped = has & (np.abs(pred) > 1.01 * lim)
    free = ~has | (np.abs(pred) < 0.99 * lim)
    integ = np.array([np.concatenate(integrator_errors(tcfg, r0[e], d0[e], r1[e], d1[e])) for e in range(n)])
    return clamped, free, d1[:, :, 1], np.sign(pred) * lim, integ


class OracleAdapter:
    """The C oracle behind the load / simulate / step / get interface of the loops above."""

    def __init__(self, o):
        self.o = o

    def get(self, name):
        return self.o.get(name)

    def load(self, root, dof, tau):
        self.o.set("ROOT_STATES", root); self.o.set("DOF_STATE", dof); self.o.set("TORQUES", tau)

    def simulate(self):
        self.o.simulate()

    def reset_all(self):
        self.o.reset_all()

    def set_step_counter(self, v):
        self.o.step_counter = v

    def step(self, a):
        self.o.step(a)
