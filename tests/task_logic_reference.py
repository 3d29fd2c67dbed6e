"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) restatement of the TASK LOGIC of one env step: everything wbc_step_kernel does after
its substeps (compute_reward, base_reward_sums, reward_accumulate, the air-time state, observe_and_store of
csrc/wbc_step_kernel.hip; compute_reward / compute_observations of oracle/wbc_oracle.c), written from the reference's reward
functions (WG = legged_gym/envs/widowGo1/widowGo1.py, LR = legged_gym/envs/base/legged_robot.py; the line numbers are cited where
the expressions stand) and evaluated ON THE SIM'S OWN POST-STATE: every input is a tensor the step itself stored (TORQUES,
DOF_STATE, ROOT_STATES, ACTIONS, COMMANDS, GOAL_STATE, BASE_LIN_VEL, BASE_ANG_VEL, FORCE_SENSOR, NET_CONTACT_FORCE,
RIGID_BODY_STATE) or was given before it (LAST_ACTIONS, LAST_DOF_VEL, FEET_AIR_TIME, LAST_CONTACTS, OBS_HISTORY). The rounding of
the physics drops out; what is left between the sim's fp32 value and this file's fp64 value is the rounding of the term itself:

    |sim - ref| <= C 2^-24 mag

mag is carried next to every value by the class V below: a sum adds the absolute sizes of its summands to their mags, a product
the size of the product, and a function passes the mag of its argument on through its first-order sensitivity (exp:
value (1 + mag_arg); atan2(y, x): (mag_y |x| + mag_x |y|) / (x^2 + y^2) + |angle|; sqrt, sin, cos likewise). Inputs are exact (mag 0).
abs / min / max / clamp are 1-Lipschitz and pass the mag on unchanged (a clamp that acts by more than 4096 roundings returns its
bound exactly: mag 0). Discontinuous pieces (the collision count at |f| > 0.1,
the foot contact f_z > 1, the stumble ratio 5, the observation's contact flags |wrench| > 1.5, the |cmd_xy| gates at 0.1, the
seam of a wrapped angle) are compared exactly; an env within a relative 1e-5 of such a threshold is flagged `near` for the terms
that pass through it and left out for those terms only.

How the raw terms are read out of a sim: a curriculum with leg_reward_scale = 1 for all 37 terms, leg_active_mask = 2^37 - 1,
arm_active_mask = 0 and zeroed EPISODE_SUMS / METRIC_SUMS before the step leave the raw term t in EPISODE_SUMS[e, t] and the metric
sources in METRIC_SUMS[e, m], for the envs that did not reset (unit_curriculum, run_steps).

The file also holds the case builders (seeds, states, curricula, task-config variants) and the loops, so that
tests/test_task_logic.py (C oracle in both precisions on the CPU: pins this checker, measures K_ref) and
tests/test_gpu_task_logic.py (the HIP step kernel) evaluate exactly the same states. Nothing under wbc_amd imports this file.

K_REF: the fp32 oracle's largest |sim - ref| / (2^-24 mag) per tier on the cases below (measured and asserted by
tests/test_task_logic.py, never taken from the kernel). C = 4 x K_ref rounded up to a power of two, at least 8 for the tiers that
pass through a transcendental (the kernel's cephes / hardware exp2, atan, sincos are in the 1-2 ulp class where libm is <= 1)."""
import numpy as np

from wbc_amd import abi

EPS = 2.0 ** -24
NREW, NMET, NPROP, NPRIV, HIST, NDOF, NACT = abi.NREW, abi.NMETRIC, abi.NPROP, abi.NPRIV, abi.HIST, abi.NDOF, abi.NACT
TERM = {name: i for i, name in enumerate(abi.REWARD_TERMS)}
ALL_MASK = (1 << NREW) - 1
NEAR = 1e-5
G_START, G_GOAL, G_GOAL_CART, G_CURR, G_CURR_CART, G_DORN, G_ORN, G_TIMER, G_TRAJ, G_TOTAL = 0, 3, 6, 9, 12, 15, 18, 21, 22, 23
POLICY_PERM = [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8, 12, 13, 14, 15, 16, 17, 18, 19]       # ig2raisim (WG:1003-1030)
FEET_PERM = [1, 0, 3, 2]
# metric slot (abi.METRIC_NAMES order) -> the reward functions that add to it as a side effect (WG:1357 ... 1468)
MET_TERMS = [["leg_energy_abs_sum"], ["tracking_lin_vel_x_l1", "tracking_lin_vel_x_exp"], ["tracking_ang_vel_yaw_exp"],
             ["tracking_ee_cart"], ["tracking_ee_sphere"], ["tracking_ee_orn_ry"], ["hip_action_l2", "leg_action_l2"], ["torques"],
             ["energy_square"], ["foot_contacts_z"]]

TIERS = ["poly", "exp", "angle", "totals", "obs_scaled", "obs_euler"]
TIER_FLOOR = {"poly": 1.0, "exp": 8.0, "angle": 8.0, "totals": 1.0, "obs_scaled": 1.0, "obs_euler": 8.0}
EXP_TERMS = ["tracking_lin_vel_x_exp", "tracking_ang_vel_yaw_exp", "tracking_lin_vel", "tracking_ang_vel"]
ANGLE_TERMS = ["tracking_ee_sphere", "tracking_ee_cart", "tracking_ee_orn", "tracking_ee_orn_ry"]
TERM_TIER = ["angle" if t in ANGLE_TERMS else ("exp" if t in EXP_TERMS else "poly") for t in abi.REWARD_TERMS]
MET_TIER = ["poly", "poly", "poly", "angle", "angle", "angle", "poly", "poly", "poly", "poly"]
# tier -> K_ref (fp32 oracle, largest ratio over every checked env-step of the cases below)
K_REF = {"poly": 2.72, "exp": 0.65, "angle": 0.33, "totals": 1.0, "obs_scaled": 0.95, "obs_euler": 0.56}


def bound(tier):
    """C of a tier: 4 x K_ref rounded up to a power of two, not below the tier's floor."""
    return float(max(TIER_FLOOR[tier], 2.0 ** np.ceil(np.log2(4.0 * max(K_REF[tier], 2.0 ** -20)))))


def term_bounds():
    return np.array([bound(t) for t in TERM_TIER])


# ------------------------------------------------------------------------------------------------ values that carry their mag
class V:
    """An fp64 value (array) with the magnitude its fp32 evaluation's rounding error is proportional to."""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.zeros_like(self.v) if m is None else np.asarray(m, dtype=np.float64)

    def __getitem__(self, idx):
        return V(self.v[idx], self.m[idx])


def lift(x):
    return x if isinstance(x, V) else V(x)


def add(*xs):
    xs = [lift(x) for x in xs]
    return V(sum(x.v for x in xs), sum(x.m for x in xs) + sum(np.abs(x.v) for x in xs))


def neg(a):
    return V(-a.v, a.m)


def sub(a, b):
    return add(a, neg(lift(b)))


def mul(a, b):
    a, b = lift(a), lift(b)
    return V(a.v * b.v, a.m * np.abs(b.v) + b.m * np.abs(a.v) + np.abs(a.v * b.v))


def sq(a):
    return mul(a, a)


def half(a):
    return V(0.5 * a.v, 0.5 * a.m)                      # (exact in binary)


def vabs(a):
    return V(np.abs(a.v), a.m)


def vsum(a, axis=-1):
    return V(a.v.sum(axis), a.m.sum(axis) + np.abs(a.v).sum(axis))


def vsqrt(a):
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return V(v, np.where(v > 0, a.m / (2 * v), np.sqrt(a.m)) + v)


def vexp(a):
    v = np.exp(a.v)
    return V(v, v * (1.0 + a.m))


def vsin(a):
    return V(np.sin(a.v), np.abs(np.cos(a.v)) * a.m + np.abs(np.sin(a.v)))


def vcos(a):
    return V(np.cos(a.v), np.abs(np.sin(a.v)) * a.m + np.abs(np.cos(a.v)))


def vatan2(y, x):
    y, x = lift(y), lift(x)
    ang = np.arctan2(y.v, x.v)
    r2 = x.v ** 2 + y.v ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return V(ang, np.where(r2 > 0, (y.m * np.abs(x.v) + x.m * np.abs(y.v)) / r2, 0.0) + np.abs(ang))


def vclip(a, lo, hi):
    """clamp: 1-Lipschitz, the mag passes through -- except where the argument lies beyond a bound by more than 2^-12 of its mag
    (4096 roundings): there the result IS the bound, exactly."""
    v = np.clip(a.v, lo, hi)
    return V(v, np.where(np.abs(a.v - v) > 2.0 ** -12 * a.m, 0.0, a.m))


def vwhere(c, a, b):
    a, b = lift(a), lift(b)
    return V(np.where(c, a.v, b.v), np.where(c, a.m, b.m))


def vwrap(a):
    """torch_wrap_to_pi_minuspi: (a + pi) mod 2 pi - pi. Returns (value, near the seam)."""
    t = (a.v + np.pi) / (2 * np.pi)
    k = np.floor(t)
    v = a.v - 2 * np.pi * k
    frac = t - k
    return V(v, a.m + np.abs(a.v) + 2 * np.pi * (1 + np.abs(k)) + 2 * np.abs(v)), (frac < NEAR) | (frac > 1 - NEAR)


def vstack(xs, axis=-1):
    xs = [lift(x) for x in xs]
    return V(np.stack([x.v for x in xs], axis), np.stack([x.m for x in xs], axis))


def euler_from_quat(q):
    """(roll, pitch, yaw) of an xyzw quaternion [n, 4] as V (isaacgym's euler_from_quat; the pitch's arcsine as the arctangent
    atan2(s, sqrt((1 - s)(1 + s))), whose conditioning it shares)."""
    x, y, z, w = [V(q[:, i]) for i in range(4)]
    roll = vatan2(mul(2.0, add(mul(w, x), mul(y, z))), sub(1.0, mul(2.0, add(sq(x), sq(y)))))
    sp = vclip(mul(2.0, sub(mul(w, y), mul(z, x))), -1.0, 1.0)
    pitch = vatan2(sp, vsqrt(vclip(mul(sub(1.0, sp), add(1.0, sp)), 0.0, None)))
    yaw = vatan2(mul(2.0, add(mul(w, z), mul(x, y))), sub(1.0, mul(2.0, add(sq(y), sq(z)))))
    return roll, pitch, yaw


def quat_rotate_inverse(q, v):
    """q: 4 V (xyzw), v: 3 V -> 3 V; isaacgym's formula a - b + c (the sims evaluate the same one)."""
    qv, w = q[:3], q[3]
    ww = sub(mul(2.0, sq(w)), 1.0)
    cr = [sub(mul(qv[1], v[2]), mul(qv[2], v[1])), sub(mul(qv[2], v[0]), mul(qv[0], v[2])), sub(mul(qv[0], v[1]), mul(qv[1], v[0]))]
    d = mul(2.0, add(mul(qv[0], v[0]), mul(qv[1], v[1]), mul(qv[2], v[2])))
    return [add(mul(v[i], ww), neg(mul(mul(cr[i], w), 2.0)), mul(qv[i], d)) for i in range(3)]


# ---------------------------------------------------------------------------------------------------------------- model tables
def tables(wmodel, tcfg):
    """The float32 tables of wbc_model / wbc_task_cfg the task logic reads, as doubles."""
    f = lambda a: np.array([float(x) for x in a])
    dt32 = np.float32(tcfg.sim_dt) * np.float32(tcfg.decimation)
    return dict(dt=float(dt32), sigma=float(tcfg.tracking_sigma), ee_sigma=float(tcfg.tracking_ee_sigma),
                sphere_scale=f(tcfg.sphere_error_scale), orn_scale=f(tcfg.orn_error_scale), zoff=float(tcfg.z_invariant_offset),
                soft_lo=f(tcfg.soft_dof_lower), soft_hi=f(tcfg.soft_dof_upper), soft_vel=f(tcfg.soft_dof_vel_limit),
                soft_tau=f(tcfg.soft_torque_limit), default=f(tcfg.default_dof_pos), max_contact_force=float(tcfg.max_contact_force),
                base_height_target=float(tcfg.base_height_target), penalize=int(tcfg.penalize_contact_rb_mask),
                feet_rb=[int(x) for x in wmodel.feet_rb], gripper_rb=int(wmodel.gripper_rb), only_positive=int(tcfg.only_positive_rewards),
                s_ang_vel=float(tcfg.obs_scale_ang_vel), s_dof_pos=float(tcfg.obs_scale_dof_pos), s_dof_vel=float(tcfg.obs_scale_dof_vel),
                s_cmd=f(tcfg.commands_scale), clip_obs=float(tcfg.clip_obs), clip_actions=float(tcfg.clip_actions),
                cart=int(tcfg.goal_command_cart), init_quat=f(tcfg.base_init_state)[3:7], action_delay=int(tcfg.action_delay))


# ------------------------------------------------------------------------------------------------------------ the reward terms
def reward_terms(tb, pre, post, air_on=True, envs=None, drop_torque_dof=None, keep_pitch_in_ry=False, sigma=None):
    """All 37 raw terms of one env-step (abi.REWARD_TERMS order) from the stored post-state `post` and the pre-step tensors `pre`.
    Returns dict(val [n, 37], mag [n, 37], near [n, 37], src (V [n, 37]: the metric side effect of each term, 0 where it has
    none), air (V [n, 4]), last_contacts [n, 4], air_near [n, 4]). envs: rows to evaluate (default all). The last three arguments
    seed WRONG formulas (tests/test_task_logic.py: the checker can fail)."""
    sel = (lambda a: np.asarray(a, dtype=np.float64)) if envs is None else (lambda a: np.asarray(a, dtype=np.float64)[envs])
    tau, dof, act = sel(post["TORQUES"]), sel(post["DOF_STATE"]), sel(post["ACTIONS"])
    q, qd = dof[:, :, 0], dof[:, :, 1]
    cmd, blv, bav, goal = sel(post["COMMANDS"]), sel(post["BASE_LIN_VEL"]), sel(post["BASE_ANG_VEL"]), sel(post["GOAL_STATE"])
    fs, ncf, rb = sel(post["FORCE_SENSOR"]).reshape(-1, 4, 6), sel(post["NET_CONTACT_FORCE"]), sel(post["RIGID_BODY_STATE"])
    root = sel(post["ROOT_STATES"])[:, 0]
    n = tau.shape[0]
    sigma = tb["sigma"] if sigma is None else sigma
    val, mag, near = np.zeros((n, NREW)), np.zeros((n, NREW)), np.zeros((n, NREW), bool)
    src = V(np.zeros((n, NREW)))

    def put(name, x, nr=None, s=None):
        t = TERM[name]
        val[:, t], mag[:, t] = x.v, x.m
        if nr is not None:
            near[:, t] = nr
        if s is not None:
            src.v[:, t], src.m[:, t] = s.v, s.m

    p = mul(tau[:, :12], qd[:, :12])
    e2 = vsum(sq(p))
    put("energy_square", e2, s=e2)                                                              # WG:1466-1469
    put("survive", V(np.ones(n)))                                                               # WG:1452
    ex = vabs(sub(cmd[:, 0], blv[:, 0]))
    put("tracking_lin_vel_x_l1", add(neg(ex), np.abs(cmd[:, 0])), s=ex)                         # WG:1427-1430
    put("tracking_lin_vel_x_exp", vexp(mul(neg(ex), 1.0 / sigma)), s=ex)                        # WG:1432-1435
    eyaw = vabs(sub(cmd[:, 2], bav[:, 2]))
    put("tracking_ang_vel_yaw_exp", vexp(mul(neg(eyaw), 1.0 / sigma)), s=eyaw)                  # WG:1441-1444
    put("tracking_ang_vel_yaw_l1", add(neg(eyaw), np.abs(cmd[:, 2])))                           # WG:1437-1439
    hip = vsum(sq(V(act[:, [0, 3, 6, 9]])))
    put("hip_action_l2", hip, s=hip)                                                            # WG:1379-1382
    fz = vsum(sq(V(fs[:, :, 2])))
    put("foot_contacts_z", fz, s=fz)                                                            # WG:1455-1458
    # base_yaw_quat (WG:882-884): the yaw of the base, then (0, 0, sin, cos) of its half
    _, _, yaw = euler_from_quat(root[:, 3:7])
    zero = V(np.zeros(n))
    yq = [zero, zero, vsin(half(yaw)), vcos(half(yaw))]
    ee = rb[:, tb["gripper_rb"]]
    rel = [sub(ee[:, 0], root[:, 0]), sub(ee[:, 1], root[:, 1]), sub(ee[:, 2], tb["zoff"])]
    loc = quat_rotate_inverse(yq, rel)                                                          # WG:1353
    h2 = add(sq(loc[0]), sq(loc[1]))
    sph = [vsqrt(add(h2, sq(loc[2]))), vatan2(loc[2], vsqrt(h2)), vatan2(loc[1], loc[0])]      # cart2sphere: asin(z / l) = atan2(z, |xy|)
    es = add(*[mul(vabs(sub(sph[j], goal[:, G_CURR + j])), tb["sphere_scale"][j]) for j in range(3)])
    put("tracking_ee_sphere", vexp(mul(neg(es), 1.0 / tb["ee_sigma"])), s=es)                   # WG:1352-1358
    tw = quat_rotate_inverse([zero, zero, neg(yq[2]), yq[3]], [V(goal[:, G_CURR_CART + j]) for j in range(3)])   # quat_apply
    tgt = [add(root[:, 0], tw[0]), add(root[:, 1], tw[1]), add(tb["zoff"], tw[2])]
    ec = add(*[vabs(sub(ee[:, j], tgt[j])) for j in range(3)])
    put("tracking_ee_cart", vexp(mul(neg(ec), 1.0 / tb["ee_sigma"])), s=ec)                     # WG:1360-1366
    eul = euler_from_quat(ee[:, 3:7])
    d, seam = zip(*[vwrap(sub(goal[:, G_ORN + j], eul[j])) for j in range(3)])
    eo = add(*[mul(vabs(d[j]), tb["orn_scale"][j]) for j in range(3)])
    ry = [0, 1, 2] if keep_pitch_in_ry else [0, 2]
    eo_ry = add(*[vabs(mul(d[j], tb["orn_scale"][j])) for j in ry])
    put("tracking_ee_orn", vexp(mul(neg(eo), 1.0 / tb["ee_sigma"])))                            # WG:1368-1377 (the seam: |d| is continuous across it)
    put("tracking_ee_orn_ry", vexp(mul(neg(eo_ry), 1.0 / tb["ee_sigma"])), s=eo_ry)             # WG:1384-1393
    eabs = vsum(vabs(p))
    put("leg_energy_abs_sum", eabs, s=eabs)                                                     # WG:1396-1399
    put("leg_energy_sum_abs", vabs(vsum(p)))                                                    # WG:1401-1403
    al2 = vsum(sq(V(act[:, :12])))
    put("leg_action_l2", al2, s=al2)                                                            # WG:1405-1408
    put("leg_energy", vsum(p))                                                                  # WG:1410-1412
    put("arm_energy_abs_sum", vsum(vabs(mul(tau[:, 12:NDOF - 2], qd[:, 12:NDOF - 2]))))         # WG:1414-1415
    dx, dy, dz = [sub(cmd[:, j], blv[:, j]) for j in range(3)]
    put("tracking_lin_vel", vexp(mul(neg(add(sq(dx), sq(dy))), 1.0 / sigma)))                   # WG:1422-1425
    put("tracking_lin_vel_y_l2", sq(dy))                                                        # WG:1446-1447
    put("tracking_lin_vel_z_l2", sq(dz))                                                        # WG:1449-1450
    tq_dofs = [j for j in range(NDOF) if j != drop_torque_dof]
    tq2 = vsum(sq(V(tau[:, tq_dofs])))
    put("torques", tq2, s=tq2)                                                                  # WG:1460-1464
    pen = [r for r in range(abi.NRB) if (tb["penalize"] >> r) & 1]
    fn = np.linalg.norm(ncf[:, pen], axis=-1)
    put("collision", V((fn > 0.1).sum(1).astype(float)), nr=(np.abs(fn / 0.1 - 1.0) < NEAR).any(1))   # LR:865-867
    # ---- the base class's terms
    put("lin_vel_z", sq(V(blv[:, 2])))                                                          # LR:832-834
    put("ang_vel_xy", vsum(sq(V(bav[:, :2]))))                                                  # LR:836-838
    put("dof_vel", vsum(sq(V(qd))))                                                             # LR:853-855
    put("dof_acc", vsum(sq(mul(sub(sel(pre["LAST_DOF_VEL"]), qd), 1.0 / tb["dt"]))))            # LR:857-859
    put("action_rate", vsum(sq(sub(sel(pre["LAST_ACTIONS"]), act))))                            # LR:861-863
    put("termination", V(((sel(post["RESET_BUF"]) != 0) & (sel(post["TIME_OUT_BUF"]) == 0)).astype(float)))      # LR:869-871
    below, above = sub(q, tb["soft_lo"][None]), sub(q, tb["soft_hi"][None])
    put("dof_pos_limits", vsum(add(neg(vclip(below, None, 0.0)), vclip(above, 0.0, None))))     # LR:873-877
    put("dof_vel_limits", vsum(vclip(sub(np.abs(qd), tb["soft_vel"][None]), 0.0, 1.0)))         # LR:879-882
    put("torque_limits", vsum(vclip(sub(np.abs(tau), tb["soft_tau"][None]), 0.0, None)))        # LR:884-886
    put("tracking_ang_vel", vexp(mul(neg(sq(sub(cmd[:, 2], bav[:, 2]))), 1.0 / sigma)))         # LR:893-896
    cmd_xy = np.hypot(cmd[:, 0], cmd[:, 1])
    gate_near = np.abs(cmd_xy / 0.1 - 1.0) < NEAR
    still = vsum(vabs(sub(q, tb["default"][None])))
    put("stand_still", vwhere(cmd_xy < 0.1, still, 0.0), nr=gate_near)                          # LR:916-918
    ff = ncf[:, tb["feet_rb"]]
    hxy = np.hypot(ff[:, :, 0], ff[:, :, 1])
    put("stumble", V((hxy > 5 * np.abs(ff[:, :, 2])).any(1).astype(float)),
        nr=((np.abs(hxy - 5 * np.abs(ff[:, :, 2])) <= NEAR * hxy) & (hxy > 0)).any(1))          # LR:911-914
    fnorm = vsqrt(vsum(sq(V(ff))))
    put("feet_contact_forces", vsum(vclip(sub(fnorm, tb["max_contact_force"]), 0.0, None)))     # LR:920-922
    put("base_height", sq(sub(root[:, 2], tb["base_height_target"])))                           # LR:844-847 (measured_heights = 0, WG:639)
    # feet_air_time (LR:898-909); its state only advances while the function is in a reward list
    at0, lc0 = sel(pre["FEET_AIR_TIME"]), sel(pre["LAST_CONTACTS"])
    if air_on:
        contact = ff[:, :, 2] > 1.0
        c_near = np.abs(ff[:, :, 2] - 1.0) < NEAR
        filt = contact | (lc0 != 0)
        first = (at0 > 0) & filt
        at = add(at0, tb["dt"])
        rew = vsum(vwhere(first, sub(at, 0.5), 0.0))
        put("feet_air_time", vwhere(cmd_xy > 0.1, rew, 0.0), nr=gate_near | c_near.any(1))
        air, lc, air_near = vwhere(filt, 0.0, at), contact.astype(float), c_near
    else:
        air, lc, air_near = V(at0), lc0, np.zeros_like(at0, bool)
    return dict(val=val, mag=mag, near=near, src=src, air=air, last_contacts=lc, air_near=air_near)


def metric_sources(T, lmask, amask):
    """What one step adds to METRIC_SUMS [n, 10] (V): each ACTIVE call of a reward function adds its side effect once, per channel."""
    n = T["val"].shape[0]
    out = V(np.zeros((n, NMET)))
    for m, names in enumerate(MET_TERMS):
        parts = [T["src"][:, TERM[t]] for mask in (lmask, amask) for t in names if (mask >> TERM[t]) & 1]
        if parts:
            s = add(*parts) if len(parts) > 1 else parts[0]
            out.v[:, m], out.m[:, m] = s.v, s.m
    return out


TINY = 2.0 ** -126


def ratio(err, scale):
    """err / (2^-24 scale); an entry whose scale is 0 has to be exact. fp32 underflow is not held against anyone: a result below
    the smallest normal number (exp(-90) of a spinning robot's tracking term) loses bits or is flushed to zero, so 2^-126 is
    taken off the error first."""
    err, scale = np.maximum(np.asarray(err, dtype=np.float64) - TINY, 0.0), np.asarray(scale, dtype=np.float64)
    out = np.where(err == 0, 0.0, np.inf)
    nz = scale > 0
    out[nz] = err[nz] / (EPS * scale[nz])
    return out


def reward_totals(tb, T, cur, term_C, termination_before_clip=False, arm_first=False):
    """The two reward totals (WG:170-205) and the episode-sum increments from the fp64 terms T under the curriculum `cur`
    (dict lsc, asc [37], lmask, amask). Per channel: sum of term x scale over the channel's list without termination, the
    only_positive_rewards clip, THEN termination, / 100. Returns dict(rew, arm_rew [n], allow, arm_allow [n]: the scale-weighted
    sum of the terms' own bounds / 100, size, arm_size [n]: sum |scale term| / 100, kink, arm_kink [n]: the unclipped total lies
    within its bound of 0 (C_totals = bound("totals")), leg, arm (V [n, 37]: the two increments of EPISODE_SUMS per slot))."""
    out = {}
    tt = TERM["termination"]
    for ch, sc, mask in (("", cur["lsc"], cur["lmask"]), ("arm_", cur["asc"], cur["amask"])):
        bits = np.array([(mask >> t) & 1 for t in range(NREW)], dtype=bool)
        sc = np.where(bits, np.asarray(sc, dtype=np.float64), 0.0)
        contrib = T["val"] * sc[None]
        allow = (np.abs(sc)[None] * term_C[None] * EPS * T["mag"]).sum(1)
        size = np.abs(contrib).sum(1)
        body = bits.copy()
        if not termination_before_clip:
            body[tt] = False
        s = contrib[:, body].sum(1)
        kink = np.zeros(len(s), bool)
        if tb["only_positive"]:
            kink = np.abs(s) <= allow + bound("totals") * EPS * size
            s = np.maximum(s, 0.0)
        if bits[tt] and not termination_before_clip:
            s = s + contrib[:, tt]
        out[ch + "rew"], out[ch + "allow"], out[ch + "size"], out[ch + "kink"] = s / 100.0, allow / 100.0, size / 100.0, kink
        out["arm" if ch else "leg"] = V(contrib, np.abs(sc)[None] * T["mag"] + np.abs(contrib))
        out[(ch or "leg_") + "clipped"] = (contrib[:, body].sum(1) < 0) & bool(tb["only_positive"])
    if arm_first:
        out["leg"], out["arm"] = out["arm"], out["leg"]
    return out


# ---------------------------------------------------------------------------------------------------------- the observation
OBS_EXACT, OBS_SCALED, OBS_EULER, OBS_WRAPPED, OBS_FLAG = 0, 1, 2, 3, 4


def obs_kinds():
    k = np.zeros(NPROP, dtype=int)
    k[0:2] = OBS_EULER
    k[2:45] = OBS_SCALED
    k[5 + POLICY_PERM.index(NDOF - 8)] = OBS_WRAPPED
    k[63:67] = OBS_FLAG
    k[67:70] = OBS_SCALED
    return k


def proprio(tb, post, envs=None):
    """The 76 proprioceptive entries (WG:966-982) from the stored post-state: V [n, 76], near [n, 76]. For an env that reset in the
    step the stored state IS the new episode's (WG:898-900: reset_idx runs before compute_observations); its roll / pitch are those
    of base_init_state's quaternion (the root the reset wrote has them), its action entries are 0 (WG:738)."""
    sel = (lambda a: np.asarray(a, dtype=np.float64)) if envs is None else (lambda a: np.asarray(a, dtype=np.float64)[envs])
    dof, cmd, bav, goal = sel(post["DOF_STATE"]), sel(post["COMMANDS"]), sel(post["BASE_ANG_VEL"]), sel(post["GOAL_STATE"])
    fs, root, ah = sel(post["FORCE_SENSOR"]).reshape(-1, 4, 6), sel(post["ROOT_STATES"])[:, 0], sel(post["ACTION_HISTORY"])
    reset = sel(post["RESET_BUF"]) != 0
    n = dof.shape[0]
    o, near = V(np.zeros((n, NPROP))), np.zeros((n, NPROP), bool)

    def put(sl, x):
        o.v[:, sl], o.m[:, sl] = x.v, x.m

    quat = np.where(reset[:, None], tb["init_quat"][None], root[:, 3:7])
    r, p, _ = euler_from_quat(quat)
    put(slice(0, 2), vstack([r, p]))                                                            # WG:973, 1101-1106
    put(slice(2, 5), mul(bav, tb["s_ang_vel"]))                                                 # WG:974
    qp = dof[:, POLICY_PERM, 0]
    w, seam = vwrap(V(qp[:, POLICY_PERM.index(NDOF - 8)]))                                      # WG:970
    j = POLICY_PERM.index(NDOF - 8)
    qv = V(qp.copy())
    qv.v[:, j], qv.m[:, j] = w.v, w.m
    near[:, 5 + j] = seam
    put(slice(5, 25), mul(sub(qv, tb["default"][POLICY_PERM][None]), tb["s_dof_pos"]))          # WG:975
    put(slice(25, 45), mul(dof[:, POLICY_PERM, 1], tb["s_dof_vel"]))                            # WG:976
    put(slice(45, 63), V(ah[:, -1][:, POLICY_PERM[:NACT]]))                                     # WG:977 (zeroed by a reset, WG:738)
    nrm = np.linalg.norm(fs[:, FEET_PERM], axis=-1)
    put(slice(63, 67), V((nrm > 1.5).astype(float)))                                            # WG:978, 1095
    near[:, 63:67] = np.abs(nrm / 1.5 - 1.0) < NEAR
    put(slice(67, 70), mul(cmd, tb["s_cmd"][None]))                                             # WG:979
    g0 = G_CURR_CART if tb["cart"] else G_CURR
    put(slice(70, 73), V(goal[:, g0:g0 + 3]))                                                   # WG:980, 589-593
    put(slice(73, 76), V(goal[:, G_DORN:G_DORN + 3]))                                           # WG:981
    return o, near


def ulps(got, ref):
    """|got - ref| in units of the float32 spacing at ref."""
    ref32 = np.abs(np.asarray(ref, dtype=np.float64)).astype(np.float32)
    sp = np.spacing(np.maximum(ref32, np.float32(2.0 ** -126))).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)) / sp


def check_observation(tb, pre, post, actions, envs=None):
    """Everything observe_and_store leaves behind, against the restatement. Returns dict(exact_bad: list of messages about entries
    that have to be bit-identical and are not; ulp: largest error of the one / two-rounding entries in float32 ulps;
    ratio_scaled / ratio_euler: largest |sim - ref| / (2^-24 mag) of tiers 5 / 6 with (env, entry); near: entries left out;
    clipped: entries of OBS_BUF at +-clip_obs per block (proprio, priv, history); resets, refills: env counts)."""
    idx = np.arange(np.asarray(post["RESET_BUF"]).shape[0]) if envs is None else np.asarray(envs)
    sel = lambda a: np.asarray(a, dtype=np.float64)[idx]
    o, near = proprio(tb, post, idx)
    obs, hist1, hist0 = sel(post["OBS_BUF"]), sel(post["OBS_HISTORY"]), sel(pre["OBS_HISTORY"])
    reset, eplen = sel(post["RESET_BUF"]) != 0, sel(post["EPISODE_LENGTH"])
    clipv = tb["clip_obs"]
    bad = []

    def exact(name, a, b, mask=None):
        ne = a != b
        if mask is not None:
            ne &= mask
        if ne.any():
            e = np.argwhere(ne)[0]
            bad.append(f"{name}: {int(ne.sum())} entries differ, first at env {idx[e[0]]} {tuple(int(x) for x in e[1:])}: {a[tuple(e)]!r} != {b[tuple(e)]!r}")

    k76 = hist1[:, -1]                                           # the newest history row IS the unclipped proprio vector
    exact("OBS_BUF[:76] = clip(newest OBS_HISTORY row)", obs[:, :NPROP], np.clip(k76, -clipv, clipv))
    mp, fr, ms = sel(post["MASS_PARAMS"]), sel(post["FRICTION"]), sel(post["MOTOR_STRENGTH"])
    priv = np.concatenate([mp, fr[:, None], (ms.astype(np.float32) - np.float32(1.0)).astype(np.float64)], axis=1)     # WG:987-991
    exact("OBS_BUF privileged block", obs[:, NPROP:NPROP + NPRIV], np.clip(priv, -clipv, clipv))
    old = np.where(reset[:, None, None], 0.0, hist0).reshape(len(idx), -1)                                                  # WG:992 after WG:736
    exact("OBS_BUF history block", obs[:, NPROP + NPRIV:], np.clip(old, -clipv, clipv))
    refill = eplen <= 1                                                                                                 # WG:994-1001
    exact("OBS_HISTORY refill", hist1[refill], np.repeat(k76[refill][:, None], HIST, 1))
    exact("OBS_HISTORY shift", hist1[~refill][:, :-1], hist0[~refill][:, 1:])
    kinds = obs_kinds()
    ex = kinds == OBS_EXACT
    exact("proprio copies", k76[:, ex], o.v[:, ex])
    fl = kinds == OBS_FLAG
    exact("contact flags", k76[:, fl], o.v[:, fl], ~near[:, fl])
    if actions is not None:                                      # the newest FIFO row is the clipped, reordered action (WG:1162-1168)
        a = np.clip(np.asarray(actions, dtype=np.float64)[idx][:, POLICY_PERM[:NACT]], -tb["clip_actions"], tb["clip_actions"])
        if tb["action_delay"] != -1:
            exact("ACTION_HISTORY newest row", sel(post["ACTION_HISTORY"])[:, -1], np.where(reset[:, None], 0.0, a))
    sc = kinds == OBS_SCALED
    u = ulps(k76[:, sc], o.v[:, sc])
    scw = (kinds == OBS_SCALED) | (kinds == OBS_WRAPPED)
    rs = np.where(near[:, scw], 0.0, ratio(np.abs(k76[:, scw] - o.v[:, scw]), o.m[:, scw]))
    eu = kinds == OBS_EULER
    re = ratio(np.abs(k76[:, eu] - o.v[:, eu]), o.m[:, eu])
    if reset.any():                                              # a constant (formed once): identical over the reset envs
        exact("roll / pitch of reset envs", k76[reset][:, :2], np.repeat(k76[reset][:1, :2], int(reset.sum()), 0))

    def where_max(r, cols):
        e, c = np.unravel_index(np.argmax(r), r.shape)
        return float(r[e, c]), int(idx[e]), int(np.flatnonzero(cols)[c])

    blocks = [slice(0, NPROP), slice(NPROP, NPROP + NPRIV), slice(NPROP + NPRIV, None)]
    return dict(exact_bad=bad, ulp=float(u.max()), ratio_scaled=where_max(rs, scw), ratio_euler=where_max(re, eu),
                near=int(near.sum()), clipped=[int((np.abs(obs[:, b]) == clipv).sum()) for b in blocks],
                over=[int((np.abs(obs[:, b]) > clipv).sum()) for b in blocks], resets=int(reset.sum()), refills=int(refill.sum()),
                roll_pitch=k76[:, :2])


# ----------------------------------------------------------------------------------------------------------------------- cases
def with_cfg(tcfg, **fields):
    """A copy of the task config with scalar fields replaced; goal_delta_orn_range takes a [3][2] list."""
    tc = type(tcfg).from_buffer_copy(tcfg)
    for k, v in fields.items():
        if k == "goal_delta_orn_range":
            abi._set(tc.goal_delta_orn_range, v)
        else:
            setattr(tc, k, v)
    return tc


def alive_cfg(robot, **fields):
    """The state-derived cases' config: nothing terminates, the base class's soft limits tightened so that its limit terms act."""
    tc = with_cfg(robot["tcfg"], term_rp_threshold=10.0, term_z_threshold=-10.0, term_contact_rb_mask=0, **fields)
    abi.set_soft_limits(tc, robot["model"], 0.7, 0.3, 0.3, 20.0, 0.35)
    return tc


def curriculum(robot, lsc, asc, lmask, amask):
    from oracle import default_curriculum
    c = default_curriculum(robot["cfg"])
    abi._set(c.leg_reward_scale, lsc)
    abi._set(c.arm_reward_scale, asc)
    c.leg_active_mask, c.arm_active_mask = int(lmask), int(amask)
    return c


def cur_arrays(c):
    return dict(lsc=np.array([float(x) for x in c.leg_reward_scale]), asc=np.array([float(x) for x in c.arm_reward_scale]),
                lmask=int(c.leg_active_mask), amask=int(c.arm_active_mask))


def unit_curriculum(robot, without=()):
    mask = ALL_MASK
    for name in without:
        mask &= ~(1 << TERM[name])
    return curriculum(robot, np.ones(NREW), np.zeros(NREW), mask, 0)


def totals_curriculum(robot, seed=10):
    """Mixed-sign scales on both channels, eight terms listed in both with different scales. Sizes: ~1 / (typical size of the term on
    the states of case_state), so that no single term decides the sign of a channel's total."""
    rng = np.random.default_rng(seed)
    typical = dict(energy_square=3e5, survive=1, tracking_lin_vel_x_l1=0.35, tracking_ang_vel_yaw_exp=0.3, hip_action_l2=7.5, foot_contacts_z=7e3,
                   tracking_ee_sphere=0.6, arm_energy_abs_sum=35, tracking_ee_cart=0.6, tracking_ee_orn=0.25, tracking_ee_orn_ry=0.4,
                   leg_energy_abs_sum=1200, leg_energy_sum_abs=750, leg_action_l2=26, leg_energy=750, tracking_lin_vel=0.5,
                   tracking_lin_vel_x_exp=0.6, tracking_ang_vel_yaw_l1=0.9, tracking_lin_vel_y_l2=0.2, tracking_lin_vel_z_l2=0.5,
                   torques=3e3, collision=1, lin_vel_z=0.5, ang_vel_xy=16, dof_vel=1400, dof_acc=4e6, action_rate=80, termination=1,
                   dof_pos_limits=0.18, dof_vel_limits=7.5, torque_limits=90, tracking_ang_vel=0.3, feet_air_time=0.2, stumble=1,
                   stand_still=3, feet_contact_forces=140, base_height=0.01)
    size = np.array([1.0 / typical[t] for t in abi.REWARD_TERMS])
    lsc = size * rng.uniform(0.5, 2.0, NREW) * rng.choice([-1.0, 1.0], NREW)
    asc = size * rng.uniform(0.5, 2.0, NREW) * rng.choice([-1.0, 1.0], NREW)
    order = rng.permutation(NREW)
    both, leg_only, arm_only = order[:8], order[8:23], order[23:]
    lmask = sum(1 << int(t) for t in np.r_[both, leg_only])
    amask = sum(1 << int(t) for t in np.r_[both, arm_only])
    return curriculum(robot, lsc, asc, lmask, amask)


def stairs():
    """Up-and-down stairs along x: rise 0.15 m, tread 0.25 m, horizontal scale 0.025 m, vertical scale 0.005 m, 8 m x 8 m about
    the origin. (heights, hs, vs, tx, ty, tz) for set_heightfield."""
    hs, vs, cells = 0.025, 0.005, 320
    k = (np.arange(cells) * hs / 0.25).astype(int) % 4
    h = np.round(np.array([0, 1, 2, 1])[k] * 0.15 / vs).astype(np.int16)
    return np.repeat(h[:, None], cells, 1).copy(), hs, vs, -0.5 * cells * hs, -0.5 * cells * hs, 0.0


def quat_from_rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], -1)


def case_state(robot, tcfg, n, seed, cart=False, tilted=False, sums=False):
    """The tensors written before the first step of a state-derived case (dict name -> float32 / float64 array) and the actions of
    its steps [3][n, 18]. cart: goal timers on both sides of t = 0.5, a tenth of the goals due for resampling; tilted: base roll /
    pitch up to +-1.4 rad, a metre up (the observation's Euler angles over their range); sums: non-zero EPISODE_SUMS."""
    import helpers
    rng = np.random.default_rng(seed)
    root, dof = helpers.random_standing_state(n, tcfg, rng, height=(0.10, 0.50))
    root[:, 0, 7:10] = rng.uniform(-1.5, 1.5, (n, 3))
    root[:, 1, 0:3] = root[:, 0, 0:3] + np.array([50.0, 0.0, 0.0])                # the box out of the way
    root[:, 1, 2] = 2.0
    root[:, 1, 7:13] = 0
    if tilted:
        rp = rng.uniform(-1.4, 1.4, (n, 2))
        rp[:4] = [[1.4, 1.4], [-1.4, 1.4], [1.4, -1.4], [-1.4, -1.4]][:min(n, 4)]
        root[:, 0, 3:7] = quat_from_rpy(rp[:, 0], rp[:, 1], rng.uniform(-np.pi, np.pi, n))
        root[:, 0, 2] = 1.0
        root[:4, 0, 10:13] = 0                                                     # (the four corners keep their attitude through the step)
    cmd = np.zeros((n, 3), dtype=np.float32)
    cmd[:, 0] = rng.uniform(0.02, 0.6, n) * rng.choice([-1.0, 1.0], n)
    cmd[:, 1] = rng.uniform(-0.05, 0.05, n)
    cmd[:, 2] = rng.uniform(-1.0, 1.0, n)
    cmd[rng.random(n) < 1.0 / 3.0] = 0
    goal = np.zeros((n, 24), dtype=np.float32)
    lo, hi = np.array([0.35, -0.5, -1.2]), np.array([0.7, 0.6, 1.2])
    goal[:, G_START:G_START + 3] = rng.uniform(lo, hi, (n, 3))
    goal[:, G_GOAL:G_GOAL + 3] = rng.uniform(lo, hi, (n, 3))
    goal[:, G_DORN:G_DORN + 3] = rng.uniform(-0.6, 0.6, (n, 3))
    goal[:, G_ORN:G_ORN + 3] = rng.uniform(-1.5, 1.5, (n, 3))
    goal[:, G_TRAJ] = np.round(rng.uniform(50, 150, n))
    goal[:, G_TOTAL] = goal[:, G_TRAJ] + np.round(rng.uniform(25, 100, n))
    goal[:, G_TIMER] = np.round(rng.uniform(0.05, 0.95, n) * goal[:, G_TRAJ])
    if cart:
        due = rng.random(n) < 0.1
        goal[due, G_TIMER] = goal[due, G_TOTAL]
    s = dict(ROOT_STATES=root, DOF_STATE=dof, COMMANDS=cmd, GOAL_STATE=goal,
             ACTION_HISTORY=(1.5 * rng.normal(size=(n, abi.ADELAY_LEN, NACT))).astype(np.float32),
             LAST_ACTIONS=(1.5 * rng.normal(size=(n, NACT))).astype(np.float32),
             LAST_DOF_VEL=(dof[:, :, 1] + rng.uniform(-0.5, 0.5, (n, NDOF))).astype(np.float32),
             FEET_AIR_TIME=(rng.uniform(0.0, 0.6, (n, 4)) * (rng.random((n, 4)) < 0.7)).astype(np.float32),
             LAST_CONTACTS=(rng.random((n, 4)) < 0.3).astype(np.float32),
             OBS_HISTORY=rng.uniform(-1.0, 1.0, (n, HIST, NPROP)).astype(np.float32),
             EPISODE_LENGTH=np.where(np.arange(n) % 8 == 3, 0, 10).astype(np.float64),      # (every eighth env: first step of an episode, the history is refilled)
             EPISODE_SUMS=(rng.uniform(-2, 2, (n, NREW)) if sums else np.zeros((n, NREW))).astype(np.float32),
             METRIC_SUMS=np.zeros((n, NMET), dtype=np.float32))
    actions = [(1.5 * rng.normal(size=(n, NACT))).astype(np.float32) for _ in range(3)]
    return s, actions


def termination_state(robot, tcfg, n, seed):
    """Case E: exact inputs. EPISODE_SUMS start from random float32 values (the order of the two channels' additions shows in the last bit). Env e % 6: 0 below term_z_threshold; 1 / 2 rolled past the threshold with the goal sign that terminates /
    that does not; 3 at max_episode_length (time-out); 4, 5 alive. Airborne 5 m up unless stated, at rest."""
    s, actions = case_state(robot, tcfg, n, seed)
    root, goal = s["ROOT_STATES"], s["GOAL_STATE"]
    kind = np.arange(n) % 6
    root[:, 0, 2] = 5.0
    root[:, 0, 3:7] = quat_from_rpy(np.zeros(n), np.zeros(n), np.linspace(-3, 3, n))
    root[:, 0, 7:13] = 0
    root[kind == 0, 0, 2] = float(tcfg.term_z_threshold) - 0.05
    rolled = (kind == 1) | (kind == 2)
    root[rolled, 0, 3:7] = quat_from_rpy(np.full(int(rolled.sum()), 0.5), np.zeros(int(rolled.sum())), np.zeros(int(rolled.sum())))
    goal[:, G_START + 2] = goal[:, G_GOAL + 2] = np.where(kind == 2, -0.6, 0.6)          # the goal's yaw: roll > th terminates with yaw >= 0 only (WG:947-950)
    goal[:, G_START + 1] = goal[:, G_GOAL + 1] = 0.3
    s["EPISODE_LENGTH"] = np.where(kind == 3, float(tcfg.max_episode_length), 10.0)
    s["EPISODE_SUMS"] = np.random.default_rng(seed + 1).uniform(0.05, 0.2, (n, NREW)).astype(np.float32)
    return s, actions[:1], kind


def termination_curriculum(robot):
    lsc, asc = np.zeros(NREW), np.zeros(NREW)
    lsc[TERM["survive"]], asc[TERM["survive"]] = 0.75, -0.375
    lsc[TERM["termination"]], asc[TERM["termination"]] = -3.5, 2.25
    mask = (1 << TERM["survive"]) | (1 << TERM["termination"])
    return curriculum(robot, lsc, asc, mask, mask)


PRE_NAMES = ["LAST_ACTIONS", "LAST_DOF_VEL", "FEET_AIR_TIME", "LAST_CONTACTS", "OBS_HISTORY", "EPISODE_SUMS", "METRIC_SUMS"]
POST_NAMES = ["TORQUES", "DOF_STATE", "ROOT_STATES", "ACTIONS", "COMMANDS", "GOAL_STATE", "BASE_LIN_VEL", "BASE_ANG_VEL", "FORCE_SENSOR",
              "NET_CONTACT_FORCE", "RIGID_BODY_STATE", "RESET_BUF", "TIME_OUT_BUF", "EPISODE_LENGTH", "EPISODE_SUMS", "METRIC_SUMS",
              "EPISODE_SUMS_DONE", "REW_BUF", "ARM_REW_BUF", "OBS_BUF", "OBS_HISTORY", "ACTION_HISTORY", "FEET_AIR_TIME", "LAST_CONTACTS",
              "MASS_PARAMS", "FRICTION", "MOTOR_STRENGTH"]
STEP_COUNTER = 1


def run_steps(sim, tcfg, cur, state, actions, zero_sums=True, heightfield=None):
    """Write `state` into `sim` (an adapter with get / set / step / set_curriculum / set_heightfield / set_step_counter), run the
    steps and return [(pre, post, action)] with every tensor the checker reads, downloaded as float64."""
    assert tcfg.push_interval == 0 or STEP_COUNTER + len(actions) < tcfg.push_interval        # no push fires
    sim.set_curriculum(cur)
    if heightfield is not None:
        sim.set_heightfield(*heightfield)
    for name, v in state.items():
        sim.set(name, v)
    sim.set_step_counter(STEP_COUNTER)
    out = []
    for a in actions:
        if zero_sums:
            sim.set("EPISODE_SUMS", np.zeros((a.shape[0], NREW)))
            sim.set("METRIC_SUMS", np.zeros((a.shape[0], NMET)))
        pre = {k: sim.get(k) for k in PRE_NAMES}
        sim.step(a)
        post = {k: sim.get(k) for k in POST_NAMES}
        for k, v in post.items():
            assert np.isfinite(v).all(), k
        out.append((pre, post, a))
    return out


class OracleAdapter:
    """OracleSim behind the interface of run_steps."""

    def __init__(self, o):
        self.o = o

    def get(self, name):
        return self.o.get(name)

    def set(self, name, v):
        self.o.set(name, v)

    def step(self, a):
        self.o.step(a)

    def set_curriculum(self, c):
        self.o.set_curriculum(c)

    def set_heightfield(self, *a):
        self.o.set_heightfield(*a)

    def set_step_counter(self, v):
        self.o.step_counter = v


# ------------------------------------------------------------------------------------------------------------------ the checker
def check_terms(tb, cur, pre, post, envs=None, kernel_scale=None, **wrong):
    """One step read out under a unit curriculum (scale 1 on the leg channel for every listed term): EPISODE_SUMS / METRIC_SUMS
    against the restatement. Returns dict(ratio [n, 37] (nan: not checked -- reset env, near a threshold, term not listed),
    met_ratio [n, 10], air_ratio [n, 4], lc_equal, val, mag, near, alive [n], T). kernel_scale [37]: multiplies the sim-side
    terms (the checker-can-fail tests)."""
    idx = np.arange(np.asarray(post["RESET_BUF"]).shape[0]) if envs is None else np.asarray(envs)
    sel = lambda a: np.asarray(a, dtype=np.float64)[idx]
    c = cur_arrays(cur)
    air_on = bool(((c["lmask"] | c["amask"]) >> TERM["feet_air_time"]) & 1)
    T = reward_terms(tb, pre, post, air_on=air_on, envs=idx, **wrong)
    alive = sel(post["RESET_BUF"]) == 0
    listed = np.array([(c["lmask"] >> t) & 1 for t in range(NREW)], dtype=bool)
    got = sel(post["EPISODE_SUMS"])
    if kernel_scale is not None:
        got = got * np.asarray(kernel_scale)[None]
    r = ratio(np.abs(got - T["val"]), T["mag"])
    r[~alive] = np.nan
    r[T["near"]] = np.nan
    r[:, ~listed] = np.nan
    ms = metric_sources(T, c["lmask"], c["amask"])
    mr = ratio(np.abs(sel(post["METRIC_SUMS"]) - ms.v), ms.m)
    mr[~alive] = np.nan
    ar = ratio(np.abs(sel(post["FEET_AIR_TIME"]) - T["air"].v), T["air"].m)
    ar[T["air_near"]] = np.nan
    lc_ok = (sel(post["LAST_CONTACTS"]) == T["last_contacts"]) | T["air_near"]
    ar[~alive] = np.nan                                         # (a reset zeroes the air time, WG:734)
    return dict(ratio=r, met_ratio=mr, air_ratio=ar, lc_equal=bool(lc_ok[alive].all()), val=T["val"], mag=T["mag"], near=T["near"],
                alive=alive, T=T, got=got, envs=idx)


def tier_maxima(res):
    """Largest ratio per tier of a check_terms result, with (value, env, term name)."""
    out = {}
    for tier in ("poly", "exp", "angle"):
        best = (0.0, -1, "")
        cols = [t for t in range(NREW) if TERM_TIER[t] == tier]
        r = np.nan_to_num(res["ratio"][:, cols], nan=0.0)
        e, c = np.unravel_index(np.argmax(r), r.shape)
        best = (float(r[e, c]), int(res["envs"][e]), abi.REWARD_TERMS[cols[c]])
        mcols = [m for m in range(NMET) if MET_TIER[m] == tier]
        mr = np.nan_to_num(res["met_ratio"][:, mcols], nan=0.0)
        if mr.size and mr.max() > best[0]:
            e, c = np.unravel_index(np.argmax(mr), mr.shape)
            best = (float(mr[e, c]), int(res["envs"][e]), "metric " + abi.METRIC_NAMES[mcols[c]])
        if tier == "poly":
            a = np.nan_to_num(res["air_ratio"], nan=0.0)
            if a.max() > best[0]:
                e, c = np.unravel_index(np.argmax(a), a.shape)
                best = (float(a[e, c]), int(res["envs"][e]), f"FEET_AIR_TIME[{c}]")
        out[tier] = best
    return out


def check_totals(tb, cur, pre, post, envs=None, **wrong):
    """REW_BUF / ARM_REW_BUF / EPISODE_SUMS after a step under an arbitrary curriculum, against the totals of the fp64 terms.
    Returns dict(ratio [n, 2]: (|sim - ref| - the terms' allowance)+ / (2^-24 sum |scale term| / 100), nan for reset envs and envs
    at the clip's kink; sums_ratio [n, 37] likewise for the episode sums; clipped [n, 2]; alive)."""
    idx = np.arange(np.asarray(post["RESET_BUF"]).shape[0]) if envs is None else np.asarray(envs)
    sel = lambda a: np.asarray(a, dtype=np.float64)[idx]
    c = cur_arrays(cur)
    air_on = bool(((c["lmask"] | c["amask"]) >> TERM["feet_air_time"]) & 1)
    T = reward_terms(tb, pre, post, air_on=air_on, envs=idx)
    tc = term_bounds()
    R = reward_totals(tb, T, c, tc, **wrong)
    alive = sel(post["RESET_BUF"]) == 0
    r = np.full((len(idx), 2), np.nan)
    near_any = np.zeros(len(idx), bool)
    for t in range(NREW):
        if ((c["lmask"] | c["amask"]) >> t) & 1:
            near_any |= T["near"][:, t]
    for k, (name, ch) in enumerate((("REW_BUF", ""), ("ARM_REW_BUF", "arm_"))):
        err = np.maximum(np.abs(sel(post[name]) - R[ch + "rew"]) - R[ch + "allow"], 0.0)
        r[:, k] = ratio(err, R[ch + "size"])
        r[R[ch + "kink"] | ~alive | near_any, k] = np.nan
    old = sel(pre["EPISODE_SUMS"])
    want = old + R["leg"].v + R["arm"].v
    allow = (R["leg"].m + R["arm"].m - np.abs(R["leg"].v) - np.abs(R["arm"].v)) * tc[None] * EPS      # the terms' own bounds, scale-weighted
    size = np.abs(old) + np.abs(R["leg"].v) + np.abs(R["arm"].v)
    sr = ratio(np.maximum(np.abs(sel(post["EPISODE_SUMS"]) - want) - allow, 0.0), size)
    sr[~alive] = np.nan
    sr[T["near"]] = np.nan
    return dict(ratio=r, sums_ratio=sr, clipped=np.stack([R["leg_clipped"], R["arm_clipped"]], 1), alive=alive, envs=idx, R=R, T=T)


def termination_expected(tb, cur, pre, post, arm_first=False, termination_before_clip=False):
    """Case E in float32 arithmetic written out: (clip(s_survive) + s_term [reset and not time_out]) / 100 per channel, and the two
    slots' episode sums old + leg + arm in that order, bit for bit. The last two arguments seed wrong formulas."""
    c = cur_arrays(cur)
    f = np.float32
    term = ((np.asarray(post["RESET_BUF"]) != 0) & (np.asarray(post["TIME_OUT_BUF"]) == 0)).astype(f)
    out = {}
    for name, sc in (("REW_BUF", c["lsc"]), ("ARM_REW_BUF", c["asc"])):
        s = np.full(len(term), f(1.0) * f(sc[TERM["survive"]]), dtype=f)
        tv = term * f(sc[TERM["termination"]])
        if termination_before_clip:
            s = s + tv
        if tb["only_positive"]:
            s = np.maximum(s, f(0.0))
        if not termination_before_clip:
            s = s + tv
        out[name] = (s / f(100.0)).astype(np.float64)
    old = np.asarray(pre["EPISODE_SUMS"]).astype(f)
    for slot, tm in (("survive", np.ones(len(term), dtype=f)), ("termination", term)):
        a, b = tm * f(c["lsc"][TERM[slot]]), tm * f(c["asc"][TERM[slot]])
        if arm_first:
            a, b = b, a
        out[slot + "_sum"] = ((old[:, TERM[slot]] + a) + b).astype(np.float64)
    return out


def coverage(results):
    """Counts over the checked env-steps of a list of check_terms results: per term the env-steps in which it is non-zero, left out
    near a threshold, lost to resets; and the two-valued pieces."""
    val = np.concatenate([r["val"][r["alive"]] for r in results])
    near = np.concatenate([r["near"][r["alive"]] for r in results])
    total = sum(len(r["alive"]) for r in results)
    return dict(steps=len(val), total=total, resets=total - len(val), nonzero=(val != 0).sum(0), near=near.sum(0), val=val)


# ------------------------------------------------------------------------------------------------------------- the case table
DELTA_ORN = [[-0.5, 0.5], [-0.4, 0.4], [-0.6, 0.6]]
# name -> (seed, steps, what differs from case A)
CASES = {"terms": (201, 3), "terms-cart": (202, 3), "air-time-off": (201, 3), "totals-positive": (204, 1), "totals-raw": (204, 1),
         "termination": (205, 1), "obs-tilted": (206, 1), "obs-clip": (206, 1)}
PARAM_SEED = 11


def build_case(robot, name, n):
    """dict(tcfg, cur, state, actions, heightfield, zero_sums) of a case of the table above; `kind` for the termination case."""
    seed, steps = CASES[name]
    c = dict(heightfield=stairs(), zero_sums=True)
    if name == "termination":
        c["tcfg"] = with_cfg(robot["tcfg"], only_positive_rewards=1)
        c["cur"] = termination_curriculum(robot)
        c["state"], c["actions"], c["kind"] = termination_state(robot, c["tcfg"], n, seed)
        c["heightfield"], c["zero_sums"] = None, False
        return c
    if name == "terms-cart":
        c["tcfg"] = alive_cfg(robot, goal_command_cart=1, goal_delta_orn_range=DELTA_ORN)
    elif name.startswith("totals"):
        c["tcfg"] = alive_cfg(robot, only_positive_rewards=int(name == "totals-positive"))
    elif name == "obs-clip":
        c["tcfg"] = alive_cfg(robot, clip_obs=0.5)
    else:
        c["tcfg"] = alive_cfg(robot)
    c["cur"] = totals_curriculum(robot) if name.startswith("totals") else \
        unit_curriculum(robot, without=("feet_air_time",) if name == "air-time-off" else ())
    c["state"], acts = case_state(robot, c["tcfg"], n, seed, cart=name == "terms-cart", tilted=name.startswith("obs-"),
                                  sums=name.startswith("totals"))
    c["actions"] = acts[:steps]
    c["zero_sums"] = not name.startswith("totals")
    return c


def run_case(make_sim, robot, name, n):
    """make_sim(tcfg, n) -> adapter. Returns the case dict with tb and steps [(pre, post, action)] added."""
    c = build_case(robot, name, n)
    c["tb"] = tables(robot["wmodel"], c["tcfg"])
    c["steps"] = run_steps(make_sim(c["tcfg"], n), c["tcfg"], c["cur"], c["state"], c["actions"], c["zero_sums"], c["heightfield"])
    return c


def conditions(tb, steps, results):
    """The coverage conditions of the term cases, as counts over the checked (alive) env-steps."""
    cov = coverage(results)
    val = cov["val"]
    dof = np.concatenate([np.asarray(post["DOF_STATE"])[r["envs"]][r["alive"]] for (_, post, _), r in zip(steps, results)])
    cmd = np.concatenate([np.asarray(post["COMMANDS"])[r["envs"]][r["alive"]] for (_, post, _), r in zip(steps, results)])
    q, qd = dof[:, :18, 0], np.abs(dof[:, :18, 1])                                 # (the locked fingers sit outside their range by construction)
    over = qd - tb["soft_vel"][None, :18]
    cmd_xy = np.hypot(cmd[:, 0], cmd[:, 1])
    col = val[:, TERM["collision"]]
    counts = np.bincount(col[col > 0].astype(int)) if (col > 0).any() else np.zeros(1, int)
    cov.update(two_valued=dict(
        stumble=(int((val[:, TERM["stumble"]] == 0).sum()), int((val[:, TERM["stumble"]] == 1).sum())),
        cmd_gate=(int((cmd_xy < 0.1).sum()), int((cmd_xy > 0.1).sum())),
        dof_pos_limits=(int((q < tb["soft_lo"][None, :18]).any(1).sum()), int((q > tb["soft_hi"][None, :18]).any(1).sum())),
        dof_vel_limits=(int(((over > 0) & (over < 1)).any(1).sum()), int((over >= 1).any(1).sum())),
        collision=(int((col == 0).sum()), int(max((counts > 0).sum() >= 2 and (col > 0).sum(), counts.max())))))
    return cov


EVENT_TERMS = ["stumble", "collision", "feet_air_time", "stand_still", "foot_contacts_z", "feet_contact_forces"]


def assert_conditions(name, cov):
    """Section "conditions": every term non-zero in 5 % of the checked env-steps (8 of them for a term that gates on an event;
    termination is zero by construction while nothing terminates -- the termination case holds it), both values of every two-valued
    piece in 8 env-steps, at most 2 % of the env-steps left out of any term at a threshold, at most 5 % lost to resets."""
    steps = cov["steps"]
    assert cov["resets"] <= 0.05 * cov["total"], (name, cov["resets"])
    for t, term in enumerate(abi.REWARD_TERMS):
        if term == "termination":
            continue
        need = 8 if term in EVENT_TERMS else 0.05 * steps
        assert cov["nonzero"][t] >= need, (name, term, int(cov["nonzero"][t]), need)
        assert cov["near"][t] <= 0.02 * steps, (name, term, int(cov["near"][t]))
    for piece, (a, b) in cov["two_valued"].items():
        assert a >= 8 and b >= 8, (name, piece, a, b)
