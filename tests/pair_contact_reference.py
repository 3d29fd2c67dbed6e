"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) statement of what the contact stage of one physics substep (physics_substep of
csrc/wbc_step_kernel.hip; the spec is oracle/wbc_oracle.c and DESIGN.md section 3) has to satisfy for a PAIR of bodies: a limb against a limb (the 44 candidates
that the broad phase promotes into dynamic slots), an arm sphere against the trunk box (static pairs), a robot sphere against the FREE
BOX (the five static pairs: feet and gripper tip; the twelve promoted ones: knees, mid-shanks, the trunk's bottom corners) and the
box's eight corner spheres against the terrain. It continues tests/contact_law_reference.py (a robot
sphere against the terrain) and imports what it can from it. Checked from tensors the sim stores anyway: ROOT_STATES (both actors) and
DOF_STATE before and after one substep, NET_CONTACT_FORCE (28 rows), FORCE_SENSOR, BODY_PARAMS, BOX_MASS, FRICTION, DROPPED_HITS,
BOX_SLEEP_TIMER, the cfg and the terrain. No articulated-body recursion and no contact solver anywhere in this file.

The box is not on the tree: a contact between it and one robot body, or between one of its corners and the terrain, alone in its env,
has nshare = 1 and the solver's block W_u = W_A + W_box + 1e-6 equals the true response up to the regulariser, whose only effect is a
contraction of 1e-6 / |W| per sweep towards the velocity-level law. These are therefore held to the CONVERGED law, like a lone foot.

A robot-internal pair alone in its env is not: its true response is W_t = J_rel (M + diag(armature))^-1 J_rel^T with J_rel = J_pA(xc) -
J_pB(xc), the solver's block W_u = W_A + W_B + 1e-6 leaves the cross blocks to the sweeps, and four sweeps contract towards the law by
|1 - W_t W_u^-1| (reported per env) without reaching it. The checker therefore ITERATES the law: cone_solve (the 3x3 cone solve of one
contact, contact_solve of the spec: the law itself) is applied `sweeps` = 4 times from lam = 0 to vref_k = vfree + (W_t - W_u) lam_k,
vfree = v+ - W_t f dt, and the stored impulse f dt has to be lam_4: W_u (f dt - lam_4) in the velocity tier, plus the slide magnitude and
direction of the final sweep; an env in which any sweep lies within 1e-3 of a decision (separating, stick / slide, the 0.05 fallback) is
left out of these. Geometry of a limb pair: limb_pair / seg_seg_closest of the spec restated (nine feature pairs, the smallest gap wins,
a tie keeps the earlier; n from B to A, xc on B's surface); an arm sphere against the trunk box: the clamp in the trunk's frame. mu =
max(0, friction) (both shapes carry the robot's material). Rows: +f on the rigid body of A's winning feature, -f on B's, bit for bit;
equations of motion with J_rel^T f (the six root rows vanish: the pair is internal); a foot in the pair reads (E^T f, E^T ((-rad n) x f))
on A's side, (E^T (-f), E^T ((rad2 n) x (-f))) on B's. Scales: as below with mag(n) = 2 (|pa| + |pb|) / dist, pa, pb the closest points; the residual W_u (f dt - lam_4) of a sliding last
sweep carries the normal's scale once more through |W_u d| / (n.W_u d), d = n - mu vhat_t (what is rounded along n comes back along the
impulse's direction; up to 20 at the fallback's threshold).

  1. geometry   frame F (origin at the robot's root, the base's axes, R0 = quat_to_mat(STORED quaternion)). The box: c = R0^T (p_box -
                p_root), E = R0^T R_box, v = R0^T v_box, w = R0^T w_box. Sphere against the box: the centre in the box frame clamped to
                [-h, h]^3 -> xc on the box's surface, n from the box to the sphere, gap = dist - rad; a centre inside leaves through the
                nearest face. A corner sphere: centre c + E pos, the terrain under its world position as contact_law_reference.
  2. activation NET_CONTACT_FORCE is non-zero only on the sphere's rigid-body row and the box row (a pair), or on the box row (a
                corner); the two rows of a lone pair are minus each other bit for bit; every other row is exactly 0; DROPPED_HITS is 0.
  3. the law    (envs with exactly one active contact) a = (nu1 - nu0) / dt; v+ = the relative velocity after the step of the two
                body-fixed points at xc: the robot's as contact_law_reference, the box's from its STORED velocities,
                v_box + w x r + dt (w x (w x r)) + dt (a_box + alpha_box x r), r = xc - c; W = J_p (M + armature)^-1 J_p^T +
                1/m + (|r|^2 1 - r r^T) / Ic, Ic = m 2/3 h^2; vfree = v+ - W f dt; vn_tgt in its three branches; mu = max(0, (box_friction
                + friction) / 2) for a pair, max(0, (box_friction + terrain_friction) / 2) for a corner. Separating (f exactly 0, n.v+ >=
                vn_tgt), stick (v+ = n vn_tgt), slide (n.v+ = vn_tgt, |f_t| = mu f_n, f_t against vfree_t above 1e-2 m/s), frictionless
                fallback (f_t = 0): the classes and the 1e-3 decision band of contact_law_reference.
  4. cone       every pair and every corner: f.n >= 0, |f_t| <= mu f.n (single-contact envs: the force is read off the row).
  5. sensors    a foot pushed by the box: FORCE_SENSOR = (E_foot^T f, E_foot^T ((-rad n) x f)); exactly 0 without a force.
  6. equations of motion, every row: ID_ref(q0, nu0, a) + armature a - (0_6, tau + t_limit) = J_pA^T f (root rows: tier "mom", joint
                rows: tier "eom", the scale of forward_dynamics_reference.substep_residual). The box: m (a_box - g) = the box row of
                NET_CONTACT_FORCE (any number of contacts), Ic alpha_box = -/+ (xc - c) x f (one contact; no gyroscopic term),
                c1 = c0 + dt v1, the quaternion first-order and renormalised (tier "box").
  7. sleeping   a resting box with its timer at the threshold: pose bit-unchanged, velocity exactly 0, box row exactly 0, timer kept.
                With a robot sphere inside the contact offset: timer 0, the box obeys its Newton row (it is awake) and the pair carries
                its force on both rows.

Every inexact check is |residual| <= C 2^-24 scale; the file returns residual / (2^-24 scale) per tier. Scales beyond those of
contact_law_reference (same names, same construction):
    n        a face of the box: mag(E) |nl| with mag(E) = mag(R0)^T mag(R_box); an edge or a corner region: plus |E| 2 mag(pl) / dist,
             pl = E^T (x_sphere - c) the centre in the box frame, mag(pl) = |E|^T (|x_sphere| + mag(R0)^T |p_box - p_root|): the
             rounding of two positions in F, amplified by the short distance the normal is taken over
    gap      |nl| . mag(pl) + h + rad (a pair); as contact_law_reference (a corner), with mag(centre) added to |X_z|
    vel      robot side as there; box side mag(R0)^T (|v0| + |v1|) + (mag(R0)^T (|w0| + |w1|)) x |r| + (|w0| + |w1|) x mag(r) +
             dt |w|^2 |r|, mag(r) = |c| + |xc| (r is the difference of two points in F); + |W| |lam| + the vn_tgt terms
    box      m (mag(R0^-1) (|v0| + |v1|) / dt + |g|) + sum over the pairs' robot rows |f| + |row + that sum| (the row's summands);  Ic mag(R0^-1) (|w0| + |w1|) / dt + (|r| + mag(r)) x |f|; the integrator rows
             as forward_dynamics_reference.integrator_errors
K_REF per tier is the fp32 ORACLE's largest ratio on exactly the cases below (measured and asserted by tests/test_pair_contact.py,
never taken from the kernel); C = 4 K_ref rounded up to a power of two, at most 1024.

The seeded generators are here too, so that tests/test_pair_contact.py (the C oracle in both precisions) and
tests/test_gpu_pair_contact.py (the HIP kernels) evaluate exactly the same states. Robot and box are in the air (root at z = 1.2 m) except
where a case says otherwise. The cases use a copy of the model with box_friction = 0.1 and a cfg copy with terrain_friction = 0.1 and
max_depenetration_vel = 0.16 m/s: with the shipped 1.0 no draw of helpers.random_env_params reaches mu = 0, and a mid-shank (r = 8 mm)
cannot sink the 25 mm at which the shipped cap takes over without its centre entering the box. Nothing under wbc_amd imports this file."""
import numpy as np

import arm_osc_oracle as ao
import constrained_dynamics_reference as cdr
import contact_law_reference as clr
import forward_dynamics_reference as fdr
import inverse_dynamics_reference as idr
import self_collision_geometry as scg
import whole_body_reference as wb
from wbc_amd import abi

EPS = clr.EPS
LIVE = fdr.LIVE
C_CAP = 1024.0
TIERS = ("vel", "cone", "dir", "sensor", "mom", "eom", "box")
CLASSES = clr.CLASSES
MARGIN_GUARD = clr.MARGIN_GUARD
DECISION_BAND = clr.DECISION_BAND
SLIDE_SPEED = clr.SLIDE_SPEED
MAX_LEFT_OUT = 0.02           # margin + feature + band, share of a case
MIN_ELIGIBLE = 0.85
MIN_COUNT = 10
BOX_FRICTION = 0.1            # of the cases' model copy
CASE_VMAX = 0.16              # of the cases' cfg copy: the cap takes over at 4 mm
BOX_ROW = 27
STATIC_BOX_SPHERES = [0, 1, 2, 3, 8]                                  # feet, gripper tip
PROMOTED_BOX_SPHERES = [4, 5, 6, 7, 23, 24, 25, 26, 15, 17, 19, 21]   # knees, mid-shanks, the trunk's bottom corners
BOX_SPHERES = STATIC_BOX_SPHERES + PROMOTED_BOX_SPHERES

# tier -> K_ref: the fp32 oracle's largest ratio over every case of tests/test_pair_contact.py (measured and asserted there)
K_REF = {"vel": 2.86, "cone": 0.94, "dir": 0.572, "sensor": 2.14, "mom": 3.93, "eom": 14.81, "box": 5.69}


def bound(tier):
    """C of a tier: 4 x K_ref rounded up to a power of two."""
    c = 2.0 ** np.ceil(np.log2(4.0 * K_REF[tier]))
    assert c <= C_CAP, (tier, c)
    return float(c)


_CASE_ROBOTS, _TABLES = {}, {}                  # model copies by the model's bytes; the checker's tables by (model, cfg) bytes


def case_robot(robot):
    """The robot fixture with the cases' model copy (box_friction = BOX_FRICTION)."""
    key = bytes(robot["wmodel"])
    if key not in _CASE_ROBOTS:
        wm = type(robot["wmodel"]).from_buffer_copy(robot["wmodel"])
        wm.box_friction = BOX_FRICTION
        _CASE_ROBOTS[key] = dict(robot, wmodel=wm)
    return _CASE_ROBOTS[key]


def case_cfg(tcfg, **kw):
    return clr.case_cfg(tcfg, **dict(dict(max_depenetration_vel=CASE_VMAX), **kw))


def box_tables(wmodel):
    """dict(half, friction, corners [8] of dict(slot, pos, rad), sleep_speed, sleep_time)."""
    corners = [dict(slot=k, pos=np.array([float(x) for x in wmodel.cp_pos[k]]), rad=float(wmodel.cp_radius[k]))
               for k in range(wmodel.ncp) if wmodel.cp_kind[k] == abi.CP_TERRAIN and wmodel.cp_body[k] == abi.BOX_BODY]
    assert len(corners) == 8
    pair_slot = {int(wmodel.cp_sph[k]): k for k in range(wmodel.ncp) if wmodel.cp_kind[k] == abi.CP_BOX and wmodel.cp_body2[k] == abi.BOX_BODY}
    assert sorted(pair_slot) == sorted(STATIC_BOX_SPHERES)
    cand = {int(wmodel.pr_a[k]): float(wmodel.pr_reach[k]) for k in range(abi.NCP) if wmodel.pr_kind[k] == abi.PR_SPHERE_BOX}
    assert sorted(cand) == sorted(PROMOTED_BOX_SPHERES)
    lanes = [(k, int(wmodel.pr_a[k])) for k in range(abi.NCP) if wmodel.pr_kind[k] == abi.PR_SPHERE_BOX]
    return dict(cand_lanes=lanes, limb_reach={k: float(wmodel.pr_reach[k]) for k in range(abi.NCP) if wmodel.pr_kind[k] == abi.PR_LIMBS}, half=float(wmodel.box_half), friction=float(wmodel.box_friction), corners=corners, pair_slot=pair_slot, reach=cand,
                sleep_speed=float(wmodel.box_sleep_speed), sleep_time=float(wmodel.box_sleep_time))


def mag_rot(quat):
    """Sizes of the summands of quat_to_mat (xyzw): what the rounding of a stored quaternion does to its matrix."""
    x, y, z, w = np.abs(np.asarray(quat, dtype=np.float64))
    return np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x)],
                     [2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y)]])


def _cross_abs(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


# -------------------------------------------------------------------------------------------------------------------- geometry
DEFAULT_SPEC = dict(normal_sign=1.0, box_about_origin=False, mu_with_terrain=False, lever_sign=1.0, inside_through_nearest=True,
                    converged=False, sweeps=4, partner_sign=-1.0)


def sphere_box(pl, half, rad, nearest=True):
    """A sphere with centre pl (box frame) against the cube [-half, half]^3: (gap, nl, ql, region) with region 1 / 2 / 3 = face / edge /
    corner of the clamp (the number of clamped coordinates), 0 = centre inside."""
    ql = np.clip(pl, -half, half)
    clamped = ql != pl
    if clamped.any():
        d = pl - ql
        dist = float(np.linalg.norm(d))
        return dist - rad, d / dist, ql, int(clamped.sum())
    depth = half - np.abs(pl)
    ax = int(np.argmin(depth)) if nearest else int(np.argmax(depth))          # the first of equal depths, as the spec's loop
    nl = np.zeros(3)
    nl[ax] = 1.0 if pl[ax] >= 0 else -1.0
    ql = pl.copy()
    ql[ax] = nl[ax] * half
    return -float(depth[ax]) - rad, nl, ql, 0


def box_geometry(tm, sph, bt, ter, cfg, root, q, spec=DEFAULT_SPEC):
    """Step 1 for one env: the robot's terrain geometry of contact_law_reference (key "robot") and
    box dict(c, E, magE, mag_c); pairs [17] of dict(sphere, gap, n, mag_n, xc, mag_gap, region, dist, mag_pl, active);
    corners [8] of dict(corner, gap, n, mag_n, xc, mag_gap, active, near_border, tri)."""
    root = np.asarray(root, dtype=np.float64)
    g = clr.geometry(tm, sph, ter, cfg, root[0], q)
    R0 = g["R0"]
    Rb = ao.quat_to_mat(root[1, 3:7])
    mR0, mRb = mag_rot(root[0, 3:7]), mag_rot(root[1, 3:7])
    c = R0.T @ (root[1, 0:3] - root[0, 0:3])
    mag_c = mR0.T @ np.abs(root[1, 0:3] - root[0, 0:3])      # the difference of two stored positions is rounded relative to its result
    E, magE = R0.T @ Rb, mR0.T @ mRb
    half = bt["half"]
    xk = g["xc"] + g["rad"][:, None] * g["n"]                                   # the robot spheres' centres in F
    pairs = []
    for k in BOX_SPHERES:
        rad = float(g["rad"][k])
        pl = E.T @ (xk[k] - c)
        mag_pl = np.abs(E).T @ (np.abs(xk[k]) + mag_c)
        gap, nl, ql, region = sphere_box(pl, half, rad, spec["inside_through_nearest"])
        dist = gap + rad
        mag_nl = np.where(ql != pl, 2.0 * mag_pl / abs(dist), 0.0) if region > 0 else np.zeros(3)
        pairs.append(dict(sphere=k, pl=pl, gap=gap, n=E @ nl, mag_n=magE @ np.abs(nl) + np.abs(E) @ mag_nl, xc=c + E @ ql, region=region, dist=dist,
                          mag_gap=float(np.abs(nl) @ mag_pl) + half + rad, mag_pl=mag_pl, active=gap < cfg["margin"],
                          centre_dist=float(np.linalg.norm(xk[k] - c))))
    cen = np.array([c + E @ cn["pos"] for cn in bt["corners"]])
    X = root[0, 0:3] + cen @ R0.T
    h, nw, aux = clr.terrain_query(ter, cfg["ground_z"], X[:, 0], X[:, 1])
    corners = []
    for i, cn in enumerate(bt["corners"]):
        gap = (X[i, 2] - h[i]) * nw[i, 2] - cn["rad"]
        n = nw[i] @ R0
        corners.append(dict(corner=i, gap=float(gap), n=n, mag_n=np.abs(nw[i]) @ mR0, xc=cen[i] - cn["rad"] * n, active=gap < cfg["margin"],
                            mag_gap=float(np.abs(X[i, 2]) + abs(h[i]) + cn["rad"] + aux["slope_mag"][i] + np.abs(R0[2]) @ (mag_c + magE @ np.abs(cn["pos"]))),
                            near_border=bool(aux["near_border"][i]), tri=int(aux["tri"][i])))
    return dict(robot=g, R0=R0, c=c, E=E, magE=magE, mag_c=mag_c, mR0=mR0, pairs=pairs, corners=corners)


def limb_tables(wmodel):
    """dict(limbs [dict(s0, s1, radius, cap0, cap1, body, rb, rb0, rb1)], cands [(lane, limb a, limb b)] (44), trunk [dict(lane, sphere,
    centre, half, body2, rb2)] (3), rest)."""
    f = float
    limbs = [dict(s0=int(wmodel.limb_s0[i]), s1=int(wmodel.limb_s1[i]), radius=f(wmodel.limb_radius[i]), cap0=f(wmodel.limb_cap0[i]),
                  cap1=f(wmodel.limb_cap1[i]), body=int(wmodel.limb_body[i]), rb=int(wmodel.limb_rb[i]), rb0=int(wmodel.limb_rb0[i]),
                  rb1=int(wmodel.limb_rb1[i])) for i in range(wmodel.nlimb)]
    cands = [(k, int(wmodel.pr_a[k]), int(wmodel.pr_b[k])) for k in range(abi.NCP) if wmodel.pr_kind[k] == abi.PR_LIMBS]
    trunk = [dict(lane=k, sphere=int(wmodel.pr_a[k]), centre=np.array([f(x) for x in wmodel.cp_a[k]]), half=np.array([f(x) for x in wmodel.cp_b[k]]),
                  body2=int(wmodel.cp_body2[k]), rb2=int(wmodel.cp_rb2[k]))
             for k in range(wmodel.ncp) if wmodel.cp_kind[k] == abi.CP_BOX and wmodel.cp_body2[k] != abi.BOX_BODY]
    assert len(cands) == 44 and len(trunk) == 3
    return dict(limbs=limbs, cands=cands, trunk=trunk, rest=f(wmodel.pair_rest_offset))


def seg_closest(a0, a1, b0, b1):
    """seg_seg_closest of the spec restated: (pa, pb, par) with par = den / (1e-7 a e) of two proper segments (inf otherwise): how far
    the shafts are from the spec's parallel threshold."""
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    a, e, f = d1 @ d1, d2 @ d2, d2 @ r
    par = np.inf
    if a <= 1e-10 and e <= 1e-10:
        sp = tp = 0.0
    elif a <= 1e-10:
        sp, tp = 0.0, min(max(f / e, 0.0), 1.0)
    else:
        c = d1 @ r
        if e <= 1e-10:
            tp, sp = 0.0, min(max(-c / a, 0.0), 1.0)
        else:
            b = d1 @ d2
            den = a * e - b * b
            par = den / (1e-7 * a * e)
            sp = min(max((b * f - c * e) / den, 0.0), 1.0) if den > 1e-7 * a * e else 0.0
            tp = (b * sp + f) / e
            if tp < 0:
                tp, sp = 0.0, min(max(-c / a, 0.0), 1.0)
            elif tp > 1:
                tp, sp = 1.0, min(max((b - c) / a, 0.0), 1.0)
    return a0 + d1 * sp, b0 + d2 * tp, par


FEATURES = ("shaft/shaft", "end/shaft", "shaft/end", "end/end")


def limb_pair(A, B, rest):
    """limb_pair of the spec restated. A, B: (end0, end1, shaft radius, cap0, cap1). dict(gap, n (B to A), xc (on B's surface), ra, rb, fa,
    fb (0 shaft, 1 end 0, 2 end 1), feature (index into FEATURES), second (the runner-up's gap), par, pa, pb, dist)."""
    aend, bend, acap, bcap = A[0:2], B[0:2], A[3:5], B[3:5]
    found = []
    for f in range(9):
        ea = -1 if f == 0 else (f - 1 if f <= 2 else (-1 if f <= 4 else (f - 5) // 2))
        eb = -1 if f <= 2 else (f - 3 if f <= 4 else (f - 5) % 2)
        if (ea >= 0 and not acap[ea] > 0) or (eb >= 0 and not bcap[eb] > 0):
            continue
        pa, pb, par = seg_closest(aend[ea] if ea >= 0 else A[0], aend[ea] if ea >= 0 else A[1], bend[eb] if eb >= 0 else B[0], bend[eb] if eb >= 0 else B[1])
        fra, frb = acap[ea] if ea >= 0 else A[2], bcap[eb] if eb >= 0 else B[2]
        found.append((float(np.linalg.norm(pa - pb)) - fra - frb - rest, f, pa, pb, fra, frb, ea + 1, eb + 1, par))
    best = min(found, key=lambda x: (x[0], x[1]))                               # a tie keeps the earlier
    gaps = sorted(x[0] for x in found)
    g, f, pa, pb, fra, frb, fa, fb, par = best
    d = pa - pb
    dist = float(np.linalg.norm(d))
    n = d / dist if dist > 1e-9 else np.array([1.0, 0.0, 0.0])
    return dict(gap=g, n=n, xc=pb + frb * n, ra=fra, rb=frb, fa=fa, fb=fb, feature=0 if f == 0 else (1 if f <= 2 else (2 if f <= 4 else 3)),
                second=gaps[1] if len(gaps) > 1 else np.inf, par=par if f == 0 else np.inf, pa=pa, pb=pb, dist=dist)


def internal_geometry(lt, sph, g, cfg):
    """The 47 internal pairs of one env from the robot geometry g of contact_law_reference.geometry (frame F): list of dict(kind "limbs" /
    "trunk", lane, name, body, body2, rb, rb2, rad, rad2, gap, n, mag_n, xc, mag_gap, active, feature / region, second, par)."""
    xk = g["xc"] + g["rad"][:, None] * g["n"]
    out = []
    for lane, la, lb in lt["cands"]:
        A, B = lt["limbs"][la], lt["limbs"][lb]
        h = limb_pair((xk[A["s0"]], xk[A["s1"]], A["radius"], A["cap0"], A["cap1"]), (xk[B["s0"]], xk[B["s1"]], B["radius"], B["cap0"], B["cap1"]), lt["rest"])
        mag_p = np.abs(h["pa"]) + np.abs(h["pb"])
        out.append(dict(kind="limbs", lane=lane, pair=(la, lb), body=A["body"], body2=B["body"], rb=(A["rb"], A["rb0"], A["rb1"])[h["fa"]],
                        rb2=(B["rb"], B["rb0"], B["rb1"])[h["fb"]], rad=h["ra"], rad2=h["rb"], gap=h["gap"], n=h["n"], xc=h["xc"],
                        mag_n=2.0 * mag_p / max(h["dist"], 1e-300), mag_gap=float(mag_p.sum()) + h["ra"] + h["rb"], active=h["gap"] < cfg["margin"],
                        feature=h["feature"], second=h["second"], par=h["par"], region=None))
    for t in lt["trunk"]:
        k = t["sphere"]
        rad = float(g["rad"][k])
        E2, p2 = g["E"][t["body2"]], g["p"][t["body2"]]
        pl = E2.T @ (xk[k] - p2) - t["centre"]
        gap, nl, ql, region = sphere_box_general(pl, t["half"], rad)
        dist = gap + rad
        mag_pl = np.abs(E2).T @ (np.abs(xk[k]) + np.abs(p2)) + np.abs(t["centre"])
        mag_nl = np.where(ql != pl, 2.0 * mag_pl / abs(dist), 0.0) if region > 0 else np.zeros(3)
        depth = np.sort(t["half"] - np.abs(pl))
        out.append(dict(kind="trunk", lane=t["lane"], pair=(k, -1), body=sph[k]["body"], body2=t["body2"], rb=sph[k]["rb"], rb2=t["rb2"], rad=rad, rad2=0.0,
                        gap=gap, n=E2 @ nl, xc=p2 + E2 @ (t["centre"] + ql), mag_n=np.abs(E2) @ mag_nl, mag_gap=float(np.abs(nl) @ mag_pl) + float(t["half"].max()) + rad,
                        active=gap < cfg["margin"], feature=None, region=region, par=np.inf, pl=pl, mag_pl=mag_pl,
                        second=gap + (depth[1] - depth[0]) if region == 0 else np.inf))
    return out


def sphere_box_general(pl, half, rad):
    """sphere_box for a box of half extents half [3] about the origin of its frame."""
    ql = np.clip(pl, -half, half)
    clamped = ql != pl
    if clamped.any():
        d = pl - ql
        dist = float(np.linalg.norm(d))
        return dist - rad, d / dist, ql, int(clamped.sum())
    depth = half - np.abs(pl)
    ax = int(np.argmin(depth))
    nl = np.zeros(3)
    nl[ax] = 1.0 if pl[ax] >= 0 else -1.0
    ql = pl.copy()
    ql[ax] = nl[ax] * half[ax]
    return -float(depth[ax]) - rad, nl, ql, 0


def cone_solve(W, n, vn_tgt, mu, vref):
    """contact_solve of the spec (the 3x3 cone solve of ONE contact: the law itself) in fp64: (lam, class, near) with near = a decision of
    this solve (separating, stick / slide, the 0.05 fallback) within DECISION_BAND."""
    vn = float(n @ vref)
    band = lambda x, y: abs(x - y) <= DECISION_BAND * max(abs(x), abs(y), 1e-3)
    if vn >= vn_tgt:
        return np.zeros(3), "separating", band(vn, vn_tgt)
    near = band(vn, vn_tgt)
    nWn = float(n @ W @ n)
    lam_fl = (vn_tgt - vn) / nWn
    st = np.linalg.solve(W, n * vn_tgt - vref)
    ln = float(n @ st)
    lt = st - ln * n
    ltn = float(np.linalg.norm(lt))
    if mu * ln > 0 or ltn > 0:
        near = near or (ln > 0 and mu > 0 and abs(ltn / (mu * ln) - 1.0) <= DECISION_BAND)
    if ln > 0 and ltn <= mu * ln:
        return st, "stick", near
    vt = vref - vn * n
    vtn = float(np.linalg.norm(vt))
    if vtn > 1e-6:
        dirv = n - mu * vt / vtn
    elif ltn > 1e-12:
        dirv = n + mu * lt / ltn
    else:
        return n * lam_fl, "fallback", near
    den = float(n @ W @ dirv)
    near = near or abs(den / (0.05 * nWn) - 1.0) <= DECISION_BAND
    if den <= 0.05 * nWn:
        return n * lam_fl, "fallback", near
    return dirv * ((vn_tgt - vn) / den), "slide", near


def box_integrator(dt, b0, b1):
    """The box's semi-implicit Euler from its STORED new velocities, as forward_dynamics_reference.integrator_errors states the robot's:
    c1 = c0 + dt v1, quat1 = normalize(quat0 + dt/2 (w1, 0) (x) quat0). Ratios ([3], [4]) over |c0| + dt |v1| and |quat0| + dt/2 times
    the sizes of the quaternion product's summands (a component's two or three products can cancel)."""
    ep = fdr._ratio(np.abs(b1[0:3] - (b0[0:3] + dt * b1[7:10])), np.abs(b0[0:3]) + dt * np.abs(b1[7:10]))
    wx, wy, wz = b1[10:13]
    x, y, z, w = b0[3:7]
    qdot = 0.5 * np.array([wx * w + wy * z - wz * y, wy * w + wz * x - wx * z, wz * w + wx * y - wy * x, -wx * x - wy * y - wz * z])
    ax, ay, az, aw = np.abs(b0[3:7])
    bx, by, bz = np.abs(b1[10:13])
    mag = 0.5 * np.array([bx * aw + by * az + bz * ay, by * aw + bz * ax + bx * az, bz * aw + bx * ay + by * ax, bx * ax + by * ay + bz * az])
    want = b0[3:7] + dt * qdot
    nn = np.linalg.norm(want)
    et = fdr._ratio(np.abs(b1[3:7] - want / nn), np.abs(b0[3:7]) + dt * mag)
    return ep, et


# ----------------------------------------------------------------------------------------------------------------- the checker
def check_env(model, wmodel, tcfg, ter, root0, dof0, root1, dof1, ncf, fs, body_params, friction, box_mass, dropped, tau, timer0=0.0,
              timer1=None, spec=DEFAULT_SPEC, tangled=False):
    """Steps 1 to 7 for one env. Returns dict(left_out (None or "clamp", "margin", "feature"), exact [...], ratio {tier: ...},
    kind ("pair" / "corner" / None: what the one active contact is), cls, near, branch, mu, sphere, region, static, asleep, dyn (the
    dynamic slots within the margin: ("limbs", lane) / ("box", sphere)), feet (the foot spheres within the margin of the terrain))."""
    key = (bytes(wmodel), bytes(tcfg))
    if key not in _TABLES:
        _TABLES[key] = (clr.table_model(model, wmodel), clr.spheres(wmodel), fdr.tables(wmodel, tcfg), box_tables(wmodel), limb_tables(wmodel))
    tm, sph, tb, bt, lt = _TABLES[key]
    cfg = clr.law_cfg(tcfg)
    dt = cfg["dt"]
    root0, root1 = np.asarray(root0, dtype=np.float64), np.asarray(root1, dtype=np.float64)
    dof0, dof1 = np.asarray(dof0, dtype=np.float64), np.asarray(dof1, dtype=np.float64)
    ncf, fs = np.asarray(ncf, dtype=np.float64).reshape(-1, 3), np.asarray(fs, dtype=np.float64).reshape(-1, 6)
    tau = np.asarray(tau, dtype=np.float64).copy()
    tau[[c_ - 6 for c_ in fdr.FINGERS]] = 0.0
    out = dict(left_out=None, exact=[], ratio={t: 0.0 for t in TIERS}, kind=None, cls=None, near=False, branch=None, mu=None, sphere=None,
               region=None, static=None, asleep=False, ncontacts=0, forced=bool(np.any(ncf != 0)), feature=None, lane=None, contraction=None, sweeps=None)
    clamped = tb["qd_limit"] > 0
    lim = (tb["lo"] < tb["hi"]) & (np.arange(len(tb["lo"])) < 18)
    if not (np.abs(dof1[clamped, 1]) < tb["qd_limit"][clamped]).all():
        out["left_out"] = "clamp"
    elif tangled and float(dropped) != 0:
        out["left_out"] = "dropped"
    G = box_geometry(tm, sph, bt, ter, cfg, root0, dof0[:, 0], spec)
    g = G["robot"]
    internal = internal_geometry(lt, sph, g, cfg)
    # the dynamic slots in contact (limb pairs by lane, promoted box spheres) and the feet on the terrain: tests/decimation_reference.py
    out["dyn"] = frozenset([("limbs", p["lane"]) for p in internal if p["kind"] == "limbs" and p["active"]]
                           + [("box", p["sphere"]) for p in G["pairs"] if p["active"] and p["sphere"] in PROMOTED_BOX_SPHERES])
    out["feet"] = frozenset(int(k) for k in np.flatnonzero(g["active"][:4]))
    gaps =[(p["gap"], p["mag_gap"]) for p in internal] + [(p["gap"], p["mag_gap"]) for p in G["pairs"]] + [(cn["gap"], cn["mag_gap"]) for cn in G["corners"]] + list(zip(g["gap"], g["mag_gap"]))
    if out["left_out"] is None and any(abs(gp - cfg["margin"]) <= MARGIN_GUARD * EPS * mg for gp, mg in gaps):
        out["left_out"] = "margin"
    if out["left_out"] is None:
        # the discrete choices of the geometry: a clamp coordinate at the face plane, a centre at the surface, two faces equally near, a
        # corner at a cell border
        for p in G["pairs"]:
            if p["gap"] > 2 * cfg["margin"]:
                continue
            pl = p["pl"]
            tol = MARGIN_GUARD * EPS * p["mag_pl"]
            depth = np.sort(bt["half"] - np.abs(pl))
            if np.any(np.abs(np.abs(pl) - bt["half"]) <= tol) or (p["region"] == 0 and depth[1] - depth[0] <= tol.max()):
                out["left_out"] = "feature"
        if any(cn["near_border"] and cn["gap"] < 2 * cfg["margin"] for cn in G["corners"]):
            out["left_out"] = "feature"
        # a limb pair: its two best feature pairs equally near, or the shafts within a factor 2 of the parallel threshold; a trunk pair: as
        # the free box
        for p in internal:
            if p["gap"] > 2 * cfg["margin"]:
                continue
            if p["second"] - p["gap"] <= MARGIN_GUARD * EPS * p["mag_gap"] or 0.5 <= p["par"] <= 2.0:
                out["left_out"] = "feature"
            if p["kind"] == "trunk" and np.any(np.abs(np.abs(p["pl"]) - lt["trunk"][0]["half"]) <= MARGIN_GUARD * EPS * p["mag_pl"]):
                out["left_out"] = "feature"
    if out["left_out"] is not None:
        return out
    R0 = G["R0"]
    Rinv = np.linalg.inv(R0)
    mRinv = G["mR0"].T                                   # |R0^-1| up to the quaternion's rounding: the sizes of R0^T's summands
    m = float(box_mass)
    Ic = m * (2.0 / 3.0) * bt["half"] ** 2
    zero3, ident = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    # 7. the sleeping box
    nsleep = float(int(np.float32(bt["sleep_time"]) * (np.float32(1.0) / np.float32(dt)) + np.float32(0.5)))
    act_pairs = [p for p in G["pairs"] if p["active"]]
    act_corners = [cn for cn in G["corners"] if cn["active"]]
    act_int = [p for p in internal if p["active"]]
    vs2 = bt["sleep_speed"] ** 2
    resting = (root0[1, 7:10] @ root0[1, 7:10] < vs2 and (root0[1, 10:13] @ root0[1, 10:13]) * bt["half"] ** 2 < vs2
               and len(act_corners) >= 3 and not act_pairs) if bt["sleep_speed"] > 0 else False
    asleep = resting and float(timer0) >= nsleep
    out["asleep"] = asleep
    if timer1 is not None:
        want_t = min(float(timer0) + 1, nsleep) if resting else 0.0
        if float(timer1) != want_t:
            out["exact"].append(f"the sleep timer is {timer1}, not {want_t}")
    if asleep:
        act_corners = []
        if not np.array_equal(root1[1, 0:7], root0[1, 0:7]):
            out["exact"].append("the sleeping box moved")
        if np.any(root1[1, 7:13] != 0):
            out["exact"].append(f"the sleeping box has the velocity {root1[1, 7:13]}")
    # 2. activation
    if float(dropped) != 0:
        out["exact"].append(f"DROPPED_HITS is {dropped}")
    may = set()
    for k in np.flatnonzero(g["active"]):
        may.add(sph[k]["rb"])
    for p in act_pairs:
        may |= {sph[p["sphere"]]["rb"], BOX_ROW}
    if act_corners:
        may.add(BOX_ROW)
    for p in act_int:
        may |= {p["rb"], p["rb2"]}
    for rb in range(ncf.shape[0]):
        if np.any(ncf[rb] != 0) and rb not in may:
            out["exact"].append(f"row {rb} is {ncf[rb]} without an active contact")
    contacts = [("pair", p) for p in act_pairs] + [("corner", cn) for cn in act_corners] + [("tree", p) for p in act_int]
    out["ncontacts"] = len(contacts) + int(g["active"].sum())
    rb_count = {}
    for rb_ in [sph[k]["rb"] for k in np.flatnonzero(g["active"])] + [sph[p["sphere"]]["rb"] for p in act_pairs] + [r_ for p in act_int for r_ in (p["rb"], p["rb2"])]:
        rb_count[rb_] = rb_count.get(rb_, 0) + 1
    # (tangled: the multi-contact case -- activation, cone, sensors, root rows and box rows only, whatever the number of contacts)
    single = len(contacts) == 1 and not g["active"].any() and not tangled
    if single and contacts[0][0] == "pair":
        rbA = sph[contacts[0][1]["sphere"]]["rb"]
        if not np.array_equal(ncf[rbA], -ncf[BOX_ROW]):
            out["exact"].append(f"row {rbA} is {ncf[rbA]}, the box row {ncf[BOX_ROW]}: not minus each other")
    if single and contacts[0][0] == "tree":
        ra_, rb_ = contacts[0][1]["rb"], contacts[0][1]["rb2"]
        if not np.array_equal(ncf[ra_], -ncf[rb_]):
            out["exact"].append(f"row {ra_} is {ncf[ra_]}, row {rb_} {ncf[rb_]}: not minus each other")
    # kinematics in F, as contact_law_reference: velocities R0^T (world), accelerations and forces R0^-1 (world)
    dnu = (np.r_[root1[0, 7:13], dof1[:, 1]] - np.r_[root0[0, 7:13], dof0[:, 1]]) / dt
    nu0 = np.r_[R0.T @ root0[0, 7:10], R0.T @ root0[0, 10:13], dof0[:, 1]]
    a = np.r_[Rinv @ dnu[0:3], Rinv @ dnu[3:6], dnu[6:]]
    nu1 = nu0 + dt * a
    M = wb.mass_matrix(tm, zero3, ident, dof0[:, 0], body_params)
    arm = tb["armature"]
    gF = R0.T @ np.asarray(tb["gravity"])
    vb0, wb0 = R0.T @ root0[1, 7:10], R0.T @ root0[1, 10:13]
    ab, alb = Rinv @ (root1[1, 7:10] - root0[1, 7:10]) / dt, Rinv @ (root1[1, 10:13] - root0[1, 10:13]) / dt
    mag_vb = G["mR0"].T @ (np.abs(root0[1, 7:10]) + np.abs(root1[1, 7:10]))
    mag_wb = G["mR0"].T @ (np.abs(root0[1, 10:13]) + np.abs(root1[1, 10:13]))
    fbox = Rinv @ ncf[BOX_ROW]
    # 6b. the box's own motion (asleep: checked exactly above)
    if not asleep:
        res = m * (ab - gF) - fbox
        fpairs = [Rinv @ ncf[rb_] for rb_ in sorted({sph[p["sphere"]]["rb"] for p in act_pairs})]
        sc = m * (mRinv @ (np.abs(root0[1, 7:10]) + np.abs(root1[1, 7:10])) / dt + np.abs(gF)) + np.abs(fbox + sum(fpairs)) + sum(np.abs(f_) for f_ in fpairs)
        box = clr._ratio(res, sc)
        out["detail"] = dict(lin=box)
        if single:
            kind, ct = contacts[0]
            f_on_box = fbox
            r = ct["xc"] - G["c"]
            mag_r = np.abs(G["c"]) + np.abs(ct["xc"])
            res = Ic * alb - wb.cross3(r, f_on_box)
            sc = Ic * (mRinv @ (np.abs(root0[1, 10:13]) + np.abs(root1[1, 10:13]))) / dt + _cross_abs(np.abs(r) + mag_r, f_on_box)
            box = max(box, clr._ratio(res, sc))
            out["detail"]["ang"] = clr._ratio(res, sc)
        elif not contacts:
            box = max(box, clr._ratio(Ic * alb, Ic * (mRinv @ (np.abs(root0[1, 10:13]) + np.abs(root1[1, 10:13]))) / dt))
        ep, et = box_integrator(dt, root0[1], root1[1])
        out["detail"].update(pos=float(ep.max()), quat=float(et.max()))
        out["ratio"]["box"] = max(box, float(ep.max()), float(et.max()))
    # 6a. the robot's equations of motion, every row
    F = []
    idt, mag_id = idr.inverse_dynamics(tm, zero3, ident, dof0[:, 0], nu0, a, body_params, gF, forces=F)
    t_lim = fdr.limit_torque(tm, tb, M, dof0[:, 0], dof0[:, 1])
    res = idt + arm * a - np.r_[np.zeros(6), tau + t_lim]
    sc = mag_id + np.abs(arm * a) + np.r_[np.zeros(6), np.abs(tau) + np.abs(t_lim)] + (np.abs(M) + np.diag(arm)) @ (np.abs(nu0) + np.abs(nu1)) / dt
    sc[6:] += fdr.base_origin_levers(tm, g["E"], g["p"], F)
    eom_ok = not g["active"].any() and len(act_pairs) + len(act_int) <= 1 and not tangled
    for p in act_int:
        JA = wb.point_jacobian(tm, g["E"], g["p"], p["body"], p["xc"])[0:3]
        JB = wb.point_jacobian(tm, g["E"], g["p"], p["body2"], p["xc"])[0:3]
        f = Rinv @ ncf[p["rb"]]
        res -= (JA + spec["partner_sign"] * JB).T @ f
        sc += (np.abs(JA) + np.abs(JB)).T @ np.abs(f)
    for p in act_pairs:
        s = sph[p["sphere"]]
        J = wb.point_jacobian(tm, g["E"], g["p"], s["body"], p["xc"])[0:3]
        f = Rinv @ ncf[s["rb"]]
        res -= J.T @ f
        sc += np.abs(J).T @ np.abs(f)
    res[fdr.FINGERS], sc[fdr.FINGERS] = a[fdr.FINGERS], 0.0
    if eom_ok:
        out["ratio"]["mom"] = clr._ratio(res[0:6], sc[0:6])
        out["ratio"]["eom"] = clr._ratio(res[6:], sc[6:])
    else:
        # any number of contacts: the root rows carry no joint torque and an internal pair cancels in them. Linear rows: the sum of the
        # robot's rows; angular rows (no terrain contact, every box pair the only contact of its rigid body): xc x f of the box pairs
        fF = ncf[:BOX_ROW] @ Rinv.T
        resm = idt[0:6].copy()
        scm = mag_id[0:6] + (np.abs(M[0:6]) @ (np.abs(nu0) + np.abs(nu1))) / dt
        resm[0:3] -= fF.sum(0)
        scm[0:3] += np.abs(fF).sum(0)
        rows = slice(0, 3)
        if not g["active"].any() and all(rb_count[sph[p["sphere"]]["rb"]] == 1 for p in act_pairs):
            for p in act_pairs:
                f = fF[sph[p["sphere"]]["rb"]]
                resm[3:6] -= wb.cross3(p["xc"], f)
                scm[3:6] += _cross_abs(p["xc"], f)
            for p in act_int:                                             # +f and -f at one point: the levers' products, which cancel
                if rb_count[p["rb"]] == 1:
                    scm[3:6] += 2.0 * _cross_abs(p["xc"], fF[p["rb"]])
                else:
                    scm[3:6] += 2.0 * _cross_abs(p["xc"], np.abs(fF[p["rb"]]) + np.abs(fF[p["rb2"]]))
            rows = slice(0, 6)
        out["ratio"]["mom"] = clr._ratio(resm[rows], scm[rows])
    bent = {}

    def the_law(kind, ct):
        """3. the velocity-level law of the one active contact; returns the slide term of the cone scale."""
        n, mag_n, xc, gap = spec["normal_sign"] * ct["n"], ct["mag_n"], ct["xc"], float(ct["gap"])
        r = xc - (zero3 if spec["box_about_origin"] else G["c"])
        mag_r = np.abs(G["c"]) + np.abs(xc)
        vbox = vb0 + wb.cross3(wb0, r) + dt * wb.cross3(wb0, wb.cross3(wb0, r)) + dt * (ab + wb.cross3(alb, r))
        sc_box = mag_vb + _cross_abs(mag_wb, r) + _cross_abs(np.abs(wb0) + dt * np.abs(alb), mag_r) + dt * (wb0 @ wb0) * np.abs(r)
        Wbox = np.eye(3) * (1.0 / m + (r @ r) / Ic) - np.outer(r, r) / Ic
        if kind == "pair":
            s = sph[ct["sphere"]]
            out.update(sphere=ct["sphere"], region=ct["region"], static=ct["sphere"] in STATIC_BOX_SPHERES)
            J = wb.point_jacobian(tm, g["E"], g["p"], s["body"], xc)
            acc, mag = cdr.body_accelerations(tm, zero3, ident, dof0[:, 0], nu0)
            origin = g["p"][s["body"]] + g["E"][s["body"]] @ tm.rb_offset[s["rb"]]
            lever, om, al = xc - origin, J[3:6] @ nu0, acc[s["rb"], 3:6]
            jdnu = acc[s["rb"], 0:3] + wb.cross3(al, lever) + wb.cross3(om, wb.cross3(om, lever))
            mag_jdnu = mag[s["rb"], 0] + (np.linalg.norm(al) + np.linalg.norm(om) ** 2) * np.linalg.norm(lever)
            Jp = J[0:3]
            vplus = Jp @ nu0 + dt * (Jp @ a + jdnu) - vbox
            W = Jp[:, LIVE] @ np.linalg.solve((M + np.diag(arm))[np.ix_(LIVE, LIVE)], Jp[:, LIVE].T) + Wbox
            scale = np.abs(Jp) @ (np.abs(nu0) + np.abs(nu1)) + dt * mag_jdnu + sc_box
            f = Rinv @ ncf[s["rb"]]
            mu_raw = (bt["friction"],) if spec["mu_with_terrain"] else (bt["friction"], float(friction))
            forced = bool(np.any(ncf[s["rb"]] != 0))
        else:
            out.update(sphere=ct["corner"], region=ct["tri"], static=None)
            vplus, W, scale, f = vbox, Wbox, sc_box, fbox
            mu_raw = (bt["friction"], cfg["terrain_friction"])
            forced = bool(np.any(ncf[BOX_ROW] != 0))
        mu, mu_mag = max(0.0, float(np.mean(mu_raw))), float(np.mean(np.abs(mu_raw)))
        out["mu"] = mu
        lam = f * dt
        vfree = vplus - W @ lam
        vn_tgt, mag_vn, branch = clr.vn_target(cfg, gap, ct["mag_gap"])
        out["branch"] = branch
        scale = scale + np.abs(W) @ np.abs(lam) + np.abs(n) * mag_vn + mag_n * abs(vn_tgt)
        scale_n = float(np.abs(n) @ scale + mag_n @ np.abs(vplus))
        vn_free, vt_free = clr._tangent(vfree, n)
        vtn = float(np.linalg.norm(vt_free))
        st = np.linalg.solve(W, n * vn_tgt - vfree)
        ln, lt = clr._tangent(st, n)
        ltn = float(np.linalg.norm(lt))
        vel = out["ratio"]["vel"]
        if vn_free >= vn_tgt:
            out["cls"] = "separating"
            out["near"] = abs(vn_free - vn_tgt) <= DECISION_BAND * max(abs(vn_tgt), abs(vn_free), 1e-3)
        elif ln > 0 and ltn <= mu * ln:
            out["cls"] = "stick"
            out["near"] = abs(ltn / (mu * ln) - 1.0) <= DECISION_BAND
        else:
            out["cls"] = "slide"
            out["near"] = mu > 0 and ln > 0 and abs(ltn / (mu * ln) - 1.0) <= DECISION_BAND
            if vtn > 1e-6 and mu > 0:
                nWn = float(n @ W @ n)
                den = float(n @ W @ (n - mu * vt_free / vtn))
                out["near"] = out["near"] or abs(den / (0.05 * nWn) - 1.0) <= DECISION_BAND
                if den <= 0.05 * nWn:
                    out["cls"] = "fallback"
        if out["cls"] != "separating":
            out["near"] = out["near"] or abs(vn_free - vn_tgt) <= DECISION_BAND * max(abs(vn_tgt), abs(vn_free), 1e-3)
        if not forced:
            out["ratio"]["vel"] = max(vel, clr._ratio(max(0.0, vn_tgt - float(n @ vplus)), scale_n))
            return 0.0
        vel = max(vel, clr._ratio(max(0.0, vn_free - vn_tgt), scale_n), clr._ratio(float(n @ vplus) - vn_tgt, scale_n))
        fn, ftan = clr._tangent(f, n)
        mag_fn = float(np.abs(f) @ mag_n)
        mag_ft = float(np.linalg.norm(np.abs(f) + mag_fn * np.abs(n) + abs(fn) * mag_n))
        bent_ = mu_mag * (2.0 * float(np.abs(vfree) @ mag_n) + abs(vn_free) * 2.0 * float(np.abs(n) @ mag_n)) / vtn if vtn > 1e-6 else 0.0
        if out["cls"] != "separating" and not out["near"]:
            if out["cls"] == "stick":
                vel = max(vel, clr._ratio(vplus - n * vn_tgt, scale))
            elif out["cls"] == "fallback":
                out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(np.linalg.norm(ftan), mag_ft))
            else:
                out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(np.linalg.norm(ftan) - mu * fn, mag_ft + mu_mag * mag_fn * (1.0 + bent_)))
                if mu > 0 and vtn > SLIDE_SPEED:
                    ftn = float(np.linalg.norm(ftan))
                    resd = np.linalg.norm(ftan / ftn + vt_free / vtn) if ftn > 0 else np.inf
                    out["ratio"]["dir"] = max(out["ratio"]["dir"], clr._ratio(resd, (mag_ft / ftn if ftn > 0 else 0.0) + np.linalg.norm(scale) / vtn))
        out["ratio"]["vel"] = vel
        # 4. cone and sign of the one contact
        out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(max(0.0, -fn), mag_fn),
                                   clr._ratio(max(0.0, np.linalg.norm(ftan) - mu * fn), mag_ft + mu_mag * mag_fn * (1.0 + bent_)))
        return bent_

    def point_motion(body, xc, acc, mag):
        """(J_p, v+, scale) of the body-fixed point at xc on moving body `body`: v+ = J_p nu0 + dt (J_p a + Jdot_p nu0)."""
        rb = list(tm.rb_body).index(body)
        J = wb.point_jacobian(tm, g["E"], g["p"], body, xc)
        origin = g["p"][body] + g["E"][body] @ tm.rb_offset[rb]
        lever, om, al = xc - origin, J[3:6] @ nu0, acc[rb, 3:6]
        jdnu = acc[rb, 0:3] + wb.cross3(al, lever) + wb.cross3(om, wb.cross3(om, lever))
        mag_jdnu = mag[rb, 0] + (np.linalg.norm(al) + np.linalg.norm(om) ** 2) * np.linalg.norm(lever)
        Jp = J[0:3]
        return Jp, Jp @ nu0 + dt * (Jp @ a + jdnu), np.abs(Jp) @ (np.abs(nu0) + np.abs(nu1)) + dt * mag_jdnu

    def the_tree_law(ct):
        """3. a robot-internal pair alone in its env: the law ITERATED as the spec's four block-Jacobi sweeps iterate it."""
        n, mag_n, xc, gap = spec["normal_sign"] * ct["n"], ct["mag_n"], ct["xc"], float(ct["gap"])
        out.update(sphere=ct["pair"][0], region=ct["region"], feature=ct["feature"], lane=ct["lane"], static=None)
        acc, mag = cdr.body_accelerations(tm, zero3, ident, dof0[:, 0], nu0)
        JA, vA, scA = point_motion(ct["body"], xc, acc, mag)
        JB, vB, scB = point_motion(ct["body2"], xc, acc, mag)
        Minv = np.linalg.inv((M + np.diag(arm))[np.ix_(LIVE, LIVE)])
        Jr = (JA - JB)[:, LIVE]
        Wt = Jr @ Minv @ Jr.T
        Wu = JA[:, LIVE] @ Minv @ JA[:, LIVE].T + JB[:, LIVE] @ Minv @ JB[:, LIVE].T + 1e-6 * np.eye(3)
        if spec["converged"]:
            Wu = Wt
        out["contraction"] = float(np.linalg.norm(np.eye(3) - Wt @ np.linalg.inv(Wu), 2))
        vplus = vA - vB
        f = Rinv @ ncf[ct["rb"]]
        lam = f * dt
        forced = bool(np.any(ncf[ct["rb"]] != 0))
        vfree = vplus - Wt @ lam
        mu_raw = (float(friction), cfg["terrain_friction"]) if spec["mu_with_terrain"] else (float(friction),)
        mu, mu_mag = max(0.0, float(np.mean(mu_raw))), float(np.mean(np.abs(mu_raw)))
        out["mu"] = mu
        vn_tgt, mag_vn, branch = clr.vn_target(cfg, gap, ct["mag_gap"])
        out["branch"] = branch
        lk, classes, near, vref = np.zeros(3), [], False, vfree
        for _ in range(spec["sweeps"]):
            vref = vfree + (Wt - Wu) @ lk
            lk, cls_k, near_k = cone_solve(Wu, n, vn_tgt, mu, vref)
            classes.append(cls_k)
            near = near or near_k
        out["cls"], out["near"], out["sweeps"] = classes[-1], near, classes
        scale = scA + scB + (np.abs(Wt) + np.abs(Wu)) @ (np.abs(lam) + np.abs(lk)) + np.abs(n) * mag_vn + mag_n * abs(vn_tgt)
        scale_n = float(np.abs(n) @ scale + mag_n @ (np.abs(vplus) + np.abs(vref)))
        if near:
            return
        if all(c_ == "separating" for c_ in classes):
            if forced:
                out["exact"].append(f"a separating pair (lane {ct['lane']}) carries the force {f}")
            out["ratio"]["vel"] = max(out["ratio"]["vel"], clr._ratio(max(0.0, vn_tgt - float(n @ vplus)), scale_n))
            return
        # the last sweep's impulse is dir (vn_tgt - n.vref) / (n.W_u dir): what is rounded along n (scale_n) comes back through W_u dir / (n.W_u dir),
        # which grows as friction eats the normal response (up to 20 at the fallback's threshold); a sticking contact has no such term
        vn_l, vt_l = clr._tangent(vref, n)
        vtn_l = float(np.linalg.norm(vt_l))
        dir_l = n - mu * vt_l / vtn_l if classes[-1] == "slide" and vtn_l > 1e-6 else n
        amp = np.zeros(3) if classes[-1] == "stick" else np.abs(Wu @ dir_l) / abs(float(n @ Wu @ dir_l))
        out["ratio"]["vel"] = max(out["ratio"]["vel"], clr._ratio(Wu @ (lam - lk), scale + amp * scale_n))
        if not forced:
            return
        fn, ftan = clr._tangent(f, n)
        mag_fn = float(np.abs(f) @ mag_n)
        mag_ft = float(np.linalg.norm(np.abs(f) + mag_fn * np.abs(n) + abs(fn) * mag_n))
        vn_ref, vt_ref = clr._tangent(vref, n)
        vtn = float(np.linalg.norm(vt_ref))
        bent_ = mu_mag * (2.0 * float(np.abs(vref) @ mag_n) + abs(vn_ref) * 2.0 * float(np.abs(n) @ mag_n)) / vtn if vtn > 1e-6 else 0.0
        if classes[-1] == "slide":
            out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(np.linalg.norm(ftan) - mu * fn, mag_ft + mu_mag * mag_fn * (1.0 + bent_)))
            if mu > 0 and vtn > SLIDE_SPEED:
                ftn = float(np.linalg.norm(ftan))
                resd = np.linalg.norm(ftan / ftn + vt_ref / vtn) if ftn > 0 else np.inf
                out["ratio"]["dir"] = max(out["ratio"]["dir"], clr._ratio(resd, (mag_ft / ftn if ftn > 0 else 0.0) + np.linalg.norm(scale) / vtn))
        elif classes[-1] == "fallback":
            out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(np.linalg.norm(ftan), mag_ft))
        out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(max(0.0, -fn), mag_fn),
                                   clr._ratio(max(0.0, np.linalg.norm(ftan) - mu * fn), mag_ft + mu_mag * mag_fn * (1.0 + bent_)))

    if single and contacts[0][0] == "tree":
        the_tree_law(contacts[0][1])
    elif single:
        the_law(*contacts[0])
    else:
        # 4. cone and sign of every pair whose force can be read off a row: the only contact of its robot body
        for p in act_pairs:
            s = sph[p["sphere"]]
            if rb_count[s["rb"]] != 1:
                continue
            f, n, mag_n = Rinv @ ncf[s["rb"]], p["n"], p["mag_n"]
            mu, mu_mag = max(0.0, 0.5 * (bt["friction"] + float(friction))), 0.5 * (abs(bt["friction"]) + abs(float(friction)))
            fn, ftan = clr._tangent(f, n)
            mag_fn = float(np.abs(f) @ mag_n)
            mag_ft = float(np.linalg.norm(np.abs(f) + mag_fn * np.abs(n) + abs(fn) * mag_n))
            out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(max(0.0, -fn), mag_fn),
                                       clr._ratio(max(0.0, np.linalg.norm(ftan) - mu * fn), mag_ft + mu_mag * mag_fn))
    if not single:
        for p in act_int:
            if rb_count[p["rb"]] != 1 or rb_count[p["rb2"]] != 1:
                continue
            if not np.array_equal(ncf[p["rb"]], -ncf[p["rb2"]]):
                out["exact"].append(f"row {p['rb']} is {ncf[p['rb']]}, row {p['rb2']} {ncf[p['rb2']]}: not minus each other")
            f, n, mag_n = Rinv @ ncf[p["rb"]], p["n"], p["mag_n"]
            mu, mu_mag = max(0.0, float(friction)), abs(float(friction))
            fn, ftan = clr._tangent(f, n)
            mag_fn = float(np.abs(f) @ mag_n)
            mag_ft = float(np.linalg.norm(np.abs(f) + mag_fn * np.abs(n) + abs(fn) * mag_n))
            out["ratio"]["cone"] = max(out["ratio"]["cone"], clr._ratio(max(0.0, -fn), mag_fn),
                                       clr._ratio(max(0.0, np.linalg.norm(ftan) - mu * fn), mag_ft + mu_mag * mag_fn))
    # 5. sensors: a foot in a pair with the box (no terrain contact on that foot)
    feet = list(tb["feet_rb"])
    in_pair = {sph[p["sphere"]]["rb"]: p for p in act_pairs}
    for ft, rb in enumerate(feet):
        if np.any(g["active"][[k for k, s in enumerate(sph) if s["rb"] == rb]]):
            continue
        if not np.any(ncf[rb] != 0):
            if np.any(fs[ft] != 0):
                out["exact"].append(f"sensor {ft} is {fs[ft]} without a force")
            continue
        if rb not in in_pair or rb_count[rb] != 1:
            continue
        p = in_pair[rb]
        s = sph[p["sphere"]]
        f, n, rad = Rinv @ ncf[rb], p["n"], float(g["rad"][p["sphere"]])
        Rb_ = g["E"][s["body"]]
        want = np.r_[Rb_.T @ f, Rb_.T @ wb.cross3(spec["lever_sign"] * (-rad) * n, f)]
        fnorm = float(np.linalg.norm(f))
        out["ratio"]["sensor"] = max(out["ratio"]["sensor"], clr._ratio(fs[ft] - want, np.full(6, fnorm + rad * fnorm * (1.0 + float(np.abs(p["mag_n"]).max())))))
    # ... or in a limb pair, on either side of it (single-contact envs: the force is the row)
    for ct in act_int:
        for side, (rb, body, lever) in enumerate(((ct["rb"], ct["body"], -ct["rad"]), (ct["rb2"], ct["body2"], ct["rad2"]))):
            if rb not in feet or not np.any(ncf[rb] != 0) or rb_count[rb] != 1:
                continue
            ft = feet.index(rb)
            f = Rinv @ ncf[rb]
            Rb_ = g["E"][body]
            want = np.r_[Rb_.T @ f, Rb_.T @ wb.cross3(spec["lever_sign"] * lever * ct["n"], f)]
            fnorm = float(np.linalg.norm(f))
            out["ratio"]["sensor"] = max(out["ratio"]["sensor"], clr._ratio(fs[ft] - want, np.full(6, fnorm + abs(lever) * fnorm * (1.0 + float(np.abs(ct["mag_n"]).max())))))
    return out


def contact_list(robot, tcfg, ter, root, q, asleep_timer=False):
    """{slot: dict(n, xc, nshare)} of the active contacts of one env as the spec lays them out: the terrain spheres and the static pairs in
    their own slots; the broad phase's hits (bounding spheres; limb pairs then the shafts' segments against LIMB_RSUM_MAX) promoted in
    ascending order of lane, limb pairs into the dynamic slots outside the box row, spheres against the free box into 45..47; the
    corners of a sleeping box dropped; nshare the larger contact count of the contact's two bodies."""
    model, wmodel = robot["model"], robot["wmodel"]
    tm, sph, bt, lt = clr.table_model(model, wmodel), clr.spheres(wmodel), box_tables(wmodel), limb_tables(wmodel)
    cfg = clr.law_cfg(tcfg)
    G = box_geometry(tm, sph, bt, ter, cfg, root, q)
    g = G["robot"]
    internal = internal_geometry(lt, sph, g, cfg)
    xk = g["xc"] + g["rad"][:, None] * g["n"]
    extra = cfg["margin"] + 1e-3
    found = []                                                                  # (slot, body a, body b or None, contact)
    for k in np.flatnonzero(g["active"]):
        found.append((sph[k]["slot"], sph[k]["body"], None, dict(n=g["n"][k], xc=g["xc"][k])))
    free = list(abi.DYN_SELF_SLOTS)
    for p in internal:
        if p["kind"] == "trunk":
            if p["active"]:
                found.append((p["lane"], p["body"], p["body2"], p))
            continue
        A, B = lt["limbs"][p["pair"][0]], lt["limbs"][p["pair"][1]]
        ca, cb = 0.5 * (xk[A["s0"]] + xk[A["s1"]]), 0.5 * (xk[B["s0"]] + xk[B["s1"]])
        if np.linalg.norm(ca - cb) >= bt["limb_reach"][p["lane"]] + extra:
            continue
        pa, pb, _ = seg_closest(xk[A["s0"]], xk[A["s1"]], xk[B["s0"]], xk[B["s1"]])
        if np.linalg.norm(pa - pb) >= abi.LIMB_RSUM_MAX + lt["rest"] + extra:
            continue
        slot = free.pop(0)
        if p["active"]:
            found.append((slot, p["body"], p["body2"], p))
    free = list(abi.DYN_BOX_SLOTS)
    by_sphere = {p["sphere"]: p for p in G["pairs"]}
    for k in STATIC_BOX_SPHERES:
        if by_sphere[k]["active"]:
            found.append((bt["pair_slot"][k], sph[k]["body"], "box", by_sphere[k]))
    for lane, k in bt["cand_lanes"]:
        if by_sphere[k]["centre_dist"] >= bt["reach"][k] + extra:
            continue
        slot = free.pop(0)
        if by_sphere[k]["active"]:
            found.append((slot, sph[k]["body"], "box", by_sphere[k]))
    corners = [cn for cn in G["corners"] if cn["active"]]
    vs2 = bt["sleep_speed"] ** 2
    resting = (root[1, 7:10] @ root[1, 7:10] < vs2 and (root[1, 10:13] @ root[1, 10:13]) * bt["half"] ** 2 < vs2 and len(corners) >= 3
               and not any(b == "box" for _, _, b, _ in found))
    if not (resting and asleep_timer):
        for cn in corners:
            found.append((bt["corners"][cn["corner"]]["slot"], "box", None, cn))
    cnt = {}
    for _, a_, b_, _ in found:
        for x in (a_, b_):
            if x is not None:
                cnt[x] = cnt.get(x, 0) + 1
    return {slot: dict(n=ct["n"], xc=ct["xc"], nshare=max(cnt[a_], cnt.get(b_, 0))) for slot, a_, b_, ct in found}


def assert_caps_and_coverage(name, s):
    """The conditions on a case's draws (summary s of any sim): at least 85 % checked, margin + feature + decision band at most 2 %, and the
    coverage counts of L-264, B-255 and T-96."""
    assert s["exact"] == [], s["exact"][:8]
    assert s["checked"] >= MIN_ELIGIBLE * s["n"], (name, s["checked"], s["n"], s["left_out"])
    assert s["left_out"].get("margin", 0) + s["left_out"].get("feature", 0) + s["near"] <= MAX_LEFT_OUT * s["n"], (name, s["left_out"], s["near"])
    assert set(s["left_out"]) <= {"margin", "feature", "clamp", "reset", "dropped"}
    if name in STEP_CASES:
        assert s["left_out"].get("reset", 0) <= 0.05 * s["n"]
    if name == "M-256":
        assert s["left_out"].get("dropped", 0) <= 0.10 * s["n"] and s["multi"] >= 10 * MIN_COUNT, (s["left_out"], s["multi"])
    if name in CASES and CASES[name]["kind"] not in ("sleep", "tangled"):
        assert s["single"] == s["checked"]                                   # every checked env has exactly one active contact
    if name in ("L-264", "B-255"):
        assert min(s["classes"][c] for c in ("separating", "stick", "slide")) >= MIN_COUNT, s["classes"]
        assert s["mu0"] >= MIN_COUNT and min(s["branches"]) >= MIN_COUNT, (s["mu0"], s["branches"])
    if name == "L-264":
        assert min(s["features"]) >= MIN_COUNT, s["features"]
    if name == "B-255":
        assert sorted(s["spheres"]) == sorted(BOX_SPHERES) and min(s["spheres"].values()) >= MIN_COUNT, s["spheres"]
        assert s["static"] >= MIN_COUNT and s["promoted"] >= MIN_COUNT and all(s["regions"].get(r, 0) >= MIN_COUNT for r in range(4)), s["regions"]
    if name == "T-96":
        assert sorted(s["spheres"]) == [8, 10] and min(s["spheres"].values()) >= MIN_COUNT, s["spheres"]
        assert all(s["regions"].get(r, 0) >= MIN_COUNT for r in (0, 1, 2, 3)), s["regions"]
    if name in ("K-128", "K-128-grid"):
        assert sorted(s["spheres"]) == list(range(8)) and min(s["spheres"].values()) >= MIN_COUNT
        assert min(s["classes"][c] for c in ("separating", "slide")) >= MIN_COUNT and min(s["branches"]) >= MIN_COUNT
    if name == "S-64":
        assert s["asleep"] == s["n"] // 2 and s["forced"] >= s["checked"] - s["asleep"] - 2      # the awake half: the corners carry the box


# ------------------------------------------------------------------------------------------------------------ case generators
def _sdf_box(pl, half):
    """Signed distance of points pl [..., 3] (box frame) to the cube's surface."""
    d = np.abs(pl) - half
    return np.linalg.norm(np.maximum(d, 0.0), axis=-1) + np.minimum(d.max(-1), 0.0)


def _rand_quat(rng, m):
    q = rng.normal(size=(m, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _robot_draw(rng, tm, tb, tcfg, m, spread=0.6):
    """Joint positions default +- spread, 0.05 rad inside the limits, |qd| <= 2 legs / 1 arm."""
    lim = tb["lo"] < tb["hi"]
    q = np.array([float(x) for x in tcfg.default_dof_pos])[None] + rng.uniform(-spread, spread, (m, 20))
    q[:, lim] = np.clip(q[:, lim], tb["lo"][lim] + 0.05, tb["hi"][lim] - 0.05)
    q[:, 18:] = 0
    qd = np.zeros((m, 20))
    qd[:, :12], qd[:, 12:18] = rng.uniform(-2, 2, (m, 12)), rng.uniform(-1, 1, (m, 6))
    return q, qd


def _self_gap(tm, names, R, p, quat):
    """Smallest gap [m] over every self-collision pair of tests/self_collision_geometry.py."""
    rbs = np.zeros((len(p), len(names), 7))
    rbs[:, :, 0:3] = np.stack([p[:, b] + R[:, b] @ tm.rb_offset[r] for r, b in enumerate(tm.rb_body)], axis=1)
    rbs[:, names.index("trunk"), 3:7] = quat
    return np.min(np.stack(list(scg.all_pairs(rbs, names).values()), 0), axis=0)


def _point_velocity(tm, R, p, qd, omega, body, x):
    """World velocity [m, 3] of the points x [m, 3] (relative to the root) riding on the bodies `body` [m], the root's origin at rest."""
    m = len(qd)
    w, v = np.zeros((m, tm.nb, 3)), np.zeros((m, tm.nb, 3))
    w[:, 0] = omega
    for b in range(1, tm.nb):
        par = tm.parent[b]
        w[:, b] = w[:, par] + R[:, b][:, :, tm.axis[b]] * qd[:, tm.body_dof[b]][:, None]
        v[:, b] = v[:, par] + np.cross(w[:, par], p[:, b] - p[:, par])
    ar = np.arange(m)
    return v[ar, body] + np.cross(w[ar, body], x - p[ar, body])


def _wanted_velocity(rng, cfg, gap, n, deficit):
    """The relative velocity of the contact point that the draw asks for: vn_tgt + U(deficit) along n, a tangential speed of U(0, 1.2)
    times that deficit (separating, stick and slide all occur)."""
    m = len(gap)
    vn_tgt = np.array([clr.vn_target(cfg, g_, 0.0)[0] for g_ in gap])
    short = rng.uniform(deficit[0], deficit[1], m)
    t1 = np.cross(n, rng.normal(size=(m, 3)))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    return n * (vn_tgt + short)[:, None] + t1 * (rng.uniform(0, 1.2, m) * np.maximum(np.abs(short), 0.05))[:, None]


def box_pair_states(model, wmodel, tcfg, targets, seed, deficit=(-1.5, 0.5)):
    """(root [n, 2, 13], dof [n, 20, 2], tau [n, 20]) float32, one env per entry of `targets` (robot sphere indices): the robot 1.2 m up at
    a uniformly random attitude, joints default +- 0.6, and the free box (random attitude and spin |w| <= 5) placed against the target
    sphere: a point of its surface in the face (40 %), edge (25 %) or corner (20 %) region of the clamp at a gap from
    (-min(12 mm, rad - 3 mm), margin - 0.5 mm), or (15 %) the sphere's centre 1 to 12 mm INSIDE a face. The box's velocity gives the
    contact point the relative velocity of _wanted_velocity. Rejected unless every other of the 17 spheres clears the box by margin + 5
    mm, every self-collision pair clears by margin + 5 mm and at most three promotable spheres pass the broad phase."""
    rng = np.random.default_rng(seed)
    tm, sph, tb, bt = clr.table_model(model, wmodel), clr.spheres(wmodel), fdr.tables(wmodel, tcfg), box_tables(wmodel)
    cfg = clr.law_cfg(tcfg)
    targets = np.asarray(targets, dtype=int)
    n, half = len(targets), bt["half"]
    rad = np.array([s["rad"] for s in sph])
    names = list(model.rb_names)
    root, dof = np.zeros((n, 2, 13)), np.zeros((n, 20, 2))
    done = np.zeros(n, dtype=bool)
    for _ in range(200):
        left = np.flatnonzero(~done)
        if len(left) == 0:
            break
        todo = np.repeat(left, min(16, max(1, 1024 // len(left))))
        m = len(todo)
        ar = np.arange(m)
        tg = targets[todo]
        q, qd = _robot_draw(rng, tm, tb, tcfg, m)
        quat = _rand_quat(rng, m)
        R, p = clr._batch_fk(tm, quat, q)
        cen = np.stack([p[:, s["body"]] + R[:, s["body"]] @ s["pos"] for s in sph], axis=1)           # relative to the root
        pr = np.c_[rng.uniform(-1, 1, (m, 2)), np.full(m, 1.2)]
        qb = _rand_quat(rng, m)
        Rb = scg.rotm(qb)
        kind = rng.random(m)
        nclamp = np.where(kind < 0.40, 1, np.where(kind < 0.65, 2, np.where(kind < 0.85, 3, 0)))
        order = np.argsort(rng.random((m, 3)), axis=1)
        sign = rng.choice([-1.0, 1.0], (m, 3))
        ql = rng.uniform(-0.9 * half, 0.9 * half, (m, 3))
        nl = np.zeros((m, 3))
        for j in range(3):
            ax = order[:, j]
            on = j < np.maximum(nclamp, 1)
            ql[ar[on], ax[on]] = sign[ar[on], ax[on]] * half
            nl[ar[on], ax[on]] = sign[ar[on], ax[on]] * (0.15 + np.abs(rng.normal(size=m)))[on]
        nl /= np.linalg.norm(nl, axis=1, keepdims=True)
        rt = rad[tg]
        gap = rng.uniform(-np.minimum(0.012, rt - 0.003), cfg["margin"] - 5e-4)
        inside = nclamp == 0
        ql[inside] = np.where(nl[inside] != 0, ql[inside], rng.uniform(-0.6 * half, 0.6 * half, (int(inside.sum()), 3)))
        depth = rng.uniform(0.001, 0.012, m)
        gap = np.where(inside, -depth - rt, gap)
        pl = ql + nl * (gap + rt)[:, None]
        ct = cen[ar, tg]
        cb = ct - np.einsum("mij,mj->mi", Rb, pl)                                                # box centre relative to the root
        plo = np.einsum("mji,mkj->mki", Rb, cen[:, BOX_SPHERES] - cb[:, None, :])
        gaps = _sdf_box(plo, half) - rad[BOX_SPHERES][None]
        gaps[ar, [BOX_SPHERES.index(t) for t in tg]] = np.inf
        ok = (gaps > cfg["margin"] + 5e-3).all(1)
        dcen = np.linalg.norm(cen[:, PROMOTED_BOX_SPHERES] - cb[:, None, :], axis=-1)
        reach = np.array([bt["reach"][k] for k in PROMOTED_BOX_SPHERES]) + cfg["margin"] + 1e-3
        ok &= (dcen < reach[None] + 1e-3).sum(1) <= 3
        if not ok.any():
            continue
        cand = np.flatnonzero(ok)
        ok[cand] = _self_gap(tm, names, R[cand], p[cand], quat[cand]) > cfg["margin"] + 5e-3
        omega, vroot = rng.uniform(-2, 2, (m, 3)), rng.uniform(-0.5, 0.5, (m, 3))
        xc = cb + np.einsum("mij,mj->mi", Rb, ql)
        nw = np.einsum("mij,mj->mi", Rb, nl)
        bt_ = np.array([sph[k]["body"] for k in tg])
        vA = vroot + _point_velocity(tm, R, p, qd, omega, bt_, xc)
        want = _wanted_velocity(rng, cfg, gap, nw, deficit)
        wbox = rng.uniform(-5, 5, (m, 3))
        vbox = vA - want - np.cross(wbox, xc - cb)
        _, first = np.unique(todo[ok], return_index=True)
        pick = np.flatnonzero(ok)[first]
        sel = todo[pick]
        root[sel, 0, 0:3], root[sel, 0, 3:7], root[sel, 0, 7:10], root[sel, 0, 10:13] = pr[pick], quat[pick], vroot[pick], omega[pick]
        root[sel, 1, 0:3], root[sel, 1, 3:7], root[sel, 1, 7:10], root[sel, 1, 10:13] = (pr + cb)[pick], qb[pick], vbox[pick], wbox[pick]
        dof[sel, :, 0], dof[sel, :, 1] = q[pick], qd[pick]
        done[sel] = True
    assert done.all(), f"no admissible pose for spheres {sorted(set(int(t) for t in targets[~done]))}"
    tau = np.zeros((n, 20))
    tau[:, :12], tau[:, 12:18] = rng.uniform(-2, 2, (n, 12)), rng.uniform(-0.3, 0.3, (n, 6))
    return root.astype(np.float32), dof.astype(np.float32), tau.astype(np.float32)


def _calm_robot(rng, tm, tb, tcfg, names, n, margin):
    """A robot near its default pose (+- 0.2 rad, |qd| <= 1 legs / 0.5 arm) at a random attitude, every self-collision pair clear."""
    q, qd = _robot_draw(rng, tm, tb, tcfg, n, spread=0.2)
    quat = _rand_quat(rng, n)
    R, p = clr._batch_fk(tm, quat, q)
    assert (_self_gap(tm, names, R, p, quat) > margin + 5e-3).all()
    return q, 0.5 * qd, quat


def box_corner_states(model, wmodel, tcfg, ter, targets, seed, deficit=(-1.5, 0.5)):
    """One env per entry of `targets` (box corner indices): the box alone, the target corner pointing down (plus noise) at a gap from
    (-12 mm, margin - 0.5 mm) over the plane or the grid (u, v 0.02 inside the cell and off its diagonal), every other corner clear of
    the terrain by 2 margin + 1 mm, spinning (|w| <= 5) with the corner's contact point at the velocity of _wanted_velocity; the robot
    calm, 5 m above the box."""
    rng = np.random.default_rng(seed)
    tm, tb, bt = clr.table_model(model, wmodel), fdr.tables(wmodel, tcfg), box_tables(wmodel)
    cfg = clr.law_cfg(tcfg)
    targets = np.asarray(targets, dtype=int)
    n = len(targets)
    pos = np.array([cn["pos"] for cn in bt["corners"]])
    rad = np.array([cn["rad"] for cn in bt["corners"]])
    root, dof = np.zeros((n, 2, 13)), np.zeros((n, 20, 2))
    done = np.zeros(n, dtype=bool)
    for _ in range(200):
        left = np.flatnonzero(~done)
        if len(left) == 0:
            break
        todo = np.repeat(left, min(16, max(1, 1024 // len(left))))
        m = len(todo)
        ar = np.arange(m)
        tg = targets[todo]
        d = pos[tg] / np.linalg.norm(pos[tg], axis=1, keepdims=True) + 0.35 * rng.normal(size=(m, 3))
        qb = clr._quat_down(d, rng.uniform(-np.pi, np.pi, m))
        Rb = scg.rotm(qb)
        off = np.einsum("mij,kj->mki", Rb, pos)                                                   # corners relative to the centre
        if ter is None:
            xy = rng.uniform(-1, 1, (m, 2))
        else:
            rows, cols = ter["heights"].shape
            cell = np.stack([rng.integers(1, rows - 2, m), rng.integers(1, cols - 2, m)], 1).astype(np.float64)
            uv = rng.uniform(0.02, 0.98, (m, 2))
            xy = np.stack([ter["tx"] + (cell[:, 0] + uv[:, 0]) * ter["hs"], ter["ty"] + (cell[:, 1] + uv[:, 1]) * ter["hs"]], 1)
        cxy = xy - off[ar, tg, 0:2]
        X = np.concatenate([cxy[:, None, :] + off[:, :, 0:2], off[:, :, 2:3]], axis=2)
        h, nrm, aux = clr.terrain_query(ter, cfg["ground_z"], X[:, :, 0], X[:, :, 1])
        gap = rng.uniform(-0.012, cfg["margin"] - 5e-4, m)
        cz = h[ar, tg] + (gap + rad[tg]) / nrm[ar, tg, 2] - off[ar, tg, 2]
        gaps = (X[:, :, 2] + cz[:, None] - h) * nrm[:, :, 2] - rad[None]
        gaps[ar, tg] = np.inf
        ok = (gaps > 2 * cfg["margin"] + 1e-3).all(1) & ~aux["near_border"][ar, tg]
        if ter is not None:
            ok &= np.abs(uv[:, 0] - uv[:, 1]) > 0.02
        nt = nrm[ar, tg]
        want = _wanted_velocity(rng, cfg, gap, nt, deficit)
        wbox = rng.uniform(-5, 5, (m, 3))
        r = off[ar, tg] - rad[tg][:, None] * nt
        vbox = want - np.cross(wbox, r)
        _, first = np.unique(todo[ok], return_index=True)
        pick = np.flatnonzero(ok)[first]
        sel = todo[pick]
        root[sel, 1, 0:2], root[sel, 1, 2], root[sel, 1, 3:7], root[sel, 1, 7:10], root[sel, 1, 10:13] = cxy[pick], cz[pick], qb[pick], vbox[pick], wbox[pick]
        done[sel] = True
    assert done.all()
    q, qd, quat = _calm_robot(rng, tm, tb, tcfg, list(model.rb_names), n, cfg["margin"])
    root[:, 0, 0:3] = root[:, 1, 0:3] + np.array([0.0, 0.0, 5.0])
    root[:, 0, 3:7], root[:, 0, 7:10], root[:, 0, 10:13] = quat, rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-1, 1, (n, 3))
    dof[:, :, 0], dof[:, :, 1] = q, qd
    tau = np.zeros((n, 20))
    tau[:, :12], tau[:, 12:18] = rng.uniform(-2, 2, (n, 12)), rng.uniform(-0.3, 0.3, (n, 6))
    return root.astype(np.float32), dof.astype(np.float32), tau.astype(np.float32)


def sleep_threshold(wmodel, tcfg):
    """Substeps of rest after which the box sleeps (the spec's fp32 expression)."""
    return float(int(np.float32(wmodel.box_sleep_time) * (np.float32(1.0) / np.float32(tcfg.sim_dt)) + np.float32(0.5)))


def sleeping_states(model, wmodel, tcfg, n, seed):
    """S: the box flat on the plane (random yaw, at rest, its four lower corners at gap 0). First half: the robot calm, 5 m above.
    Second half: the robot a little above the plane (its lowest sphere margin + 2 .. 20 mm up, attitude within 0.1 rad of level, joints
    default +- 0.2), one foot sphere at a gap from (-3 mm, margin - 1 mm) beside a vertical face of the box, every other of the 17 spheres
    clear of the box by margin + 2 mm. Returns (root, dof, tau, awake [n])."""
    rng = np.random.default_rng(seed)
    tm, sph, tb, bt = clr.table_model(model, wmodel), clr.spheres(wmodel), fdr.tables(wmodel, tcfg), box_tables(wmodel)
    cfg = clr.law_cfg(tcfg)
    half, names = bt["half"], list(model.rb_names)
    rad = np.array([s["rad"] for s in sph])
    root, dof = np.zeros((n, 2, 13)), np.zeros((n, 20, 2))
    awake = np.arange(n) >= n // 2
    yaw = rng.uniform(-np.pi, np.pi, n)
    root[:, 1, 0:2], root[:, 1, 2] = rng.uniform(-1, 1, (n, 2)), cfg["ground_z"] + half
    root[:, 1, 5], root[:, 1, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    q, qd, quat = _calm_robot(rng, tm, tb, tcfg, names, n, cfg["margin"])
    root[:, 0, 0:3] = root[:, 1, 0:3] + np.array([0.0, 0.0, 5.0])
    root[:, 0, 3:7], root[:, 0, 7:10], root[:, 0, 10:13] = quat, rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-1, 1, (n, 3))
    dof[:, :, 0], dof[:, :, 1] = q, qd
    done = ~awake
    for _ in range(200):
        left = np.flatnonzero(~done)
        if len(left) == 0:
            break
        todo = np.repeat(left, 16)
        m = len(todo)
        ar = np.arange(m)
        tg = todo % 4
        q, qd = _robot_draw(rng, tm, tb, tcfg, m, spread=0.2)
        ang = rng.uniform(-0.1, 0.1, (m, 3))
        quat = np.c_[ang / 2, np.ones(m)]
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        R, p = clr._batch_fk(tm, quat, q)
        cen = np.stack([p[:, s["body"]] + R[:, s["body"]] @ s["pos"] for s in sph], axis=1)
        rz = cfg["ground_z"] + cfg["margin"] + rng.uniform(0.002, 0.02, m) - (cen[:, :, 2] - rad[None]).min(1)
        cen[:, :, 2] += rz[:, None]                                                                # relative to the root's (x, y), absolute z
        ft = cen[ar, tg]
        gap = rng.uniform(-0.003, cfg["margin"] - 1e-3, m)
        sgn = rng.choice([-1.0, 1.0], m)
        axis = rng.integers(0, 2, m)
        pl = np.zeros((m, 3))
        pl[ar, axis] = sgn * (half + rad[tg] + gap)
        pl[ar, 1 - axis] = rng.uniform(-0.6 * half, 0.6 * half, m)
        pl[:, 2] = ft[:, 2] - (cfg["ground_z"] + half)
        yb = yaw[todo]
        Rb = np.zeros((m, 3, 3))
        Rb[:, 0, 0], Rb[:, 0, 1], Rb[:, 1, 0], Rb[:, 1, 1], Rb[:, 2, 2] = np.cos(yb), -np.sin(yb), np.sin(yb), np.cos(yb), 1.0
        cb = ft - np.einsum("mij,mj->mi", Rb, pl)
        plo = np.einsum("mji,mkj->mki", Rb, cen[:, BOX_SPHERES] - cb[:, None, :])
        gaps = _sdf_box(plo, half) - rad[BOX_SPHERES][None]
        gaps[ar, tg] = np.inf
        ok = (gaps > cfg["margin"] + 2e-3).all(1) & (np.abs(pl[:, 2]) < 0.8 * half)
        ok[ok] = _self_gap(tm, names, R[ok], p[ok], quat[ok]) > cfg["margin"] + 5e-3
        _, first = np.unique(todo[ok], return_index=True)
        pick = np.flatnonzero(ok)[first]
        sel = todo[pick]
        root[sel, 0, 0:2], root[sel, 0, 2], root[sel, 0, 3:7] = root[sel, 1, 0:2] - cb[pick, 0:2], rz[pick], quat[pick]
        root[sel, 0, 7:10], root[sel, 0, 10:13] = rng.uniform(-0.2, 0.2, (len(sel), 3)), rng.uniform(-0.5, 0.5, (len(sel), 3))
        dof[sel, :, 0], dof[sel, :, 1] = q[pick], 0.25 * qd[pick]
        done[sel] = True
    assert done.all()
    tau = np.zeros((n, 20))
    tau[:, :12], tau[:, 12:18] = rng.uniform(-2, 2, (n, 12)), rng.uniform(-0.3, 0.3, (n, 6))
    return root.astype(np.float32), dof.astype(np.float32), tau.astype(np.float32), awake


def _target_gap(tm, sph, lt, cfg, q, target):
    """(internal_geometry, robot geometry) at joint positions q, the root at the origin of F (only what internal_geometry reads)."""
    E, p = ao.fk(tm, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), np.asarray(q, dtype=np.float64))
    xk = np.array([p[s_["body"]] + E[s_["body"]] @ s_["pos"] for s_ in sph])
    rad = np.array([s_["rad"] for s_ in sph])
    g = dict(E=E, p=p, xc=xk, n=np.zeros((len(sph), 3)), rad=rad)
    return internal_geometry(lt, sph, g, cfg), g


def internal_pair_states(model, wmodel, tcfg, targets, seed, deficit=(-0.45, 0.15), inside_share=0.0, probe=False):
    """(root, dof, tau) float32, one env per entry of `targets` (indices into the 47 internal pairs: 0..43 the candidate limb pairs in the
    order of their lanes, 44..46 gripper / wrist / elbow against the trunk box). A pose is searched among random draws (half default +-
    0.9, half uniform inside the limits; self_collision_geometry's vectorised gaps) with the target pair within (-20, 40) mm and every other
    pair 16 mm clear and 8 mm behind the target (a pose may serve up to three envs, each with its own gap, joint and velocities); one joint on the path of one of the pair's bodies alone is then turned until the pair's gap is the drawn
    one: 35 % from (0, 3 mm), 10 % from (3 mm, margin - 0.5 mm), 55 % from (-12 mm, 0); inside_share of the trunk-box draws instead with the
    sphere's centre 1 to 10 mm inside the box. Kept if every other internal pair (the spec's geometry, and self_collision_geometry's) clears
    the margin by 5 mm, the runner-up feature pair is 0.1 mm behind and the joints are 0.05 rad inside their limits. Joint velocities:
    random (|qd| <= 1 legs / 0.5 arm) plus the smallest change (arm joints weighted 1/4) that gives the contact point the relative velocity
    of _wanted_velocity; rejected above half a joint's velocity limit. The root 1.2 m up at a random attitude, the box 50 m away."""
    rng = np.random.default_rng(seed)
    tm, sph, tb, lt = clr.table_model(model, wmodel), clr.spheres(wmodel), fdr.tables(wmodel, tcfg), limb_tables(wmodel)
    cfg = clr.law_cfg(tcfg)
    margin = cfg["margin"]
    targets = np.asarray(targets, dtype=int)
    n = len(targets)
    names = list(model.rb_names)
    lnames = list(abi.LIMB_NAMES)
    keys = [(lnames[a], lnames[b]) for _, a, b in lt["cands"]] + [({8: "gripper", 10: "wrist", 9: "elbow"}[t["sphere"]], "trunk") for t in lt["trunk"]]
    lim = tb["lo"] < tb["hi"]
    lim &= np.arange(20) < 18
    lo, hi = np.where(lim, tb["lo"] + 0.05, 0.0), np.where(lim, tb["hi"] - 0.05, 0.0)
    qdef = np.array([float(x) for x in tcfg.default_dof_pos])
    root, dof = np.zeros((n, 2, 13)), np.zeros((n, 20, 2))
    done = np.zeros(n, dtype=bool)
    ident = np.array([0.0, 0.0, 0.0, 1.0])
    wq = np.r_[np.ones(12), 0.25 * np.ones(6), np.zeros(2)]
    def gaps_of(qs):
        R, p = clr._batch_fk(tm, np.tile(ident, (len(qs), 1)), qs)
        rbs = np.zeros((len(qs), len(names), 7))
        rbs[:, :, 0:3] = np.stack([p[:, b] + R[:, b] @ tm.rb_offset[r] for r, b in enumerate(tm.rb_body)], axis=1)
        rbs[:, names.index("trunk"), 6] = 1.0
        table = scg.all_pairs(rbs, names)
        return np.stack(list(table.values()), 1), list(table)

    def place(e, st):
        dof[e, :, 0], dof[e, :, 1] = st[0], st[1]
        quat = _rand_quat(rng, 1)[0]
        Rw = ao.quat_to_mat(quat)
        root[e, 0, 0:3], root[e, 0, 3:7] = np.r_[rng.uniform(-1, 1, 2), 1.2], quat
        root[e, 0, 7:10], root[e, 0, 10:13] = rng.uniform(-0.5, 0.5, 3), Rw @ st[2]
        done[e] = True

    if inside_share > 0:
        # the corner region of the trunk box: only the gripper tip reaches it, in 2 of 10 000 arm poses. 60 000 arm-only draws (legs at
        # their default), those with the tip in the corner region within 30 mm, refined with that region asked for; 14 envs at most
        m = 60000
        qa = np.tile(qdef, (m, 1))
        qa[:, 12:18] = rng.uniform(lo[12:18], hi[12:18], (m, 6))
        qa[:, 18:] = 0
        R, p = clr._batch_fk(tm, np.tile(ident, (m, 1)), qa)
        tip = p[:, sph[8]["body"]] + R[:, sph[8]["body"]] @ sph[8]["pos"]
        d = np.abs(tip - lt["trunk"][0]["centre"]) - lt["trunk"][0]["half"]
        cand = np.repeat(np.flatnonzero((d > 0).all(1) & (np.linalg.norm(np.maximum(d, 0), axis=1) - sph[8]["rad"] < 0.03)), 4)
        for e in np.flatnonzero(targets == 44)[:14]:
            while len(cand):
                i, cand = cand[0], cand[1:]
                st = _refine(rng, tm, sph, tb, lt, cfg, qa[i].copy(), 44, lo, hi, wq, deficit, names, 0.0, want=3)
                if st is not None:
                    place(e, st)
                    break
    for _ in range(12):
        if done.all():
            break
        m = 6000
        q = qdef[None] + rng.uniform(-0.9, 0.9, (m, 20))
        uni = rng.random(m) < 0.5
        q[uni] = rng.uniform(lo, hi, (int(uni.sum()), 20))
        q = np.clip(q, lo, hi)
        q[:, 18:] = 0
        allg, tkeys = gaps_of(q)
        for tgt in sorted(set(targets[~done])):
            col = tkeys.index(keys[tgt]) if keys[tgt] in tkeys else tkeys.index(keys[tgt][::-1])
            others = np.delete(allg, col, axis=1).min(1)
            cand = np.repeat(np.flatnonzero((allg[:, col] > -0.02) & (allg[:, col] < 0.04) & (others > margin + 6e-3) & (others > allg[:, col] + 8e-3)), 3)
            for e in np.flatnonzero(~done & (targets == tgt)):
                if len(cand) == 0:
                    break
                i, cand = cand[0], cand[1:]
                # (two calves: half of the tries ask for end sphere against end sphere, the rarest of the four features)
                both = tgt < 44 and lt["limbs"][lt["cands"][tgt][1]]["cap0"] > 0 and lt["limbs"][lt["cands"][tgt][2]]["cap0"] > 0
                st = _refine(rng, tm, sph, tb, lt, cfg, q[i].copy(), int(tgt), lo, hi, wq, deficit, names, inside_share,
                             want=3 if both and rng.random() < 0.5 else None)
                if st is not None:
                    place(e, st)
        # the pairs that the draws do not show alone (a neighbour with a larger end sphere touches first): a directed search. The 48
        # best draws by (smallest other gap - the pair's gap) are perturbed (12 children each, sigma 0.1 then 0.04 rad) and re-selected
        # for 14 rounds; what then passes the filter above goes through the same refinement.
        for tgt in sorted(set(targets[~done])):
            col = tkeys.index(keys[tgt]) if keys[tgt] in tkeys else tkeys.index(keys[tgt][::-1])

            def score(G):
                t_, o_ = G[:, col], np.delete(G, col, axis=1).min(1)
                return ((np.minimum(o_, 0.05) - t_) - 3 * np.maximum(0, t_ - 0.02) - 3 * np.maximum(0, -0.01 - t_)
                        - 3 * np.maximum(0, margin + 7e-3 - o_)), t_, o_
            pop = q[np.argsort(-score(allg)[0])[:48]]
            for it in range(14):
                allq = np.r_[pop, np.clip(np.repeat(pop, 12, 0) + rng.normal(0, 0.10 if it < 8 else 0.04, (len(pop) * 12, 20)) * lim, lo, hi)]
                sc_, t_, o_ = score(gaps_of(allq)[0])
                idx = np.argsort(-sc_)[:48]
                pop = allq[idx]
            if probe:
                return pop, t_[idx], o_[idx]
            good = (t_[idx] > -0.02) & (t_[idx] < 0.04) & (o_[idx] > margin + 6e-3) & (o_[idx] > t_[idx] + 8e-3)
            cand = np.repeat(rng.permutation(np.flatnonzero(good)), 3)
            for e in np.flatnonzero(~done & (targets == tgt)):
                while len(cand):
                    i, cand = cand[0], cand[1:]
                    # (the neighbours follow the joint that is turned: the gap is not asked to close by more than their slack)
                    st = _refine(rng, tm, sph, tb, lt, cfg, pop[i].copy(), int(tgt), lo, hi, wq, deficit, names, inside_share,
                                 min_gap=t_[idx][i] - (o_[idx][i] - margin - 6e-3))
                    if st is not None:
                        place(e, st)
                        break
    assert done.all(), f"no admissible pose for pairs {sorted(set(int(t) for t in targets[~done]))}"
    root[:, 1, 0:3] = root[:, 0, 0:3] + np.array([50.0, 0.0, 0.0])
    root[:, 1, 2] = 6.2
    root[:, 1, 6] = 1
    tau = np.zeros((n, 20))
    tau[:, :12], tau[:, 12:18] = rng.uniform(-2, 2, (n, 12)), rng.uniform(-0.3, 0.3, (n, 6))
    return root.astype(np.float32), dof.astype(np.float32), tau.astype(np.float32)


def _refine(rng, tm, sph, tb, lt, cfg, q, tgt, lo, hi, wq, deficit, names, inside_share, min_gap=None, want=None):
    """One candidate pose of internal_pair_states: (q, qd, omega in F) or None."""
    margin = cfg["margin"]
    u = rng.random()
    want_gap = rng.uniform(0, 0.003) if u < 0.35 else (rng.uniform(0.003, margin - 5e-4) if u < 0.45 else rng.uniform(-0.012, 0))
    if min_gap is not None:
        want_gap = max(want_gap, min_gap)
        if want_gap > margin - 5e-4:
            return None
    internal, g = _target_gap(tm, sph, lt, cfg, q, tgt)
    ct = internal[tgt]
    if ct["kind"] == "trunk":
        rad = ct["rad"]
        want_gap = max(want_gap, -(rad - 0.003))
        if rng.random() < inside_share:
            want_gap = -rad - rng.uniform(0.001, 0.01)
    pa, pb = wb.ancestors(tm, ct["body"]) - {0}, wb.ancestors(tm, ct["body2"]) - {0}
    joints = [tm.body_dof[b] for b in sorted(pa ^ pb) if hi[tm.body_dof[b]] > lo[tm.body_dof[b]]]
    one = dict(lt, cands=[lt["cands"][tgt]], trunk=[]) if tgt < 44 else dict(lt, cands=[], trunk=[lt["trunk"][tgt - 44]])
    fn = lambda d, th: _target_gap(tm, sph, one, cfg, np.r_[q[:d], th, q[d + 1:]], tgt)[0][0]["gap"] - want_gap
    q_start = q
    for d in rng.permutation(joints):
        ths = np.clip(q_start[d] + np.linspace(-0.5, 0.5, 21), lo[d], hi[d])
        vals = np.array([fn(d, th) for th in ths])
        flips = np.flatnonzero(np.sign(vals[:-1]) * np.sign(vals[1:]) < 0)
        if len(flips) == 0:
            continue
        i = flips[np.argmin(np.abs(flips - 10))]
        a_, b_, fa_ = ths[i], ths[i + 1], vals[i]
        for _ in range(40):
            mid = 0.5 * (a_ + b_)
            fm = fn(d, mid)
            if np.sign(fm) == np.sign(fa_):
                a_, fa_ = mid, fm
            else:
                b_ = mid
        q = q_start.copy()
        q[d] = 0.5 * (a_ + b_)
        st = _finish(rng, tm, sph, tb, lt, cfg, q, tgt, want_gap, wq, deficit, names, want)
        if st is not None:
            return st
    return None


def _finish(rng, tm, sph, tb, lt, cfg, q, tgt, want_gap, wq, deficit, names, want=None):
    """The checks and the velocities of one refined pose of internal_pair_states."""
    margin = cfg["margin"]
    q = np.float32(q).astype(np.float64)                                     # the pose the sims will see
    internal, g = _target_gap(tm, sph, lt, cfg, q, tgt)
    ct = internal[tgt]
    if abs(ct["gap"] - want_gap) > 2e-6 or ct["second"] - ct["gap"] < 1e-4 or not (0.5 > ct["par"] or ct["par"] > 2.0):
        return None
    if any(p_["gap"] < margin + 5e-3 for j, p_ in enumerate(internal) if j != tgt):
        return None
    if want is not None and (ct["feature"] if ct["kind"] == "limbs" else ct["region"]) != want:
        return None
    R, p = clr._batch_fk(tm, np.array([[0.0, 0.0, 0.0, 1.0]]), q[None])
    rbs = np.zeros((1, len(names), 7))
    rbs[:, :, 0:3] = np.stack([p[:, b] + R[:, b] @ tm.rb_offset[r] for r, b in enumerate(tm.rb_body)], axis=1)
    rbs[:, names.index("trunk"), 6] = 1.0
    if np.sort(np.array([v[0] for v in scg.all_pairs(rbs, names).values()]))[1] < margin + 5e-3:
        return None
    # velocities
    qd = np.zeros(20)
    qd[:12], qd[12:18] = rng.uniform(-1, 1, 12), rng.uniform(-0.5, 0.5, 6)
    omega = rng.uniform(-2, 2, 3)
    JA = wb.point_jacobian(tm, g["E"], g["p"], ct["body"], ct["xc"])[0:3]
    JB = wb.point_jacobian(tm, g["E"], g["p"], ct["body2"], ct["xc"])[0:3]
    Jr = (JA - JB)[:, 6:]
    want = _wanted_velocity(rng, cfg, np.array([ct["gap"]]), ct["n"][None], deficit)[0]
    A = Jr * wq[None]
    qd = qd + wq * (Jr.T @ np.linalg.solve(A @ Jr.T + 1e-12 * np.eye(3), want - Jr @ qd))
    lim = tb["qd_limit"]
    if np.any((lim > 0) & (np.abs(qd) > 0.5 * lim)):
        return None
    return q, qd, omega


def tangled_states(model, wmodel, tcfg, n, seed):
    """M: robots 1.2 m up at a random yaw with EVERY joint drawn uniformly inside its limits (legs crossing, the arm in the legs: several
    pairs at once, some deep), |qd| <= 0.5, and a box at rest with a random attitude at a shin (5 cm in front of a calf's origin or of its
    middle) or 11 cm under the trunk of every third robot, +- 3 cm; the other boxes 50 m away."""
    rng = np.random.default_rng(seed)
    tm, tb = clr.table_model(model, wmodel), fdr.tables(wmodel, tcfg)
    names = list(model.rb_names)
    lim = (tb["lo"] < tb["hi"]) & (np.arange(20) < 18)
    q = np.where(lim, rng.uniform(np.where(lim, tb["lo"], 0.0), np.where(lim, tb["hi"], 0.0), (n, 20)), 0.0)
    yaw = rng.uniform(-np.pi, np.pi, n)
    quat = np.c_[np.zeros((n, 2)), np.sin(yaw / 2), np.cos(yaw / 2)]
    R, p = clr._batch_fk(tm, quat, q)
    root, dof = np.zeros((n, 2, 13)), np.zeros((n, 20, 2))
    root[:, 0, 0:2], root[:, 0, 2], root[:, 0, 3:7] = rng.uniform(-1, 1, (n, 2)), 1.2, quat
    dof[:, :, 0] = q
    dof[:, :18, 1] = rng.uniform(-0.5, 0.5, (n, 18))
    root[:, 1, 0:3] = root[:, 0, 0:3] + np.array([50.0, 0.0, 5.0])
    root[:, 1, 6] = 1
    targets = [names.index(k) for k in ("FL_calf", "FR_calf", "RL_calf", "RR_calf", "trunk")]
    for e in range(0, n, 3):
        t = targets[(e // 3) % 5]
        b = tm.rb_body[t]
        off = rng.uniform(-0.03, 0.03, 3) + (np.array([0, 0, -0.11]) if names[t] == "trunk" else np.array([0.05, 0, rng.choice([0.0, -0.1])]))
        root[e, 1, 0:3] = root[e, 0, 0:3] + p[e, b] + R[e, b] @ tm.rb_offset[t] + off
        root[e, 1, 3:7] = _rand_quat(rng, 1)[0]
    tau = np.zeros((n, 20))
    tau[:, :12], tau[:, 12:18] = rng.uniform(-2, 2, (n, 12)), rng.uniform(-0.3, 0.3, (n, 6))
    return root.astype(np.float32), dof.astype(np.float32), tau.astype(np.float32)


GRID_SEED = clr.GRID_SEED
# The 44 candidate limb pairs, by their index in limb_tables()["cands"] (ascending lane).
# The upper arm against a rear calf (19, 21) is not staged alone: the arm reaches that calf only at its knee sphere (r = 20 mm), whose
# centre is the end of the thigh's shaft (r = 17 mm), so the arm's gap to the thigh is at most 3 mm more: the two pairs are within margin
# together (tests/test_pair_contact.py asserts both statements on a directed search).
LIMB_TARGETS = [i for i in range(44) if i not in (19, 21)]
# name -> dict(n, seed, kind, grid): "pair" a robot sphere against the free box, "corner" a box corner against the terrain, "sleep"
CASES = {
    "L-1": dict(n=1, seed=611, kind="tree", grid=False, targets=[0]),
    "L-13": dict(n=13, seed=612, kind="tree", grid=False, targets=[LIMB_TARGETS[(7 * i) % len(LIMB_TARGETS)] for i in range(13)]),
    "L-264": dict(n=264, seed=613, kind="tree", grid=False, targets=[LIMB_TARGETS[i % len(LIMB_TARGETS)] for i in range(264)]),
    "T-96": dict(n=96, seed=614, kind="tree", grid=False, targets=[44 + i % 2 for i in range(96)], inside_share=0.2),
    "B-255": dict(n=255, seed=601, kind="pair", grid=False),
    "K-128": dict(n=128, seed=602, kind="corner", grid=False),
    "K-128-grid": dict(n=128, seed=603, kind="corner", grid=True),
    "S-64": dict(n=64, seed=604, kind="sleep", grid=False),
    "M-256": dict(n=256, seed=607, kind="tangled", grid=False, substeps=2),
}
STEP_CASES = {"E-13": dict(n=13, seed=615, source="L-264"), "E-2560": dict(n=2560, seed=616, source="L-264"),
              "E-13-box": dict(n=13, seed=605, source="B-255"), "E-2560-box": dict(n=2560, seed=606, source="B-255")}
STEP_SIGMA, STEP_COUNTER = 0.3, 1
_STATES = {}


def case_params(name):
    """helpers.random_env_params of the case's seed (negative and > 1 frictions, randomised BODY_PARAMS) with a randomised box mass."""
    import helpers
    case = CASES.get(name) or STEP_CASES[name]
    params = helpers.random_env_params(case["n"], seed=case["seed"])
    params["box_dmass"] = np.random.default_rng(case["seed"] + 5000).uniform(-0.5, 1.5, case["n"]).astype(np.float32)
    return params


def case_states(robot, name):
    """(tcfg, terrain, root, dof, tau, timer [n], awake [n] or None) of a case; computed once per process. `robot`: case_robot(...)."""
    if name not in _STATES:
        case = CASES[name]
        tc = case_cfg(robot["tcfg"])
        ter = clr.rough_grid(GRID_SEED) if case["grid"] else None
        n = case["n"]
        timer, awake = np.zeros(n), None
        if case["kind"] == "tree":
            st = internal_pair_states(robot["model"], robot["wmodel"], tc, case["targets"], case["seed"], inside_share=case.get("inside_share", 0.0))
        elif case["kind"] == "pair":
            st = box_pair_states(robot["model"], robot["wmodel"], tc, [BOX_SPHERES[i % 17] for i in range(n)], case["seed"])
        elif case["kind"] == "tangled":
            st = tangled_states(robot["model"], robot["wmodel"], tc, n, case["seed"])
        elif case["kind"] == "corner":
            st = box_corner_states(robot["model"], robot["wmodel"], tc, ter, [i % 8 for i in range(n)], case["seed"])
        else:
            root, dof, tau, awake = sleeping_states(robot["model"], robot["wmodel"], tc, n, case["seed"])
            st = (root, dof, tau)
            timer[:] = sleep_threshold(robot["wmodel"], tc)
        _STATES[name] = (tc, ter) + st + (timer, awake)
    return _STATES[name]


def step_states(robot, name, case=None, **cfg):
    """Tier E: (tcfg, terrain, root, dof, actions) -- the staged states of B-255 tiled over the envs; decimation = 1, the attitude and
    height terminations out of reach, the arm slower (as contact_law_reference.step_states). case: dict(n, seed, source[, sigma]) instead
    of STEP_CASES[name]; cfg: further fields of the task cfg (tests/decimation_reference.py)."""
    case = STEP_CASES[name] if case is None else case
    tc, ter, root, dof = case_states(robot, case["source"])[:4]
    tc = case_cfg(tc, **dict(dict(decimation=1, term_rp_threshold=100.0, term_z_threshold=-100.0), **cfg))
    if CASES[case["source"]]["kind"] == "tree":
        # the staged limb pairs are poses anywhere inside the joint limits, far from the default pose the actions are offsets of: with
        # the shipped gains the PD torques alone take 60 % of them into the velocity clamp within the substep. A twentieth of the
        # stiffness and a quarter of the damping keep the torques of the size the staged velocities were drawn for.
        for i in range(len(tc.p_gains)):
            tc.p_gains[i] *= 0.05
            tc.d_gains[i] *= 0.25
    idx = np.arange(case["n"]) % len(root)
    rng = np.random.default_rng(case["seed"])
    act = (case.get("sigma", STEP_SIGMA) * rng.normal(size=(case["n"], 18))).astype(np.float32)
    root, dof = root[idx].copy(), dof[idx].copy()
    dof[:, 12:18, 1] *= 0.25
    return tc, ter, root, dof, act


# -------------------------------------------------------------------------------------------------------- running a sim through
def evaluate(robot, tcfg, ter, root0, dof0, root1, dof1, ncf, fs, bp, friction, box_mass, dropped, tau, timer0, timer1, envs=None, skip=None,
             spec=DEFAULT_SPEC, tangled=False):
    """check_env over a batch -> list of per-env results (None for the envs not in `envs`); skip: mask of envs to leave out ("reset")."""
    n = len(dof0)
    out = [None] * n
    for e in (range(n) if envs is None else envs):
        r = check_env(robot["model"], robot["wmodel"], tcfg, ter, root0[e], dof0[e], root1[e], dof1[e], ncf[e], fs[e], bp[e], friction[e],
                      box_mass[e], dropped[e], tau[e], timer0[e], timer1[e], spec=spec, tangled=tangled)
        if skip is not None and skip[e]:
            r["left_out"] = "reset"
        out[e] = r
    return out


def _snapshot(sim, r0, d0, timer0, tau, params):
    return dict(root0=r0, dof0=d0, root1=sim.get("ROOT_STATES"), dof1=sim.get("DOF_STATE"), ncf=sim.get("NET_CONTACT_FORCE"),
                fs=sim.get("FORCE_SENSOR"), bp=sim.get("BODY_PARAMS"), friction=np.asarray(params["friction"], dtype=np.float64),
                box_mass=sim.get("BOX_MASS"), dropped=sim.get("DROPPED_HITS"), tau=np.asarray(tau, dtype=np.float64), timer0=timer0,
                timer1=sim.get("BOX_SLEEP_TIMER"))


def run_case(sim, robot, name, params):
    """Load a case into `sim` (an adapter with load / set / simulate / get) and check the substep. Returns (results, state)."""
    tc, ter, root, dof, tau, timer, _ = case_states(robot, name)
    sim.load(root, dof, tau)
    sim.set("BOX_SLEEP_TIMER", timer)
    out = []
    for _ in range(CASES[name].get("substeps", 1)):                     # every substep from the sim's own previous state
        r0, d0, t0, drop0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE"), sim.get("BOX_SLEEP_TIMER"), sim.get("DROPPED_HITS")
        sim.simulate()
        st = _snapshot(sim, r0, d0, t0, tau, params)
        st["dropped"] = st["dropped"] - drop0                            # (the counter accumulates)
        out += evaluate(robot, tc, ter, **st, tangled=CASES[name]["kind"] == "tangled")
    return out, st


def run_step(sim, robot, name, params):
    """Tier E: reset_all, the staged states loaded over the reset ones, ONE env step of one substep under 0.3-sigma actions; the torques
    are the TORQUES tensor after the step; envs that reset in the step are left out, the step counter keeps the push away."""
    tc, ter, root, dof, act = step_states(robot, name)
    assert tc.decimation == 1
    sim.reset_all()
    sim.set_step_counter(STEP_COUNTER)
    assert tc.push_interval == 0 or STEP_COUNTER + 1 < tc.push_interval
    sim.load(root, dof, np.zeros((len(root), 20), dtype=np.float32))
    timer = np.zeros(len(root))
    sim.set("BOX_SLEEP_TIMER", timer)
    r0, d0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
    sim.step(act)
    st = _snapshot(sim, r0, d0, timer, sim.get("TORQUES"), params)
    return evaluate(robot, tc, ter, envs=fdr.step_envs(len(root)), skip=sim.get("RESET_BUF") != 0, **st), st


def summarise(out):
    """Counts and the largest ratio per tier of a case: dict(n, checked, left_out {why: count}, single, classes, near, mu0, branches [3],
    regions {region: count}, spheres {sphere or corner: count}, static, promoted, asleep, forced (envs with any force), features [4]
    (winning feature pair of a limb pair, FEATURES), lanes (set of the internal pairs seen alone), contraction (largest |1 - W_t W_u^-1|),
    exact [...], worst {tier: (ratio, env)})."""
    s = dict(n=0, checked=0, left_out={}, single=0, classes={c: 0 for c in CLASSES}, near=0, mu0=0, branches=[0, 0, 0], regions={}, spheres={},
             static=0, promoted=0, asleep=0, exact=[], worst={t: (0.0, -1) for t in TIERS}, features=[0, 0, 0, 0], lanes=set(), contraction=0.0,
             forced=0, multi=0)
    for e, r in enumerate(out):
        if r is None:
            continue
        s["n"] += 1
        if r["left_out"] is not None:
            s["left_out"][r["left_out"]] = s["left_out"].get(r["left_out"], 0) + 1
            continue
        s["checked"] += 1
        s["asleep"] += int(r["asleep"])
        s["forced"] += int(r["forced"])
        s["multi"] += int(r["ncontacts"] >= 2)
        s["exact"] += [f"env {e}: {x}" for x in r["exact"]]
        for t in TIERS:
            if r["ratio"][t] > s["worst"][t][0]:
                s["worst"][t] = (r["ratio"][t], e)
        if r["cls"] is not None:
            s["single"] += 1
            s["classes"][r["cls"]] += 1
            s["near"] += int(r["near"])
            s["mu0"] += int(r["mu"] == 0.0)
            s["branches"][r["branch"]] += 1
            s["regions"][r["region"]] = s["regions"].get(r["region"], 0) + 1
            s["spheres"][r["sphere"]] = s["spheres"].get(r["sphere"], 0) + 1
            if r["feature"] is not None:
                s["features"][r["feature"]] += 1
            if r["lane"] is not None:
                s["lanes"].add(r["lane"])
                s["contraction"] = max(s["contraction"], r["contraction"])
            s["static"] += int(r["static"] is True)
            s["promoted"] += int(r["static"] is False)
    return s


def report(name, s):
    w = ", ".join(f"{t} {s['worst'][t][0]:.3f} (env {s['worst'][t][1]})" for t in TIERS)
    return (f"{name}: {s['checked']} of {s['n']} checked (left out {s['left_out']}), {s['single']} single-contact: {s['classes']}, "
            f"{s['near']} in a decision band, mu = 0: {s['mu0']}, vn_tgt branches {s['branches']}, regions {s['regions']}, static / promoted "
            f"{s['static']} / {s['promoted']}, asleep {s['asleep']}, with a force {s['forced']}, {s['multi']} with several contacts, features {s['features']}, {len(s['lanes'])} lanes, "
            f"largest contraction {s['contraction']:.3f}; largest ratios: {w}")


class OracleAdapter(fdr.OracleAdapter):
    def set(self, name, value):
        self.o.set(name, value)
