"""TEST INFRASTRUCTURE ONLY -- CPU (numpy, fp64) statement of what the CONTACT stage of one physics substep (physics_substep /
contact_solve of csrc/wbc_step_kernel.hip; the spec is oracle/wbc_oracle.c and DESIGN.md section 3) has to satisfy, checked from
tensors the sim stores anyway: ROOT_STATES and DOF_STATE before and after the substep, NET_CONTACT_FORCE, FORCE_SENSOR, BODY_PARAMS, the
env's friction, the task cfg and the terrain. No articulated-body recursion and no contact solver anywhere in this file.

  1. geometry   world centre X of each of the robot's 28 terrain spheres from the fp64 body poses (arm_osc_oracle.fk on the float32 model
                tables), terrain height h and normal n under it (plane, or the height grid's terrain_query restated), gap =
                (X_z - h) n_z - rad, contact point xc = X - rad n, active iff gap < contact_margin.
  2. activation a rigid body's NET_CONTACT_FORCE row may be non-zero only if one of its spheres is active; every other row, the box's
                included, is exactly 0. An env with a gap within 64 2^-24 mag(gap) of the margin is left out.
  3. the law    envs with exactly ONE active sphere (nshare = 1: W is that body's exact response, four sweeps converge to the
                velocity-level law far below fp32 rounding). a = (nu1 - nu0) / dt; the post-step velocity of the body-fixed point at xc
                is v+ = J_p nu0 + dt (J_p a + Jdot_p nu0) (point Jacobian of whole_body_reference, classical point acceleration on the
                recursion of constrained_dynamics_reference); f = the contact body's NET_CONTACT_FORCE row, lam = f dt,
                W = J_p (M + diag(armature))^-1 J_p^T with the fp64 mass matrix of whole_body_reference, vfree = v+ - W lam,
                mu = max(0, (friction + terrain_friction) / 2), vn_tgt = -gap/dt (gap >= 0) or min(erp (-gap)/dt, max_depenetration_vel).
                  separating  n.vfree >= vn_tgt  ->  f exactly 0        (a zero f needs n.v+ >= vn_tgt; a non-zero f needs n.v+ = vn_tgt,
                                                                         and n.vfree < vn_tgt)
                  stick       W^-1 (n vn_tgt - vfree) inside the cone  ->  v+ = n vn_tgt, all three components
                  slide       otherwise  ->  n.v+ = vn_tgt, |f_t| = mu f_n, f_t anti-parallel to vfree_t (|vfree_t| > 1e-2 m/s)
                  frictionless fallback  n.W (n - mu vhat_t) <= 0.05 n.W n  ->  f_t = 0, n.v+ = vn_tgt
                An env whose |lt| / (mu ln) or den / (0.05 nWn) lies within 1e-3 of 1 is left out of the class-specific checks.
  4. cone       every foot rigid body (one sphere each), any number of contacts: f.n >= 0, |f_t| <= mu f.n; on the plane every row has
                f_z >= 0.
  5. sensors    FORCE_SENSOR[ft] = (E_foot^T f, E_foot^T ((-rad n) x f)), or exactly 0 for a foot without force.
  6. momentum   the six root rows of the equations of motion carry no joint torque: ID_ref(q0, nu0, a)[0:3] = sum of the rows of
                NET_CONTACT_FORCE (every env), ID_ref[3:6] = xc x f (single-contact envs), ID_ref the fp64 inverse dynamics of
                tests/inverse_dynamics_reference.py with gravity. Steps 3 to 5 are blind to the SIZE of a force that keeps its direction
                (v+ is read off the stored velocities, the cone is scale-free); this ties the size, and xc, to the motion.

Frames: the spec works in frame F (origin at the root, the base's axes) and maps it to the world with R0 = quat_to_mat(STORED
quaternion), which is orthonormal only up to that quaternion's float32 rounding: world velocities enter as R0^T v, the new world velocity
is v + dt R0 acc_F, forces leave as R0 f_F, n = R0^T nw. Steps 3 to 6 are therefore evaluated in F in exactly that way (velocities by
R0^T, accelerations and forces by R0^-1, the fp64 references called with the root at the origin of F): with a unit quaternion that is the
world-frame statement above, and the fp64 oracle obeys it to 1e-9 instead of to the quaternion's rounding.

Every check is |residual| <= C 2^-24 scale; this file returns residual / (2^-24 scale) per tier ("vel", "cone", "dir", "sensor", "mom"),
the tests compare with C. Scales are carried as the earlier checkers carry mag (sums add the sizes of their summands; sqrt and divisions
pass the size on through their first-order sensitivity):
    n        mag(n) = mag(R0)^T |nw|, mag(R0) the sizes of quat_to_mat's summands (1 + 2 (y^2 + z^2), 2 (|x y| + |w z|), ...): n = R0^T nw
             inherits the rounding of the stored quaternion, its length included
    vel      |J_p| (|nu0| + |nu1|) + dt mag(Jdot_p nu0) + |W| |lam| + |n| mag(vn_tgt) + mag(n) |vn_tgt|; along n: + mag(n).|v+|,
             mag(vn_tgt) = s (|X_z| + |h| + rad + |dh/dx| mag(x - tx) + |dh/dy| mag(y - ty)) / dt with s the branch's d vn_tgt / d gap
             (1 speculative, erp while erp pen / dt is below the cap, 0 at the cap), mag(x - tx) = |x| + |tx|: the rounding of a
             world coordinate tens of metres from the origin, carried down the slope
    cone     mag(|f_t|) + (|friction| + |terrain_friction|) / 2 mag(f.n), mag(f.n) = |f|.mag(n); a sliding contact: mag(f.n) times
             1 + mu mag(vhat_t . n), vhat_t . n = (vfree.n - (n.vfree)(n.n)) / |vfree_t| (n is a unit vector only up to its rounding)
    dir      mag(f_t) / |f_t| + |vel scale| / |vfree_t|: the two unit vectors compared, each with the conditioning of its own direction
             (f_t is the small difference f - (f.n) n where mu is small)
    sensor   |f| + rad |f|
    mom      mag(ID_ref) + |M| (|nu0| + |nu1|) / dt + sum |f| (+ |xc| x |f|), as forward_dynamics_reference.substep_residual
K_REF (per tier: the fp32 ORACLE's largest ratio on exactly the tests' states) is measured and asserted by tests/test_contact_law.py and
never taken from the kernel; C = 4 K_ref rounded up to a power of two, at most 1024.

The file also holds the seeded case generators (fp64, one chosen sphere placed at a drawn gap over the plane or a rough height grid,
every other sphere and every self-collision pair clear) and the loops that run them through a sim, so that tests/test_contact_law.py
(the C oracle in both precisions) and tests/test_gpu_contact_law.py (the HIP kernels) evaluate exactly the same states. `spec` is how
tests/test_contact_law.py hands the checker a deliberately different law. Nothing under wbc_amd imports this file."""
import copy

import numpy as np

import arm_osc_oracle as ao
import constrained_dynamics_reference as cdr
import forward_dynamics_reference as fdr
import inverse_dynamics_reference as idr
import self_collision_geometry as scg
import whole_body_reference as wb
from wbc_amd import abi

EPS = 2.0 ** -24
NSPH = abi.NSPH
LIVE = fdr.LIVE
C_CAP = 1024.0
TIERS = ("vel", "cone", "dir", "sensor", "mom")
MARGIN_GUARD = 64.0           # a gap within MARGIN_GUARD 2^-24 mag(gap) of the margin leaves its env out
BORDER_GUARD = 8.0            # a sphere within BORDER_GUARD 2^-24 |x| of a cell border or diagonal leaves its env out
DECISION_BAND = 1e-3          # |lt| / (mu ln), den / (0.05 nWn) this close to 1: no class-specific check
SLIDE_SPEED = 1e-2            # the direction of f_t is checked above this |vfree_t| (m/s)
MAX_LEFT_OUT = 0.02           # share of a case the decision band / the cell borders may leave out
MIN_ELIGIBLE = 0.85
MIN_COUNT = 10
TERRAIN_FRICTION = 0.1        # of the contact-law cases: friction_env from helpers.random_env_params is >= -0.5, so the shipped 1.0
#                               never reaches mu = 0; with 0.1 every draw below -0.1 (11 %) does, and mu still goes up to 1.55

# tier -> K_ref: the fp32 oracle's largest ratio over every case of tests/test_contact_law.py (measured and asserted there)
K_REF = {"vel": 16.09, "cone": 1.89, "dir": 1.21, "sensor": 3.02, "mom": 3.15}


def bound(tier):
    """C of a tier: 4 x K_ref rounded up to a power of two."""
    c = 2.0 ** np.ceil(np.log2(4.0 * K_REF[tier]))
    assert c <= C_CAP, (tier, c)
    return float(c)


# ---------------------------------------------------------------------------------------------------------------- model tables
def table_model(model, wmodel):
    """The RobotModel with the float32 tables of the wbc_model (what the kernel and the oracle read) as doubles."""
    tm = copy.copy(model)
    nb, nrb = model.nb, len(model.rb_body)
    f = lambda a, n: np.array([[float(x) for x in row] for row in list(a)[:n]])
    tm.joint_xyz, tm.com, tm.inertia = f(wmodel.joint_xyz, nb), f(wmodel.com, nb), f(wmodel.inertia, nb)
    tm.mass = np.array([float(x) for x in list(wmodel.mass)[:nb]])
    tm.rb_offset = f(wmodel.rb_offset, nrb)
    return tm


def spheres(wmodel):
    """The robot's 28 terrain spheres in the order of their compact index: dicts slot, body (moving body), rb, rad, pos (body frame)."""
    out = [None] * NSPH
    for k in range(wmodel.ncp):
        if wmodel.cp_kind[k] == abi.CP_TERRAIN and wmodel.cp_body[k] != abi.BOX_BODY:
            out[wmodel.cp_sph[k]] = dict(slot=k, body=int(wmodel.cp_body[k]), rb=int(wmodel.cp_rb[k]), rad=float(wmodel.cp_radius[k]),
                                         pos=np.array([float(x) for x in wmodel.cp_pos[k]]))
    assert all(s is not None for s in out)
    return out


def law_cfg(tcfg):
    return dict(margin=float(tcfg.contact_margin), erp=float(tcfg.contact_erp), vmax=float(tcfg.max_depenetration_vel),
                terrain_friction=float(tcfg.terrain_friction), dt=float(tcfg.sim_dt), ground_z=float(tcfg.ground_z))


def case_cfg(tcfg, **kw):
    """The task cfg of the contact-law cases: terrain_friction = TERRAIN_FRICTION; kw: further fields."""
    tc = type(tcfg).from_buffer_copy(tcfg)
    tc.terrain_friction = TERRAIN_FRICTION
    for k, v in kw.items():
        setattr(tc, k, v)
    return tc


def cap_depth(cfg):
    """Penetration from which vn_tgt is max_depenetration_vel."""
    return cfg["vmax"] * cfg["dt"] / cfg["erp"]


# --------------------------------------------------------------------------------------------------------------------- terrain
def terrain_query(ter, ground_z, x, y, other_diagonal=False, unit_normal=True):
    """terrain_query of the spec restated, vectorised over x, y: (h, n [..., 3], aux). ter: None (the plane z = ground_z) or
    dict(heights int16 [rows, cols], hs, vs, tx, ty, tz). Indices truncate toward zero and clip to [0, rows - 2]; u, v are clamped to
    [0, 1]; the cell is split along the (i, j)-(i+1, j+1) diagonal, u >= v choosing the triangle; n = (-gx, -gy, 1) / |.|.
    aux: tri (0: u >= v), clipped (an index or u, v was clipped), near_border (within the guard of a border or the diagonal),
    slope_mag = |dh/dx| mag(x - tx) + |dh/dy| mag(y - ty). other_diagonal / unit_normal = False: two of the seeded faults."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if ter is None:
        n = np.zeros(x.shape + (3,))
        n[..., 2] = 1.0
        z = np.zeros(x.shape)
        return np.full(x.shape, float(ground_z)), n, dict(tri=z.astype(int), clipped=z.astype(bool), near_border=z.astype(bool), slope_mag=z)
    H, hs, vs = np.asarray(ter["heights"]), float(ter["hs"]), float(ter["vs"])
    rows, cols = H.shape
    fx, fy = (x - ter["tx"]) / hs, (y - ter["ty"]) / hs
    ix, iy = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
    ix, iy = np.clip(ix, 0, rows - 2), np.clip(iy, 0, cols - 2)
    uu, vv = fx - ix, fy - iy
    u, v = np.clip(uu, 0.0, 1.0), np.clip(vv, 0.0, 1.0)
    h00, h10, h01, h11 = H[ix, iy] * vs, H[ix + 1, iy] * vs, H[ix, iy + 1] * vs, H[ix + 1, iy + 1] * vs
    if not other_diagonal:
        tri = ~(u >= v)
        dhdx, dhdy = np.where(tri, h11 - h01, h10 - h00), np.where(tri, h01 - h00, h11 - h10)
        hh = h00 + u * dhdx + v * dhdy
    else:                                                                    # split along (i+1, j)-(i, j+1)
        tri = ~(u + v <= 1.0)
        dhdx, dhdy = np.where(tri, h11 - h01, h10 - h00), np.where(tri, h11 - h10, h01 - h00)
        hh = np.where(tri, h11 - (1 - u) * dhdx - (1 - v) * dhdy, h00 + u * dhdx + v * dhdy)
    gx, gy = dhdx / hs, dhdy / hs
    inv = 1.0 / np.sqrt(gx * gx + gy * gy + 1.0) if unit_normal else np.ones(x.shape)
    n = np.stack([-gx * inv, -gy * inv, inv], axis=-1)
    cx, cy = (uu != u), (vv != v)
    du, dv = BORDER_GUARD * EPS * np.abs(x) / hs, BORDER_GUARD * EPS * np.abs(y) / hs
    near = (~cx & (np.minimum(uu, 1 - uu) <= du)) | (~cy & (np.minimum(vv, 1 - vv) <= dv)) | (np.abs(u - v) <= du + dv)
    slope_mag = np.abs(gx) * (np.abs(x) + abs(ter["tx"])) + np.abs(gy) * (np.abs(y) + abs(ter["ty"]))
    return hh + ter["tz"], n, dict(tri=tri.astype(int), clipped=cx | cy, near_border=near, slope_mag=slope_mag)


# -------------------------------------------------------------------------------------------------------------------- geometry
DEFAULT_SPEC = dict(erp=None, terrain_friction=None, radius_delta=None, gap_without_nz=False, other_diagonal=False, unit_normal=True,
                    direction_from_stick=False, lever_sign=1.0)


def geometry(tm, sph, ter, cfg, root, q, spec=DEFAULT_SPEC):
    """Step 1 for one env, in the spec's frame F (origin at the root, the base's axes; R0 = quat_to_mat of the STORED quaternion maps it to
    the world, as the spec does -- a float32 quaternion is not exactly of unit length and R0 not exactly orthonormal): dict(R0, E, p
    (fk in F), X [28, 3] world centres, rad, h, nw (world normal), n = R0^T nw, mag_n (the sizes of the summands of n: what its
    rounding, the stored quaternion's included, is proportional to), gap, xc = centre - rad n (F), active, mag_gap, aux)."""
    E, p = ao.fk(tm, np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]), np.asarray(q, dtype=np.float64))
    R0 = ao.quat_to_mat(np.asarray(root[3:7], dtype=np.float64))
    xk = np.array([p[s["body"]] + E[s["body"]] @ s["pos"] for s in sph])
    X = np.asarray(root[0:3], dtype=np.float64) + xk @ R0.T
    rad = np.array([s["rad"] for s in sph])
    if spec["radius_delta"] is not None:
        rad = rad.copy()
        rad[spec["radius_delta"][0]] += spec["radius_delta"][1]
    h, nw, aux = terrain_query(ter, cfg["ground_z"], X[:, 0], X[:, 1], spec["other_diagonal"], spec["unit_normal"])
    gap = (X[:, 2] - h) * (1.0 if spec["gap_without_nz"] else nw[:, 2]) - rad
    mag_gap = np.abs(X[:, 2]) + np.abs(h) + rad + aux["slope_mag"]
    n = nw @ R0
    x, y, z, w = np.abs(np.asarray(root[3:7], dtype=np.float64))
    mag_R0 = np.array([[1 + 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 + 2 * (x * x + z * z), 2 * (y * z + w * x)],
                       [2 * (x * z + w * y), 2 * (y * z + w * x), 1 + 2 * (x * x + y * y)]])
    return dict(R0=R0, E=E, p=p, X=X, rad=rad, h=h, nw=nw, n=n, mag_n=np.abs(nw) @ mag_R0, gap=gap, xc=xk - rad[:, None] * n, active=gap < cfg["margin"],
                mag_gap=mag_gap, aux=aux)


def vn_target(cfg, gap, mag_gap, erp=None):
    """(vn_tgt, mag, branch) with branch 0 speculative, 1 erp pen / dt, 2 the max_depenetration_vel cap."""
    erp, dt = cfg["erp"] if erp is None else erp, cfg["dt"]
    if gap >= 0:
        return -gap / dt, mag_gap / dt, 0
    v = erp * (-gap) / dt
    if v < cfg["vmax"]:
        return v, erp * mag_gap / dt, 1
    return cfg["vmax"], 0.0, 2


def _ratio(res, scale):
    """res / (2^-24 scale), entry-wise; an entry whose scale is 0 has to be exactly 0."""
    res, scale = np.atleast_1d(np.abs(res)).astype(np.float64), np.atleast_1d(scale).astype(np.float64)
    out = np.where(res == 0, 0.0, np.inf)
    nz = scale > 0
    out[nz] = res[nz] / (EPS * scale[nz])
    return float(out.max())


def _tangent(v, n):
    vn = float(v @ n)
    return vn, v - vn * n


# ----------------------------------------------------------------------------------------------------------------- the checker
CLASSES = ("separating", "stick", "slide", "fallback")


def check_env(model, wmodel, tcfg, ter, root0, dof0, root1, dof1, ncf, fs, body_params, friction, law=True, spec=DEFAULT_SPEC,
              self_clear=True, _cache={}):
    """Steps 1 to 5 for one env. Returns dict(
         left_out   None or why the env is not checked at all: "clamp", "limit", "margin", "border", "self" (self_clear False)
         nactive, active [28], exact [..] descriptions of violated EXACT requirements (activation, zero rows, zero sensors)
         ratio {tier: largest residual / (2^-24 scale) of this env}
         cls        fp64 class of a single-contact env (CLASSES) or None; near (in a decision band); branch; mu; tri; clipped; sphere)"""
    key = (id(model), id(wmodel), bytes(tcfg))
    if key not in _cache:
        _cache[key] = (table_model(model, wmodel), spheres(wmodel), fdr.tables(wmodel, tcfg))
    tm, sph, tb = _cache[key]
    cfg = law_cfg(tcfg)
    if spec["terrain_friction"] is not None:
        cfg["terrain_friction"] = spec["terrain_friction"]
    dt = cfg["dt"]
    r0, r1 = fdr._robot_row(root0), fdr._robot_row(root1)
    dof0, dof1 = np.asarray(dof0, dtype=np.float64), np.asarray(dof1, dtype=np.float64)
    ncf, fs = np.asarray(ncf, dtype=np.float64).reshape(-1, 3), np.asarray(fs, dtype=np.float64).reshape(-1, 6)
    out = dict(left_out=None, exact=[], ratio={t: 0.0 for t in TIERS}, cls=None, near=False, branch=None, mu=None, tri=None, clipped=None,
               sphere=None, nactive=0)
    clamped = tb["qd_limit"] > 0
    lim = (tb["lo"] < tb["hi"]) & (np.arange(len(tb["lo"])) < 18)
    if not (np.abs(dof1[clamped, 1]) < tb["qd_limit"][clamped]).all():
        out["left_out"] = "clamp"
    elif not ((dof0[lim, 0] >= tb["lo"][lim]) & (dof0[lim, 0] <= tb["hi"][lim])).all():
        out["left_out"] = "limit"
    elif not self_clear:
        out["left_out"] = "self"
    g = geometry(tm, sph, ter, cfg, r0, dof0[:, 0], spec)
    out["active"], out["nactive"] = g["active"], int(g["active"].sum())
    if out["left_out"] is None and np.any(np.abs(g["gap"] - cfg["margin"]) <= MARGIN_GUARD * EPS * g["mag_gap"]):
        out["left_out"] = "margin"
    if out["left_out"] is None and np.any(g["aux"]["near_border"] & (g["gap"] < 2 * cfg["margin"])):
        out["left_out"] = "border"
    if out["left_out"] is not None:
        return out
    mu_mag = 0.5 * (abs(float(friction)) + abs(cfg["terrain_friction"]))
    mu = max(0.0, 0.5 * (float(friction) + cfg["terrain_friction"]))
    out["mu"] = mu
    # 2. activation
    by_rb = {}
    for k, s in enumerate(sph):
        by_rb.setdefault(s["rb"], []).append(k)
    for rb in range(ncf.shape[0]):
        if np.any(ncf[rb] != 0) and not any(g["active"][k] for k in by_rb.get(rb, [])):
            out["exact"].append(f"row {rb} is {ncf[rb]} without an active sphere")
    feet = list(tb["feet_rb"])
    R0 = g["R0"]
    Rinv = np.linalg.inv(R0)
    zero3, ident = np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    # in F: velocities are R0^T (world), accelerations and forces R0^-1 (world) -- the spec adds dt R0 acc_F to the world velocity
    dnu = (np.r_[r1[7:13], dof1[:, 1]] - np.r_[r0[7:13], dof0[:, 1]]) / dt
    nu0 = np.r_[R0.T @ r0[7:10], R0.T @ r0[10:13], dof0[:, 1]]
    a = np.r_[Rinv @ dnu[0:3], Rinv @ dnu[3:6], dnu[6:]]
    nu1 = nu0 + dt * a
    M = wb.mass_matrix(tm, zero3, ident, dof0[:, 0], body_params) + np.diag(tb["armature"])
    # 6. momentum: the root rows of the equations of motion carry no joint torque -- the rate of the robot's momentum about the root's
    # origin is gravity's and the contact forces' wrench (linear rows: every env; angular rows: the one contact's point is known)
    idt, mag_id = idr.inverse_dynamics(tm, zero3, ident, dof0[:, 0], nu0, a, body_params, R0.T @ np.asarray(tb["gravity"]))
    fF = ncf[:27] @ Rinv.T
    res, sc = idt[0:6].copy(), mag_id[0:6] + (np.abs(M[0:6]) @ (np.abs(nu0) + np.abs(nu1))) / dt
    res[0:3] -= fF.sum(0)
    sc[0:3] += np.abs(fF).sum(0)
    rows = slice(0, 3)
    if out["nactive"] == 1:
        k1 = int(np.flatnonzero(g["active"])[0])
        f1, x1 = fF[sph[k1]["rb"]], g["xc"][k1]
        res[3:6] -= wb.cross3(x1, f1)
        sc[3:6] += np.array([abs(x1[1] * f1[2]) + abs(x1[2] * f1[1]), abs(x1[2] * f1[0]) + abs(x1[0] * f1[2]), abs(x1[0] * f1[1]) + abs(x1[1] * f1[0])])
        rows = slice(0, 6)
    out["ratio"]["mom"] = _ratio(res[rows], sc[rows])
    bent = {}

    def the_law():
        """3. the velocity-level law of the one active contact; returns the slide term of the cone scale."""
        k = int(np.flatnonzero(g["active"])[0])
        s, n, mag_n, xc, gap = sph[k], g["n"][k], g["mag_n"][k], g["xc"][k], float(g["gap"][k])
        out.update(sphere=k, tri=int(g["aux"]["tri"][k]), clipped=bool(g["aux"]["clipped"][k]))
        J = wb.point_jacobian(tm, g["E"], g["p"], s["body"], xc)
        acc, mag = cdr.body_accelerations(tm, zero3, ident, dof0[:, 0], nu0)
        origin = g["p"][s["body"]] + g["E"][s["body"]] @ tm.rb_offset[s["rb"]]
        lever, om, al = xc - origin, J[3:6] @ nu0, acc[s["rb"], 3:6]
        jdnu = acc[s["rb"], 0:3] + wb.cross3(al, lever) + wb.cross3(om, wb.cross3(om, lever))
        mag_jdnu = mag[s["rb"], 0] + (np.linalg.norm(al) + np.linalg.norm(om) ** 2) * np.linalg.norm(lever)
        Jp = J[0:3]
        vplus = Jp @ nu0 + dt * (Jp @ a + jdnu)
        f = Rinv @ ncf[s["rb"]]
        lam = f * dt
        W = Jp[:, LIVE] @ np.linalg.solve(M[np.ix_(LIVE, LIVE)], Jp[:, LIVE].T)
        vfree = vplus - W @ lam
        vn_tgt, mag_vn, branch = vn_target(cfg, gap, g["mag_gap"][k], spec["erp"])
        out["branch"] = branch
        scale = np.abs(Jp) @ (np.abs(nu0) + np.abs(nu1)) + dt * mag_jdnu + np.abs(W) @ np.abs(lam) + np.abs(n) * mag_vn + mag_n * abs(vn_tgt)
        scale_n = float(np.abs(n) @ scale + mag_n @ np.abs(vplus))
        vn_free, vt_free = _tangent(vfree, n)
        vtn = float(np.linalg.norm(vt_free))
        st = np.linalg.solve(W, n * vn_tgt - vfree)                               # the stick impulse
        ln, lt = _tangent(st, n)
        ltn = float(np.linalg.norm(lt))
        vel = out["ratio"]["vel"]
        forced = bool(np.any(ncf[s["rb"]] != 0))
        if vn_free >= vn_tgt:
            out["cls"] = "separating"
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
        if not forced:
            # no force: the point must leave at least as fast as the target asks
            out["ratio"]["vel"] = max(vel, _ratio(max(0.0, vn_tgt - float(n @ vplus)), scale_n))
            return 0.0
        # a force: the free velocity was short of the target, and the force closes exactly the gap along n
        vel = max(vel, _ratio(max(0.0, vn_free - vn_tgt), scale_n), _ratio(float(n @ vplus) - vn_tgt, scale_n))
        fn, ftan = _tangent(f, n)
        mag_fn = float(np.abs(f) @ mag_n)
        mag_ft = float(np.linalg.norm(np.abs(f) + mag_fn * np.abs(n) + abs(fn) * mag_n))
        # n = R0^T nw is of unit length only up to the rounding of the stored quaternion; vhat_t . n = (vfree . n - (n.vfree) (n.n)) /
        # |vfree_t|, the difference of two terms of size |n.vfree|, passes that on to f.n of a sliding contact
        bent = mu_mag * (2.0 * float(np.abs(vfree) @ mag_n) + abs(vn_free) * 2.0 * float(np.abs(n) @ mag_n)) / vtn if vtn > 1e-6 else 0.0
        if out["cls"] != "separating" and not out["near"]:
            if out["cls"] == "stick":
                vel = max(vel, _ratio(vplus - n * vn_tgt, scale))
            elif out["cls"] == "fallback":
                out["ratio"]["cone"] = max(out["ratio"]["cone"], _ratio(np.linalg.norm(ftan), mag_ft))
            else:
                out["ratio"]["cone"] = max(out["ratio"]["cone"],
                                           _ratio(np.linalg.norm(ftan) - mu * fn, mag_ft + mu_mag * mag_fn * (1.0 + bent)))
                if mu > 0 and vtn > SLIDE_SPEED:
                    ref = lt / ltn if spec["direction_from_stick"] else -vt_free / vtn
                    ftn = float(np.linalg.norm(ftan))
                    res = np.linalg.norm(ftan / ftn - ref) if ftn > 0 else np.inf
                    out["ratio"]["dir"] = max(out["ratio"]["dir"], _ratio(res, (mag_ft / ftn if ftn > 0 else 0.0) + np.linalg.norm(scale) / vtn))
        out["ratio"]["vel"] = vel
        return bent

    if law and out["nactive"] == 1:
        bent[int(np.flatnonzero(g["active"])[0])] = the_law()
    # 4. cone and sign, 5. sensors
    plane = ter is None
    for rb in range(27):
        f = ncf[rb]
        if plane and np.any(f != 0):
            out["ratio"]["cone"] = max(out["ratio"]["cone"], _ratio(max(0.0, -f[2]), np.abs(f).sum()))
    for ft, rb in enumerate(feet):
        (k,) = by_rb[rb]
        f, n, rad = Rinv @ ncf[rb], g["n"][k], g["rad"][k]
        if not np.any(ncf[rb] != 0):
            if np.any(fs[ft] != 0):
                out["exact"].append(f"sensor {ft} is {fs[ft]} without a force")
            continue
        fn, ftan = _tangent(f, n)
        mag_fn = float(np.abs(f) @ g["mag_n"][k])
        mag_ft = float(np.linalg.norm(np.abs(f) + mag_fn * np.abs(n) + abs(fn) * g["mag_n"][k]))
        out["ratio"]["cone"] = max(out["ratio"]["cone"], _ratio(max(0.0, -fn), mag_fn),
                                   _ratio(max(0.0, np.linalg.norm(ftan) - mu * fn), mag_ft + mu_mag * mag_fn * (1.0 + bent.get(k, 0.0))))
        Rb = g["E"][sph[k]["body"]]
        want = np.r_[Rb.T @ f, Rb.T @ wb.cross3(spec["lever_sign"] * (-rad) * n, f)]
        fnorm = float(np.linalg.norm(f))
        out["ratio"]["sensor"] = max(out["ratio"]["sensor"], _ratio(fs[ft] - want, np.full(6, fnorm + rad * fnorm)))
    return out


# ------------------------------------------------------------------------------------------------------------ case generators
def _batch_fk(tm, quat, q):
    """Body rotations [n, nb, 3, 3] and origins [n, nb, 3] with the root at the origin (generator only; the checker uses ao.fk)."""
    n = len(q)
    R, p = np.zeros((n, tm.nb, 3, 3)), np.zeros((n, tm.nb, 3))
    R[:, 0] = scg.rotm(quat)
    for i in range(1, tm.nb):
        par, ax = tm.parent[i], tm.axis[i]
        p[:, i] = p[:, par] + R[:, par] @ tm.joint_xyz[i]
        c, s = np.cos(q[:, tm.body_dof[i]]), np.sin(q[:, tm.body_dof[i]])
        Rq = np.zeros((n, 3, 3))
        a1, a2 = (ax + 1) % 3, (ax + 2) % 3
        Rq[:, ax, ax] = 1.0
        Rq[:, a1, a1], Rq[:, a1, a2], Rq[:, a2, a1], Rq[:, a2, a2] = c, -s, s, c
        R[:, i] = R[:, par] @ Rq
    return R, p


def _quat_down(d, yaw):
    """Unit quaternions (xyzw) of the rotations that take the body-frame directions d [n, 3] to world -z, then turn by yaw about z."""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    t = np.array([0.0, 0.0, -1.0])
    ax = np.cross(d, t)
    s, c = np.linalg.norm(ax, axis=1), d @ t
    ang = np.arctan2(s, c)
    ax = np.where(s[:, None] > 1e-9, ax / np.maximum(s, 1e-30)[:, None], np.array([1.0, 0.0, 0.0]))
    q1 = np.c_[ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)]
    qz = np.c_[np.zeros((len(d), 2)), np.sin(yaw / 2), np.cos(yaw / 2)]
    x1, y1, z1, w1 = q1.T
    x2, y2, z2, w2 = qz.T                                                        # qz (x) q1
    return np.stack([w2 * x1 + x2 * w1 + y2 * z1 - z2 * y1, w2 * y1 - x2 * z1 + y2 * w1 + z2 * x1,
                     w2 * z1 + x2 * y1 - y2 * x1 + z2 * w1, w2 * w1 - x2 * x1 - y2 * y1 - z2 * z1], axis=1)


def rough_grid(seed, rows=48, cols=48):
    """A rough int16 height grid: neighbours differ by up to one cell width (slopes to 45 degrees and a little beyond on the diagonal
    triangle), so the two triangles of most cells differ strongly. hs = 1/8 m, vs = 1/256 m and a translation of about 20 m, all
    exact in float32 (the kernel stores them as floats). (heights, hs, vs, tx, ty, tz) as set_heightfield takes them."""
    rng = np.random.default_rng(seed)
    return dict(heights=rng.integers(-16, 17, (rows, cols)).astype(np.int16), hs=0.125, vs=1.0 / 256.0, tx=20.5, ty=-19.75, tz=0.25)


def heightfield_args(ter):
    return (ter["heights"], ter["hs"], ter["vs"], ter["tx"], ter["ty"], ter["tz"])


def single_contact_states(model, wmodel, tcfg, ter, targets, seed, border_share=0.0, clip_share=0.0, wide=False, deficit=(-1.5, 0.5)):
    """(root [n, 2, 13], dof [n, 20, 2], tau [n, 20]) float32, one env per entry of `targets` (sphere indices): a pose drawn as
    fdr.airborne_states draws it (joints 0.05 rad inside their limits, |qd| <= 2 legs / 1 arm, |omega| <= 2) with the attitude turned so
    that the target sphere points down (plus noise), the root moved so that the target sphere's gap is a draw from
    (-0.04, margin - 0.5 mm) (speculative, erp and capped targets) and its contact point has a drawn velocity: approach
    vn_tgt + U(deficit) along the normal, tangential speed U(0, 1.2) times that deficit (stick, slide and separating all occur; the
    deficit is the velocity the impulse has to supply: 1.5 m/s on a foot, 0.45 m/s on the trunk and the arm, whose joints would
    otherwise be thrown into their velocity clamp). A draw is rejected unless every other sphere clears the margin by 1 mm and every self-collision pair of
    tests/self_collision_geometry.py by 5 mm. On a grid the sphere's (x, y) is drawn over the grid, a share border_share within 1e-3
    cell of a cell border or the diagonal, a share clip_share beyond the grid's edge. Small torques (|tau| <= 2 legs / 0.3 arm) keep the
    approach the draw asked for; the box is parked 50 m away, 5 m up."""
    rng = np.random.default_rng(seed)
    tm, sph, tb = table_model(model, wmodel), spheres(wmodel), fdr.tables(wmodel, tcfg)
    cfg = law_cfg(tcfg)
    targets = np.asarray(targets, dtype=int)
    n = len(targets)
    rad = np.array([s["rad"] for s in sph])
    names = list(model.rb_names)
    trunk = names.index("trunk")
    root, dof = np.zeros((n, 2, 13)), np.zeros((n, 20, 2))
    done = np.zeros(n, dtype=bool)
    lim = tb["lo"] < tb["hi"]
    for _ in range(400):
        left = np.flatnonzero(~done)
        if len(left) == 0:
            break
        todo = np.repeat(left, min(64, max(1, 2048 // len(left))))               # several candidates per open env, the first admissible one wins
        m = len(todo)
        tg = targets[todo]
        q = np.array([float(x) for x in tcfg.default_dof_pos])[None] + rng.uniform(-0.6, 0.6, (m, 20))
        if wide:
            q[:, lim] = rng.uniform(tb["lo"][lim], tb["hi"][lim], (m, int(lim.sum())))
        q[:, lim] = np.clip(q[:, lim], tb["lo"][lim] + 0.05, tb["hi"][lim] - 0.05)
        q[:, 18:] = 0
        qd = np.zeros((m, 20))
        qd[:, :12], qd[:, 12:18] = rng.uniform(-2, 2, (m, 12)), rng.uniform(-1, 1, (m, 6))
        ident = np.tile([0.0, 0.0, 0.0, 1.0], (m, 1))
        R, p = _batch_fk(tm, ident, q)
        cen = np.stack([p[:, s["body"]] + R[:, s["body"]] @ s["pos"] for s in sph], axis=1)            # [m, 28, 3] in the base frame
        gap_t = rng.uniform(-0.04, cfg["margin"] - 5e-4, m)
        # the attitude: among 192 random directions, one along which the target sphere sticks out beyond every other sphere by what the
        # draw needs over a plane (any of them, at random); where there is none, one of the eight along which it comes closest
        dirs = rng.normal(size=(192, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        reach = cen @ dirs.T + rad[None, :, None]                                 # [m, 28, 192]
        own = reach[np.arange(m), tg]
        reach[np.arange(m), tg] = -np.inf
        clear = own - reach.max(1) - (cfg["margin"] + 1.5e-3 - gap_t)[:, None]    # [m, 192]
        feas = clear > 0
        best8 = ~feas.any(1)[:, None] & (clear >= np.sort(clear, axis=1)[:, -8][:, None])
        score = np.where(feas | best8, rng.random(clear.shape), -1.0)
        quat = _quat_down(dirs[np.argmax(score, axis=1)], rng.uniform(-np.pi, np.pi, m))
        R, p = _batch_fk(tm, quat, q)
        cen = np.stack([p[:, s["body"]] + R[:, s["body"]] @ s["pos"] for s in sph], axis=1)            # root at the origin
        ct = cen[np.arange(m), tg]
        if ter is None:
            xy = rng.uniform(-1, 1, (m, 2))
        else:
            rows, cols = ter["heights"].shape
            cell = np.stack([rng.integers(1, rows - 2, m), rng.integers(1, cols - 2, m)], 1).astype(np.float64)
            uv = rng.uniform(0.02, 0.98, (m, 2))
            kind = rng.random(m)
            nb_ = kind < border_share
            which = rng.integers(0, 3, m)
            tiny = rng.uniform(-1e-3, 1e-3, m)
            uv[nb_ & (which == 0), 0] = tiny[nb_ & (which == 0)]
            uv[nb_ & (which == 1), 1] = tiny[nb_ & (which == 1)]
            uv[nb_ & (which == 2), 1] = (uv[:, 0] + tiny)[nb_ & (which == 2)]
            cl = ~nb_ & (kind < border_share + clip_share)
            side = rng.integers(0, 4, m)
            off = rng.uniform(0.3, 4.0, m)
            cell[cl & (side == 0), 0] = -off[cl & (side == 0)]
            cell[cl & (side == 1), 0] = (rows - 1 + off)[cl & (side == 1)]
            cell[cl & (side == 2), 1] = -off[cl & (side == 2)]
            cell[cl & (side == 3), 1] = (cols - 1 + off)[cl & (side == 3)]
            xy = np.stack([ter["tx"] + (cell[:, 0] + uv[:, 0]) * ter["hs"], ter["ty"] + (cell[:, 1] + uv[:, 1]) * ter["hs"]], 1)
        pos = np.zeros((m, 3))
        pos[:, 0:2] = xy - ct[:, 0:2]
        X = cen + pos[:, None, :]
        h, nrm, _ = terrain_query(ter, cfg["ground_z"], X[:, :, 0], X[:, :, 1])
        ht, nt = h[np.arange(m), tg], nrm[np.arange(m), tg]
        pos[:, 2] = ht + (gap_t + rad[tg]) / nt[:, 2] - ct[:, 2]
        X = cen + pos[:, None, :]
        gaps = (X[:, :, 2] - h) * nrm[:, :, 2] - rad[None]
        gaps[np.arange(m), tg] = np.inf
        ok = (gaps > cfg["margin"] + 1e-3).all(1)
        if not ok.any():
            continue
        cand = np.flatnonzero(ok)
        rbs = np.zeros((len(cand), len(names), 7))
        rbs[:, :, 0:3] = np.stack([p[cand, b] + R[cand, b] @ tm.rb_offset[r] for r, b in enumerate(tm.rb_body)], axis=1)
        rbs[:, trunk, 3:7] = quat[cand]
        ok[cand] = np.min(np.stack(list(scg.all_pairs(rbs, names).values()), 0), axis=0) > cfg["margin"] + 5e-3
        # velocities: the contact point's velocity with the root at rest, then the root's linear velocity makes up the difference
        omega = rng.uniform(-2, 2, (m, 3))
        w, v = np.zeros((m, tm.nb, 3)), np.zeros((m, tm.nb, 3))
        w[:, 0] = omega
        for b in range(1, tm.nb):
            par = tm.parent[b]
            w[:, b] = w[:, par] + R[:, b][:, :, tm.axis[b]] * qd[:, tm.body_dof[b]][:, None]
            v[:, b] = v[:, par] + np.cross(w[:, par], p[:, b] - p[:, par])
        bt = np.array([sph[k]["body"] for k in tg])
        xc = ct - rad[tg][:, None] * nt
        vp = v[np.arange(m), bt] + np.cross(w[np.arange(m), bt], xc - p[np.arange(m), bt])
        vn_tgt = np.array([vn_target(cfg, g_, 0.0)[0] for g_ in gap_t])
        short = rng.uniform(deficit[0], deficit[1], m)
        t1 = np.cross(nt, rng.normal(size=(m, 3)))
        t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
        want = nt * (vn_tgt + short)[:, None] + t1 * (rng.uniform(0, 1.2, m) * np.maximum(np.abs(short), 0.05))[:, None]
        _, first = np.unique(todo[ok], return_index=True)
        pick = np.flatnonzero(ok)[first]
        sel = todo[pick]
        root[sel, 0, 0:3], root[sel, 0, 3:7] = pos[pick], quat[pick]
        root[sel, 0, 7:10], root[sel, 0, 10:13] = (want - vp)[pick], omega[pick]
        dof[sel, :, 0], dof[sel, :, 1] = q[pick], qd[pick]
        done[sel] = True
    assert done.all(), f"no admissible pose for spheres {sorted(set(int(t) for t in targets[~done]))}"
    root[:, 1, 0:3] = root[:, 0, 0:3] + np.array([50.0, 0.0, 0.0])
    root[:, 1, 2] = 5.0 + np.abs(root[:, 0, 2])
    root[:, 1, 6] = 1
    tau = np.zeros((n, 20))
    tau[:, :12], tau[:, 12:18] = rng.uniform(-2, 2, (n, 12)), rng.uniform(-0.3, 0.3, (n, 6))
    return root.astype(np.float32), dof.astype(np.float32), tau.astype(np.float32)


FEET = [0, 1, 2, 3]
SHANKS = [23, 24, 25, 26]   # the mid-shank spheres (r = 0.008) lie on the segment between knee and foot (r = 0.02 each): over a PLANE one of
#                             those two is always lower, a mid-shank can be the only active sphere on a ridge of the height grid alone
OTHERS = [k for k in range(4, NSPH) if k not in SHANKS]  # knees, gripper tip, elbow, wrist, thigh tops, trunk corners, shoulder
GRID_TARGETS = list(range(8)) + SHANKS                   # feet, knees, mid-shanks
GRID_SEED = 411
# name -> dict(n, seed, grid, targets, substeps, kind). kind "single": the law; "standing": fdr.contact_states, checks 2, 4, 5.
CASES = {
    "A-1": dict(n=1, seed=401, grid=False, targets=[2], substeps=1, kind="single"),
    "A-13": dict(n=13, seed=402, grid=False, targets=[i % 4 for i in range(13)], substeps=1, kind="single"),
    "A-256": dict(n=256, seed=403, grid=False, targets=[i % 4 for i in range(256)], substeps=1, kind="single"),
    "B-192": dict(n=192, seed=404, grid=False, targets=[OTHERS[i % 20] for i in range(192)], substeps=1, kind="single", wide=True, deficit=(-0.45, 0.15)),
    "C-256": dict(n=256, seed=405, grid=True, targets=[GRID_TARGETS[i % 12] for i in range(256)], substeps=1, kind="single"),
    "D-256": dict(n=256, seed=406, grid=False, targets=None, substeps=3, kind="standing"),
}
COVERED = ("A-256", "B-192", "C-256")                   # the cases large enough for the coverage counts
STEP_CASES = {"E-13": dict(n=13, seed=407, source="A-256"), "E-13-grid": dict(n=13, seed=412, source="C-256"),
              "E-2560": dict(n=2560, seed=408, source="A-256"), "E-2560-grid": dict(n=2560, seed=410, source="C-256")}
STEP_SIGMA, STEP_COUNTER = 0.6, 1


def case_terrain(case):
    return rough_grid(GRID_SEED) if case["grid"] else None


_STATES = {}


def case_states(robot, name):
    """(tcfg, terrain, root, dof, tau) of a case; computed once per process."""
    if name not in _STATES:
        case = CASES[name]
        tc = case_cfg(robot["tcfg"])
        ter = case_terrain(case)
        if case["kind"] == "single":
            st = single_contact_states(robot["model"], robot["wmodel"], tc, ter, case["targets"], case["seed"],
                                       border_share=0.12 if ter is not None else 0.0, clip_share=0.15 if ter is not None else 0.0,
                                       wide=case.get("wide", False), deficit=case.get("deficit", (-1.5, 0.5)))
        else:
            root, dof, tau = fdr.contact_states(tc, case["n"], case["seed"])
            root[:, 1, 2] = 5.0                                   # the box in the air: its row has to be exactly 0 as well
            st = (root, dof, tau)
        _STATES[name] = (tc, ter) + st
    return _STATES[name]


def step_states(robot, name, case=None, **cfg):
    """Tier E: (tcfg, terrain, root, dof, actions) -- the staged states of A-256 (plane) or C-256 (grid) tiled over the envs;
    decimation = 1, the attitude and height terminations out of reach (the staged poses are random attitudes a few cm above the ground).
    case: dict(n, seed, source[, sigma]) instead of STEP_CASES[name]; cfg: further fields of the task cfg (tests/decimation_reference.py)."""
    case = STEP_CASES[name] if case is None else case
    tc, ter, root, dof, _ = case_states(robot, case["source"])
    tc = case_cfg(tc, **dict(dict(decimation=1, term_rp_threshold=100.0, term_z_threshold=-100.0), **cfg))
    idx = np.arange(case["n"]) % len(root)
    rng = np.random.default_rng(case["seed"])
    act = (case.get("sigma", STEP_SIGMA) * rng.normal(size=(case["n"], 18))).astype(np.float32)
    root, dof = root[idx].copy(), dof[idx].copy()
    dof[:, 12:18, 1] *= 0.25          # the arm slower: the PD torques of the step would otherwise take its light joints into the velocity clamp
    return tc, ter, root, dof, act


def self_clear(model, wmodel, tcfg, root, dof):
    """Mask [n]: every self-collision pair of tests/self_collision_geometry.py clears the margin by 5 mm."""
    tm = table_model(model, wmodel)
    root, dof = np.asarray(root, dtype=np.float64), np.asarray(dof, dtype=np.float64)
    names = list(model.rb_names)
    R, p = _batch_fk(tm, root[:, 0, 3:7], dof[:, :, 0])
    rbs = np.zeros((len(root), len(names), 7))
    rbs[:, :, 0:3] = np.stack([p[:, b] + R[:, b] @ tm.rb_offset[r] for r, b in enumerate(tm.rb_body)], axis=1)
    rbs[:, names.index("trunk"), 3:7] = root[:, 0, 3:7]
    return np.min(np.stack(list(scg.all_pairs(rbs, names).values()), 0), axis=0) > float(tcfg.contact_margin) + 5e-3


# -------------------------------------------------------------------------------------------------------- running a sim through
def evaluate(robot, tcfg, ter, root0, dof0, root1, dof1, ncf, fs, bp, friction, law=True, envs=None, skip=None, spec=DEFAULT_SPEC):
    """check_env over a batch -> list of per-env results (None for the envs not in `envs`); skip: mask of envs to leave out."""
    n = len(dof0)
    clear = self_clear(robot["model"], robot["wmodel"], tcfg, root0, dof0)
    out = [None] * n
    for e in (range(n) if envs is None else envs):
        r = check_env(robot["model"], robot["wmodel"], tcfg, ter, root0[e], dof0[e], root1[e], dof1[e], ncf[e], fs[e], bp[e], friction[e],
                      law=law, spec=spec, self_clear=bool(clear[e]))
        if skip is not None and skip[e]:
            r["left_out"] = "reset"
        out[e] = r
    return out


def run_case(sim, robot, name, friction):
    """Load a case into `sim` (the adapters of forward_dynamics_reference) and check every substep from the sim's own previous state.
    Returns (results per substep, states per substep) -- the states for the seeded faults."""
    tc, ter, root, dof, tau = case_states(robot, name)
    case = CASES[name]
    sim.load(root, dof, tau)
    bp = sim.get("BODY_PARAMS")
    outs, states = [], []
    for _ in range(case["substeps"]):
        r0, d0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
        sim.simulate()
        st = dict(root0=r0, dof0=d0, root1=sim.get("ROOT_STATES"), dof1=sim.get("DOF_STATE"), ncf=sim.get("NET_CONTACT_FORCE"),
                  fs=sim.get("FORCE_SENSOR"), bp=bp, friction=np.asarray(friction, dtype=np.float64))
        outs.append(evaluate(robot, tc, ter, law=case["kind"] == "single", **st))
        states.append(st)
    return outs, states


def step_envs(n):
    return fdr.step_envs(n)


def run_step(sim, robot, name, friction):
    """Tier E: reset_all, the staged states loaded over the reset ones, ONE env step of one substep under 0.6-sigma actions; envs that
    reset in the step are left out, the step counter keeps the push away."""
    tc, ter, root, dof, act = step_states(robot, name)
    assert tc.decimation == 1
    sim.reset_all()
    sim.set_step_counter(STEP_COUNTER)
    assert tc.push_interval == 0 or STEP_COUNTER + 1 < tc.push_interval
    sim.load(root, dof, np.zeros((len(root), 20), dtype=np.float32))
    bp = sim.get("BODY_PARAMS")
    r0, d0 = sim.get("ROOT_STATES"), sim.get("DOF_STATE")
    sim.step(act)
    st = dict(root0=r0, dof0=d0, root1=sim.get("ROOT_STATES"), dof1=sim.get("DOF_STATE"), ncf=sim.get("NET_CONTACT_FORCE"),
              fs=sim.get("FORCE_SENSOR"), bp=bp, friction=np.asarray(friction, dtype=np.float64))
    return [evaluate(robot, tc, ter, envs=step_envs(len(root)), skip=sim.get("RESET_BUF") != 0, **st)], [st]


def summarise(outs):
    """Counts and the largest ratio per tier over the per-substep results of a case: dict(n, checked, left_out {why: count}, single,
    classes {class: count of forced or separating single-contact envs}, near, mu0, branches [3], tri [2], clipped, spheres (set),
    exact [...], worst {tier: (ratio, substep, env)})."""
    s = dict(n=0, checked=0, left_out={}, single=0, classes={c: 0 for c in CLASSES}, near=0, mu0=0, branches=[0, 0, 0], tri=[0, 0],
             clipped=0, spheres=set(), exact=[], worst={t: (0.0, -1, -1) for t in TIERS}, slow=0)
    for i, out in enumerate(outs):
        for e, r in enumerate(out):
            if r is None:
                continue
            s["n"] += 1
            if r["left_out"] is not None:
                s["left_out"][r["left_out"]] = s["left_out"].get(r["left_out"], 0) + 1
                continue
            s["checked"] += 1
            s["exact"] += [f"substep {i} env {e}: {x}" for x in r["exact"]]
            for t in TIERS:
                if r["ratio"][t] > s["worst"][t][0]:
                    s["worst"][t] = (r["ratio"][t], i, e)
            if r["cls"] is not None:
                s["single"] += 1
                s["classes"][r["cls"]] += 1
                s["near"] += int(r["near"])
                s["mu0"] += int(r["mu"] == 0.0)
                s["branches"][r["branch"]] += 1
                s["tri"][r["tri"]] += 1
                s["clipped"] += int(r["clipped"])
                s["spheres"].add(r["sphere"])
    return s


def report(name, s):
    w = ", ".join(f"{t} {s['worst'][t][0]:.3f} (substep {s['worst'][t][1]}, env {s['worst'][t][2]})" for t in TIERS)
    return (f"{name}: {s['checked']} of {s['n']} checked (left out {s['left_out']}), {s['single']} single-contact: {s['classes']}, "
            f"{s['near']} in a decision band, mu = 0: {s['mu0']}, vn_tgt branches {s['branches']}, triangles {s['tri']}, clipped {s['clipped']}; "
            f"largest ratios: {w}")
