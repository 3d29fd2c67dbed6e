"""TEST INFRASTRUCTURE ONLY -- CPU (numpy) restatement of the gait clock, the footholds and the swing references that
wbc_sim_footstep_plan computes (include/wbc_sim.h has the text; the step numbers below are its), batched over envs, in fp64 or -- the same
text, `dtype=np.float32` -- in fp32 as the yardstick of what single precision costs. Nothing here comes from the kernel: the leg kinematics
are estimator_reference's walk of widowgo1_model.json, the terrain query restates the step kernel's terrain_query on a numpy heightfield.

plan() also returns the MAGNITUDES an error is judged against (2^-24 mag), per env:
    pos        max(1, the env's largest |coordinate|: base position, foot origins, stored lift-off and target, nominal footholds, terrain heights met)
    vel        max(pos / T_sw, the largest size of a foot velocity's terms: |v| + rate_i reach_i)         (T_sw = 1 where duty >= 1)
    acc        pos / T_sw^2
    swing_acc  acc + kp pos + kd vel
    cost       per foot, the largest finite cost among its candidates (1 where there is none)
and, in `diag`, what thinness is judged from: the foot and stage phases, every candidate's cost, rough and n_z, the smallest distance of a
query point of the foot from a cell edge or diagonal of the grid (metres), and the index of the chosen candidate (-1: none, -2: no search)."""
import numpy as np

import estimator_reference as er

NS, NFEET = 32, 4
INFO_RESET, INFO_FAILED, INFO_NO_SAFE, INFO_LIFT = 1, 2, 16, 256
CFG_FIELDS = ("dt", "period", "duty", "offset", "horizon", "mpc_dt", "stance_offset", "k_v", "com_height", "max_reach", "swing_height", "latch",
              "kp", "kd", "search_radius", "search_step", "probe_radius", "w_dist", "w_rough", "w_slope", "rough_max", "nz_min")
OUTPUTS = ("swing_ref", "swing_acc", "foothold", "foot_pos", "state")                  # the continuous ones
EPS = 2.0 ** -24
GAITS = {"stand": (0.0, 0.0, 0.0, 0.0), "trot": (0.0, 0.5, 0.5, 0.0), "pace": (0.0, 0.5, 0.0, 0.5), "bound": (0.0, 0.0, 0.5, 0.5),
         "walk": (0.0, 0.5, 0.75, 0.25)}


def frac(x):
    return x - np.floor(x)


def bump(s):
    """b(s) = s^3 (10 - 15 s + 6 s^2), b'(s), b''(s)."""
    return s * s * s * (10 - 15 * s + 6 * s * s), 30 * s * s * (1 - s) * (1 - s), 60 * s * (1 - s) * (1 - 2 * s)


def terrain_query(terrain, x, y, ground_z=0.0, dtype=np.float64):
    """(h, n_z, margin) at the points x, y (any shape): the step kernel's terrain_query -- cell (ix, iy) = trunc of (x - tx) / hs clamped to
    [0, rows - 2], (u, v) clamped to [0, 1], the triangle u >= v or u < v of the cell, the plane z = ground_z without a heightfield -- and the
    point's distance in metres from the nearest interior grid line or from its cell's diagonal, across which the normal jumps."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    if terrain is None:
        return np.full(x.shape, ground_z, dtype=dtype), np.ones(x.shape, dtype=dtype), np.full(x.shape, np.inf)
    Hs = np.asarray(terrain["heights"])
    rows, cols = Hs.shape
    hs, vs = dtype(terrain["hs"]), dtype(terrain["vs"])
    t = [dtype(v) for v in terrain["t"]]
    fx, fy = (x - t[0]) / hs, (y - t[1]) / hs
    ix = np.clip(np.trunc(fx), 0, rows - 2).astype(np.int64)
    iy = np.clip(np.trunc(fy), 0, cols - 2).astype(np.int64)
    u = np.clip(fx - ix.astype(dtype), 0, 1).astype(dtype)
    v = np.clip(fy - iy.astype(dtype), 0, 1).astype(dtype)
    h00, h10 = Hs[ix, iy].astype(dtype) * vs, Hs[ix + 1, iy].astype(dtype) * vs
    h01, h11 = Hs[ix, iy + 1].astype(dtype) * vs, Hs[ix + 1, iy + 1].astype(dtype) * vs
    lower = u >= v
    dhdx = np.where(lower, h10 - h00, h11 - h01)
    dhdy = np.where(lower, h11 - h10, h01 - h00)
    h = h00 + u * dhdx + v * dhdy + t[2]
    gx, gy = dhdx / hs, dhdy / hs
    nz = 1 / np.sqrt(gx * gx + gy * gy + 1)
    # margins, in fp64 from the same numbers
    fx64, fy64, hs64 = fx.astype(np.float64), fy.astype(np.float64), float(hs)

    def line(f, count):                                                                # interior lines 1 .. count - 2
        if count <= 2:
            return np.full(f.shape, np.inf)
        return np.abs(f - np.clip(np.round(f), 1, count - 2)) * hs64
    both_clamped = ((u == 0) | (u == 1)) & ((v == 0) | (v == 1))
    diag = np.where(both_clamped, np.inf, np.abs(u.astype(np.float64) - v.astype(np.float64)) * hs64)
    margin = np.minimum(np.minimum(line(fx64, rows), line(fy64, cols)), diag)
    return h.astype(dtype), nz.astype(dtype), margin


def candidates(cfg, nom, terrain, ground_z, dtype):
    """Per candidate of the searches around nom [..., 2]: (c [..., K, 2], h, cost (inf: rejected), rough, nz, margin), index (a + R)(2R + 1) + (b + R)."""
    R = int(cfg["search_radius"])
    ab = np.array([(a, b) for a in range(-R, R + 1) for b in range(-R, R + 1)], dtype=dtype)           # [K, 2]
    d = ab * dtype(cfg["search_step"])
    c = nom[..., None, :] + d
    pr = dtype(cfg["probe_radius"])
    h, nz, margin = terrain_query(terrain, c[..., 0], c[..., 1], ground_z, dtype)
    rough = np.zeros_like(h)
    for dx, dy in ((pr, 0), (-pr, 0), (0, pr), (0, -pr)):
        hp, _, mp = terrain_query(terrain, c[..., 0] + dtype(dx), c[..., 1] + dtype(dy), ground_z, dtype)
        rough = np.maximum(rough, np.abs(hp - h))
        margin = np.minimum(margin, mp)
    ok = ~((rough > dtype(cfg["rough_max"])) | (nz < dtype(cfg["nz_min"])))
    cost = dtype(cfg["w_dist"]) * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + dtype(cfg["w_rough"]) * (rough * rough) + dtype(cfg["w_slope"]) * (1 - nz)
    return c, h, np.where(ok, cost, np.inf), rough, nz, margin


def plan(model, cfg, state, base_pos, base_vel, quat, ang_vel, dof, vel_cmd=None, yaw_rate=None, terrain=None, gravity=(0.0, 0.0, -9.81),
         ground_z=0.0, reset=None, phase_init=None, hold=False, dtype=np.float64):
    """One call of wbc_sim_footstep_plan for a batch. state [N, 32]; ang_vel the root's WORLD angular velocity; reset: None, True (every env) or
    a mask [N]. Returns a dict: the new `state`, every output, `mag` and `diag` (module docstring)."""
    D = dtype
    f = lambda a: np.asarray(a, dtype=D)                                               # noqa: E731
    state, b, v, dof = f(state), f(base_pos), f(base_vel), f(dof)
    n = b.shape[0]
    H, R = int(cfg["horizon"]), int(cfg["search_radius"])
    K = (2 * R + 1) ** 2
    cmd = np.zeros((n, 2), dtype=D) if vel_cmd is None else f(vel_cmd)
    wz = np.zeros(n, dtype=D) if yaw_rate is None else f(yaw_rate)
    rs = np.zeros(n, dtype=bool) if reset is None else (np.ones(n, dtype=bool) if reset is True else np.asarray(reset) != 0)
    p_init = np.zeros(n, dtype=D) if phase_init is None else f(phase_init)
    period, duty, dt = D(cfg["period"]), D(cfg["duty"]), D(cfg["dt"])
    offset, so = f(cfg["offset"]), f(cfg["stance_offset"])
    always = bool(duty >= 1)
    Tst, Tsw = duty * period, (1 - duty) * period

    with np.errstate(all="ignore"):
        Rm = er.quat_to_mat(quat, D)
        wb = np.einsum("nji,nj->ni", Rm, f(ang_vel))
        _, r, rdot, rate = er.measurement(model, quat, wb, dof, D)
        p, pd = b[:, None, :] + r, v[:, None, :] + rdot                                # [N, 4, 3]
        # 1 reset
        phase = np.where(rs, p_init, state[:, 0])
        feet = state[:, 4:].reshape(n, NFEET, 7)
        lift = np.where(rs[:, None, None], p, feet[:, :, 0:3])
        target = np.where(rs[:, None, None], p, feet[:, :, 3:6])
        flag = np.where(rs[:, None], 0, feet[:, :, 6])
        finite = np.isfinite(b).all(1) & np.isfinite(v).all(1) & np.isfinite(f(quat)).all(1) & np.isfinite(f(ang_vel)).all(1) & \
            np.isfinite(p).all((1, 2)) & np.isfinite(pd).all((1, 2)) & np.isfinite(cmd).all(1) & np.isfinite(wz) & np.isfinite(phase) & \
            (rs | np.isfinite(state).all(1))
        failed = ~finite
        # 2 clock
        x0 = phase[:, None] + offset[None, :]
        phi = x0 - np.floor(x0)
        stand = np.ones((n, NFEET), dtype=bool) if always else phi < duty
        s = np.zeros((n, NFEET), dtype=D) if always else np.where(stand, 0, (phi - duty) / (1 - duty)).astype(D)
        lifted = ~stand & (flag == 0)
        lift = np.where(lifted[..., None], p, lift)
        touched = stand & (flag != 0)
        target = np.where(touched[..., None], p, target)
        flag = np.where(lifted, 1, np.where(touched, 0, flag)).astype(D)
        # 3 nominal foothold
        t = np.where(stand, 0 if always else (duty - phi) * period + Tsw, (1 - s) * Tsw).astype(D)
        hn = np.sqrt(Rm[:, 0, 0] ** 2 + Rm[:, 1, 0] ** 2)
        ch, sh = np.where(hn > 0, Rm[:, 0, 0] / hn, 1).astype(D), np.where(hn > 0, Rm[:, 1, 0] / hn, 0).astype(D)
        vc = np.stack([ch * cmd[:, 0] - sh * cmd[:, 1], sh * cmd[:, 0] + ch * cmd[:, 1]], axis=-1)             # [N, 2]
        ang = wz[:, None] * t
        ca, sa = np.cos(ang), np.sin(ang)
        ct, st = ch[:, None] * ca - sh[:, None] * sa, sh[:, None] * ca + ch[:, None] * sa
        hip = b[:, None, 0:2] + vc[:, None, :] * t[..., None] + np.stack([ct * so[:, 0] - st * so[:, 1], st * so[:, 0] + ct * so[:, 1]], axis=-1)
        g = float(np.sqrt(sum(float(np.float32(c)) ** 2 for c in gravity)))
        k_c = D(np.float32(0.5 * np.sqrt(float(np.float32(cfg["com_height"])) / g))) if g > 0 else D(0)       # the host forms it in fp64 and hands a float over
        add = (D(0.5) * Tst) * v[:, 0:2] + D(cfg["k_v"]) * (v[:, 0:2] - vc) + k_c * np.stack([v[:, 1] * wz, -v[:, 0] * wz], axis=-1)
        ln = np.sqrt((add * add).sum(-1))
        long = ln > D(cfg["max_reach"])
        add = np.where(long[:, None], add * (D(cfg["max_reach"]) / np.where(long, ln, 1))[:, None], add).astype(D)
        nom = (hip + add[:, None, :]).astype(D)                                        # [N, 4, 2]
        nom_h, _, nom_margin = terrain_query(terrain, nom[..., 0], nom[..., 1], ground_z, D)
        # 4 terrain search
        search = ~stand & (s < D(cfg["latch"])) & ~failed[:, None]
        c, ch_, cost, rough, nz, cmargin = candidates(cfg, nom, terrain, ground_z, D)   # [N, 4, K, ...]
        best = np.argmin(cost, axis=-1)                                                # the first of equal minima: the lowest index
        take = lambda a: np.take_along_axis(a, best[..., None], axis=-1)[..., 0]       # noqa: E731
        none = ~np.isfinite(take(cost))
        found = np.stack([np.where(none, nom[..., 0], take(c[..., 0])), np.where(none, nom[..., 1], take(c[..., 1])), np.where(none, nom_h, take(ch_))], axis=-1)
        target = np.where(search[..., None], found, target).astype(D)
        nosafe = search & none
        # 5 swing reference
        sd = 1 / Tsw if not always else D(0)
        bb, b1, b2 = bump(s)
        dxy = target[..., 0:2] - lift[..., 0:2]
        pos = np.empty((n, NFEET, 3), dtype=D); vel = np.empty_like(pos); acc = np.empty_like(pos)
        pos[..., 0:2] = lift[..., 0:2] + dxy * bb[..., None]
        vel[..., 0:2] = dxy * (b1 * sd)[..., None]
        acc[..., 0:2] = dxy * (b2 * sd * sd)[..., None]
        za = np.maximum(lift[..., 2], target[..., 2]) + D(cfg["swing_height"])
        up = s < D(0.5)
        bb, b1, b2 = bump(np.where(up, 2 * s, 2 * s - 1).astype(D))
        z0, dz = np.where(up, lift[..., 2], za), np.where(up, za - lift[..., 2], target[..., 2] - za)
        pos[..., 2] = z0 + dz * bb
        vel[..., 2] = dz * (b1 * (2 * sd))
        acc[..., 2] = dz * (b2 * (2 * sd) * (2 * sd))
        sacc = acc + D(cfg["kp"]) * (pos - p) + D(cfg["kd"]) * (vel - pd)
        sw = ~stand[..., None]
        swing_ref = np.concatenate([np.where(sw, pos, p), np.where(sw, vel, 0), np.where(sw, acc, 0)], axis=-1).astype(D)
        swing_acc = np.where(sw, sacc, 0).astype(D)
        foothold = np.where(sw, target, np.concatenate([nom, nom_h[..., None]], axis=-1)).astype(D)
        # per-stage outputs
        schedule = np.zeros((n, H, NFEET), dtype=np.uint8)
        foot_pos = np.zeros((n, H, NFEET, 3), dtype=D)
        stage_phase = np.zeros((n, H, NFEET), dtype=D)
        if H > 0:
            k = np.arange(H, dtype=D)
            xk = (phase[:, None] + (k + D(0.5))[None, :] * (D(cfg["mpc_dt"]) / period))[:, :, None] + offset[None, None, :]     # [N, H, 4]
            flk = np.floor(xk)
            stage_phase = (xk - flk).astype(D)
            sk = np.ones(xk.shape, dtype=bool) if always else stage_phase < duty
            m = np.zeros(xk.shape, dtype=np.int64) if always else (flk - np.floor(x0)[:, None, :]).astype(np.int64)
            schedule = sk.astype(np.uint8)
            value = np.where((m <= 0)[..., None], p[:, None], foothold[:, None] + np.concatenate(
                [(np.maximum(m - 1, 0).astype(D) * period)[..., None] * vc[:, None, None, :], np.zeros(xk.shape + (1,), dtype=D)], axis=-1))
            for i in range(NFEET):
                nxt = None                                                             # backwards: the next stance stage's value
                fill = np.zeros((n, H), dtype=bool)
                for kk in range(H - 1, -1, -1):
                    cur = value[:, kk, i]
                    if nxt is None:
                        nxt, have = cur.copy(), sk[:, kk, i].copy()
                    else:
                        nxt = np.where(sk[:, kk, i][:, None], cur, nxt); have = have | sk[:, kk, i]
                    foot_pos[:, kk, i] = nxt
                    fill[:, kk] = have
                last, seen = foothold[:, i].copy(), np.zeros(n, dtype=bool)           # forwards: failing that, the last stance stage's, then the foothold
                for kk in range(H):
                    last = np.where(sk[:, kk, i][:, None], value[:, kk, i], last); seen = seen | sk[:, kk, i]
                    foot_pos[:, kk, i] = np.where(fill[:, kk][:, None], foot_pos[:, kk, i], last)
        # 6 advance
        adv = phase + dt / period
        new_phase = phase if hold else adv - np.floor(adv)
        new_state = np.concatenate([new_phase[:, None], np.zeros((n, 3), dtype=D), np.concatenate([lift, target, flag[..., None]], axis=-1).reshape(n, 28)], axis=1).astype(D)
        info = np.where(rs, INFO_RESET, 0) + (nosafe * (INFO_NO_SAFE << np.arange(NFEET))).sum(-1) + (lifted * (INFO_LIFT << np.arange(NFEET))).sum(-1)

    out = dict(state=new_state, stance=stand.astype(np.uint8), contact=stand.astype(D), schedule=schedule, foot_pos=foot_pos, foothold=foothold,
               swing_ref=swing_ref, swing_acc=swing_acc, info=info.astype(np.int64))
    if failed.any():
        for kname in ("stance", "contact", "schedule", "foot_pos", "foothold", "swing_ref", "swing_acc"):
            out[kname][failed] = 0
        out["state"][failed] = state[failed]
        out["info"][failed] = INFO_FAILED
    with np.errstate(all="ignore"):
        A = lambda a: np.abs(np.asarray(a, dtype=np.float64)).reshape(n, -1).max(1)    # noqa: E731
        hmet = np.where(np.isfinite(ch_), ch_, 0)
        posmag = np.maximum(1.0, np.max([A(b), A(p), A(lift), A(target), A(nom), A(nom_h), A(hmet), A(c)], axis=0))
        tsw = 1.0 if always else float(Tsw)
        velmag = np.maximum(posmag / tsw, (A(v)[:, None] + rate * er.reach(model)[None, :]).max(1))
        accmag = posmag / tsw ** 2
        fin = np.where(np.isfinite(cost), cost, 0).astype(np.float64).max(-1)
        mag = dict(pos=posmag, vel=velmag, acc=accmag, swing_acc=accmag + float(cfg["kp"]) * posmag + float(cfg["kd"]) * velmag,
                   cost=np.where(fin > 0, fin, 1.0))
    chosen = np.where(search, np.where(none, -1, best), -2)
    out["mag"] = mag
    out["diag"] = dict(phi=phi, s=s, stand=stand, search=search, stage_phase=stage_phase, cost=cost, rough=rough, nz=nz,
                       margin=np.where(search, cmargin.min(-1), np.where(stand, nom_margin, np.inf)), chosen=chosen, nom=nom, cand=c, cand_h=ch_,
                       failed=failed, lifted=lifted, vc=vc, p=p, pd=pd, t=t, hip=hip, add=add)
    return out


def entry_mags(ref):
    """The magnitude of every entry of the continuous outputs, shaped like them."""
    m = ref["mag"]
    n = m["pos"].shape[0]
    one = np.ones((n, NFEET, 3))
    sr = np.concatenate([one * m["pos"][:, None, None], one * m["vel"][:, None, None], one * m["acc"][:, None, None]], axis=-1)
    st = np.ones((n, NS)) * m["pos"][:, None]
    st[:, 0:4] = 1.0
    st[:, 10::7] = 1.0
    H = ref["foot_pos"].shape[1]
    return dict(swing_ref=sr, swing_acc=one * m["swing_acc"][:, None, None], foothold=one * m["pos"][:, None, None],
                foot_pos=np.ones((n, H, NFEET, 3)) * m["pos"][:, None, None, None], state=st)


def ratios(got, ref, keep=None):
    """{output: the largest |got - ref| / (2^-24 mag)} over the entries kept (keep: {output: bool mask shaped like it}, None: all)."""
    mags = entry_mags(ref)
    out = {}
    for k in OUTPUTS:
        err = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)) / (EPS * mags[k])
        if keep is not None:
            err = np.where(keep[k], err, 0.0)
        out[k] = float(err.max()) if err.size else 0.0
    return out
