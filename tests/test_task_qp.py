"""Whole-body inverse dynamics with torque limits and friction pyramids (wbc_sim_task_inverse_dynamics_qp; wbc_taskqp_solve_kernel in
csrc/wbc_arm_kernel.hip, definition in include/wbc_sim.h). The CPU tests pin the fp64 active-set reference of
tests/task_qp_reference.py to its own certificate, to tir.kkt_reference where nothing binds and to a closed form, and measure the fp32
yardstick; the GPU tests hold the kernel, for every env and row, to the sibling's equality tiers and to that certificate (feasibility,
the exact torque box, stationarity over the reported set, the reported set itself), and to its own invariances. No comparison of
torques is asserted: feasibility plus stationarity over the reported set proves optimality of this convex problem.

Limit sets (mu, fn_min, torque-limit scale) over the 60 members of test_task_inverse_dynamics._family: nominal (0.6, 2, 1), tight
(0.4, 5, 0.5), loose (1.0, 0, 1). In fp64 all 180 problems are feasible, 38 / 39 / 36 members have an active row and the largest active sets have 10 / 14 / 9 rows; the reference needs at most 28 / 32 / 22 iterations.

Bounds: ratio = residual / (2^-24 scale) <= C. K_ref is the fp32 numpy yardstick's largest ratio over the 180 problems (asserted
<= C / 16 on the CPU), C the smallest power of two >= 16 K_ref, capped at 16384 (C_F) and 32768 (C_S); the last column is the kernel's
largest ratio on an MI355X over every case of test_every_env_and_row (n = 1, 13, 64; three limit sets):

    check                                   K_ref     C        kernel's largest ratio
    feasibility and reported contact rows   304       8192     6212 (n = 64, force0 / no_tasks families; 454 with tilted normals)
    stationarity over the reported set      650       16384    7502 (n = 64, no tasks, loose)

Both share the scale of an fp32 evaluation of a row, sum_c |a_c| (|lambda_0c| + sum_j |G_cj tau_j|) + |b|, and tir's reduced-gradient
scale + sum_i y_i |n_i|. The yardstick is status 0 on all 180 problems with the fp64 active set on all of them, in at most 28 / 32 /
22 iterations (a violation tolerance of 8 x 2^-24 instead of the kernel's 256 x 2^-24 made two loose members cycle at a pyramid's
apex to the cap). Families without tasks keep a nudot_ref, as in the sibling. Printed per case and never asserted: |tau - tau_64| /
max |tau|, the relative objective excess and the iteration counts (kernel: 3.0e-3, 2.6e-5, at most 47 iterations on nominal and loose
and 53 on tight; sets of up to 14 rows; every env status 0 but 3 of 64 of the armature case under the tight set).
The factor of 20 between K_ref and the kernel's feasibility ratio is the states: the yardstick runs on the CPU
families, the kernel's largest ratios come from rollout states with joint speeds of 20-30 rad/s in the cases without tasks or with w_force = 0.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import arm_codegen
import constrained_dynamics_reference as cdr
import mass_solve_reference as msr
import task_inverse_dynamics_reference as tir
import task_qp_reference as tq
import test_task_inverse_dynamics as tti
from wbc_amd import abi

JOINTS, EPS, FINGERS = tir.JOINTS, tir.EPS, tir.FINGERS
SENTINEL = tti.SENTINEL
LDS_BYTES = 22336                                  # static LDS of wbc_taskqp_solve_kernel in this build
LDS_CAP = 32 * 1024                                # five workgroups per CU of the 160 KiB
SETS = list(tq.LIMIT_SETS)
FLT_MAX = 3.4028234663852886e38


def _cfg_limits(tcfg):
    """wbc_task_cfg.torque_limits of the 18 revolute joints, in the order of tau[:, 6:24]."""
    return np.array([tcfg.torque_limits[c - 6] for c in JOINTS], dtype=np.float64)


def _bits(x):
    return [i for i in range(64) if (int(x) >> i) & 1]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_abi_refusals_and_workspace_without_a_device():
    from wbc_amd.native import lib
    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    idx = (C.c_int32 * 4)(3, 7, 11, 15)
    w = abi.WbcTaskIdWeights(1e-2, 1e-4, 1e-3, 0.0)
    Q = lambda *a: C.byref(abi.WbcTaskQpLimits(*a))
    call = lambda lim, **kw: L.wbc_sim_task_inverse_dynamics_qp(None, idx, 4, None, None, idx, 2, p, None, None, C.byref(w), lim, kw.get("tau_limit"),
                                                                 kw.get("normal"), kw.get("mu"), 0, p, p, p, kw.get("status"), kw.get("set"),
                                                                 kw.get("iters"), p, None)
    assert call(Q(0.5, 0.0, 0)) == -1 and b"sim is NULL" in L.wbc_last_error()
    # the new entry point's own arguments are refused before the sim is looked at
    inf, nan = float("inf"), float("nan")
    for lim, kw, word in [(None, {}, b"limits is NULL"), (Q(0.0, 0.0, 0), {}, b"mu"), (Q(-1.0, 0.0, 0), {}, b"mu"), (Q(inf, 0.0, 0), {}, b"mu"),
                          (Q(nan, 0.0, 0), {}, b"mu"), (Q(0.5, inf, 0), {}, b"fn_min"), (Q(0.5, -inf, 0), {}, b"fn_min"), (Q(0.5, nan, 0), {}, b"fn_min"),
                          (Q(0.5, 0.0, -1), {}, b"max_iter"), (Q(0.5, 0.0, abi.TASKQP_MAX_ITER + 1), {}, b"max_iter"),
                          (Q(0.5, 0.0, 0), dict(tau_limit=p + 2), b"aligned"), (Q(0.5, 0.0, 0), dict(normal=p + 1), b"aligned"),
                          (Q(0.5, 0.0, 0), dict(mu=p + 3), b"aligned"), (Q(0.5, 0.0, 0), dict(status=p + 2), b"aligned"),
                          (Q(0.5, 0.0, 0), dict(iters=p + 1), b"aligned"), (Q(0.5, 0.0, 0), dict(set=p + 4), b"aligned")]:
        assert call(lim, **kw) == -1 and word in L.wbc_last_error(), (word, L.wbc_last_error())
    assert call(Q(0.5, -3.0, abi.TASKQP_MAX_ITER), tau_limit=p, normal=p, mu=p, status=p, set=p, iters=p) == -1 and b"sim is NULL" in L.wbc_last_error()
    assert C.sizeof(abi.WbcTaskQpLimits) == 12 and abi.TASKQP_MAX_ITER == 128
    ws, ws0 = L.wbc_sim_task_inverse_dynamics_qp_workspace_floats, L.wbc_sim_task_inverse_dynamics_workspace_floats
    assert ws(10, 4, 6) == 10 * (2 * 31 * 26 + 16 + 36 * 26 + 36) == ws0(10, 4, 6) and ws(10, 0, 0) == 10 * (2 * 19 * 26 + 16 + 36)
    assert ws(0, 4, 6) == 0 and ws(10, 5, 6) == 0 and ws(10, -1, 6) == 0 and ws(10, 4, 7) == 0 and ws(10, 4, -1) == 0


def test_new_kernel_codegen():
    """No scratch, no flat memory instructions, the launch's workgroup size, static LDS as stated and no more than 32 kB."""
    kernel = "wbc_taskqp_solve_kernel"
    assert arm_codegen.meta(kernel, "private_segment_fixed_size") == 0
    assert arm_codegen.meta(kernel, "max_flat_workgroup_size") == 64
    assert arm_codegen.meta(kernel, "group_segment_fixed_size") == LDS_BYTES <= LDS_CAP
    body = arm_codegen.body(kernel)
    assert "s_endpgm" in body and re.search(r"\bglobal_store_dword", body)
    assert not re.search(r"\bflat_", body) and "scratch_" not in body


@functools.lru_cache(maxsize=None)
def _cpu_model():
    from wbc_amd.config import WidowGo1RoughCfg
    m = abi.load_default_model()
    tcfg = abi.fill_task_cfg(WidowGo1RoughCfg(), m)
    return m, msr.armature_vector(tcfg), _cfg_limits(tcfg)


@functools.lru_cache(maxsize=None)
def _references():
    """The fp64 reference of the 180 problems: {set: [(P, rows, (tau, nudot, lam, bits, status, iterations, multipliers))]}."""
    m, A, lim0 = _cpu_model()
    out = {}
    for name, (mu, fn_min, scale) in tq.LIMIT_SETS.items():
        out[name] = []
        for seed in range(60):
            P, _, _ = tti._family(m, seed, A)
            out[name].append((P, tq.rows_of(P, scale * lim0, mu, fn_min), tq.reference(P, scale * lim0, mu, fn_min)))
    return out


def test_reference_satisfies_its_own_certificate_on_the_180_problems():
    """All feasible; 36-39 of each 60 members have an active row; the certificate holds at 1e-9 of its scales."""
    for name, members in _references().items():
        active, largest, iters = 0, 0, 0
        for seed, (P, rows, (tau, nudot, lam, bits, status, it, u)) in enumerate(members):
            assert status == 0, (name, seed)
            cert = tq.certificate(P, rows, tau, nudot, lam, bits)
            assert cert["box"] and cert["bits"], (name, seed)
            for k in ("feas", "stat", "set"):
                assert cert[k] * EPS <= 1e-9, (name, seed, k, cert[k] * EPS)
            for k, (r, s) in tir.tiers(P, tau, nudot, lam).items():
                assert k == "grad" or np.all(r <= 1e-9 * s), (name, seed, k)
            assert all(v >= -1e-9 for v in u.values())
            active, largest, iters = active + (bits != 0), max(largest, len(_bits(bits))), max(iters, it)
        print(f"{name}: {active} of 60 members with an active row, largest set {largest}, at most {iters} iterations")
        assert 36 <= active <= 39


def test_reference_where_nothing_binds_is_the_kkt_reference():
    m, A, lim0 = _cpu_model()
    checked, with_stance = 0, 0
    for seed in range(24):
        P, _, _ = tti._family(m, seed, A)
        tau, nudot, lam, bits, status, it, _ = tq.reference(P, 1e9 * np.ones(18), 1e6, -1e12)
        t0, n0, l0 = tir.kkt_reference(P)
        if P.on.any() and np.any(l0.reshape(-1, 3)[:, 2][P.on[::3]] < 0):
            continue                                                                # a pulling foot binds whatever mu is
        checked, with_stance = checked + 1, with_stance + bool(P.on.any())
        assert status == 0 and bits == 0 and it == 0
        for a, b in ((tau, t0), (nudot, n0), (lam, l0)):
            assert np.abs(a - b).max(initial=0.0) <= 1e-9 * max(1.0, np.abs(b).max(initial=0.0)), seed
    print(f"nothing binds: {checked} of 24 members compared, {with_stance} of them with stance bodies")
    assert checked >= 8 and with_stance >= 2


def test_pressing_feet_closed_form(robot):
    """A standing robot (nu = 0, level trunk) told to press every foot with fn_min = F above a quarter of its weight, with friction and
    torque limits out of the way and the force term making any force above F cost: all four normal rows are active, every normal
    force equals F, and Newton's law for the whole robot gives the centre of mass the acceleration (4 F - m g) / m: the first three
    rows of M nudot + h = sum lambda read (M nudot)[2] = 4 F - h[2] with h[2] = m g."""
    import inverse_dynamics_reference as idr
    import test_mass_solve as tms
    import whole_body_reference as wb
    m = robot["model"]
    feet, grip, trunk = tti._bodies(m)
    rng = np.random.default_rng(7)
    pos, quat, q, _ = tms._random_state(rng)
    q, quat, nu = 0.3 * q, np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(26)
    M = msr.mass_matrix(m, pos, quat, q)
    h, _ = idr.bias_forces(m, pos, quat, q, nu)
    J = wb.jacobian(m, pos, quat, q)
    jd, _ = cdr.body_accelerations(m, pos, quat, q, nu)
    P = tti._problem(M, h, J, jd, feet, np.ones(4, dtype=bool), None, [trunk], np.zeros((1, 6)), np.ones((1, 6)), None, (1e-2, 1e-2, 1e-3, 0.0))
    weight = h[2]
    assert abs(weight - 9.81 * sum(float(x) for x in m.mass)) <= 1e-3 * weight
    F = 0.5 * weight
    tau, nudot, lam, bits, status, _, u = tq.reference(P, 1e6 * np.ones(18), 1e3, F)
    assert status == 0 and {36, 41, 46, 51} <= set(_bits(bits)) and all(u[b] > 0 for b in (36, 41, 46, 51))
    assert np.abs(lam.reshape(4, 3)[:, 2] - F).max() <= 1e-9 * F
    assert abs((M @ nudot)[2] - (4 * F - weight)) <= 1e-9 * weight
    cert = tq.certificate(P, tq.rows_of(P, 1e6 * np.ones(18), 1e3, F), tau, nudot, lam, bits)
    assert max(cert["feas"], cert["stat"], cert["set"]) * EPS <= 1e-9


def test_tangent_rule():
    for normal in ([0.0, 0.0, 2.0], [0.3, -0.2, 0.9], [0.95, 0.1, 0.2], [-1.0, 0.0, 0.0]):
        n, t1, t2 = tq.tangents(normal)
        B = np.array([n, t1, t2])
        assert np.abs(B @ B.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(B) > 0
        e = np.array([0.0, 1.0, 0.0]) if abs(n[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
        assert abs(t1 @ e) <= 1e-12
    assert [list(v) for v in tq.tangents(None)] == [[0, 0, 1], [1, 0, 0], [0, 1, 0]]


@functools.lru_cache(maxsize=None)
def _yardsticks():
    """K_ref of the certificate's ratios over the 180 problems, the yardstick's statuses and the reported figures."""
    _, _, lim0 = _cpu_model()
    worst = {"feas": 0.0, "stat": 0.0, "set": 0.0}
    status, rep = {}, {"tau": 0.0, "excess": 0.0, "iterations": 0, "same_set": 0}
    for name, members in _references().items():
        mu, fn_min, scale = tq.LIMIT_SETS[name]
        status[name] = []
        for P, rows, ref in members:
            tau, nudot, lam, bits, st, it = tq.yardstick_f32(P, scale * lim0, mu, fn_min)
            status[name].append(st)
            rep["iterations"] = max(rep["iterations"], it)
            if st != 0:
                continue
            cert = tq.certificate(P, rows, tau, nudot, lam, bits)
            assert cert["box"] and cert["bits"]
            for k in worst:
                worst[k] = max(worst[k], cert[k])
            f64 = tir.objective(P, *ref[:3])
            rep["tau"] = max(rep["tau"], float(np.abs(tau - ref[0]).max() / np.abs(ref[0]).max()))
            rep["excess"] = max(rep["excess"], float((tir.objective(P, tau, nudot, lam) - f64) / f64))
            rep["same_set"] += bits == ref[3]
    return worst, status, rep


def test_fp32_yardstick_sits_well_inside_the_bounds():
    worst, status, rep = _yardsticks()
    print(f"yardstick: K_ref = {worst} against C_F = {tq.C_F}, C_S = {tq.C_S}; status 0 in "
          f"{ {k: v.count(0) for k, v in status.items()} } of 60; reported (never asserted): {rep}")
    k_f = max(worst["feas"], worst["set"])
    assert k_f <= tq.C_F / 16 and worst["stat"] <= tq.C_S / 16
    assert tq.C_F == 2.0 ** np.ceil(np.log2(16 * k_f)) <= 16384 and tq.C_S == 2.0 ** np.ceil(np.log2(16 * worst["stat"])) <= 32768
    assert status["nominal"].count(0) == 60 and status["loose"].count(0) == 60 and status["tight"].count(0) >= 54


# ------------------------------------------------------------------------------------------------------------ GPU
def _dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device="cuda").contiguous()


def _limits(env, n, name):
    """(mu, fn_min, tau_limit tensor or None, limits [n, 18] as doubles) of a limit set; scale 1 goes through the NULL pointer."""
    mu, fn_min, scale = tq.LIMIT_SETS[name]
    lim = np.tile(tti._f32(scale * _cfg_limits(env.tcfg)), (n, 1))
    return mu, fn_min, (None if scale == 1.0 else _dev(lim)), lim


def _call(env, args, mu, fn_min, tau_limit, **kw):
    """WbcSim.task_inverse_dynamics_qp with a case's arguments (tti._arguments): (tau, nudot, lam, info)."""
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    return env.sim.task_inverse_dynamics_qp(stance, tasks, _dev(acc), _dev(w), active=active, stance_acc=_dev(a_s), nudot_ref=_dev(ref),
                                            posture=weights[0], force=weights[1], torque=weights[2], damping=weights[3], armature=armature,
                                            mu=mu, fn_min=fn_min, tau_limit=tau_limit, **kw)


def _sibling(env, args):
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    return env.sim.task_inverse_dynamics(stance, tasks, _dev(acc), _dev(w), active=active, stance_acc=_dev(a_s), nudot_ref=_dev(ref),
                                         posture=weights[0], force=weights[1], torque=weights[2], damping=weights[3], armature=armature)


_WORST = {"root": 0.0, "joint": 0.0, "stance": 0.0, "feas": 0.0, "stat": 0.0, "set": 0.0, "tau": 0.0, "excess": 0.0, "iterations": 0,
          "largest_set": 0}


def _check(n, args, mu, fn_min, lim, tau, nudot, lam, info, unconstrained, normals=None):
    """Every env and row: the sibling's equality tiers and, for status 0, the certificate; the documented fallback otherwise. mu: a
    scalar or [n, K]; lim [n, 18]; unconstrained: the sibling's tau [n, 26] (torch). Returns the statuses."""
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    env, M, h, magh, _, J, jd, jmag = tti._case(n)
    if armature:
        M = M + np.diag(msr.armature_vector(env.tcfg))
    K, T = len(stance), len(tasks)
    t64, nd, lm = (x.double().cpu().numpy() for x in (tau, nudot, lam.reshape(n, 3 * K)))
    status, aset, iters = (info[k].cpu().numpy() for k in ("status", "active_set", "iterations"))
    assert np.isfinite(t64).all() and np.isfinite(nd).all() and np.isfinite(lm).all()
    assert np.all(t64[:, :6] == 0) and np.all(t64[:, FINGERS] == 0) and np.all(nd[:, FINGERS] == 0)
    assert np.all(np.abs(t64[:, JOINTS]) <= lim)                                   # the torque box, exactly, whatever the status
    act = np.ones((n, K), dtype=bool) if active is None else active.cpu().numpy().astype(bool)
    mu_all = np.broadcast_to(np.asarray(mu, dtype=np.float64), (n, K)) if K else np.zeros((n, 0))
    worst = {k: 0.0 for k in ("root", "joint", "stance", "feas", "stat", "set")}
    for e in range(n):
        P = tti._problem(M[e], h[e], J[e], jd[e], stance, act[e], None if a_s is None else np.nan_to_num(a_s[e]), tasks,
                         np.zeros((0, 6)) if T == 0 else np.nan_to_num(acc[e]), np.zeros((0, 6)) if T == 0 else w[e],
                         None if ref is None else ref[e], weights)
        assert np.all(lm[e][~P.on] == 0)
        magg = np.concatenate([jmag[e, r, 0:3] for r in stance])[P.on] if K else np.zeros(0)
        extra = {"root": tti.C_ID * EPS * magh[e][:6], "joint": tti.C_ID * EPS * magh[e][JOINTS], "stance": tti.C_A * EPS * magg}
        for k, (r, s) in tir.tiers(P, t64[e], nd[e], lm[e]).items():
            if k == "grad":
                continue
            bound = tti.C_TIER[k] * EPS * s + extra[k]
            assert np.all(r <= bound), (k, e, float((r / bound).max()))
            if len(r):
                worst[k] = max(worst[k], float((r / (EPS * s)).max()))
        assert status[e] in (0, 1, 2) and 0 <= iters[e] <= abi.TASKQP_MAX_ITER
        if status[e] != 0:
            want = torch.minimum(torch.maximum(unconstrained[e, JOINTS], _dev(-lim[e])), _dev(lim[e]))
            assert aset[e] == 0 and torch.equal(tau[e, JOINTS], want), e
            continue
        rows = tq.rows_of(P, lim[e], np.nan_to_num(mu_all[e], nan=1.0), fn_min, None if normals is None else np.nan_to_num(normals[e], nan=1.0))
        cert = tq.certificate(P, rows, t64[e], nd[e], lm[e], int(aset[e]))
        assert cert["box"] and cert["bits"], (e, _bits(aset[e]))
        assert cert["feas"] <= tq.C_F and cert["set"] <= tq.C_F and cert["stat"] <= tq.C_S, (e, cert, _bits(aset[e]), int(iters[e]))
        for k in ("feas", "stat", "set"):
            worst[k] = max(worst[k], cert[k])
        if normals is None:
            tq64 = tq.reference(P, lim[e], mu_all[e], fn_min)
            f64 = tir.objective(P, *tq64[:3])
            _WORST["tau"] = max(_WORST["tau"], float(np.abs(t64[e] - tq64[0]).max() / np.abs(tq64[0]).max()))
            _WORST["excess"] = max(_WORST["excess"], float((tir.objective(P, t64[e], nd[e], lm[e]) - f64) / f64))
        _WORST["iterations"] = max(_WORST["iterations"], int(iters[e]))
        _WORST["largest_set"] = max(_WORST["largest_set"], len(_bits(aset[e])))
    for k in worst:
        _WORST[k] = max(_WORST[k], worst[k])
    return status, worst


def _raw_call(env, args, mu, fn_min, tau_limit, want_nudot, want_lam):
    """The C-ABI call into sentinel-filled buffers; the tails and the outputs that are not asked for stay untouched."""
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    n, K, T = env.num_envs, len(stance), len(tasks)
    L, sim = env.sim.L, env.sim
    nws = int(L.wbc_sim_task_inverse_dynamics_qp_workspace_floats(n, K, T))
    tb, nb, lb, ws = (tti._sentinel_buffer(k) for k in (n * 26, n * 26, n * 3 * K, nws))
    st = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    it = torch.full((n + 8,), 77, dtype=torch.int32, device="cuda")
    aset = torch.full((n + 8,), 77, dtype=torch.int64, device="cuda")
    ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    keep = [_dev(a_s), _dev(acc), _dev(w), _dev(ref)]
    rc = L.wbc_sim_task_inverse_dynamics_qp(sim.h, (C.c_int32 * max(K, 1))(*stance), K, ptr(active), ptr(keep[0]), (C.c_int32 * max(T, 1))(*tasks), T,
                                            ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), C.byref(abi.WbcTaskIdWeights(*weights)),
                                            C.byref(abi.WbcTaskQpLimits(mu, fn_min, 0)), ptr(tau_limit), None, None, 1 if armature else 0,
                                            tb.data_ptr(), nb.data_ptr() if want_nudot else None, lb.data_ptr() if want_lam and K else None,
                                            st.data_ptr(), aset.data_ptr(), it.data_ptr(), ws.data_ptr(), None)
    assert rc == 0, L.wbc_last_error()
    torch.cuda.synchronize()
    for buf, used in ((tb, n * 26), (nb, n * 26 if want_nudot else 0), (lb, n * 3 * K if want_lam else 0), (ws, nws)):
        assert bool((buf[used:] == SENTINEL).all())
    for buf in (st, it, aset):
        assert bool((buf[n:] == 77).all())
    return (tb[:n * 26].view(n, 26), nb[:n * 26].view(n, 26) if want_nudot else None, lb[:n * 3 * K].view(n, K, 3) if want_lam else None,
            {"status": st[:n], "active_set": aset[:n], "iterations": it[:n]})


@pytest.mark.gpu
@pytest.mark.parametrize("limits", SETS)
@pytest.mark.parametrize("case", tti.CASES)
@pytest.mark.parametrize("n", [1, 13, 64])
def test_every_env_and_row(n, case, limits):
    env = tti._case(n)[0]
    args = tti._arguments(env, n, case)
    mu, fn_min, tau_limit, lim = _limits(env, n, limits)
    tau, nudot, lam, info = _raw_call(env, args, mu, fn_min, tau_limit, case not in ("nudot_null", "both_null"), case not in ("lambda_null", "both_null"))
    t2, n2, l2, i2 = _call(env, args, mu, fn_min, tau_limit)                      # the Python entry point is the same call
    unconstrained = _sibling(env, args)[0]
    torch.cuda.synchronize()
    assert l2.shape == (n, len(args[0]), 3) and torch.equal(t2, tau) and all(torch.equal(info[k], i2[k]) for k in info)
    assert (nudot is None or torch.equal(n2, nudot)) and (lam is None or torch.equal(l2, lam))
    status, worst = _check(n, args, mu, fn_min, lim, t2, n2, l2, i2, unconstrained)
    print(f"task QP n={n} {case} {limits}: status 0 in {int((status == 0).sum())} of {n}, envs with an active row "
          f"{int((i2['active_set'] != 0).sum())}, iterations up to {int(i2['iterations'].max())}; largest ratios {worst}; running maxima {_WORST}")
    if limits == "tight":
        assert (status == 0).mean() >= 0.9, status
    else:
        assert np.all(status == 0), status
    if case == "masks16" and limits == "nominal":
        # WidowGo1.whole_body_controller is the same call with the feet's weights taken from the stance mask
        stance, active, a_s, tasks, acc, w, ref, weights, armature = args
        wts = dict(posture=weights[0], force=weights[1], torque=weights[2], damping=weights[3])
        w_env = torch.zeros(n, 6, 6, device="cuda")
        w_env[:, :2] = 1.0
        w_env[:, 2:, :3] = (~active.bool()).float().unsqueeze(-1)
        clean = torch.nan_to_num(_dev(acc), nan=0.0)
        t3, n3, l3, i3 = env.sim.task_inverse_dynamics_qp(stance, tasks, clean, w_env, active=active.bool(), mu=mu, fn_min=fn_min, **wts)
        tq_, nq, lq, iq = env.whole_body_controller(clean[:, 0], clean[:, 1], clean[:, 2:, :3].contiguous(), stance=active.bool(), weights=wts,
                                                    mu=mu, fn_min=fn_min)
        assert tq_.shape == (n, 20) and torch.equal(tq_, t3[:, 6:]) and torch.equal(nq, n3) and torch.equal(lq, l3)
        assert all(torch.equal(i3[k], iq[k]) for k in i3)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13, 64])
def test_tilted_normals_and_per_body_friction(n):
    """normal and mu as tensors: tilted, unnormalised normals (some with |n_x| > 0.9: the other tangent rule) and a friction
    coefficient per env and body, NaN where the body is inactive."""
    env = tti._case(n)[0]
    args = tti._arguments(env, n, "masks16")
    on = args[1].cpu().numpy().astype(bool)
    rng = np.random.default_rng(1300 + n)
    normals = tti._f32(np.concatenate([rng.uniform(-0.4, 0.4, (n, 4, 2)), rng.uniform(0.8, 2.0, (n, 4, 1))], axis=2))
    normals[::5, 0] = tti._f32([0.95, 0.1, 0.25])
    mus = tti._f32(rng.uniform(0.3, 1.0, (n, 4)))
    normals[~on], mus[~on] = np.nan, np.nan
    _, fn_min, tau_limit, lim = _limits(env, n, "nominal")
    tau, nudot, lam, info = _call(env, args, _dev(mus), fn_min, tau_limit, normal=_dev(normals))
    unconstrained = _sibling(env, args)[0]
    torch.cuda.synchronize()
    status, worst = _check(n, args, mus, fn_min, lim, tau, nudot, lam, info, unconstrained, normals=normals)
    print(f"task QP n={n} tilted normals: status {np.bincount(status, minlength=3)}, largest ratios {worst}")
    assert (status == 0).mean() >= 0.9 and bool((info["active_set"] != 0).any())


def _never(env, args, **kw):
    return _call(env, args, 1e6, -FLT_MAX, torch.full((env.num_envs, 18), FLT_MAX, device="cuda"), **kw)


@functools.lru_cache(maxsize=None)
def _resting_env(n):
    """n robots standing in the reset pose with every velocity set to zero (randomised body parameters): their feet carry them."""
    import test_inverse_dynamics as tid
    env = tid._env(n, seed=11, steps=0)
    root, dof = env.sim.tensor("ROOT_STATES").clone(), env.sim.tensor("DOF_STATE").clone()
    root[..., 7:13] = 0.0
    dof[..., 1] = 0.0
    env.sim.set_root_state(root.contiguous()); env.sim.set_dof_state(dof.contiguous())
    torch.cuda.synchronize()
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["airborne", "resting", "resting_armature"])
@pytest.mark.parametrize("n", [1, 13, 64])
def test_limits_that_never_bind_give_the_siblings_bits(n, case):
    """tau_limit = FLT_MAX, fn_min = -FLT_MAX, mu = 1e6: tau, nudot and lambda of wbc_sim_task_inverse_dynamics bit for bit, status 0,
    set 0, iterations 0, for every env whose unconstrained foot forces lie inside that pyramid. A foot that PULLS violates
    |t . lam| <= mu n . lam whatever mu is, and on the other GPU cases' rollout states (joint speeds of 20-30 rad/s) most envs have
    one. The stance cases therefore use robots at rest on four feet, asked for gentle trunk and gripper accelerations: their feet
    push (at least three quarters of the envs are required to; the count is printed), and those envs are compared."""
    feet_on = case != "airborne"
    env = _resting_env(n) if feet_on else tti._case(n)[0]
    stance, active, a_s, tasks, acc, w, ref, weights, armature = tti._arguments(env, n, "armature" if case == "resting_armature" else "airborne")
    if feet_on:
        feet, grip, trunk = tti._bodies(env.robot_model)
        stance, tasks = feet, [trunk, grip] + feet
        acc, w = tti._f32(np.random.default_rng(1400 + n).uniform(-0.5, 0.5, (n, 6, 6))), np.zeros((n, 6, 6))
        w[:, :2] = 1.0
    args = (stance, active, a_s, tasks, acc, w, ref, weights, armature)
    want = _sibling(env, args)
    got = _never(env, args)
    torch.cuda.synchronize()
    lz = want[2].double().cpu().numpy()
    push = torch.tensor(np.all(1e6 * lz[:, :, 2] >= np.abs(lz[:, :, :2]).max(axis=2), axis=1), device="cuda")   # [n]; all True without stance bodies
    print(f"never-binding limits n={n} {case}: {int(push.sum())} of {n} envs inside the pyramid at the unconstrained optimum")
    assert int(push.sum()) >= max(1, (3 * n) // 4)
    for x, y in zip(got[:3], want):
        assert bool(y.abs().sum() > 0 or y.numel() == 0) and torch.equal(x[push], y[push])
    for k in ("status", "active_set", "iterations"):
        assert bool((got[3][k][push] == 0).all()), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["airborne", "masks16"])
def test_the_torque_box_holds_exactly_for_the_smallest_excess(case):
    """Per-env limits just below the unconstrained |tau_j|: lim = |tau_j| (1 - 1e-5) in the odd envs and the next float32 below |tau_j|
    in the even ones, an excess far inside the 256 x 2^-24 of a row's scale that a contact row is allowed. A box row has no such
    allowance: every returned torque is inside its limit exactly, whatever the status, and every env is worked on (steps taken), not
    passed through. The odd envs must be solved (status 0) and sit on the reported limits bit for bit. In the even envs all 18 rows are
    active with multipliers of one unit in the last place of tau_j, below what fp32 resolves: no active set is decidable there, so
    status 1 is accepted too, with the documented fallback -- the unconstrained optimum clamped, which is within that unit of the optimum."""
    n = 13
    env = tti._case(n)[0]
    args = tti._arguments(env, n, case)
    unc = _sibling(env, args)[0]
    torch.cuda.synchronize()
    mag = unc[:, JOINTS].abs()
    lim = mag * (1.0 - 1e-5)
    lim[::2] = torch.nextafter(mag[::2], torch.zeros_like(mag[::2]))
    lim = torch.clamp(lim, min=1e-6).contiguous()
    assert bool((mag > lim).float().mean() > 0.9)
    tau, nudot, lam, info = _call(env, args, 1e6, -FLT_MAX, lim)
    torch.cuda.synchronize()
    assert bool((tau[:, JOINTS].abs() <= lim).all())
    status = info["status"].cpu().numpy()
    print(f"smallest excess {case}: statuses {status.tolist()}, iterations {info['iterations'].cpu().tolist()}")
    assert bool((info["iterations"] > 0).all()) and np.all(status[1::2] == 0) and np.all(status[::2] <= 1)
    capped = info["status"] == 1
    assert torch.equal(tau[:, JOINTS][capped], torch.minimum(torch.maximum(unc[:, JOINTS], -lim), lim)[capped])
    assert bool((info["active_set"][capped] == 0).all())
    at = (info["active_set"][:, None] >> torch.arange(36, device="cuda")[None]) & 1
    hit = (at[:, :18] | at[:, 18:]).bool()
    assert bool(hit[1::2].any(dim=1).all()) and torch.equal(tau[:, JOINTS].abs()[hit], lim[hit])


@pytest.mark.gpu
def test_permuting_the_envs_permutes_every_output_bit_for_bit():
    import test_inverse_dynamics as tid
    n = 13
    env = tid._env(n, seed=9, steps=12)
    args = tti._arguments(env, n, "masks16")
    mu, fn_min, tau_limit, _ = _limits(env, n, "tight")
    first = _call(env, args, mu, fn_min, tau_limit)
    torch.cuda.synchronize()
    perm = np.random.default_rng(5).permutation(n)
    pt = _dev(perm, torch.int64)
    for name in ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS"):
        t = env.sim.tensor(name)
        t.copy_(t[pt].clone())
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    args2 = (stance, active[pt].contiguous(), a_s[perm], tasks, acc[perm], w[perm], ref[perm], weights, armature)
    second = _call(env, args2, mu, fn_min, tau_limit)
    torch.cuda.synchronize()
    assert bool((first[3]["active_set"] != 0).any())
    for x, y in zip(first[:3] + tuple(first[3].values()), second[:3] + tuple(second[3].values())):
        assert torch.equal(x[pt], y)


@pytest.mark.gpu
def test_an_infeasible_env_falls_back_and_leaves_its_neighbours_alone():
    """fn_min is a host scalar, so the env that cannot be satisfied is singled out by the stance mask and its torque limits: under
    fn_min = 1e4 env 5 stands on four feet with limits of 1 N m (no torque within them presses a foot with 1e4 N) while its
    neighbours are airborne and have no contact rows. Env 5 has status 2 and the fallback; its neighbours are bit-identical to a run
    in which env 5 is airborne as well and has ordinary limits. A second pair of runs, with every env on its masks16 feet under the
    nominal set, shows the same for env 5's torque limits alone."""
    n = 13
    env = tti._case(n)[0]
    stance, active, a_s, tasks, acc, w, ref, weights, armature = tti._arguments(env, n, "masks16")
    mu, fn_min, _, lim = _limits(env, n, "nominal")
    lim5 = lim.copy()
    lim5[5] = 1.0
    others = [e for e in range(n) if e != 5]
    only5 = torch.zeros_like(active)
    only5[5] = 1
    hard = _call(env, (stance, only5, np.zeros_like(a_s), tasks, acc, w, ref, weights, armature), mu, 1e4, _dev(lim5))
    without = _call(env, (stance, torch.zeros_like(active), np.zeros_like(a_s), tasks, acc, w, ref, weights, armature), mu, 1e4, _dev(lim))
    unconstrained = _sibling(env, (stance, only5, np.zeros_like(a_s), tasks, acc, w, ref, weights, armature))[0]
    nd, lam = env.sim.constrained_dynamics(stance, tau=hard[0].contiguous(), active=only5, damping=weights[3])
    torch.cuda.synchronize()
    assert int(hard[3]["status"][5]) == 2 and int(hard[3]["active_set"][5]) == 0 and bool((hard[3]["status"][others] == 0).all())
    assert torch.equal(hard[0][5, JOINTS], torch.clamp(unconstrained[5, JOINTS], -1.0, 1.0))
    scale = float(hard[2][5].abs().max())
    assert float((nd[5] - hard[1][5]).abs().max()) <= 1e-3 * float(nd[5].abs().max()) and float((lam[5] - hard[2][5]).abs().max()) <= 1e-3 * scale
    for x, y in zip(hard[:3] + tuple(hard[3].values()), without[:3] + tuple(without[3].values())):
        assert torch.equal(x[others], y[others])
    args = (stance, active, a_s, tasks, acc, w, ref, weights, armature)
    soft, base = _call(env, args, mu, fn_min, _dev(lim5)), _call(env, args, mu, fn_min, _dev(lim))
    torch.cuda.synchronize()
    assert not torch.equal(soft[0][5], base[0][5])
    for x, y in zip(soft[:3] + tuple(soft[3].values()), base[:3] + tuple(base[3].values())):
        assert torch.equal(x[others], y[others])


@pytest.mark.gpu
def test_nan_where_nothing_is_read_leaves_every_output_bit_identical():
    n = 64
    env = tti._case(n)[0]
    args = tti._arguments(env, n, "masks16")
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    on = active.cpu().numpy().astype(bool)
    assert np.isnan(a_s).any() and np.isnan(acc).any() and not on.all()
    rng = np.random.default_rng(3)
    normals, mus = tti._f32(rng.uniform(0.5, 1.0, (n, 4, 3))), tti._f32(rng.uniform(0.4, 0.9, (n, 4)))
    mu, fn_min, tau_limit, _ = _limits(env, n, "nominal")
    clean_args = (stance, active, np.nan_to_num(a_s, nan=-7.0), tasks, np.nan_to_num(acc, nan=3.0), w, ref, weights, armature)
    clean = _call(env, clean_args, _dev(mus), fn_min, tau_limit, normal=_dev(normals))
    normals[~on], mus[~on] = np.nan, np.nan
    dirty = _call(env, args, _dev(mus), fn_min, tau_limit, normal=_dev(normals))
    torch.cuda.synchronize()
    for x, y in zip(dirty[:3] + tuple(dirty[3].values()), clean[:3] + tuple(clean[3].values())):
        assert bool(torch.isfinite(x.float()).all()) and torch.equal(x, y)
    assert bool((dirty[3]["active_set"] != 0).any())


@pytest.mark.gpu
def test_translation_invariance_is_bit_exact(robot):
    import test_inverse_dynamics as tid
    n = 64
    feet, grip, trunk = tti._bodies(robot["model"])
    rng = np.random.default_rng(1201)
    acc, w = tti._task_arrays(rng, (n,), tti._masks(n, 4).cpu().numpy().astype(bool))
    outs = []
    for shift in ((0.0, 0.0, 0.0), (3.0, 110.0, 0.0)):
        env, _ = tid._airborne_env(robot, n, shift)
        out = env.sim.task_inverse_dynamics_qp(feet, [trunk, grip] + feet, _dev(acc), _dev(w), active=tti._masks(n, 4), damping=1e-3, mu=0.4, fn_min=5.0,
                                               tau_limit=_dev(0.5 * np.tile(_cfg_limits(env.tcfg), (n, 1))))
        torch.cuda.synchronize()
        outs.append([x.clone() for x in out[:3] + tuple(out[3].values())])
    assert bool((outs[0][4] != 0).any())
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_graph_capture_replays_the_same_bits():
    n = 13
    env = tti._case(n)[0]
    args = tti._arguments(env, n, "masks16")
    mu, fn_min, tau_limit, _ = _limits(env, n, "tight")
    first = _call(env, args, mu, fn_min, tau_limit)
    want = [x.clone() for x in first[:3] + tuple(first[3].values())]
    outs = tuple(torch.zeros_like(x) for x in want)
    stance, active, a_s, tasks, acc, w, ref, weights, armature = args
    d = [_dev(acc), _dev(w), _dev(a_s), _dev(ref)]
    run = lambda: env.sim.task_inverse_dynamics_qp(stance, tasks, d[0], d[1], active=active, stance_acc=d[2], nudot_ref=d[3], posture=weights[0],
                                                   force=weights[1], torque=weights[2], damping=weights[3], mu=mu, fn_min=fn_min,
                                                   tau_limit=tau_limit, out=outs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for x in outs:
        x.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    torch.cuda.synchronize()
    assert bool((want[4] != 0).any())
    for x, y in zip(outs, want):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_every_refusal_leaves_the_outputs_untouched():
    n = 13
    env = tti._case(n)[0]
    feet, grip, trunk = tti._bodies(env.robot_model)
    L, h = env.sim.L, env.sim.h
    tb, nb, lb = (tti._sentinel_buffer(k) for k in (n * 26, n * 26, n * 12))
    ws = tti._sentinel_buffer(int(L.wbc_sim_task_inverse_dynamics_qp_workspace_floats(n, 4, 6)))
    st, it = (torch.full((n + 2,), 77, dtype=torch.int32, device="cuda") for _ in range(2))
    aset = torch.full((n + 2,), 77, dtype=torch.int64, device="cuda")
    acc = torch.ones(n, 6, 6, device="cuda")
    lims = torch.full((n, 18), 20.0, device="cuda")
    sidx, tidx = (C.c_int32 * 4)(*feet), (C.c_int32 * 6)(trunk, grip, *feet)
    good, lim = abi.WbcTaskIdWeights(1e-2, 1e-4, 1e-3, 0.0), abi.WbcTaskQpLimits(0.6, 2.0, 0)
    W = lambda *a: C.byref(abi.WbcTaskIdWeights(*a))
    Q = lambda *a: C.byref(abi.WbcTaskQpLimits(*a))
    call = lambda **kw: L.wbc_sim_task_inverse_dynamics_qp(*[kw.get(k, d) for k, d in (
        ("sim", h), ("srb", sidx), ("ns", 4), ("active", None), ("a_s", None), ("trb", tidx), ("nt", 6), ("acc", acc.data_ptr()), ("w", None),
        ("ref", None), ("weights", C.byref(good)), ("limits", C.byref(lim)), ("tau_limit", lims.data_ptr()), ("normal", None), ("mu", None),
        ("flags", 0), ("tau", tb.data_ptr()), ("nudot", nb.data_ptr()), ("lam", lb.data_ptr()), ("status", st.data_ptr()),
        ("set", aset.data_ptr()), ("iters", it.data_ptr()), ("ws", ws.data_ptr()), ("stream", None))])
    inf, nan = float("inf"), float("nan")
    refusals = [
        (dict(sim=None), b"NULL"), (dict(tau=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(weights=None), b"NULL"), (dict(acc=None), b"NULL"),
        (dict(srb=None), b"NULL"), (dict(trb=None), b"NULL"), (dict(limits=None), b"limits is NULL"),
        (dict(ns=-1), b"nstance"), (dict(ns=5), b"nstance"), (dict(nt=-1), b"ntasks"), (dict(nt=7), b"ntasks"),
        (dict(srb=(C.c_int32 * 4)(feet[0], feet[1], 27, feet[3])), b"index"), (dict(trb=(C.c_int32 * 6)(trunk, -1, *feet)), b"index"),
        (dict(srb=(C.c_int32 * 4)(feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(trb=(C.c_int32 * 6)(trunk, grip, feet[0], feet[1], feet[0], feet[3])), b"same moving body"),
        (dict(weights=W(1e-2, 1e-4, 0.0, 0.0)), b"torque"), (dict(weights=W(1e-2, 1e-4, nan, 0.0)), b"torque"),
        (dict(weights=W(-1e-2, 1e-4, 1e-3, 0.0)), b"posture"), (dict(weights=W(1e-2, inf, 1e-3, 0.0)), b"force"),
        (dict(weights=W(1e-2, 1e-4, 1e-3, -1e-3)), b"damping"),
        (dict(limits=Q(0.0, 2.0, 0)), b"mu"), (dict(limits=Q(-0.5, 2.0, 0)), b"mu"), (dict(limits=Q(inf, 2.0, 0)), b"mu"), (dict(limits=Q(nan, 2.0, 0)), b"mu"),
        (dict(limits=Q(0.6, inf, 0)), b"fn_min"), (dict(limits=Q(0.6, -inf, 0)), b"fn_min"), (dict(limits=Q(0.6, nan, 0)), b"fn_min"),
        (dict(limits=Q(0.6, 2.0, -1)), b"max_iter"), (dict(limits=Q(0.6, 2.0, abi.TASKQP_MAX_ITER + 1)), b"max_iter"),
        (dict(flags=2), b"flag"), (dict(flags=4), b"flag"),
        (dict(a_s=acc.data_ptr() + 2), b"aligned"), (dict(acc=acc.data_ptr() + 1), b"aligned"), (dict(tau=tb.data_ptr() + 2), b"aligned"),
        (dict(lam=lb.data_ptr() + 3), b"aligned"), (dict(ws=ws.data_ptr() + 2), b"aligned"),
        (dict(tau_limit=lims.data_ptr() + 2), b"aligned"), (dict(normal=acc.data_ptr() + 1), b"aligned"), (dict(mu=acc.data_ptr() + 3), b"aligned"),
        (dict(status=st.data_ptr() + 2), b"aligned"), (dict(iters=it.data_ptr() + 1), b"aligned"), (dict(set=aset.data_ptr() + 4), b"aligned"),
    ]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        assert word in L.wbc_last_error(), (kw, L.wbc_last_error())
    torch.cuda.synchronize()
    for t in (tb, nb, lb, ws):
        assert bool((t == SENTINEL).all())
    for t in (st, it, aset):
        assert bool((t == 77).all())
    # max_iter at its cap and NULL status / set / iterations are fine; max_iter = 1 stops a binding env at the cap with the fallback
    assert call(limits=Q(0.6, 2.0, abi.TASKQP_MAX_ITER), status=None, set=None, iters=None) == 0, L.wbc_last_error()
    want = env.sim.task_inverse_dynamics_qp(feet, [trunk, grip] + feet, acc, posture=1e-2, force=1e-4, torque=1e-3, mu=0.6, fn_min=2.0, tau_limit=lims)
    torch.cuda.synchronize()
    assert torch.equal(tb[:n * 26].view(n, 26), want[0]) and bool((st == 77).all())
    one = env.sim.task_inverse_dynamics_qp(feet, [trunk, grip] + feet, acc, posture=1e-2, force=1e-4, torque=1e-3, mu=0.6, fn_min=2.0, tau_limit=lims,
                                           max_iter=1)
    torch.cuda.synchronize()
    multi = want[3]["iterations"] > 1
    assert bool(multi.any()) and bool((one[3]["status"][multi] == 1).all()) and bool((one[3]["active_set"][multi] == 0).all())
    assert bool((one[3]["iterations"][multi] == 1).all())


@pytest.mark.gpu
def test_step_is_untouched_by_the_new_call():
    import test_inverse_dynamics as tid
    n = 64
    finals = []
    for use in (False, True):
        env = tid._env(n, seed=6, steps=0)
        g = torch.Generator(device="cuda"); g.manual_seed(31)
        a = torch.ones(n, 6, device="cuda")
        for _ in range(5):
            if use:
                env.whole_body_controller(base_acc=a, ee_acc=a, stance=env.get_foot_contacts())
            env.step(torch.randn(n, 18, device="cuda", generator=g) * 0.8)
            if use:
                env.whole_body_controller(base_acc=a, swing_acc=torch.ones(n, 4, 3, device="cuda"), stance=env.get_foot_contacts(), armature=True,
                                          weights=dict(damping=1e-3), mu=0.4, fn_min=5.0)
        torch.cuda.synchronize()
        finals.append([env.sim.tensor(k).clone() for k in ("ROOT_STATES", "DOF_STATE", "OBS_BUF")])
    for x, y in zip(*finals):
        assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13, 64])
def test_returned_torques_through_constrained_dynamics(n):
    """wbc_sim_constrained_dynamics with the returned tau and the same stance, mask, stance accelerations and damping: its (nudot,
    lambda) satisfy the dynamics and stance rows within THAT call's own bounds (tests/test_constrained_dynamics.py), the scales
    taken at the new call's outputs, as the sibling's test of the same name."""
    env, M, h, magh, _, J, jd, jmag = tti._case(n)
    stance, active, a_s, tasks, acc, w, ref, _, armature = tti._arguments(env, n, "masks16")
    weights = tti._weights(4)                                                     # damping > 0, w_force = 0
    clean_as = np.nan_to_num(a_s)
    mu, fn_min, tau_limit, _ = _limits(env, n, "tight")
    tau, nudot, lam, info = _call(env, (stance, active, clean_as, tasks, acc, w, ref, weights, armature), mu, fn_min, tau_limit)
    nd2, lam2 = env.sim.constrained_dynamics(stance, tau=tau, active=active, acc_des=_dev(clean_as), damping=weights[3])
    torch.cuda.synchronize()
    assert bool((info["active_set"] != 0).any())
    t64, a1, l1, a2, l2 = (x.double().cpu().numpy().reshape(n, -1) for x in (tau, nudot, lam, nd2, lam2))
    act = active.cpu().numpy().astype(bool)
    own = []
    for e in range(n):
        P = tti._problem(M[e], h[e], J[e], jd[e], stance, act[e], clean_as[e], [], np.zeros((0, 6)), np.zeros((0, 6)), None, weights)
        magg = np.concatenate([jmag[e, r, 0:3] for r in stance]) * P.on
        assert np.all(l2[e][~P.on] == 0) and np.all(l1[e][~P.on] == 0)
        _, s1 = cdr.dynamics_residual_and_scale(P.M, P.h, t64[e], P.Jc, a1[e], l1[e])
        r2, _ = cdr.dynamics_residual_and_scale(P.M, P.h, t64[e], P.Jc, a2[e], l2[e])
        bound = cdr.C_S * EPS * s1 + tti.C_ID * EPS * magh[e]
        own.append(("dynamics", e, float((r2[tir.LIVE] / bound[tir.LIVE]).max())))
        if P.on.any():
            _, s1 = cdr.constraint_residual_and_scale(P.M, P.Jc, P.gamma, P.a_stance, P.damping, a1[e], l1[e])
            r2, _ = cdr.constraint_residual_and_scale(P.M, P.Jc, P.gamma, P.a_stance, P.damping, a2[e], l2[e])
            bound = cdr.C_K * EPS * s1 + tti.C_A * EPS * magg
            own.append(("stance", e, float((r2[P.on] / bound[P.on]).max())))
    worst = max(own, key=lambda x: x[2])
    print(f"returned torques through wbc_sim_constrained_dynamics n={n}: largest residual / its own bound = {worst}")
    assert worst[2] <= 1.0, worst
