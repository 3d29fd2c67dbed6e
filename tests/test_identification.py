"""Recursive identification of inertial parameters (wbc_sim_identification_accumulate, wbc_sim_identification_solve,
csrc/wbc_arm_kernel.hip; definitions in include/wbc_sim.h). The CPU tests pin the fp64 restatement tests/identification_reference.py to
the least squares of tests/test_inverse_dynamics_regressor.py (_identify), to weighted and ridge least squares and to a payload that
changes; the GPU tests hold the two kernels to that restatement element-wise, to the existing kernels, to their own invariances, the
solve in residual form, and the whole chain to the parameters a randomisation put into the sim.

Element-wise bound of the accumulate kernel: |kernel - ref| <= C * 2^-24 * mag, mag the restatement's magnitude arrays (next to every
entry the sum of the absolute values of its terms), entries of magnitude 0 exactly 0. The constants follow the convention of
tests/test_inverse_dynamics_regressor.py: 4 x the larger of the fp32 yardstick's largest ratio K_ref (numpy float32, the same chain, on
the CPU, on the GPU tests' own cases) and the kernel's largest ratio measured on an MI355X, rounded up to a power of two. Cases: n = 1,
13, 64 envs x the body lists [gb], [0, gb], [gb, 3, 0], after a RESET call and after a second call with forget 0.9 and random weights.

                     K_ref (CPU, numpy float32)   kernel (MI355X; n = 1, 13, 64)   4 x the larger, rounded up
    target z         1.71                         1.40, 2.03, 2.36                 C_T = 16
    A                4.05                         0.73, 1.49, 3.55                 C_A = 32
    b                0.462                        0.61, 0.71, 0.80                 C_B = 4
    stat             0.74                         0.66, 1.46, 1.42                 C_STAT = 8
    solve residual   0.885                        0.74, 1.01, 1.48                 C_X = 8   (|M pi - rhs| / (2^-24 row scale), msr.row_scale's pattern)
    cov_diag         0.427                        0.45, 0.86, 1.09                 C_X       (the unit right-hand side's row scale carried through |M^-1|)
The largest ratio of A sits in the three-body list at n = 64; no list or call stands out otherwise.

theta_hat is held to the fp64 map of the kernel's own pi_hat within C_TH 2^-24 (|Ibar| + m |shift|): c = h / m is two roundings, every
product of the shift three more and the subtraction one, so C_TH = 8 holds whatever the data (measured: 1.85, 2.38, 3.47). sse is held
to fp64 on the kernel's own bits within C_SSE 2^-24 of the sum of the absolute values of its terms: the rows' sums of P products and the
sum of the P rows are at most 2 P + 4 = 64 roundings deep (measured: 0.76, 0.99, 2.05)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import arm_codegen
import constrained_dynamics_reference as cdr
import identification_reference as ir
import inverse_dynamics_reference as idr
import mass_solve_reference as msr
import regressor_reference as rr
import whole_body_reference as wb
from test_inverse_dynamics import C_ID, _env
from test_inverse_dynamics_regressor import (C_Y, EPS, FINGERS, LIVE, MODEL, NB, NCOL, NP, PARENT_CODEGEN, SENTINEL, _case, _gpu_env,
                                             _gripper, _identification_states, _identify, _ratio, _set_states, _waves)
from wbc_amd import abi
from wbc_amd.abi import IDENT_MAX_BODIES, IDENT_RESET, linear_body_params          # new with the identification: every test here needs them

C_T = 16.0
C_A = 32.0
C_B = 4.0
C_STAT = 8.0
C_X = 8.0
C_TH = 8.0
C_SSE = 64.0
assert max(C_T, C_A, C_B, C_STAT, C_X) <= 4096
FORGET2 = 0.9
GROUPS = (slice(0, 1), slice(1, 4), slice(4, 10))
RANDOMISATION = (1.7, (0.04, -0.07, 0.02), 0.08)              # base_dmass, base_dcom, gripper_dmass of the recovery tests


def _lists():
    gb = MODEL().gripper_piece["body"]
    return ([gb], [0, gb], [gb, 3, 0])


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ shared cases
@functools.lru_cache(maxsize=None)
def _inputs(n):
    """What the two accumulate calls of the element-wise cases take besides the state of _case(n), rounded to fp32: tau_gen of both,
    the second call's nudot and row weights (a fifth of them 0; env 3 sees nothing in the second call)."""
    rng = np.random.default_rng(7000 + n)
    w2 = rng.uniform(0.0, 2.0, (n, NCOL))
    w2[rng.uniform(size=(n, NCOL)) < 0.2] = 0.0
    if n > 3:
        w2[3] = 0.0
    return {"tau1": _f32(msr.force_rhs(rng, (n,))), "tau2": _f32(msr.force_rhs(rng, (n,))), "nudot2": _f32(-0.5 * _case(n)["nudot"]), "w2": _f32(w2)}


@functools.lru_cache(maxsize=None)
def _regressors(n, call, dtype):
    """[(Y, mag)] of every env of _case(n) at the nudot of call 0 / 1."""
    c, m = _case(n), MODEL()
    nd = c["nudot"] if call == 0 else _inputs(n)["nudot2"]
    return [rr.regressor(m, c["quat"][e], c["q"][e], c["nu"][e], nd[e], c["gravity"], dtype) for e in range(n)]


def _reference(n, bodies, bp, dtype=np.float64):
    """The restatement on the element-wise cases: a list over the two calls of dicts of [n, ...] arrays (z, zmag, A, Amag, b, bmag, stat,
    statmag) at body_params bp [n, 20]."""
    m, inp = MODEL(), _inputs(n)
    calls = [[], []]
    for e in range(n):
        acc = None
        for call in (0, 1):
            Y, mag = _regressors(n, call, dtype)[e]
            Phi, Phimag, z, zmag = ir.split(m, Y, mag, bp[e], bodies, inp["tau1" if call == 0 else "tau2"][e])
            acc = ir.accumulate(m, acc, Phi, Phimag, z, zmag, None if call == 0 else inp["w2"][e], 1.0 if call == 0 else FORGET2)
            calls[call].append(dict(acc, z=z, zmag=zmag))
    return [{k: np.array([d[k] for d in per]).astype(np.float64) for k in per[0]} for per in calls]


def _ratios(got, ref):
    """{name: ratio} of one call's (z, A, b, stat) against the restatement's dict."""
    return {k: _ratio(np.asarray(got[k], dtype=np.float64), ref[k], ref[k + "mag"]) for k in ("z", "A", "b", "stat")}


def _solve_scale(M, x, rhs):
    """msr.row_scale's pattern for a P x P system: d_k sum_j d_j |x_j| + |rhs_k|, d = sqrt(diag M)."""
    d = np.sqrt(np.diag(M))
    return d * (np.abs(x) @ d) + np.abs(rhs)


def _solve_ratios(A, b, lam, p0, pi, cov):
    """(residual ratio, cov_diag ratio) of one env's solve: |M pi - rhs| / (2^-24 row scale), and |cov - diag(M^-1)| over the same kind
    of scale: the unit right-hand side's row scale in the equilibrated system (sum_j |x_j| + e_i), carried through |M^-1|."""
    A, b, lam, p0, pi, cov = (np.asarray(x, dtype=np.float64) for x in (A, b, lam, p0, pi, cov))
    M, rhs = A + np.diag(lam), b + lam * p0
    res = float((np.abs(M @ pi - rhs) / (EPS * _solve_scale(M, pi, rhs))).max())
    s = 1 / np.sqrt(np.diag(M))
    Xi = np.linalg.inv(s[:, None] * M * s[None, :])
    scale = np.abs(Xi).sum(axis=0)[None, :] + np.eye(len(b))                         # [k, i]: row k of right-hand side e_i
    allow = EPS * s * s * np.einsum("ik,ki->i", np.abs(Xi), scale)
    return res, float((np.abs(cov - s * s * np.diag(Xi)) / allow).max())


def _prior_weight(A):
    """Lambda of the solve cases: a twentieth of A's diagonal plus 1e-6, rounded to fp32 -- every case is solvable, whatever it saw."""
    return _f32(0.05 * np.diagonal(A, axis1=-2, axis2=-1) + 1e-6)


def _nominal_pi(bodies):
    m = MODEL()
    nominal = abi.body_params_from_randomisation(m, np.zeros(1), np.zeros((1, 3)), np.zeros(1))
    return linear_body_params(m, nominal)[0, list(bodies)]


def _theta_error(theta_hat, theta):
    """Largest relative error over the groups (m | c | I_c) of every body; [nb, 10] each."""
    return max(np.linalg.norm(theta_hat[b, sl] - theta[b, sl]) / np.linalg.norm(theta[b, sl]) for b in range(len(theta)) for sl in GROUPS)


# ------------------------------------------------------------------------------------------------------------ CPU: restatement
def _rows(states, bodies, bps):
    """[(Phi, Phimag, z, zmag)] of the states with tau_gen = idr.inverse_dynamics at body_params bps[i]."""
    m = MODEL()
    return [ir.regress(m, quat, q, nu, nd, bps[i], bodies, idr.inverse_dynamics(m, pos, quat, q, nu, nd, bps[i])[0])
            for i, (pos, quat, q, nu, nd) in enumerate(states)]


def _run(rows, forget=1.0, weight=None):
    acc = None
    for Phi, Phimag, z, zmag in rows:
        acc = ir.accumulate(MODEL(), acc, Phi, Phimag, z, zmag, weight, forget)
    return acc


def _group_diff(a, b):
    return max(np.linalg.norm(a[s, sl] - b[s, sl]) / np.linalg.norm(b[s, sl]) for s in range(len(b)) for sl in GROUPS)


def test_recursion_is_the_batch_least_squares():
    """(a) forget 1, no prior, the 8 states of _identification_states: the solution is _identify's lstsq to 1e-9 per group."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp, states = _identification_states()
    pi = linear_body_params(m, bp)[0]
    Ys = [rr.regressor(m, quat, q, nu, nd)[0] for pos, quat, q, nu, nd in states]
    taus = [idr.inverse_dynamics(m, pos, quat, q, nu, nd, bp)[0] for pos, quat, q, nu, nd in states]
    want, _ = _identify(Ys, taus, pi, [0, gb])
    acc = _run(_rows(states, [0, gb], [bp] * 8))
    assert acc["stat"][1] == 8 * len(LIVE) and np.array_equal(acc["A"], acc["A"].T)
    sol = ir.solve(acc["A"], acc["b"], acc["stat"])
    got = sol["pi_hat"].reshape(2, NP)
    err = _group_diff(got, want)
    print(f"recursion against lstsq: {err:.3g}; against the truth {_group_diff(got, pi[[0, gb]]):.3g}; sse {sol['sse']:.3g}")
    assert err <= 1e-9 and np.all(sol["status"] == 0)
    assert np.abs(sol["theta_hat"].reshape(2, NP) - bp.reshape(2, NP)).max() <= 1e-8
    assert np.allclose(sol["cov_diag"], np.diag(np.linalg.inv(acc["A"])), rtol=1e-9)


def test_forgetting_is_exponentially_weighted_least_squares():
    """(b) forget 0.8: the weighted least squares with weights 0.8^(T - t)."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp, states = _identification_states()
    rows = _rows(states, [0, gb], [bp] * 8)
    acc = _run(rows, forget=0.8)
    live = ir.live_rows(m)
    wt = [np.sqrt(0.8 ** (len(rows) - 1 - t)) for t in range(len(rows))]
    Phi = np.concatenate([w * r[0][live] for w, r in zip(wt, rows)])
    z = np.concatenate([w * r[2][live] for w, r in zip(wt, rows)])
    s = np.linalg.norm(Phi, axis=0)
    want = (np.linalg.lstsq(Phi / s, z, rcond=None)[0] / s).reshape(2, NP)
    got = ir.solve(acc["A"], acc["b"])["pi_hat"].reshape(2, NP)
    assert np.isclose(acc["stat"][1], len(LIVE) * sum(0.8 ** t for t in range(8)))
    assert _group_diff(got, want) <= 1e-9, _group_diff(got, want)


def test_prior_is_the_ridge_solution():
    """(c) Lambda > 0: the minimiser of |Phi pi - z|^2 + (pi - pi_0)^T Lambda (pi - pi_0), from the stacked rows; three states only, so
    that the prior decides what the data leave open."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp, states = _identification_states()
    rows = _rows(states[:3], [0, gb], [bp] * 3)
    acc = _run(rows)
    live = ir.live_rows(m)
    rng = np.random.default_rng(3)
    lam, p0 = rng.uniform(0.5, 5.0, 2 * NP), _nominal_pi([0, gb]).reshape(-1) * rng.uniform(0.8, 1.2, 2 * NP)
    Phi = np.concatenate([r[0][live] for r in rows] + [np.diag(np.sqrt(lam))])
    z = np.concatenate([r[2][live] for r in rows] + [np.sqrt(lam) * p0])
    want = np.linalg.lstsq(Phi, z, rcond=None)[0].reshape(2, NP)
    sol = ir.solve(acc["A"], acc["b"], prior=p0, prior_weight=lam)
    assert _group_diff(sol["pi_hat"].reshape(2, NP), want) <= 1e-9
    assert np.allclose(sol["cov_diag"], np.diag(np.linalg.inv(acc["A"] + np.diag(lam))), rtol=1e-9)
    # an env that saw nothing: bit 0 and the prior
    none = ir.solve(np.zeros((20, 20)), np.zeros(20), np.zeros(2), prior=p0)
    assert np.all(none["status"] == 1) and np.array_equal(none["pi_hat"], p0) and np.all(np.isinf(none["cov_diag"]))


def test_a_changed_payload_is_tracked_with_forgetting_only():
    """(d) The gripper body gains 0.5 kg after state 8 of 24: forget 0.7 ends within 2 % of the change at the new mass (the old payload's
    states weigh 0.7^16 and less), forget 1 stays more than 10 % of it away (a third of its states carry the old payload)."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp, states = _identification_states(k=24)
    bp2 = bp.copy()
    bp2[10] += 0.5
    rows = _rows(states, [0, gb], [bp] * 8 + [bp2] * 16)
    for forget, tracked in ((0.7, True), (1.0, False)):
        acc = _run(rows, forget=forget)
        mass = ir.solve(acc["A"], acc["b"])["pi_hat"][NP]
        print(f"forget {forget}: gripper-body mass {mass:.4f}, before {bp[10]:.4f}, after {bp2[10]:.4f}")
        assert (abs(mass - bp2[10]) <= 0.02 * 0.5) == tracked and (abs(mass - bp2[10]) >= 0.1 * 0.5) == (not tracked)


def test_gripper_body_alone_from_the_arm_joint_rows():
    """(e) The gripper body's ten parameters from the rows of the six arm joints only (row_weight 0 elsewhere)."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp, states = _identification_states()
    w = (rr.subtree_mask(m)[:, gb] & (np.arange(NCOL) >= 6)).astype(np.float64)
    assert w.sum() == 6
    acc = _run(_rows(states, [gb], [bp] * 8), weight=w)
    assert acc["stat"][1] == 48
    sol = ir.solve(acc["A"], acc["b"], acc["stat"])
    err = _group_diff(sol["pi_hat"].reshape(1, NP), linear_body_params(m, bp)[0][[gb]])
    print(f"gripper body from the arm rows: {err:.3g}, smallest squared pivot {sol['pivot2'].min():.3g}")
    assert err <= 1e-8 and np.all(sol["status"] == 0)


def test_fp32_yardstick_sits_inside_the_bounds():
    """(f) K_ref: the numpy-float32 chain's largest ratios on the GPU tests' cases; the constants hold 4 x them."""
    k = {name: 0.0 for name in ("z", "A", "b", "stat", "solve", "cov")}
    for n in (1, 13, 64):
        bp = _case(n)["bp"]
        for bodies in _lists():
            ref, got = _reference(n, bodies, bp), _reference(n, bodies, bp, np.float32)
            for call in (0, 1):
                for name, r in _ratios(got[call], ref[call]).items():
                    k[name] = max(k[name], r)
            lam, p0 = _prior_weight(ref[1]["A"]), _nominal_pi(bodies).reshape(-1)
            for e in range(n):
                sol = ir.solve(ref[1]["A"][e], ref[1]["b"][e], prior=p0, prior_weight=lam[e], dtype=np.float32)
                assert sol["pi_hat"].dtype == np.float32 and np.all(sol["status"] & 1 == 0)
                rs, rc = _solve_ratios(_f32(ref[1]["A"][e]), _f32(ref[1]["b"][e]), lam[e], _f32(p0), sol["pi_hat"], sol["cov_diag"])
                k["solve"], k["cov"] = max(k["solve"], rs), max(k["cov"], rc)
    print("fp32 yardstick: K_ref " + ", ".join(f"{name} {v:.3g}" for name, v in k.items()))
    assert 4 * k["z"] <= C_T and 4 * k["A"] <= C_A and 4 * k["b"] <= C_B and 4 * k["stat"] <= C_STAT, k
    assert 4 * max(k["solve"], k["cov"]) <= C_X, k


def test_null_and_bad_arguments_are_rejected_without_a_device():
    """(g) The refusals that need no device, through raw ctypes: the status and the entry point's own name in wbc_last_error()."""
    from wbc_amd.native import EXPORTED_SYMBOLS, lib
    L = lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    idx = (C.c_int32 * 1)(0)
    assert L.wbc_sim_identification_accumulate(None, idx, 1, None, p, None, 1.0, p, p, p, None, 0, None) == -1
    assert b"wbc_sim_identification_accumulate: " in L.wbc_last_error() and b"NULL" in L.wbc_last_error()
    assert L.wbc_sim_identification_solve(None, 1, p, p, p, None, None, 1e-5, p, None, None, None, None, None) == -1
    assert b"wbc_sim_identification_solve: " in L.wbc_last_error() and b"NULL" in L.wbc_last_error()
    assert IDENT_RESET == 8 and IDENT_MAX_BODIES == 3 and IDENT_RESET not in (abi.SOLVE_ARMATURE, abi.DERIV_TRANSPOSED, abi.REGRESSOR_NATIVE)
    assert "wbc_sim_identification_accumulate" in EXPORTED_SYMBOLS and "wbc_sim_identification_solve" in EXPORTED_SYMBOLS


def test_identification_kernels_codegen():
    """(h) Both new kernels: no scratch, no flat memory instructions, LDS for 8 workgroups per CU, 64 lanes. The kernels that were
    there, the regressor among them: LDS, scratch and register class as before."""
    for k in ("wbc_identification_accumulate_kernel", "wbc_identification_solve_kernel"):
        assert arm_codegen.meta(k, "private_segment_fixed_size") == 0
        assert arm_codegen.meta(k, "group_segment_fixed_size") <= 20480
        assert arm_codegen.meta(k, "max_flat_workgroup_size") == 64
        body = arm_codegen.body(k)
        assert "s_endpgm" in body and not re.search(r"\bflat_", body) and "scratch_" not in body
    assert re.search(r"\bglobal_store_dwordx4\b", arm_codegen.body("wbc_identification_accumulate_kernel"))
    before = dict(PARENT_CODEGEN, wbc_inverse_dynamics_regressor_kernel=(11248, 0, 8), wbc_impulse_rhs_kernel=(1032, 0, 8),
                  wbc_impulse_solve_kernel=(8880, 0, 7), wbc_impulse_solve_map_kernel=(14288, 0, 6), wbc_ik_kernel=(19888, 0, 3),
                  wbc_coriolis_kernel=(12264, 0, 6), wbc_momentum_kernel=(3040, 0, 3))
    assert len(before) == 22 and arm_codegen.assembly().count(".amdhsa_kernel ") == 24
    for name, want in before.items():
        got = (arm_codegen.meta(name, "group_segment_fixed_size"), arm_codegen.meta(name, "private_segment_fixed_size"),
               _waves(arm_codegen.meta(name, "vgpr_count")))
        assert got == want, (name, got, want)


# ------------------------------------------------------------------------------------------------------------ GPU: the kernels
def _dev(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device="cuda").contiguous()


def _poisoned(n, p):
    nan = float("nan")
    return (torch.full((n, p, p), nan, device="cuda"), torch.full((n, p), nan, device="cuda"), torch.full((n, 2), nan, device="cuda"))


def _two_calls(env, n, bodies, nudot, state=None):
    """The element-wise cases' two accumulate calls; returns [(A, b, stat, target)] after each as float64 numpy, and the tensors."""
    inp = _inputs(n)
    A, b, st = state if state is not None else _poisoned(n, NP * len(bodies))
    out = []
    for call in (0, 1):
        tgt = env.sim.identification_accumulate(bodies, _dev(inp["tau1" if call == 0 else "tau2"]), nudot=nudot if call == 0 else _dev(inp["nudot2"]),
                                                row_weight=None if call == 0 else _dev(inp["w2"]), forget=1.0 if call == 0 else FORGET2,
                                                info_mat=A, info_vec=b, stat=st, reset=call == 0)[3]
        torch.cuda.synchronize()
        out.append({"A": A.cpu().numpy().astype(np.float64), "b": b.cpu().numpy().astype(np.float64),
                    "stat": st.cpu().numpy().astype(np.float64), "z": tgt.cpu().numpy().astype(np.float64)})
    return out, (A, b, st)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_accumulate_matches_reference_elementwise(n):
    """target, A, b and stat of every env after the RESET call and after the second call, for the three body lists; A bit-symmetric;
    the measured ratios stand in the module's docstring."""
    env, nudot, bp = _gpu_env(n)
    worst = {}
    for bodies in _lists():
        ref = _reference(n, bodies, bp)
        got, _ = _two_calls(env, n, bodies, nudot)
        for call in (0, 1):
            assert np.array_equal(got[call]["A"], got[call]["A"].transpose(0, 2, 1))
            assert np.all(got[call]["z"][:, FINGERS] == _inputs(n)["tau1" if call == 0 else "tau2"][:, FINGERS])
            r = _ratios(got[call], ref[call])
            print(f"identification n={n} bodies={bodies} call {call}: largest |kernel - ref| / (2^-24 mag): {r}")
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
        if n > 3:                                             # env 3 saw nothing in the second call: no decay, bit for bit
            for k in ("A", "b", "stat"):
                assert np.array_equal(got[1][k][3], got[0][k][3])
    print(f"identification n={n}: largest ratios {worst}")
    assert worst["z"] <= C_T and worst["A"] <= C_A and worst["b"] <= C_B and worst["stat"] <= C_STAT, worst


@pytest.mark.gpu
def test_target_is_the_listed_bodies_share_of_inverse_dynamics():
    """With tau_gen the existing kernel's inverse_dynamics(nudot), target equals Phi pi_S from the regressor kernel within the sum of
    both allowances: C_Y 2^-24 sum_b mag_b |pi_b| over all bodies and C_ID 2^-24 of inverse dynamics' own magnitude."""
    n = 13
    env, nudot, bp = _gpu_env(n)
    c, m = _case(n), env.robot_model
    pi = linear_body_params(m, bp)
    tau = env.inverse_dynamics(nudot)
    Y = env.sim.inverse_dynamics_regressor(nudot=nudot).cpu().numpy().astype(np.float64)
    mag = np.array([r[1] for r in _regressors(n, 0, np.float64)])
    tmag = np.array([idr.inverse_dynamics(m, c["pos"][e], c["quat"][e], c["q"][e], c["nu"][e], c["nudot"][e], bp[e], c["gravity"])[1] for e in range(n)])
    allow = EPS * (C_Y * np.einsum("ncbk,nbk->nc", mag, np.abs(pi)) + C_ID * tmag)
    for bodies in _lists():
        tgt = env.sim.identification_accumulate(bodies, tau, nudot=nudot)[3].cpu().numpy().astype(np.float64)
        want = np.einsum("ncbk,nbk->nc", Y[:, :, bodies], pi[:, bodies])
        worst = float((np.abs(tgt - want)[:, LIVE] / allow[:, LIVE]).max())
        print(f"target against the regressor kernel's Phi pi, bodies={bodies}: {worst:.3g} of the allowance")
        assert np.all(np.abs(tgt - want) <= allow), worst


@pytest.mark.gpu
def test_bits_reset_zero_weights_repeat_and_translation():
    """A poisoned buffer with RESET equals a zeroed buffer without; an env with all-zero weights is untouched (its target is written);
    two runs give identical bits; a robot 110 m away gives the same bits."""
    n = 13
    env, nudot, _ = _gpu_env(n)
    c, inp = _case(n), _inputs(n)
    bodies = _lists()[2]
    p = NP * len(bodies)
    first, (A, b, st) = _two_calls(env, n, bodies, nudot)
    again, (A2, b2, st2) = _two_calls(env, n, bodies, nudot)
    assert all(torch.equal(x, y) for x, y in ((A, A2), (b, b2), (st, st2)))
    assert all(np.array_equal(first[k][key], again[k][key]) for k in (0, 1) for key in ("A", "b", "stat", "z"))
    # zeroed buffers, no RESET: the first call's bits
    zero = (torch.zeros((n, p, p), device="cuda"), torch.zeros((n, p), device="cuda"), torch.zeros((n, 2), device="cuda"))
    env.sim.identification_accumulate(bodies, _dev(inp["tau1"]), nudot=nudot, forget=FORGET2, info_mat=zero[0], info_vec=zero[1], stat=zero[2])
    torch.cuda.synchronize()
    for t, key in zip(zero, ("A", "b", "stat")):
        assert np.array_equal(t.cpu().numpy().astype(np.float64), first[0][key])
    # all-zero weights in env 5, poisoned buffers, no RESET: the poison stays, the target is written; with RESET: zeros
    w = torch.ones((n, NCOL), device="cuda")
    w[5] = 0.0
    for reset in (False, True):
        P3 = _poisoned(n, p)
        tgt = env.sim.identification_accumulate(bodies, _dev(inp["tau1"]), nudot=nudot, row_weight=w, info_mat=P3[0], info_vec=P3[1], stat=P3[2],
                                                reset=reset)[3]
        torch.cuda.synchronize()
        assert np.array_equal(tgt.cpu().numpy().astype(np.float64), first[0]["z"])
        for t, key in zip(P3, ("A", "b", "stat")):
            got = t.cpu().numpy().astype(np.float64)
            keep = [e for e in range(n) if e != 5]
            assert bool((t[5] == 0).all()) if reset else bool(torch.isnan(t[5]).all())
            assert not reset or np.array_equal(got[keep], first[0][key][keep])
    # translation: the same states 110 m away
    _set_states(env, c["pos"], c["quat"], c["q"], c["nu"], shift=(3.0, 110.0, 0.0))
    far, (A3, b3, st3) = _two_calls(env, n, bodies, nudot)
    assert all(torch.equal(x, y) for x, y in ((A, A3), (b, b3), (st, st3))) and np.array_equal(far[1]["z"], first[1]["z"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 13, 64])
def test_solve_in_residual_form(n):
    """(A + Lambda) pi_hat = b + Lambda pi_0 with A and b the accumulate kernel's own bits: the residual within C_X 2^-24 of the row
    scale, theta_hat against the fp64 map of the kernel's pi_hat, cov_diag against the fp64 inverse, sse against fp64 within what its
    three terms resolve, status against the fp64 flags of the kernel's theta wherever these are clear (ir.flags_are_clear: at least half of
    the bodies)."""
    env, nudot, _ = _gpu_env(n)
    worst = {"solve": 0.0, "cov": 0.0, "theta": 0.0, "sse": 0.0}
    clear = 0
    for bodies in _lists():
        got, (A, b, st) = _two_calls(env, n, bodies, nudot)
        lam, p0 = _prior_weight(got[1]["A"]), np.tile(_f32(_nominal_pi(bodies))[None], (n, 1, 1))
        r = env.sim.identification_solve(A, b, st, prior=_dev(p0), prior_weight=_dev(lam.reshape(p0.shape)))
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy().astype(np.float64 if k != "status" else np.int32) for k, v in r.items()}
        assert all(np.isfinite(r[k]).all() for k in ("pi_hat", "theta_hat", "cov_diag", "sse")) and np.all(r["status"] & 1 == 0)
        for e in range(n):
            Ae, be, pi = got[1]["A"][e], got[1]["b"][e], r["pi_hat"][e].reshape(-1)
            rs, rc = _solve_ratios(Ae, be, lam[e], p0[e].reshape(-1), pi, r["cov_diag"][e].reshape(-1))
            worst["solve"], worst["cov"] = max(worst["solve"], rs), max(worst["cov"], rc)
            th = ir.theta_map(r["pi_hat"][e])
            m_, c_ = np.abs(r["pi_hat"][e][:, 0:1]), th[:, 1:4]
            thmag = np.concatenate([m_, np.abs(c_), np.abs(r["pi_hat"][e][:, 4:10]) + m_ * np.abs(rr._shift(c_))], axis=1)
            worst["theta"] = max(worst["theta"], float((np.abs(r["theta_hat"][e] - th) / (EPS * thmag)).max()))
            for s, t in enumerate(th):                            # random tau_gen gives unphysical estimates: every flag occurs
                if ir.flags_are_clear(t):
                    clear += 1
                    assert r["status"][e, s] == ir.flags(t), (e, s, r["status"][e, s], ir.flags(t))
            terms = np.array([got[1]["stat"][e, 0], 2 * abs(pi @ be), np.abs(pi) @ np.abs(Ae) @ np.abs(pi)])
            sse = max(got[1]["stat"][e, 0] - 2 * pi @ be + pi @ Ae @ pi, 0.0)
            worst["sse"] = max(worst["sse"], float(abs(r["sse"][e] - sse) / (EPS * terms.sum())))
    print(f"solve n={n}: largest ratios {worst}; status compared on {clear} of {6 * n} bodies")
    assert clear >= 3 * n
    assert worst["solve"] <= C_X and worst["cov"] <= C_X and worst["theta"] <= C_TH and worst["sse"] <= C_SSE, worst


@pytest.mark.gpu
def test_status_flags():
    """An env that was never excited (all weights zero from the start) gives bit 0 and the prior, with or without a prior weight of
    zero; a constructed b = A pi with a negated mass gives bit 1. Clear cases only."""
    n = 13
    env, nudot, _ = _gpu_env(n)
    bodies = _lists()[1]
    inp = _inputs(n)
    w = torch.ones((n, NCOL), device="cuda")
    w[4] = 0.0
    A, b, st, _ = env.sim.identification_accumulate(bodies, _dev(inp["tau1"]), nudot=nudot, row_weight=w)
    A, b, st, _ = env.sim.identification_accumulate(bodies, _dev(inp["tau2"]), nudot=_dev(inp["nudot2"]), row_weight=w, info_mat=A, info_vec=b, stat=st)
    p0 = _dev(np.tile(_f32(_nominal_pi(bodies))[None], (n, 1, 1)))
    lam = _dev(_prior_weight(A.cpu().numpy().astype(np.float64)).reshape(n, 2, NP))
    lam[4] = 0.0
    r = env.sim.identification_solve(A, b, st, prior=p0, prior_weight=lam)
    torch.cuda.synchronize()
    assert bool((A[4] == 0).all()) and r["status"][4].tolist() == [1, 1] and torch.equal(r["pi_hat"][4], p0[4])
    assert bool(torch.isinf(r["cov_diag"][4]).all()) and float(r["sse"][4]) == 0.0
    assert torch.allclose(r["theta_hat"][4], _dev(ir.theta_map(p0[4].cpu().numpy().astype(np.float64))), rtol=1e-5, atol=1e-7)
    keep = [e for e in range(n) if e != 4]
    assert bool((r["status"][keep] & 1 == 0).all())
    bare = env.sim.identification_solve(A, b, st)                                    # no prior: zeros
    assert bare["status"][4].tolist() == [1, 1] and bool((bare["pi_hat"][4] == 0).all()) and bool((bare["theta_hat"][4] == 0).all())
    # m_hat < 0 by construction: b = (A + Lambda) pi_neg - Lambda pi_0 in fp64, rounded
    pneg = p0.cpu().numpy().astype(np.float64).reshape(n, -1)
    pneg[:, NP] *= -1.0                                                               # the gripper body's mass
    A64, l64 = A.cpu().numpy().astype(np.float64), lam.cpu().numpy().astype(np.float64).reshape(n, -1)
    bneg = np.einsum("nij,nj->ni", A64, pneg) + l64 * (pneg - p0.cpu().numpy().astype(np.float64).reshape(n, -1))
    r = env.sim.identification_solve(A, _dev(bneg), st, prior=p0, prior_weight=lam)
    torch.cuda.synchronize()
    status = r["status"].cpu().numpy()
    assert np.all(status[keep, 1] & 2 == 2) and np.all(status[keep, 0] & 2 == 0) and np.all(status[keep] & 1 == 0), status
    assert bool((r["pi_hat"][keep, 1, 0] < -0.5 * p0[0, 1, 0]).all())


def _recovery_env(n):
    dm, dcom, gd = RANDOMISATION
    env = _env(n, seed=2, steps=0)
    env.sim.set_env_params(base_dmass=np.full(n, dm, np.float32), base_dcom=np.tile(np.float32(dcom), (n, 1)), gripper_dmass=np.full(n, gd, np.float32))
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    assert np.all(bp == bp[0]) and bp[0, 0] > MODEL().mass[0] + 1.6
    states = [tuple(_f32(x) for x in s) for s in _identification_states()[1]]
    return env, bp, states


def _show(env, n, state):
    """All n envs into the one state (pos, quat, q, nu, nudot); returns nudot as a tensor."""
    _set_states(env, *[np.tile(state[i][None], (n,) + (1,) * state[i].ndim) for i in range(4)])
    return _dev(np.tile(state[4][None], (n, 1)))


def _yardstick_error(states, theta, taus=None):
    """The fp32 yardstick's recovery error on the states (pos, quat, q, nu, nudot): numpy-float32 regressor, normal equations and
    Cholesky, tau_gen from numpy-float32 inverse dynamics (or taus, where another fp32 chain made them); per group (m | c | I_c) of the
    root and the gripper body."""
    m = MODEL()
    gb = m.gripper_piece["body"]
    bp = np.concatenate([theta[0], theta[gb]])
    acc = None
    for i, s in enumerate(states):
        tau = rr.inverse_dynamics_yardstick(m, s[1], s[2], s[3], s[4], theta) if taus is None else taus[i]
        acc = ir.accumulate(m, acc, *ir.regress(m, s[1], s[2], s[3], s[4], bp, [0, gb], tau, dtype=np.float32))
    sol = ir.solve(acc["A"], acc["b"], dtype=np.float32)
    assert sol["pi_hat"].dtype == np.float32 and np.all(sol["status"] == 0)
    return _theta_error(sol["theta_hat"].astype(np.float64).reshape(2, NP), theta[[0, gb]])


@pytest.mark.gpu
def test_recovers_the_randomisation():
    """A known randomisation through set_env_params, eight accumulate calls on the eight states of _identification_states (one state per
    call, all envs the same), tau_gen from the existing inverse-dynamics kernel: env.parameter_identifier() recovers BODY_PARAMS per
    group (m | c | I_c) within 4 x the fp32 yardstick's error on the same states, in every env."""
    n = 13
    m = MODEL()
    gb = m.gripper_piece["body"]
    env, bp, states = _recovery_env(n)
    ident = env.parameter_identifier()
    assert ident.bodies == [0, gb]
    for s in states:
        nudot = _show(env, n, s)
        ident.update(env.inverse_dynamics(nudot), nudot)
    est, status = ident.estimate()
    payload = ident.payload()
    torch.cuda.synchronize()
    assert est.shape == (n, 20) and status.shape == (n, 2) and bool((status == 0).all())
    assert bool((ident.stat[:, 1] == 8 * len(LIVE)).all())
    theta = rr.theta_of(m, bp[0])
    yard = _yardstick_error(states, theta)
    est = est.cpu().numpy().astype(np.float64)
    got = max(_theta_error(est[e].reshape(2, NP), bp[e].reshape(2, NP)) for e in range(n))
    print(f"recovery on the GPU: error {got:.3g}, fp32 yardstick {yard:.3g}")
    assert got <= 4 * yard, (got, yard)
    assert np.allclose(payload.cpu().numpy(), est[:, 10] - _nominal_pi([gb])[0, 0], atol=1e-6) and abs(float(payload[0]) - RANDOMISATION[2]) < 1e-3
    ident.reset([2])
    assert bool((ident.info_mat[2] == 0).all()) and bool((ident.info_mat[3] != 0).any())
    assert ident.estimate()[1][2].tolist() == [1, 1]


@pytest.mark.gpu
def test_recovers_the_randomisation_under_contact():
    """nudot and the foot forces from stance_forward_dynamics with four feet under random joint torques: env.generalised_force(tau,
    forces) equals inverse_dynamics(nudot) within the allowances of tests/constrained_dynamics_reference.py's dynamics rows (C_S 2^-24
    row scale + C_ID 2^-24 mag(h)) plus inverse dynamics' own (C_ID 2^-24 mag(nudot)), and the identifier fed with it recovers the
    parameters to the bound of test_recovers_the_randomisation: 4 x the fp32 yardstick's error on the same states, the yardstick being the
    same chain in numpy float32 -- cdr.yardstick_f32's (nudot, forces), tau + Jc^T forces, normal equations, Cholesky. (With tau_gen from
    numpy-float32 inverse dynamics at the kernel's nudot instead, which leaves the constrained solve's own residual out of the
    yardstick, the yardstick's error was 4.85e-7 and the kernels' 2.41e-6 on an MI355X.)"""
    n = 13
    m = MODEL()
    env, bp, states = _recovery_env(n)
    feet = [int(i) for i in env.feet_indices.tolist()]
    ident = env.parameter_identifier()
    rng = np.random.default_rng(11)
    seen, taus32, worst = [], [], 0.0
    for s in states:
        _show(env, n, s)
        tau = msr.force_rhs(rng, ())
        tau[:6] = 0.0
        tau_t = _dev(np.tile(tau[None], (n, 1)))
        nudot, lam = env.stance_forward_dynamics(tau_t)
        tau_gen = env.generalised_force(tau_t, lam)
        back = env.inverse_dynamics(nudot)
        ident.update(tau_gen, nudot)
        torch.cuda.synchronize()
        assert torch.equal(nudot, nudot[0:1].expand(n, -1)) and torch.equal(tau_gen, tau_gen[0:1].expand(n, -1))
        nd, lm, tg = (x[0].cpu().numpy().astype(np.float64) for x in (nudot, lam, tau_gen))
        M = msr.mass_matrix(m, s[0], s[1], s[2], bp[0])
        Jc = np.concatenate([wb.jacobian(m, s[0], s[1], s[2])[r][0:3] for r in feet])
        d = np.zeros(NCOL)
        d[LIVE] = np.sqrt(np.diag(M)[LIVE])
        scale = d * (np.abs(nd) @ d) + np.abs(_f32(tau)) + np.abs(Jc).T @ np.abs(lm.reshape(-1))
        allow = EPS * (msr.C_S * scale + C_ID * idr.inverse_dynamics(m, s[0], s[1], s[2], s[3], None, bp[0])[1]
                       + C_ID * idr.inverse_dynamics(m, s[0], s[1], s[2], s[3], nd, bp[0])[1])
        diff = np.abs(tg - back[0].cpu().numpy().astype(np.float64))
        worst = max(worst, float((diff[LIVE] / allow[LIVE]).max()))
        assert np.all(diff[LIVE] <= allow[LIVE]), worst
        # the yardstick's own fp32 chain on this state: constrained dynamics, then tau + Jc^T lambda, all in numpy float32
        h = idr.inverse_dynamics(m, s[0], s[1], s[2], s[3], None, bp[0])[0]
        gamma = cdr.constraint_rows(m, s[0], s[1], s[2], s[3], feet)[1]
        nd32, lm32 = cdr.yardstick_f32(M, h, _f32(tau), Jc, gamma, np.zeros(12), 0.0, np.ones(12, bool))
        seen.append((s[0], s[1], s[2], s[3], nd32))
        taus32.append(np.float32(tau) + Jc.astype(np.float32).T @ lm32.astype(np.float32))
    est, status = ident.estimate()
    torch.cuda.synchronize()
    yard = _yardstick_error(seen, rr.theta_of(m, bp[0]), taus32)
    est = est.cpu().numpy().astype(np.float64)
    got = max(_theta_error(est[e].reshape(2, NP), bp[e].reshape(2, NP)) for e in range(n))
    print(f"recovery under contact: generalised force against inverse dynamics {worst:.3g} of the allowance; error {got:.3g}, fp32 yardstick {yard:.3g}")
    assert bool((status == 0).all()) and got <= 4 * yard, (got, yard)


@pytest.mark.gpu
def test_refusals_leave_the_buffers_untouched():
    """Every -1 case of both entry points, one call at a time: the status, the word in wbc_last_error() under the entry point's own
    name, and at the end every poisoned buffer as it was."""
    n = 13
    env, nudot, _ = _gpu_env(n)
    L, h = env.sim.L, env.sim.h
    gb = _gripper(env)
    p = 2 * NP
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    A, b, st, tgt, tau, w = full(n, p, p), full(n, p), full(n, 2), full(n, NCOL), full(n, NCOL), full(n, NCOL)
    pi, th, cov, sse, prior, lam = full(n, 2, NP), full(n, 2, NP), full(n, 2, NP), full(n), full(n, 2, NP), full(n, 2, NP)
    status = torch.full((n, 2), 12345, dtype=torch.int32, device="cuda")
    idx = lambda *v: (C.c_int32 * len(v))(*v)
    names = ("sim", "bodies", "nbodies", "nudot", "tau_gen", "row_weight", "forget", "A", "b", "stat", "target", "flags", "stream")
    base = dict(sim=h, bodies=idx(0, gb), nbodies=2, nudot=nudot.data_ptr(), tau_gen=tau.data_ptr(), row_weight=w.data_ptr(), forget=C.c_float(1.0),
                A=A.data_ptr(), b=b.data_ptr(), stat=st.data_ptr(), target=tgt.data_ptr(), flags=0, stream=None)
    call = lambda **kw: L.wbc_sim_identification_accumulate(*[kw.get(k, base[k]) for k in names])
    refusals = [(dict(sim=None), b"NULL")] + [({k: None}, b"NULL") for k in ("tau_gen", "A", "b", "stat")]
    refusals += [(kw, b"bodies") for kw in (dict(bodies=None), dict(bodies=None, nbodies=0), dict(nbodies=0), dict(nbodies=-1),
                                            dict(bodies=idx(0, 1, 2, 3), nbodies=4), dict(bodies=idx(0, NB)), dict(bodies=idx(-1, 0)), dict(bodies=idx(gb, gb)))]
    refusals += [(dict(forget=C.c_float(f)), b"forget") for f in (0.0, -0.5, 1.5, float("nan"))]
    refusals += [(dict(flags=f), b"flag") for f in (1, 2, 4, IDENT_RESET | 16)]
    refusals += [({k: base[k] + off}, b"aligned") for k in ("nudot", "tau_gen", "row_weight", "A", "b", "stat", "target") for off in (4, 8)]
    refusals += [(dict(b=base["A"] + 16), b"overlap"), (dict(stat=base["b"] + 4 * (n * p - 4)), b"overlap"), (dict(target=base["tau_gen"]), b"overlap"),
                 (dict(nudot=base["A"] + 4 * (n * p * p - 4)), b"overlap"), (dict(row_weight=base["target"] + 16), b"overlap")]
    for kw, word in refusals:
        assert call(**kw) == -1, kw
        err = L.wbc_last_error()
        assert word in err and b"wbc_sim_identification_accumulate: " in err, (kw, err)
    names_s = ("sim", "nbodies", "A", "b", "stat", "prior", "lam", "tol", "pi", "theta", "cov", "sse", "status", "stream")
    base_s = dict(sim=h, nbodies=2, A=A.data_ptr(), b=b.data_ptr(), stat=st.data_ptr(), prior=prior.data_ptr(), lam=lam.data_ptr(), tol=C.c_float(1e-5),
                  pi=pi.data_ptr(), theta=th.data_ptr(), cov=cov.data_ptr(), sse=sse.data_ptr(), status=status.data_ptr(), stream=None)
    call_s = lambda **kw: L.wbc_sim_identification_solve(*[kw.get(k, base_s[k]) for k in names_s])
    refusals = [(dict(sim=None), b"NULL")] + [({k: None}, b"NULL") for k in ("A", "b", "pi", "stat", "prior")]
    refusals += [(dict(nbodies=k), b"nbodies") for k in (0, -1, 4)]
    refusals += [(dict(tol=C.c_float(t)), b"pivot_tol") for t in (0.0, -1.0, float("nan"), float("inf"))]
    refusals += [({k: base_s[k] + off}, b"aligned") for k in names_s[2:7] + names_s[8:13] for off in (4, 8)]
    refusals += [(dict(theta=base_s["pi"] + 16), b"overlap"), (dict(pi=base_s["A"]), b"overlap"), (dict(cov=base_s["prior"]), b"overlap"),
                 (dict(sse=base_s["stat"]), b"overlap"), (dict(status=base_s["b"]), b"overlap")]
    for kw, word in refusals:
        assert call_s(**kw) == -1, kw
        err = L.wbc_last_error()
        assert word in err and b"wbc_sim_identification_solve: " in err, (kw, err)
    torch.cuda.synchronize()
    for t in (A, b, st, tgt, tau, w, pi, th, cov, sse, prior, lam):
        assert bool((t == SENTINEL).all())
    assert bool((status == 12345).all())
    # the same buffers are filled by good calls
    tau.copy_(_dev(_inputs(n)["tau1"])); w.fill_(1.0)
    assert call(flags=IDENT_RESET) == 0
    prior.copy_(_dev(np.tile(_f32(_nominal_pi([0, gb]))[None], (n, 1, 1)))); lam.fill_(0.5)
    assert call_s() == 0
    torch.cuda.synchronize()
    want = env.sim.identification_accumulate([0, gb], tau, nudot=nudot)
    assert all(torch.equal(x, y) for x, y in zip((A, b, st, tgt), want))
    r = env.sim.identification_solve(A, b, st, prior=prior, prior_weight=lam)
    assert all(torch.equal(x, r[k]) for x, k in zip((pi, th, cov, sse, status), env.sim.IDENT_OUTPUTS))
