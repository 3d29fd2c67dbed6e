"""One physics substep against the fp64 equations of motion, on the CPU: pins the checker of tests/forward_dynamics_reference.py
(substep_residual, integrator_errors, eligible) to the C oracle and measures the constants that tests/test_gpu_forward_dynamics.py
holds the HIP kernels to. Every case family and state set of the GPU test runs here through OracleSim(precision="f64") and
OracleSim(precision="f32"), same seeds, same n.

  * fp64 build: |res| / (2^-24 scale) <= 1 on every eligible env and live row (measured: 0.05 to 0.74; not 1e-9 because the oracle
    reads float32 model tables and the checker the asset's doubles).
  * fp32 build: its largest ratio per family is that family's K_ref, asserted against forward_dynamics_reference.K_REF
    (measured: airborne 6.61, feet contact 9.51, limit stop 5.01, single-substep step 14.06, integrator 3.82).
  * eligibility: the share of envs the equations describe is a condition on the draws, asserted on the fp64 build alone.

The single-substep step holds on the fp64 oracle (decimation = 1: TORQUES after the step are the substep's, FORCE_SENSOR is not
post-processed, the step counter is placed so that no push fires, envs that reset are left out), so the step tier is part of both
files. Five steps from reset_all do not bring a foot to the ground (the robots spawn 0.42 m up): that tier is the step kernel's
airborne substep under the PD torques of _compute_torques."""
import numpy as np
import pytest

import forward_dynamics_reference as fdr
import helpers
import inverse_dynamics_reference as idr
import whole_body_reference as wb

LIVE, FINGERS = fdr.LIVE, fdr.FINGERS


@pytest.fixture(scope="module")
def runs(robot):
    """(precision, case name) -> the per-substep results of fdr.run_substeps / run_steps, each computed once."""
    cache = {}
    model, wm = robot["model"], robot["wmodel"]

    def get(prec, name):
        if (prec, name) in cache:
            return cache[prec, name]
        if name.startswith("step-"):
            n, seed = next(c for c in fdr.STEP_CASES if f"step-{c[0]}" == name)
            tc = fdr.with_cfg(robot["tcfg"], decimation=1)
            o = helpers.make_oracle(robot, n, helpers.random_env_params(n, seed=seed), prec, tcfg=tc)
            out = fdr.run_steps(fdr.OracleAdapter(o), model, wm, tc, fdr.step_actions(n, seed), fdr.step_envs(n))
        else:
            family, _, n, seed, grav, substeps = next(c for c in fdr.SUBSTEP_CASES if c[1] == name)
            tc = fdr.with_cfg(robot["tcfg"], gravity=grav)
            o = helpers.make_oracle(robot, n, helpers.random_env_params(n, seed=seed), prec, tcfg=tc)
            root, dof, tau = fdr.case_states(family, wm, tc, n, seed)
            out = fdr.run_substeps(fdr.OracleAdapter(o), model, wm, tc, family, root, dof, tau, substeps)
        cache[prec, name] = out
        return out
    return get


CASES = [(c[0], c[1]) for c in fdr.SUBSTEP_CASES] + [("step", f"step-{n}") for n, _ in fdr.STEP_CASES]


def _evaluated(o):
    return ~np.isnan(o["ratio"][:, 0])


def _worst(outs):
    """Largest ratio over the evaluated envs and live rows of every substep; the finger rows have to be exactly 0."""
    worst = 0.0
    for o in outs:
        r = o["ratio"][_evaluated(o)]
        assert np.all(r[:, FINGERS] == 0)
        worst = max(worst, float(r[:, LIVE].max()))
    return worst


def _worst_integ(outs):
    return max(float(np.nanmax(o["integ"])) for o in outs)


@pytest.mark.parametrize("family,name", CASES)
def test_f64_oracle_satisfies_the_equations_of_motion(robot, runs, family, name):
    outs = runs("f64", name)
    worst = _worst(outs)
    print(f"{name}: fp64 oracle, largest |res| / (2^-24 scale) = {worst:.3f}, integrator {_worst_integ(outs):.2e}")
    assert worst <= 1.0
    assert _worst_integ(outs) <= 1e-3                       # the fp64 integrator IS the restatement
    for o in outs:                                          # every live row is exercised
        assert np.all(np.nanmax(o["scale"][:, LIVE], axis=0) > 0)


@pytest.mark.parametrize("family,name", CASES)
def test_eligibility_of_the_draws(robot, runs, family, name):
    outs = runs("f64", name)
    envs = fdr.step_envs(len(outs[0]["elig"]))
    for i, o in enumerate(outs):
        share = o["elig"][envs].mean()
        print(f"{name} substep {i}: {int(o['elig'][envs].sum())} of {len(envs)} eligible, {o['contacts']} foot contacts")
        assert share >= fdr.MIN_ELIGIBLE[family], (name, i, share)
        assert np.array_equal(_evaluated(o)[envs], o["elig"][envs])
    if family == "contact":
        assert sum(o["contacts"] for o in outs) >= len(outs[0]["elig"])
    if family in ("airborne", "limit"):
        assert all(o["contacts"] == 0 for o in outs)


def test_limit_case_has_both_signs_of_approach(robot):
    family, _, n, seed, _, _ = next(c for c in fdr.SUBSTEP_CASES if c[0] == "limit")
    tb = fdr.tables(robot["wmodel"], robot["tcfg"])
    _, dof, _ = fdr.limit_states(robot["wmodel"], robot["tcfg"], n, seed)
    q, qd = dof[:, :18, 0].astype(np.float64), dof[:, :18, 1].astype(np.float64)
    viol = np.where(q > tb["hi"][:18], q - tb["hi"][:18], np.where(q < tb["lo"][:18], q - tb["lo"][:18], 0.0))
    viol[:, ~(tb["lo"] < tb["hi"])[:18]] = 0
    assert np.all((viol != 0).sum(1) == 2)
    assert np.all((np.abs(viol[viol != 0]) > 0.0049) & (np.abs(viol[viol != 0]) < 0.0501))
    assert (qd * viol > 0).sum() > n // 2 and (qd * viol < 0).sum() > n // 2
    assert (viol > 0).sum() > n // 2 and (viol < 0).sum() > n // 2


def test_k_ref_of_every_family(robot, runs):
    """The fp32 oracle's largest ratios: printed, and asserted against the committed K_REF (not above it; not below 80 % of it,
    so that a committed constant cannot be looser than what was measured)."""
    k = {}
    integ = 0.0
    for family, name in CASES:
        outs = runs("f32", name)
        k[family] = max(k.get(family, 0.0), _worst(outs))
        integ = max(integ, _worst_integ(outs))
    _, _, _, _, ig = fdr.clamp_check(fdr.OracleAdapter(_clamp_oracle(robot, "f32")), robot["model"], robot["wmodel"], robot["tcfg"])
    k["integrator"] = max(integ, float(ig.max()))
    print("K_ref (fp32 oracle):", {f: round(v, 3) for f, v in k.items()}, "C:", {f: fdr.bound(f) for f in k})
    for f, v in k.items():
        assert 0.8 * fdr.K_REF[f] <= v <= fdr.K_REF[f], (f, v, fdr.K_REF[f])
        assert fdr.bound(f) <= fdr.C_CAP


# ------------------------------------------------------------------------------------------------------- the checker can fail
def _one_case(robot, family, prec="f64"):
    _, name, n, seed, grav, _ = next(c for c in fdr.SUBSTEP_CASES if c[0] == family and c[2] >= 64)
    n = 32
    tc = fdr.with_cfg(robot["tcfg"], gravity=grav)
    o = fdr.OracleAdapter(helpers.make_oracle(robot, n, helpers.random_env_params(n, seed=seed), prec, tcfg=tc))
    root, dof, tau = fdr.case_states(family, robot["wmodel"], tc, n, seed)
    o.load(root, dof, tau)
    state = dict(root0=o.get("ROOT_STATES"), dof0=o.get("DOF_STATE"), tau=tau, body_params=o.get("BODY_PARAMS"))
    o.simulate()
    state.update(root1=o.get("ROOT_STATES"), dof1=o.get("DOF_STATE"), force_sensor=o.get("FORCE_SENSOR"),
                 net_contact_force=o.get("NET_CONTACT_FORCE"))
    return tc, state


def _worst_with(robot, family, tc, state, **kw):
    out = fdr.evaluate(robot["model"], robot["wmodel"], tc, family, **state, **kw)
    return float(out["ratio"][out["elig"]][:, LIVE].max()), out


def test_the_checker_can_fail(robot):
    """A wrong armature on one joint, a gripper mass off by 1 % and a limit stop whose D lacks the armature each put the fp64
    oracle's substep at least 10 x beyond the constant its family is held to."""
    tc, st = _one_case(robot, "airborne")
    good, _ = _worst_with(robot, "airborne", tc, st)
    assert good <= 1.0
    for j in (1, 8, 16):                                                   # a thigh, a calf, a wrist joint
        bad_tc = fdr.with_cfg(tc)
        bad_tc.joint_armature[j] = 0.0
        worst, out = _worst_with(robot, "airborne", bad_tc, st)
        print(f"armature of joint {j} zeroed: {worst:.4g} (row {int(np.nanargmax(np.nanmax(out['ratio'][:, LIVE], axis=0)))})")
        assert worst >= 10 * fdr.bound("airborne")
    bp = st["body_params"].copy()
    bp[:, 10] *= 1.01
    worst, _ = _worst_with(robot, "airborne", tc, dict(st, body_params=bp))
    print(f"gripper mass off by 1 %: {worst:.4g}")
    assert worst >= 10 * fdr.bound("airborne")
    tc, st = _one_case(robot, "limit")
    good, _ = _worst_with(robot, "limit", tc, st)
    worst, _ = _worst_with(robot, "limit", tc, st, limit_with_armature=False)
    print(f"limit stop's D without the armature: {worst:.4g} (with: {good:.3f})")
    assert good <= 1.0 and worst >= 10 * fdr.bound("limit")


def test_joint_inertia_reproduces_the_oracles_stop_torque(robot):
    """The oracle does not expose its articulated D, so D is read off its motion: one joint at rest 0.02 rad beyond a limit gets
    t_limit = -kappa D / dt^2 viol and nothing else; (ID + armature a - tau) on that row is t_limit, hence D. The subtree inverse
    gives the same number for every limited joint, on either side."""
    model, wm, tc = robot["model"], robot["wmodel"], robot["tcfg"]
    tb = fdr.tables(wm, tc)
    limited = [d for d in range(18) if tb["lo"][d] < tb["hi"][d]]
    n = 2 * len(limited)
    root, dof, tau = fdr.airborne_states(wm, tc, n, 301)
    viol = np.zeros(n)
    for e in range(n):
        d = limited[e // 2]
        viol[e] = 0.02 if e % 2 else -0.02
        dof[e, d, 0] = (tb["hi"][d] if e % 2 else tb["lo"][d]) + viol[e]
        dof[e, d, 1] = 0.0
    o = fdr.OracleAdapter(helpers.make_oracle(robot, n, helpers.random_env_params(n, seed=301), "f64"))
    o.load(root, dof, tau)
    r0, d0, bp = o.get("ROOT_STATES"), o.get("DOF_STATE"), o.get("BODY_PARAMS")
    o.simulate()
    r1, d1 = o.get("ROOT_STATES"), o.get("DOF_STATE")
    ok = fdr.eligible(wm, tc, d0, d1, o.get("NET_CONTACT_FORCE"), o.get("FORCE_SENSOR"), "limit")   # (a limb folded to its stop can touch another)
    assert {limited[e // 2] for e in np.flatnonzero(ok)} == set(limited) and ok.sum() >= n - 4
    worst = 0.0
    for e in np.flatnonzero(ok):
        d = limited[e // 2]
        v = d0[e, d, 0] - (tb["hi"][d] if e % 2 else tb["lo"][d])          # the violation of the float32 state
        a = (np.r_[r1[e, 0, 7:13], d1[e, :, 1]] - np.r_[r0[e, 0, 7:13], d0[e, :, 1]]) / tb["dt"]
        idt, _ = idr.inverse_dynamics(model, r0[e, 0, 0:3], r0[e, 0, 3:7], d0[e, :, 0], np.r_[r0[e, 0, 7:13], d0[e, :, 1]], a, bp[e],
                                      tb["gravity"])
        t_lim = (idt + tb["armature"] * a)[6 + d] - float(tau[e, d])
        D_oracle = -t_lim * tb["dt"] ** 2 / (tb["kappa"] * v)
        M = wb.mass_matrix(model, r0[e, 0, 0:3], r0[e, 0, 3:7], d0[e, :, 0], bp[e])
        D = fdr.joint_inertia(model, M, tb["armature"], d)
        worst = max(worst, abs(D / D_oracle - 1.0))
        assert abs(D / D_oracle - 1.0) < 1e-5, (e, d, D, D_oracle)
        assert abs(fdr.joint_inertia(model, M, tb["armature"], d, with_armature=False) / D_oracle - 1.0) > 1e-3
    print(f"joint inertia from the subtree inverse vs the oracle's stop torque: worst relative difference {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------- clamp
def _clamp_oracle(robot, prec):
    n = fdr.CLAMP_CASE["n"]
    return helpers.make_oracle(robot, n, helpers.random_env_params(n, seed=fdr.CLAMP_CASE["seed"]), prec)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_velocity_clamp_on_the_oracle(robot, prec):
    clamped, free, stored, limit, integ = fdr.clamp_check(fdr.OracleAdapter(_clamp_oracle(robot, prec)), robot["model"],
                                                          robot["wmodel"], robot["tcfg"])
    print(f"velocity clamp ({prec}): {int(clamped.sum())} joints of {int(clamped.any(1).sum())} envs predicted beyond the limit")
    assert clamped.sum() >= fdr.CLAMP_CASE["n"] and clamped[:, 12:18].any(0).sum() >= 4
    assert np.all(stored[clamped] == limit[clamped])                       # bit-exactly +-qd_limit
    bounded = free & (limit != 0)
    assert np.all(np.abs(stored[bounded]) < np.abs(limit[bounded]))
    assert integ.max() <= (1e-3 if prec == "f64" else fdr.K_REF["integrator"])
