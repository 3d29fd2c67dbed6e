"""The task logic of the HIP step kernel (everything after the substeps of wbc_step_kernel: compute_reward, base_reward_sums,
reward_accumulate, the air-time state, observe_and_store) held to the fp64 restatement of tests/task_logic_reference.py, term by
term, from the kernel's own stored post-state: |kernel - ref| <= C 2^-24 mag, the discontinuous pieces and every copy bit for bit.
Everything goes through the C-ABI (helpers.make_gpu) with per-env randomised body parameters. The cases, seeds and states are
those tests/test_task_logic.py runs through the C oracle on the CPU, at n = 13 (the grid is rounded up to 8), 256 and -- case A
and the totals -- 2560 (the envs are dealt to the XCDs from 2048 on; every tenth env plus the last is checked).

Constants: C = 4 x K_ref rounded up to a power of two, K_ref the fp32 ORACLE's largest ratio per tier (measured and asserted on
the CPU by tests/test_task_logic.py, never taken from the kernel); at least 8 where the tier passes through a transcendental.

    tier                                   K_ref    C    kernel's largest ratio on an MI355X
    1 polynomial terms, metrics, air time   2.72   16    2.54   terms n = 256, step 2, env 185: torques
    2 terms through exp                     0.65    8    0.77   terms n = 256, step 2, env 18: tracking_ang_vel_yaw_exp
    3 terms through angles                  0.33    8    0.40   terms n = 2560, step 0, env 2390: metric source of tracking_ee_orn_ry
    4 totals and episode sums               1.00    4    1.21   totals n = 2560, env 1450: EPISODE_SUMS[tracking_lin_vel_z_l2]
    5 scaled observation entries            0.95    4    0.95   termination n = 256, env 232: entry 41 (0.5 ulp)
    6 Euler observation entries             0.56    8    0.71   terms-cart n = 256, step 0, env 117: roll

Both reward totals stay inside the scale-weighted bounds of their terms (ratio 0 beyond them) at every n; every exact comparison
(flags, copies, privileged block, history blocks, the termination case) holds bit for bit.
"""
import numpy as np
import pytest

import forward_dynamics_reference as fdr
import helpers
import task_logic_reference as tl
from wbc_amd import abi

pytestmark = pytest.mark.gpu

TERM = tl.TERM
WORST = {}           # tier -> (ratio, case, n, step, env, what): the kernel's largest ratios, printed by the last test


class GpuAdapter:
    """WbcSim (the C-ABI) behind the get / set / step interface of task_logic_reference.run_steps."""

    def __init__(self, g):
        import torch
        self.g, self.torch = g, torch

    def get(self, name):
        self.torch.cuda.synchronize()
        return self.g.tensor(name).detach().cpu().numpy().astype(np.float64)

    def set(self, name, value):
        t = self.g.tensor(name)
        v = np.array(np.broadcast_to(np.asarray(value, dtype=np.float64), tuple(t.shape)))
        t.copy_(self.torch.from_numpy(v).to(t.dtype))

    def step(self, a):
        self.g.step(self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda())

    def set_curriculum(self, c):
        self.g.set_curriculum(c)

    def set_heightfield(self, *a):
        self.g.set_heightfield(*a)

    def set_step_counter(self, v):
        self.g.step_counter = v


@pytest.fixture(scope="module")
def runs(robot):
    """(case name, n) -> the case with its steps on the GPU, each run once."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            sims = []

            def mk(tc, n):
                params = helpers.random_env_params(n, seed=tl.PARAM_SEED)
                g = helpers.make_gpu(robot, n, params, tcfg=tc)
                sims.append(g)
                sim = GpuAdapter(g)
                bp = sim.get("BODY_PARAMS")
                assert np.ptp(bp[:, 0]) > 0 and np.ptp(bp[:, 10]) > 0                  # randomised per env
                return sim
            cache[name, n] = tl.run_case(mk, robot, name, n)
            for g in sims:
                g.close()
        return cache[name, n]
    return get


def _upd(tier, r, case, n, step, env, what):
    if tier not in WORST or r > WORST[tier][0]:
        WORST[tier] = (float(r), case, n, step, env, what)


def _check_terms(c, name, n):
    """Every step of a unit-curriculum case: terms, metric sources, air-time state within C; the flags exact."""
    C = tl.term_bounds()
    envs = fdr.step_envs(n)
    results = []
    for i, (pre, post, a) in enumerate(c["steps"]):
        res = tl.check_terms(c["tb"], c["cur"], pre, post, envs=envs)
        results.append(res)
        for tier, (r, env, what) in tl.tier_maxima(res).items():
            print(f"{name} n = {n} step {i}: tier {tier}: largest ratio {r:.3f} (env {env}, {what})")
            _upd(tier, r, name, n, i, env, what)
        assert res["lc_equal"], (name, i)
        bad = np.argwhere(np.nan_to_num(res["ratio"], nan=0.0) > C[None])
        assert bad.size == 0, (f"{name} n = {n} step {i}: {len(bad)} terms beyond C: " +
                               "; ".join(f"env {envs[e]} {abi.REWARD_TERMS[t]}: {res['ratio'][e, t]:.1f} (C = {C[t]:.0f})" for e, t in bad[:8]))
        mC = np.array([tl.bound(t) for t in tl.MET_TIER])
        bad = np.argwhere(np.nan_to_num(res["met_ratio"], nan=0.0) > mC[None])
        assert bad.size == 0, (name, i, [(envs[e], abi.METRIC_NAMES[m], float(res["met_ratio"][e, m])) for e, m in bad[:8]])
        assert np.nanmax(res["air_ratio"]) <= tl.bound("poly"), (name, i, float(np.nanmax(res["air_ratio"])))
    return results


@pytest.mark.parametrize("n", [13, 256, 2560])
def test_reward_terms(runs, n):
    """Case A: all 37 raw terms, the 10 metric sources and the air-time state over three consecutive steps on the stairs, each
    from the kernel's own state; at n >= 256 the coverage conditions hold on the KERNEL's output."""
    c = runs("terms", n)
    results = _check_terms(c, "terms", n)
    if n >= 256:
        cov = tl.conditions(c["tb"], c["steps"], results)
        print(f"terms n = {n}: {cov['steps']} env-steps, {cov['resets']} lost to resets, two-valued {cov['two_valued']}, "
              f"near a threshold {int(cov['near'].sum())}")
        tl.assert_conditions("terms", cov)


@pytest.mark.parametrize("n", [13, 256])
def test_reward_terms_cart_mode(runs, n):
    """Case B: goal_command_cart = 1, non-zero goal_delta_orn_range, goal timers on both sides of t = 0.5, goals resampled."""
    c = runs("terms-cart", n)
    results = _check_terms(c, "terms-cart", n)
    if n >= 256:
        tl.assert_conditions("terms-cart", tl.conditions(c["tb"], c["steps"], results))
        g0, g1 = c["state"]["GOAL_STATE"], c["steps"][0][1]["GOAL_STATE"]
        due = g0[:, tl.G_TIMER] + 1 > g0[:, tl.G_TOTAL]
        assert due.sum() >= 8 and np.all(g1[due, tl.G_TIMER] == 0) and np.all(g1[~due, tl.G_TIMER] == g0[~due, tl.G_TIMER] + 1)


@pytest.mark.parametrize("n", [13, 256])
def test_air_time_state_rests_while_the_term_is_off(runs, n):
    """Case C: FEET_AIR_TIME / LAST_CONTACTS bit-identical, every other term as in case A (same kernel, same states: bit for bit)."""
    a, c = runs("terms", n), runs("air-time-off", n)
    _check_terms(c, "air-time-off", n)
    others = [t for t in range(abi.NREW) if t != TERM["feet_air_time"]]
    for (_, pa, _), (_, pc, _) in zip(a["steps"], c["steps"]):
        assert np.array_equal(pc["FEET_AIR_TIME"], c["state"]["FEET_AIR_TIME"]) and np.array_equal(pc["LAST_CONTACTS"], c["state"]["LAST_CONTACTS"])
        assert np.array_equal(pc["EPISODE_SUMS"][:, others], pa["EPISODE_SUMS"][:, others])
        assert np.all(pc["EPISODE_SUMS"][:, TERM["feet_air_time"]] == 0) and np.array_equal(pc["METRIC_SUMS"], pa["METRIC_SUMS"])
    assert any((pa["FEET_AIR_TIME"] != a["state"]["FEET_AIR_TIME"]).any() for _, pa, _ in a["steps"])


@pytest.mark.parametrize("n", [13, 256, 2560])
@pytest.mark.parametrize("name", ["totals-positive", "totals-raw"])
def test_reward_totals(runs, name, n):
    """Case D: mixed-sign scales on both channels, eight terms in both lists, EPISODE_SUMS from non-zero values; with and without
    only_positive_rewards. Bound: the scale-weighted sum of the terms' bounds + C 2^-24 sum |scale term|, / 100."""
    c = runs(name, n)
    envs = fdr.step_envs(n)
    pre, post, _ = c["steps"][0]
    res = tl.check_totals(c["tb"], c["cur"], pre, post, envs=envs)
    for r, what in ((res["ratio"], "reward totals"), (res["sums_ratio"], "EPISODE_SUMS")):
        z = np.nan_to_num(r, nan=0.0)
        e, k = np.unravel_index(np.argmax(z), z.shape)
        print(f"{name} n = {n}: {what}: largest ratio {z[e, k]:.3f} (env {envs[e]}, column {k})")
        _upd("totals", z[e, k], name, n, 0, envs[e], f"{what}[{k}]")
        assert z.max() <= tl.bound("totals"), (name, what, envs[e], k, float(z[e, k]))
    assert res["alive"].mean() >= 0.95 and np.all(np.isnan(res["ratio"]).mean(0) <= 0.05)
    if name == "totals-positive":
        got = np.stack([post["REW_BUF"][envs], post["ARM_REW_BUF"][envs]], 1)
        ok = ~np.isnan(res["ratio"])
        assert np.all((got == 0)[ok] == res["clipped"][ok]) and got.min() >= 0
        if n >= 256:
            frac = res["clipped"][res["alive"]].mean(0)
            assert np.all(frac >= 0.25) and np.all(frac <= 0.75), frac
    else:
        assert (post["REW_BUF"][envs] < 0).sum() >= len(envs) // 4


@pytest.mark.parametrize("n", [13, 256])
def test_termination_case(runs, n):
    """Case E: only survive and termination, on both channels, the clip biting on the arm channel; envs forced below the height
    threshold, past the roll threshold with either goal sign, onto the time-out. Exact inputs: both totals, the two slots' sums
    (moved to EPISODE_SUMS_DONE by the reset) and the zeroed EPISODE_SUMS bit for bit against float32 arithmetic written out."""
    c = runs("termination", n)
    pre, post, _ = c["steps"][0]
    kind = c["kind"]
    reset, tout = post["RESET_BUF"] != 0, post["TIME_OUT_BUF"] != 0
    assert np.array_equal(reset, np.isin(kind, [0, 1, 3])) and np.array_equal(tout, kind == 3)
    ex = tl.termination_expected(c["tb"], c["cur"], pre, post)
    got = dict(REW_BUF=post["REW_BUF"], ARM_REW_BUF=post["ARM_REW_BUF"],
               survive_sum=np.where(reset, post["EPISODE_SUMS_DONE"][:, TERM["survive"]], post["EPISODE_SUMS"][:, TERM["survive"]]),
               termination_sum=np.where(reset, post["EPISODE_SUMS_DONE"][:, TERM["termination"]], post["EPISODE_SUMS"][:, TERM["termination"]]))
    for k, v in got.items():
        assert np.array_equal(v, ex[k]), (k, np.flatnonzero(v != ex[k])[:8], v[v != ex[k]][:4], ex[k][v != ex[k]][:4])
    assert np.all(post["EPISODE_SUMS"][reset] == 0)
    assert (ex["ARM_REW_BUF"] == 0).sum() >= n // 4 and (ex["ARM_REW_BUF"] > 0).sum() >= n // 8 and (ex["REW_BUF"] < 0).sum() >= n // 8
    for kw in (dict(termination_before_clip=True), dict(arm_first=True)):          # the case tells the wrong orders apart
        w = tl.termination_expected(c["tb"], c["cur"], pre, post, **kw)
        assert any((w[k] != got[k]).any() for k in got), kw


@pytest.mark.parametrize("n", [13, 256])
@pytest.mark.parametrize("name", ["terms", "terms-cart", "termination", "obs-tilted", "obs-clip"])
def test_observations(runs, name, n):
    """Case F: the 76 proprioceptive entries from the stored state (copies, constants and flags bit for bit, scaled entries to 2
    ulp, roll / pitch and the wrapped DoF to their mag), the privileged block, the clipped old history in OBS_BUF and the new
    OBS_HISTORY (refilled at the first step of an episode, shifted otherwise) bit for bit; reset envs included."""
    c = runs(name, n)
    for i, (pre, post, a) in enumerate(c["steps"]):
        ob = tl.check_observation(c["tb"], pre, post, a)
        print(f"{name} n = {n} step {i}: scaled entries {ob['ulp']:.2f} ulp, ratio {ob['ratio_scaled'][0]:.3f} (env {ob['ratio_scaled'][1]}, entry "
              f"{ob['ratio_scaled'][2]}); roll / pitch ratio {ob['ratio_euler'][0]:.3f} (env {ob['ratio_euler'][1]}, entry {ob['ratio_euler'][2]}); "
              f"{ob['resets']} resets, {ob['refills']} refills, {ob['near']} flags at the threshold, at the clip {ob['clipped']}")
        _upd("obs_scaled", ob["ratio_scaled"][0], name, n, i, ob["ratio_scaled"][1], f"entry {ob['ratio_scaled'][2]}")
        _upd("obs_euler", ob["ratio_euler"][0], name, n, i, ob["ratio_euler"][1], f"entry {ob['ratio_euler'][2]}")
        assert not ob["exact_bad"], ob["exact_bad"]
        assert ob["ulp"] <= 2.0
        assert ob["ratio_scaled"][0] <= tl.bound("obs_scaled") and ob["ratio_euler"][0] <= tl.bound("obs_euler")
        assert ob["near"] <= 0.02 * 4 * n
        if name == "termination":
            assert ob["resets"] >= n // 4 and ob["refills"] >= ob["resets"]
            r0, p0, _ = tl.euler_from_quat(c["tb"]["init_quat"][None])
            assert np.all(np.abs(ob["roll_pitch"][post["RESET_BUF"] != 0] - np.array([r0.v[0], p0.v[0]])) <= 1e-6)
        if name.startswith("obs-"):
            rp = ob["roll_pitch"]
            assert np.abs(rp).max(0).min() >= 1.3
            for sr in (-1, 1):
                for sp in (-1, 1):
                    assert ((sr * rp[:, 0] > 1.0) & (sp * rp[:, 1] > 1.0)).sum() >= 1
        if name == "obs-clip":
            assert min(ob["clipped"]) >= 8 and ob["over"] == [0, 0, 0]
        else:
            assert ob["over"] == [0, 0, 0] and ob["clipped"] == [0, 0, 0]


def test_print_the_kernels_largest_ratios():
    """The table for the module docstring and DESIGN.md section 4 (run after the tests above: they fill it)."""
    print("kernel's largest ratio per tier:")
    for tier in tl.TIERS:
        if tier in WORST:
            r, case, n, step, env, what = WORST[tier]
            print(f"  {tier:11s} {r:7.3f}   K_ref {tl.K_REF[tier]:5.2f}   C {tl.bound(tier):3.0f}   ({case} n = {n} step {step} env {env} {what})")
            assert r <= tl.bound(tier)
