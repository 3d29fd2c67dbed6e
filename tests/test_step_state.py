"""What produces the inputs of the step's task logic -- the rigid-body pass, the base-frame velocities, the action path with its PD
torques, the goal machine and the random events -- against the fp64 restatement of tests/step_state_reference.py, on the CPU: pins
the checker to the C oracle in both precisions and measures the constants tests/test_gpu_step_state.py holds the HIP kernels to.
Every case runs through OracleSim(precision="f64") and ("f32") at the sizes the GPU test runs it at (n = 13 and 256, the events case
at 2048 as well; the delay and all-collide cases at 13), same seeds.

  * fp64 oracle: every ratio |sim - ref| / (2^-24 mag) stays below 1e-6 (observed: <= 6.1e-9); every exact comparison holds.
  * fp32 oracle: its largest ratio per tier is K_ref, asserted against step_state_reference.K_REF (not above it, not below 80 % of it):

        tier                                          K_ref    C = 4 K_ref rounded up to 2^k (floor 8 through a transcendental)
        rigid-body positions                           2.00     8    (events, third step, env 125: ee_gripper_link x)
        rigid-body quaternions                         4.17    32    (resets, env 179: gripper_link qw)
        rigid-body linear / angular velocities         2.69    16    (resets, env 194: RL_calf vx)
        BASE_LIN_VEL / BASE_ANG_VEL                    1.36     8    (resets, env 233: BASE_LIN_VEL[1])
        PD torques                                     0.68     4    (action_delay 1, n = 13, env 5: DoF 6)
        goal values through sin / cos / atan2          0.48     8    (reset_all, env 206: G_GOAL_CART[2])
        goal values by lerp                            0.94     4    (events n = 2048, third step, env 290: G_CURR[0])
        RESET_TRAVEL                                   0.62     4    (resets, env 24: the command's norm)

  * the counter RNG restated in numpy equals the oracle's draws bit for bit (a config whose ranges hand the draws out unscaled).
  * the recorded fixtures (tests/golden): an env that reset in a step keeps the rigid-body rows and base velocities of the refresh
    before the reset -- what check_step_kinematics asserts of the oracle and of the kernel.
  * the exclusion rule: at most 2 % of the events of a case left out at a threshold (fp64 oracle); the coverage counts of the cases.
  * the checker can fail: fourteen seeded errors, each rejected by 10 x C or by an exact mismatch. The 3e-4 / 5e-4 bound the same
    tensors were held to before lets the 4 um rb_offset error through (asserted). It does NOT let a dropped `w x offset` or a flipped
    half-angle sign through on these states (errors of 1 m/s and 1 in a quaternion component; measured and asserted as such), nor on
    the states the earlier tests ran -- except that with every velocity zero a dropped `w x offset` is no error at all.
  * a NaN in any output is rejected, never counted as an entry left out."""
import numpy as np
import pytest

import helpers
import step_state_reference as ss
import task_logic_reference as tl
from wbc_amd import abi

N = 256


@pytest.fixture(scope="module")
def runs(robot):
    """(precision, case name) -> the case, each computed once. "fk" and "reset_all" are the two cases without a step."""
    cache = {}

    def get(prec, name, n=N):
        if (prec, name, n) not in cache:
            mk = lambda tc, m: ss.OracleAdapter(helpers.make_oracle(robot, m, helpers.random_env_params(m, seed=ss.PARAM_SEED), prec, tcfg=tc))
            if name == "fk":
                cache[prec, name, n] = ss.run_fk(mk, robot, n)
            elif name == "reset_all":
                cache[prec, name, n] = ss.run_reset_all(mk, robot, n)
            else:
                cache[prec, name, n] = ss.run_case(mk, robot, name, n)
        return cache[prec, name, n]
    return get


def everything(runs, prec):
    """(Worst per tier, exact mismatches, counts per case at n = 256) of every case at every size the GPU test runs it at."""
    worst, bad, counts = ss.Worst(), [], {}
    for n in (13, N):
        ss.check_fk_case(runs(prec, "fk", n), n, worst, bad)
        counts["reset_all"] = ss.check_reset_all_case(runs(prec, "reset_all", n), n, worst, bad)
        for name in ("events", "resets"):
            c = runs(prec, name, n)
            counts[name + "-kin"] = ss.check_step_kinematics(c, n, name, worst, bad)
            counts[name] = ss.check_case_events(c, n, name, worst, bad)
        counts["torques"] = ss.check_torque_case(runs(prec, "torques", n), n, "torques", worst, bad)
    c = runs(prec, "events", 2048)                              # (the deal path's size: every tenth env plus the last)
    ss.check_step_kinematics(c, 2048, "events", worst, bad)
    counts["events-2048"] = ss.check_case_events(c, 2048, "events", worst, bad)
    counts["all-collide"] = ss.check_case_events(runs(prec, "all-collide", 13), 13, "all-collide", worst, bad)
    for d in ss.DELAYS:
        counts[f"torques-delay{d}"] = ss.check_torque_case(runs(prec, f"torques-delay{d}", 13), 13, f"torques-delay{d}", worst, bad)
    return worst, bad, counts


@pytest.fixture(scope="module")
def checked(runs):
    cache = {}

    def get(prec):
        if prec not in cache:
            cache[prec] = everything(runs, prec)
        return cache[prec]
    return get


def test_f64_oracle_is_the_restatement(checked):
    worst, bad, _ = checked("f64")
    print("fp64 oracle, largest ratio per tier:", {t: f"{worst.get(t)[0]:.2e} ({worst.get(t)[1]})" for t in ss.TIERS})
    assert not bad, bad[:8]
    for t in ss.TIERS:
        assert worst.get(t)[0] <= 1e-6, (t, worst.get(t))


def test_k_ref_of_every_tier(checked):
    """The fp32 oracle's largest ratios: printed, and asserted against the committed K_REF (not above it; not below 80 % of it, so
    that a committed constant cannot be looser than what was measured). Its exact comparisons hold as the fp64 oracle's do."""
    worst, bad, _ = checked("f32")
    print("K_ref (fp32 oracle):")
    for t in ss.TIERS:
        print(f"  {t:10s} {worst.get(t)[0]:6.3f}   C = {ss.bound(t):4.0f}   ({worst.get(t)[1]})")
    assert not bad, bad[:8]
    for t in ss.TIERS:
        r = worst.get(t)[0]
        assert 0.8 * ss.K_REF[t] <= r <= ss.K_REF[t], (t, worst.get(t), ss.K_REF[t])
        assert ss.bound(t) >= ss.TIER_FLOOR[t] and ss.bound(t) >= 4 * r


def test_the_restated_rng_is_the_oracles(robot):
    """mix64 / rng_u01 in numpy against the oracle's draws, bit for bit: a config whose ranges are [0, 1] (or [-0.5, 0.5]) hands the
    draws out unscaled -- G_DORN (slots 0-2 / 67-69), the first goal candidate (3-5 / 70-72; nothing collides), COMMANDS (33-34 /
    65-66), the push (35-36), the reset's root velocity (59-64) and its DoF positions (37-56, default_dof_pos x u: the same fp64
    product) -- for every env, through reset_all and two steps."""
    n = 64
    tc = tl.alive_cfg(robot, goal_delta_orn_range=[[0.0, 1.0]] * 3, init_vel_perturb_range=0.5, max_push_vel=0.5, push_interval=1,
                      resample_interval=1, lin_vel_x_clip=-1.0, goal_underground_limit=-10.0, dof_reset_lo=0.0, dof_reset_hi=1.0)
    abi._set(tc.goal_collision_lower, [0.0, 0.0, 0.0])
    abi._set(tc.goal_collision_upper, [0.0, 0.0, 0.0])
    cur = ss.zero_curriculum(robot)
    for name in ("lin_vel_x_range", "ang_vel_yaw_range", "goal_l_range", "goal_p_range", "goal_y_range"):
        abi._set(getattr(cur, name), [0.0, 1.0])
    o = helpers.make_oracle(robot, n, helpers.random_env_params(n, seed=ss.PARAM_SEED), "f64", tcfg=tc)
    o.set_curriculum(cur)
    envs = np.arange(n)
    o.step_counter = 5
    o.reset_all()
    g, root, dof = o.get("GOAL_STATE"), o.get("ROOT_STATES"), o.get("DOF_STATE")
    assert np.array_equal(g[:, ss.G_DORN:ss.G_DORN + 3], ss.draws(envs, 5, ss.SLOT["RESET_GOAL_ORN"], 3))
    assert np.array_equal(g[:, ss.G_GOAL:ss.G_GOAL + 3], ss.draws(envs, 5, ss.SLOT["RESET_GOAL_SPHERE"], 3))
    assert np.array_equal(o.get("COMMANDS")[:, [0, 2]], ss.draws(envs, 5, ss.SLOT["RESET_CMD"], 2))
    assert np.array_equal(root[:, 0, 7:13], ss.draws(envs, 5, ss.SLOT["RESET_VEL"], 6) - 0.5)
    default = np.array([float(x) for x in tc.default_dof_pos])
    assert np.array_equal(dof[:, :, 0], default[None] * ss.draws(envs, 5, ss.SLOT["RESET_DOF"], abi.NDOF))
    for step in (6, 7):
        g = o.get("GOAL_STATE")
        g[:, ss.G_TIMER] = g[:, ss.G_TOTAL]
        o.set("GOAL_STATE", g)
        o.step(np.zeros((n, 18)))
        assert o.step_counter == step and not o.get("RESET_BUF").any()
        g = o.get("GOAL_STATE")
        assert np.array_equal(g[:, ss.G_DORN:ss.G_DORN + 3], ss.draws(envs, step, ss.SLOT["GOAL_ORN"], 3))
        assert np.array_equal(g[:, ss.G_GOAL:ss.G_GOAL + 3], ss.draws(envs, step, ss.SLOT["GOAL_SPHERE"], 3))
        assert np.array_equal(o.get("COMMANDS")[:, [0, 2]], ss.draws(envs, step, ss.SLOT["CMD"], 2))
        assert np.array_equal(o.get("ROOT_STATES")[:, 0, 7:9], ss.draws(envs, step, ss.SLOT["PUSH"], 2) - 0.5)
    assert len(np.unique(ss.draws(envs, 6, 0, 37))) > 0.99 * n * 37


def test_quaternion_chain_and_rotation_matrices_agree(robot):
    """Two algebras for one quantity: the rotation matrix of the fp64 quaternion product down the chain is arm_osc_oracle.fk's."""
    import arm_osc_oracle as ao
    bt = ss.body_tables(robot["model"], robot["wmodel"])
    rng = np.random.default_rng(3)
    for _ in range(32):
        rq, q = helpers.random_quat(rng), rng.uniform(-np.pi, np.pi, abi.NDOF)
        R, _ = ao.fk(bt["model"], np.zeros(3), rq, q)
        Q = ss.quat_chain(bt["model"], rq, q)
        assert max(np.abs(ao.quat_to_mat(Q[b]) - R[b]).max() for b in range(bt["model"].nb)) <= 1e-12


def test_exclusion_cap_and_coverage(checked):
    """On the fp64 oracle: at most 2 % of the events of a case left out at a threshold (band 1e-5); the coverage counts."""
    _, _, counts = checked("f64")
    for name in ("events", "resets", "all-collide", "reset_all"):
        t = counts[name]
        share = ss.excluded_share(t)
        print(f"{name}: {t['goal_events']} goal resamples ({t['goal_uncertain']} uncertain, {t['first_rejected']} with the first candidate rejected, "
              f"picks {sorted(set(t['picks']))}), commands kept / zeroed / near {t['cmd_keep']} / {t['cmd_zero']} / {t['cmd_near']}, "
              f"pushes x1 / x2.5 {t.get('push_1', 0)} / {t.get('push_25', 0)}, resets {t['resets']}; left out {share:.4f}")
        assert share <= 0.02, (name, share)
    ss.assert_event_coverage(counts["events"], N)
    ss.assert_event_coverage(counts["events-2048"], 2048)
    assert set(counts["all-collide"]["picks"]) == {9} and counts["all-collide"]["goal_events"] == 13
    r = counts["resets"]
    assert r["resets"] > N // 3 and r["time_outs"] >= N // 8 and r["falls"] >= N // 8 and r["both"] == 0
    assert counts["reset_all"]["cmd_keep"] >= 8 and counts["reset_all"]["cmd_zero"] >= 8
    tq = counts["torques"]
    print("torques:", tq)
    assert tq["clamped"] >= 64 and tq["free"] >= 64 and tq["clipped"] >= 64 and tq["near"] <= 0.02 * (tq["clamped"] + tq["free"])
    assert counts["events-kin"] >= 0.9 * 3 * N and counts["resets-kin"] < 2 * N // 3


# ------------------------------------------------------------------------------------------------------- the checker can fail
def _old_bound_passes(got, val):
    return bool(np.all(np.abs(got - val) <= ss.OLD_ATOL + ss.OLD_RTOL * np.abs(val)))


def _fk_mutation(c, **wrong):
    """(largest ratio per tier of the fp64 oracle's rows against the WRONG restatement, old bound passes)."""
    worst, bad = ss.Worst(), []
    ss.check_fk_case(c, N, worst, bad, **wrong)
    vals = np.array([ss.rigid_body_reference(c["bt"], c["root"][e, 0], c["dof"][e, :, 0], c["dof"][e, :, 1], **wrong)[0] for e in range(N)])
    return worst, _old_bound_passes(c["rb"][:, :abi.NRB], vals)


def test_seeded_kinematics_errors_are_rejected(runs):
    """(1) rb_offset of the gripper body off by 4 um, (2) w x offset dropped from the linear velocity, (3) one joint's half-angle sine
    with the wrong sign, (4) body velocities rotated by R^T instead of R: each beyond 10 x C. The old 3e-4 / 5e-4 bound passes (1);
    (2) and (3) are errors of order 1 on these states (|w| 0.2 m and sin(q / 2)) and do not pass it."""
    c = runs("f64", "fk")
    w, old = _fk_mutation(c)
    assert all(w.get(t)[0] <= 1e-6 for t in ("pos", "quat", "vel")) and old
    for wrong, tier, old_passes in ((dict(offset_error=4e-6), "pos", True), (dict(drop_w_cross_offset=True), "vel", False),
                                    (dict(flip_dof=13), "quat", False), (dict(rotate_by_RT=True), "vel", False)):
        w, old = _fk_mutation(c, **wrong)
        print(wrong, {t: f"{w.get(t)[0]:.3g}" for t in ("pos", "quat", "vel")}, "old bound passes:", old)
        assert w.get(tier)[0] >= 10 * ss.bound(tier), (wrong, w.get(tier))
        assert old == old_passes, (wrong, old)


def test_seeded_kinematics_errors_on_the_earlier_tests_states(robot):
    """Why the suite could not see them before. The states the rigid-body pass met in tests/test_gpu_sim_parity.py were (a)
    helpers.random_standing_state (+-0.25 rad about the default pose, |w_root| <= 1 rad/s), held at 2e-5 / 1e-5 through wbc_fk_kernel
    and at 3e-4 / 5e-4 through the step, and (b) the same with every velocity zero (the box-placement refreshes). Measured on the fp64
    oracle's rows: the 4 um rb_offset error passes both bounds on both families; a dropped w x offset is no error at all on (b) --
    there the new checker cannot see it either, which is what the velocity family of fk_states is for -- and an error of up to
    0.3 m/s on (a), which both old bounds reject; a flipped half-angle sign is rejected wherever the joint is not at 0."""
    n = 32
    mk = lambda tc, m: ss.OracleAdapter(helpers.make_oracle(robot, m, helpers.random_env_params(m, seed=ss.PARAM_SEED), "f64", tcfg=tc))
    root, dof = helpers.random_standing_state(n, robot["tcfg"], np.random.default_rng(4))
    rest = (root.copy(), dof.copy())
    rest[0][:, 0, 7:], rest[1][:, :, 1] = 0, 0
    passes = {}
    for fam, states in (("a", (root, dof)), ("b", rest)):
        c = ss.run_fk(mk, robot, n, states=states)
        for name, wrong in (("offset", dict(offset_error=4e-6)), ("w x offset", dict(drop_w_cross_offset=True)), ("half angle", dict(flip_dof=13))):
            val = np.array([ss.rigid_body_reference(c["bt"], c["root"][e, 0], c["dof"][e, :, 0], c["dof"][e, :, 1], **wrong)[0] for e in range(n)])
            err = np.abs(c["rb"][:, :abi.NRB] - val)
            passes[fam, name] = (bool(np.all(err <= 2e-5 + 1e-5 * np.abs(val))), bool(np.all(err <= ss.OLD_ATOL + ss.OLD_RTOL * np.abs(val))), float(err.max()))
    print(passes)
    assert passes["a", "offset"][:2] == (True, True) and passes["b", "offset"][:2] == (True, True)
    assert passes["b", "w x offset"][2] <= 1e-12 and passes["a", "w x offset"][:2] == (False, False)
    assert passes["a", "half angle"][:2] == (False, False) and passes["b", "half angle"][:2] == (False, False)


def test_non_finite_outputs_are_rejected(runs):
    """A NaN in anything the checker reads is an error, never an entry left out: through the ratios (inf), the bounded comparisons
    and the exact ones, in each of the three entry points' cases."""
    import copy
    c = copy.deepcopy(runs("f64", "fk"))
    c["rb"][:, :abi.NRB] = np.nan
    worst, bad = ss.Worst(), []
    ss.check_fk_case(c, N, worst, bad)
    assert all(worst.get(t)[0] >= 10 * ss.bound(t) for t in ("pos", "quat", "vel")), worst.w
    c = copy.deepcopy(runs("f64", "fk"))
    c["rb"][5, abi.NRB, 2] = np.nan
    worst, bad = ss.Worst(), []
    ss.check_fk_case(c, N, worst, bad)
    assert any("box row" in b for b in bad)
    for name, sl, hit in (("COMMANDS", np.s_[:, 0], "COMMANDS"), ("ROOT_STATES", np.s_[:, 0, 7:13], "reset root velocity"), ("DOF_STATE", np.s_[:, :, 0], "reset DoF positions"),
                          ("GOAL_STATE", np.s_[:, ss.G_GOAL:ss.G_GOAL + 3], "picked candidate"), ("GOAL_STATE", np.s_[:, ss.G_DORN], "G_DORN"),
                          ("GOAL_STATE", np.s_[:, ss.G_GOAL_CART], "goal_trig"), ("GOAL_STATE", np.s_[:, ss.G_ORN + 2], "goal_trig"),
                          ("RESET_TRAVEL", np.s_[:, 0], "travel"), ("RIGID_BODY_STATE", np.s_[:, 3, 4], "quat")):
        c = copy.deepcopy(runs("f64", "reset_all"))
        c["post"][name][sl] = np.nan
        worst, bad = ss.Worst(), []
        ss.check_reset_all_case(c, N, worst, bad)
        assert (worst.get(hit)[0] >= 10 * ss.bound(hit)) if hit in ss.TIERS else any(hit in b for b in bad), (name, hit, bad[:3], worst.w)
    for case, name, sl, hit in (("events", "BASE_LIN_VEL", np.s_[:, 1], "base_vel"), ("events", "RIGID_BODY_STATE", np.s_[:, 9, 8], "vel"),
                                ("events", "GOAL_STATE", np.s_[:, ss.G_CURR], "goal_lerp"), ("events", "GOAL_STATE", np.s_[:, ss.G_CURR_CART + 1], "goal_trig"),
                                ("events", "GOAL_STATE", np.s_[:, ss.G_TIMER], "goal timer"), ("events", "COMMANDS", np.s_[:, 2], "COMMANDS"),
                                ("events", "ROOT_STATES", np.s_[:, 0, 7], "pushed root velocity"), ("torques", "TORQUES", np.s_[:, 4], "torque"),
                                ("torques", "ACTIONS", np.s_[:, 4], "ACTIONS"), ("resets", "RESET_TRAVEL", np.s_[:, 1], "travel")):
        c = copy.deepcopy(runs("f64", case))
        for pre, post, a, step in c["steps"]:
            post[name][sl] = np.nan
        worst, bad = ss.Worst(), []
        if case == "torques":
            ss.check_torque_case(c, N, case, worst, bad)
        else:
            ss.check_step_kinematics(c, N, case, worst, bad)
            ss.check_case_events(c, N, case, worst, bad)
        assert (worst.get(hit)[0] >= 10 * ss.bound(hit)) if hit in ss.TIERS else any(hit in b for b in bad), (case, name, hit, bad[:3], worst.w)


def test_seeded_action_path_errors_are_rejected(runs):
    """(5) the motor strength left out, (6) the Q2 wrap on column WBC_NDOF - 8, (7) FL and FR not swapped, (8) the FIFO read one row
    late: beyond 10 x C in the torques, or an exact mismatch."""
    c = runs("f64", "torques")
    for wrong in (dict(no_motor=True), dict(q2_dof=abi.NDOF - 8), dict(no_leg_swap=True), dict(fifo_late=True)):
        worst, bad = ss.Worst(), []
        ss.check_torque_case(c, N, "torques", worst, bad, **wrong)
        print(wrong, f"{worst.get('torque')[0]:.3g}", len(bad))
        if "no_leg_swap" in wrong:                              # (delay 2: the newest row reaches the torques two steps later, as a row the sim stored itself)
            assert any("ACTION_HISTORY" in b for b in bad), bad[:4]
            continue
        assert worst.get("torque")[0] >= 10 * ss.bound("torque"), (wrong, worst.get("torque"))
        assert bool(bad) == ("fifo_late" in wrong), bad[:4]
    c0 = runs("f64", "torques-delay0", 13)                           # delay 0: the unswapped legs reach the torques in the same step
    worst, bad = ss.Worst(), []
    ss.check_torque_case(c0, 13, "torques-delay0", worst, bad, no_leg_swap=True)
    assert worst.get("torque")[0] >= 10 * ss.bound("torque") and bad
    d = runs("f64", "torques-delay-1", 13)                          # without the FIFO the history rests and the newest action is used
    assert np.array_equal(d["steps"][0][1]["ACTION_HISTORY"], d["steps"][0][0]["ACTION_HISTORY"])


def test_seeded_event_errors_are_rejected(runs):
    """(9) the lerp evaluated with timer + 1, (10) >= for > on the goal timer, (11) the draws shifted by one slot, (12) the pick off by
    one (the ninth for the tenth in the all-collide case), (13) commands resampled on a non-time-out reset, (14) the push factor
    applied before the command update."""
    def run(name, n, **wrong):
        worst, bad = ss.Worst(), []
        ss.check_case_events(runs("f64", name, n), n, name, worst, bad, **wrong)
        return worst, bad
    w, bad = run("events", N, lerp_timer_plus_one=True)
    assert w.get("goal_lerp")[0] >= 10 * ss.bound("goal_lerp"), w.get("goal_lerp")
    for name, n, wrong, what in (("events", N, dict(timer_ge=True), "goal timer"), ("events", N, dict(slot_shift=1), "picked candidate"),
                                 ("events", N, dict(slot_shift=1), "COMMANDS"), ("events", N, dict(slot_shift=1), "pushed root velocity"),
                                 ("events", N, dict(pick_off=True), "picked candidate"), ("all-collide", 13, dict(pick_off=True), "picked candidate"),
                                 ("resets", N, dict(slot_shift=1), "reset DoF positions"), ("resets", N, dict(cmd_on_any_reset=True), "COMMANDS"),
                                 ("events", N, dict(push_before_cmd=True), "pushed root velocity")):
        w, bad = run(name, n, **wrong)
        print(name, wrong, [b[:90] for b in bad[:3]])
        assert any(what in b for b in bad), (name, wrong, what, bad[:4])
    c = runs("f64", "reset_all")
    ev = ss.check_reset_all(c["gt"], c["pre"], c["post"], c["step"], "reset_all", slot_shift=1)
    assert any("reset DoF positions" in b for b in ev.bad) and any("COMMANDS" in b for b in ev.bad)


@pytest.mark.parametrize("fixture", ["wg_reference_allrewards.npz", "wg_reference_contacts.npz", "wg_reference_cart.npz"])
def test_recorded_reference_keeps_the_pre_reset_rows(fixture):
    """What the reference project's own recorded steps (tests/golden) hold for an env that reset in the step: RIGID_BODY_STATE and the
    base velocities are those of the refresh BEFORE the reset (the trunk row is not the new root, BASE_LIN_VEL / BASE_ANG_VEL are R^T of
    the trunk row's velocities); the envs that did not reset have their trunk row at the stored root. step_state_reference's
    check_step_kinematics asserts the same of the oracle and of the kernel."""
    import arm_osc_oracle as ao
    import test_wg_golden as wg
    g = wg.load(fixture)
    resets = 0
    for k in range(int(g["steps"])):
        rb, root = g[f"s{k}/RIGID_BODY_STATE"].astype(np.float64), g[f"s{k}/ROOT_STATES"].astype(np.float64)
        reset = g[f"s{k}/RESET_BUF"].astype(bool)
        assert np.array_equal(rb[~reset, 0, 0:7], root[~reset, 0, 0:7])
        for e in np.flatnonzero(reset):
            Rt = ao.quat_to_mat(rb[e, 0, 3:7]).T
            assert np.abs(rb[e, 0, 0:3] - root[e, 0, 0:3]).max() > 1e-3
            assert np.abs(Rt @ rb[e, 0, 7:10] - g[f"s{k}/BASE_LIN_VEL"][e]).max() <= 2e-5
            assert np.abs(Rt @ rb[e, 0, 10:13] - g[f"s{k}/BASE_ANG_VEL"][e]).max() <= 2e-5
        resets += int(reset.sum())
    assert resets >= 10
