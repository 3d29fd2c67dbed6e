"""What produces the inputs of the step's task logic, on the HIP kernels: rigid_body_pass through all three of its callers
(wbc_fk_kernel, wbc_reset_kernel, wbc_step_kernel), the base-frame velocities, the action reorder / clip / delay FIFO with the PD
torques (decimation = 1), update_curr_ee_goal, the wave-parallel goal_pick with goal_apply, resample_commands, the push and reset_env
-- held to the fp64 restatement of tests/step_state_reference.py: |kernel - ref| <= C 2^-24 mag per entry, every copy, every drawn
slot and every discrete decision exactly. Everything goes through the C-ABI (helpers.make_gpu) with per-env randomised parameters;
the cases, seeds and states are those tests/test_step_state.py runs through the C oracle on the CPU. wbc_step_kernel runs at n = 13
(the grid is rounded up to 8), 256 and -- the kinematics and the goal machine -- 2048 (the envs are dealt to the XCDs from there
on; every tenth env plus the last is checked); wbc_fk_kernel and wbc_reset_kernel (one env per block) at n = 13 and 256.

Constants: C = 4 x K_ref rounded up to a power of two, K_ref the fp32 ORACLE's largest ratio per tier (measured and asserted on the
CPU by tests/test_step_state.py, never taken from the kernel); at least 8 where the tier passes through a transcendental.

    tier                                      K_ref    C    kernel's largest ratio on an MI355X
    rigid-body positions                       2.00    8    1.71   events n = 256, second step, env 36: gripper_link z
    rigid-body quaternions                     4.17   32    5.15   fk n = 256, env 207: wrist_link qz
    rigid-body linear / angular velocities     2.69   16    8.17   events n = 2048, third step, env 940: RL_calf vz
    BASE_LIN_VEL / BASE_ANG_VEL                1.36    8    2.37   resets n = 13, env 12 (a reset env, from its trunk row): BASE_ANG_VEL[1]
    PD torques                                 0.68    4    0.55   torques n = 256, first step, env 41: DoF 13
    goal values through sin / cos / atan2      0.48    8    0.91   events n = 256, first step, env 95: G_CURR_CART[1]
    goal values by lerp                        0.94    4    0.93   events n = 2048, third step, env 290: G_CURR[0]
    RESET_TRAVEL                               0.62    4    0.96   resets n = 256, env 108: RESET_TRAVEL[1]

Every exact comparison (the box row, ACTIONS, LAST_ACTIONS, the ACTION_HISTORY shift for every action_delay, DoFs 18 and 19, the
goal timer and the resample decision at `timer + 1 == total`, the picked candidate, G_START, the reset's zeroed tensors and
EPISODE_SUMS_DONE) holds bit for bit; every drawn value lies within 2 ulp of its float32 evaluation.
"""
import numpy as np
import pytest

import helpers
import step_state_reference as ss
import test_gpu_task_logic as tg

pytestmark = pytest.mark.gpu

WORST = ss.Worst()          # the kernel's largest ratios, printed by the last test


class GpuAdapter(tg.GpuAdapter):
    def refresh_rigid_body_state(self):
        self.g.refresh_rigid_body_state()

    def reset_all(self):
        self.g.reset_all()


@pytest.fixture(scope="module")
def runs(robot):
    """(case name, n) -> the case on the GPU, each run once."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            sims = []

            def mk(tc, m):
                g = helpers.make_gpu(robot, m, helpers.random_env_params(m, seed=ss.PARAM_SEED), tcfg=tc)
                sims.append(g)
                return GpuAdapter(g)
            if name == "fk":
                cache[name, n] = ss.run_fk(mk, robot, n)
            elif name == "reset_all":
                cache[name, n] = ss.run_reset_all(mk, robot, n)
            else:
                cache[name, n] = ss.run_case(mk, robot, name, n)
            for g in sims:
                g.close()
        return cache[name, n]
    return get


def _settle(worst, bad, where):
    for t in ss.TIERS:
        r, at = worst.get(t)
        if at:
            print(f"{where}: {t}: largest ratio {r:.3f} ({at})")
    WORST.merge(worst)
    assert not bad, bad[:8]
    for t in ss.TIERS:
        assert worst.get(t)[0] <= ss.bound(t), (t, worst.get(t), ss.bound(t))


@pytest.mark.parametrize("n", [13, 256])
def test_rigid_bodies_through_the_fk_kernel(runs, n):
    """Random base attitudes, every joint over its limit interval, root velocities to 2 m/s and 5 rad/s with qd to qd_limit, joints
    exactly at 0, +-pi/2 and their limits: all 27 x 13 entries per env, the box row bit for bit."""
    worst, bad = ss.Worst(), []
    ss.check_fk_case(runs("fk", n), n, worst, bad)
    _settle(worst, bad, f"fk n = {n}")


@pytest.mark.parametrize("n", [13, 256])
def test_reset_kernel(runs, n):
    """reset_all: the 20 DoF draws, the xy perturbation on the origins, the six velocity draws, the box row, commands always
    resampled, the goal from slots 67.. and 70.., RESET_TRAVEL, the zeroed tensors; then the rigid-body pass from the reset's own
    ROOT_STATES / DOF_STATE."""
    worst, bad = ss.Worst(), []
    cnt = ss.check_reset_all_case(runs("reset_all", n), n, worst, bad)
    _settle(worst, bad, f"reset_all n = {n}")
    assert ss.excluded_share(cnt) <= 0.02
    if n >= 256:
        assert cnt["first_rejected"] >= 20 and len(set(cnt["picks"])) >= 3 and cnt["cmd_keep"] >= 8 and cnt["cmd_zero"] >= 8


@pytest.mark.parametrize("n", [13, 256, 2048])
def test_step_kinematics_and_goal_machine(runs, n):
    """Three steps, the second one pushing: RIGID_BODY_STATE, BASE_LIN_VEL, BASE_ANG_VEL from the step's own post-state (on the push
    step without what read the root's linear velocity before the push); the goal update on both sides of t = 0.5, at 0 and beyond
    traj; the resample decision including `timer + 1 == total`; every candidate of every resample decided in fp64, the picked index
    exact; the command gate and the push with both factors."""
    c = runs("events", n)
    worst, bad = ss.Worst(), []
    checked = ss.check_step_kinematics(c, n, "events", worst, bad)
    cnt = ss.check_case_events(c, n, "events", worst, bad)
    print(f"events n = {n}: {checked} env-steps; {cnt['goal_events']} goal resamples ({cnt['goal_uncertain']} uncertain, "
          f"{cnt['first_rejected']} with the first candidate rejected, picks {sorted(set(cnt['picks']))}), commands kept / zeroed "
          f"{cnt['cmd_keep']} / {cnt['cmd_zero']}, pushes x1 / x2.5 {cnt['push_1']} / {cnt['push_25']}")
    _settle(worst, bad, f"events n = {n}")
    assert ss.excluded_share(cnt) <= 0.02 and cnt["resets"] == 0
    if n >= 256:
        ss.assert_event_coverage(cnt, n)


def test_all_ten_candidates_collide(runs):
    """The collision box covers the whole goal range: every env takes the tenth candidate."""
    worst, bad = ss.Worst(), []
    cnt = ss.check_case_events(runs("all-collide", 13), 13, "all-collide", worst, bad)
    _settle(worst, bad, "all-collide n = 13")
    assert cnt["goal_events"] == 13 and set(cnt["picks"]) == {9} and cnt["goal_uncertain"] == 0


@pytest.mark.parametrize("n", [13, 256])
def test_action_path_and_torques(runs, n):
    """decimation = 1, clip_actions = 2 with actions beyond it, actions that differ in every column, every eighth env with
    q[WBC_NACT - 8] outside (-pi, pi] (torques only): TORQUES against the PD sum, a clamped one exactly the limit; ACTIONS,
    LAST_ACTIONS, ACTION_HISTORY, DoFs 18 and 19 exactly."""
    worst, bad = ss.Worst(), []
    cnt = ss.check_torque_case(runs("torques", n), n, "torques", worst, bad)
    print(f"torques n = {n}:", cnt)
    _settle(worst, bad, f"torques n = {n}")
    assert cnt["near"] <= 0.02 * (cnt["clamped"] + cnt["free"])
    if n >= 256:
        assert cnt["clamped"] >= 64 and cnt["free"] >= 64 and cnt["clipped"] >= 64


@pytest.mark.parametrize("delay", ss.DELAYS)
def test_action_fifo_for_every_delay(runs, delay):
    """The FIFO shift and the row handed to the torques for every action_delay a four-row FIFO admits; -1: no FIFO, the history rests."""
    c = runs(f"torques-delay{delay}", 13)
    worst, bad = ss.Worst(), []
    ss.check_torque_case(c, 13, f"torques-delay{delay}", worst, bad)
    _settle(worst, bad, f"torques-delay{delay} n = 13")
    if delay == -1:
        assert np.array_equal(c["steps"][0][1]["ACTION_HISTORY"], c["steps"][0][0]["ACTION_HISTORY"])


@pytest.mark.parametrize("n", [13, 256])
def test_resets_within_the_step(runs, n):
    """Half of the envs reset (fallen, rolled over, timed out): the reset's draws, commands only on a time-out, the goal from slots
    67.. and 70.. with the pre-reset yaw, RESET_TRAVEL, the zeroed ACTION_HISTORY, EPISODE_SUMS_DONE a copy; the rigid-body rows and
    base velocities of a reset env are those of the pass BEFORE the reset, of the others those of their post-state."""
    c = runs("resets", n)
    worst, bad = ss.Worst(), []
    ss.check_step_kinematics(c, n, "resets", worst, bad)
    cnt = ss.check_case_events(c, n, "resets", worst, bad)
    _settle(worst, bad, f"resets n = {n}")
    assert cnt["resets"] > n // 3 and cnt["time_outs"] >= n // 8 and cnt["falls"] >= n // 8 and cnt["both"] == 0
    assert ss.excluded_share(cnt) <= 0.02
    reset = c["steps"][0][1]["RESET_BUF"] != 0
    assert np.array_equal(reset, np.isin(c["kind"], [0, 1, 3]))


def test_print_the_kernels_largest_ratios():
    """The table for the module docstring and DESIGN.md section 4 (run after the tests above: they fill it)."""
    print("kernel's largest ratio per tier:")
    for t in ss.TIERS:
        r, at = WORST.get(t)
        if at:
            print(f"  {t:10s} {r:7.3f}   K_ref {ss.K_REF[t]:5.2f}   C {ss.bound(t):3.0f}   ({at})")
            assert r <= ss.bound(t)
