"""Torque-supervision inputs: the arm's mass-matrix block, end-effector Jacobian and gravity
torques (csrc/wbc_arm_kernel.hip) against the independent fp64 restatement oracle/arm_osc_oracle.py, and the
operational-space control law (WG:1217-1242) assembled from them.

Per-entry bound: every entry of mm, ee_j_eef and g_torque of every env satisfies |kernel - ref| <= C 2^-24 mag against the fp64 values
and magnitudes of tests/body_dynamics_reference.py (the whole-body M's and J's on the arm's slices; g_torque: the link masses times 9.81
times the levers' path lengths), at n = 1, 63, 64, 65 and 129: the edges of the kernel's blocks of 64 threads, one thread per env. The
states, the yardstick and the rule C = 4 K_ref (a power of two, at least 8) are those of tests/test_whole_body_dynamics.py; the kernel's
column is what an MI355X gave, printed by the test:

    output     K_ref    C     kernel's largest ratio (n, env, entry)
    mm         1.69     8     2.67  (n = 129, env 120, mm[0, 0])
    ee_j_eef   5.70     32    6.92  (n = 63, env 2, ee_j_eef[1, 4])
    g_torque   7.10     32    6.73  (n = 129, env 69, g_torque[4])

Against the whole-body kernel (mm_whole[:, -8:-2, -8:-2], jacobian_whole[:, gripper_idx, :6, -8:-2]) the difference stays within the sum
of both allowances: at most 0.105 (mm, n = 129) and 0.148 (ee_j_eef) of it. The old tolerances on the same states, entry by entry: mm 2e-6 + 2e-4 |ref|
against 8 2^-24 mag = 3.2e-9 .. 6.0e-7, 5.4 x to 810 x below it; ee_j_eef 2e-6 + 1e-4 |ref| against 1.8e-7 .. 1.9e-6, 1.05 x to 59 x; g_torque
2e-5 + 2e-4 |ref| against 1.3e-7 .. 6.8e-6, 2.9 x to 160 x (test_reference_slices_are_the_arm_oracle_and_... asserts that every ratio is
above 1; the old test stays as it is)."""
import ctypes as C

import numpy as np
import pytest
import torch

import arm_osc_oracle as ao
import body_dynamics_reference as bd
from wbc_amd import abi


def _model():
    return abi.load_default_model()


def test_oracle_jacobian_matches_finite_differences():
    m = _model()
    rng = np.random.default_rng(0)
    ee_rb = m.rb_names.index("wx250s/ee_gripper_link")
    chain = ao.arm_chain(m, m.rb_body[ee_rb])
    for _ in range(5):
        q = rng.uniform(-1, 1, 20); q[-2:] = 0
        quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
        pos = rng.normal(size=3)
        M, J, g = ao.arm_quantities(m, pos, quat, q, ee_rb, list(range(m.num_rigid_bodies - 9, m.num_rigid_bodies)), m.rb_mass[-9:])
        h = 1e-6
        for j, b in enumerate(chain):
            dq = np.zeros(20); dq[m.body_dof[b]] = h
            p1, R1 = ao.ee_pose(m, pos, quat, q + dq, ee_rb); p0, R0 = ao.ee_pose(m, pos, quat, q - dq, ee_rb)
            np.testing.assert_allclose((p1 - p0) / (2 * h), J[:3, j], atol=1e-6)
            W = (R1 - R0) / (2 * h) @ (0.5 * (R0 + R1)).T                  # [omega]x
            np.testing.assert_allclose([W[2, 1], W[0, 2], W[1, 0]], J[3:, j], atol=1e-6)
        assert np.allclose(M, M.T) and np.all(np.linalg.eigvalsh(M) > 0)


def test_fp32_yardsticks_are_the_ones_the_constants_were_taken_from():
    import test_whole_body_dynamics as twb
    twb._assert_yardsticks(("mm", "ee", "g"))


def test_reference_slices_are_the_arm_oracle_and_the_new_allowances_lie_below_the_old_ones():
    """The fp64 reference of the per-entry bound against oracle/arm_osc_oracle.py (mass matrix and Jacobian: another algebra on the same
    kinematics; gravity torques: central differences of the potential, good to 1e-8 N m), and C 2^-24 mag against the tolerances of
    test_arm_dynamics_kernel_matches_oracle on every entry with a magnitude."""
    import test_whole_body_dynamics as twb
    m = _model()
    ee_rb, link_rb = bd.arm_links(m)
    link_mass = np.array(m.rb_mass[-9:], dtype=np.float64)
    link_mass[link_rb.index(ee_rb)] += 0.05
    old = {"mm": (2e-4, 2e-6), "ee": (1e-4, 2e-6), "g": (2e-4, 2e-5)}
    span = {f: [np.inf, 0.0, np.inf, 0.0] for f in old}            # new allowance: least, most; old / new: least, most
    for pos, quat, q, _, bp in twb._yardstick_states()[::8] + list(twb._edge_states()):
        out, mag = bd.reference(m, pos, quat, q, bp, link_mass)
        M, J, g = ao.arm_quantities(m, pos, quat, q, ee_rb, link_rb, link_mass, gripper_params=(bp[10], bp[11:14], bp[14:20]))
        np.testing.assert_allclose(out["mm"], M, rtol=0, atol=1e-13)
        np.testing.assert_allclose(out["ee"], J, rtol=0, atol=1e-13)
        np.testing.assert_allclose(out["g"], g, rtol=0, atol=1e-8)
        assert np.all(mag["mm"] > 0) and np.all(mag["g"] > 0) and np.all(mag["ee"][3:6] == 1)
        for f, (rtol, atol) in old.items():
            live = mag[f] > 0
            new = twb.CONST[f] * bd.EPS * mag[f][live]
            r = (atol + rtol * np.abs(out[f][live])) / new
            s = span[f]
            span[f] = [min(s[0], new.min()), max(s[1], new.max()), min(s[2], r.min()), max(s[3], r.max())]
    for f, s in span.items():
        print(f"{f}: new allowance {s[0]:.3g} .. {s[1]:.3g}; old / new per entry {s[2]:.3g} .. {s[3]:.3g}")
        assert s[2] > 1


def _launch_arm(env):
    """A direct C-ABI call into sentinel-framed buffers: {mm [n, 6, 6], ee [n, 6, 6], g [n, 6]}."""
    import test_whole_body_dynamics as twb
    n, m = env.num_envs, env.robot_model
    shape = {"mm": (n, 6, 6), "ee": (n, 6, 6), "g": (n, 6)}
    bufs = {k: twb._framed(int(np.prod(s))) for k, s in shape.items()}
    ptr = lambda k: bufs[k].data_ptr() + 4 * twb.FRAME
    rb = (C.c_int * 9)(*[int(x) for x in env._arm_link_rb])
    ms = (C.c_float * 9)(*[float(x) for x in m.rb_mass[-9:]])
    rc = env.sim.L.wbc_sim_arm_dynamics(env.sim.h, rb, ms, ptr("mm"), ptr("ee"), ptr("g"), env.sim._stream())
    assert rc == 0, env.sim.L.wbc_last_error()
    torch.cuda.synchronize()
    return {k: twb._unframed(b, shape[k], k) for k, b in bufs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_every_env_and_entry_at_the_block_edges(n):
    """One thread per env in blocks of 64: a lone env, one short of a block, a full block, one env in a second block, one in a third.
    Every env against the fp64 reference; nothing written outside the outputs; and the whole-body kernel's slices agree within the sum of
    both kernels' allowances."""
    import test_whole_body_dynamics as twb
    env, refs, _, _ = twb._case(n)
    keys = ("ROOT_STATES", "DOF_STATE", "BODY_PARAMS")
    before = [env.sim.tensor(k).clone() for k in keys]
    got = _launch_arm(env)
    g64 = {k: v.double().cpu().numpy() for k, v in got.items()}
    worst = twb._worst(g64, refs, ("mm", "ee", "g"), n)
    for f, w in worst.items():
        assert w[0] <= twb.CONST[f], (f, w)
    assert np.array_equal(g64["mm"], g64["mm"].transpose(0, 2, 1))
    # the Python entry points are the same call
    assert torch.equal(env.get_arm_mm(), got["mm"]) and torch.equal(env.get_ee_jac(), got["ee"]) and torch.equal(env.get_g_torques(), got["g"])
    # the whole-body kernel, through the reference's own slicing expressions (WG:557-558)
    whole = twb._launch_body(env)
    mm_w = whole["M"][:, -8:-2, -8:-2].double().cpu().numpy()
    ee_w = whole["J"][:, env.gripper_idx, :6, -8:-2].double().cpu().numpy()
    share = {"mm": 0.0, "ee": 0.0}
    for e, (_, mag) in enumerate(refs):
        for f, mine, theirs, c in (("mm", g64["mm"][e], mm_w[e], twb.CONST["mm"] + twb.CONST["M"]), ("ee", g64["ee"][e], ee_w[e], twb.CONST["ee"] + twb.CONST["J"])):
            r, at = bd.ratio(mine, theirs, mag[f])                            # equal where there is no magnitude
            assert r <= c, (f, e, at, r)
            share[f] = max(share[f], r / c)
    print(f"n={n}: arm kernel against the whole-body kernel, largest difference / summed allowances: mm {share['mm']:.3g}, ee_j_eef {share['ee']:.3g}")
    torch.cuda.synchronize()
    for k, t in zip(keys, before):
        assert torch.equal(env.sim.tensor(k), t), k


@pytest.mark.gpu
def test_arm_dynamics_kernel_matches_oracle():
    from wbc_amd.config import WidowGo1RoughCfg
    from wbc_amd.envs import WidowGo1
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = 64; cfg.terrain.mesh_type = "plane"
    env = WidowGo1(cfg, sim_device="cuda:0", seed=5)
    for _ in range(15):                                                       # leave the reset pose
        env.step(torch.randn(64, 18, device="cuda") * 0.8)
    mm, jac, gt = env.get_arm_mm().cpu().numpy(), env.get_ee_jac().cpu().numpy(), env.get_g_torques().cpu().numpy()
    m = env.robot_model
    root, dof = env.root_states.cpu().numpy().astype(np.float64), env.dof_pos.cpu().numpy().astype(np.float64)
    bp = env.sim.tensor("BODY_PARAMS").cpu().numpy().astype(np.float64)
    dm0 = float(env.mass_params_tensor[0, 4])
    link_rb = list(range(m.num_rigid_bodies - 9, m.num_rigid_bodies))
    link_mass = np.array(m.rb_mass[-9:], dtype=np.float64)
    link_mass[link_rb.index(env.gripper_idx)] += dm0                         # env 0's randomised gripper mass (WG:664-670)
    for e in range(0, 64, 7):
        M, J, g = ao.arm_quantities(m, root[e, :3], root[e, 3:7], dof[e], env.gripper_idx, link_rb, link_mass,
                                    gripper_params=(bp[e, 10], bp[e, 11:14], bp[e, 14:20]))
        np.testing.assert_allclose(mm[e], M, rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(jac[e], J, rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(gt[e], g, rtol=2e-4, atol=2e-5)


@pytest.mark.gpu
def test_torque_supervision_path_runs_end_to_end():
    """control.torque_supervision=True: the env supplies target_arm_torques / current arm state every step and the
    (eager) learner consumes them (WG:1178-1181, PPO:136-142, 234-238)."""
    from wbc_amd.config import WidowGo1RoughCfg, WidowGo1RoughCfgPPO, class_to_dict
    from wbc_amd.envs import WidowGo1
    from wbc_amd.rsl_rl.runners import OnPolicyRunner
    cfg = WidowGo1RoughCfg(); cfg.env.num_envs = 128; cfg.terrain.mesh_type = "plane"; cfg.control.torque_supervision = True
    env = WidowGo1(cfg, sim_device="cuda:0", seed=2)
    env.reset()
    obs, _, _, _, _, infos = env.step(torch.zeros(128, 18, device="cuda"))
    u = infos["target_arm_torques"]
    assert u.shape == (128, 6) and torch.isfinite(u).all() and infos["current_arm_dof_pos"].shape == (128, 6)
    # the controller holds the arm against gravity near the goal: torques are of the order of the arm's weight moments
    assert float(u.abs().max()) < 50.0
    train = class_to_dict(WidowGo1RoughCfgPPO())
    train["runner"]["num_steps_per_env"] = 8
    train["algorithm"]["torque_supervision"] = True
    train["algorithm"]["torque_supervision_schedule"] = [0.1, 1000, 1000]
    runner = OnPolicyRunner(env, train, log_dir=None, device="cuda:0")
    runner.learn(3)
    rec = runner.history[-1]
    assert np.isfinite(rec["mean_arm_torques_loss"]) and rec["mean_arm_torques_loss"] > 0 and rec["torque_supervision_weight"] > 0
