"""`LeggedRobot` / `WidowGo1`: the task classes with the reference's public surface (constructor
arguments, attribute names, tensor views, `step` / `reset` / `update_command_curriculum`), backed by
the fused HIP step instead of Isaac Gym + ~150 eager torch ops.

Reference: legged_gym/envs/widowGo1/widowGo1.py:49 (WidowGo1), legged_gym/envs/base/legged_robot.py:52-77
and legged_gym/envs/base/base_task.py:41-131 (constructor, buffers, reset). Everything the reference
computes per step in Python lives in csrc/wbc_step_kernel.hip; this file only does what the reference
does on the host at construction time (domain randomisation draws, WG:207-228,402-408,431-496,574-575)
and exposes views.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import abi
from .curriculum import make_curriculum
from .rsl_rl.env import VecEnv
from .sim import WbcSim
from .urdf_model import RobotModel, build_model


# isaacgym.torch_utils helpers the operational-space controller uses (quaternions are xyzw)
def _quat_mul(a, b):
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    return torch.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], dim=-1)


def _quat_apply(q, v):
    xyz = q[:, :3]
    t = torch.linalg.cross(xyz, v, dim=-1) * 2
    return v + q[:, 3:] * t + torch.linalg.cross(xyz, t, dim=-1)


def _quat_rotate_inverse(q, v):
    """R(q)^T v."""
    return _quat_apply(torch.cat([-q[:, :3], q[:, 3:]], dim=-1), v)


def _orientation_error(desired, current):                                           # widowGo1.py orientation_error
    cc = torch.cat([-current[:, :3], current[:, 3:]], dim=-1)
    q_r = _quat_mul(desired, cc)
    return q_r[:, 0:3] * torch.sign(q_r[:, 3]).unsqueeze(-1)


def _yaw_quat(quat):
    """Quaternion of the yaw of `quat` alone (base_yaw_quat, WG:878-880)."""
    x, y, z, w = quat.unbind(-1)
    yaw = torch.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    zero = torch.zeros_like(yaw)
    return torch.stack([zero, zero, torch.sin(yaw / 2), torch.cos(yaw / 2)], dim=-1)


def stale_time_outs(prev, time_out_buf, reset_buf):
    """extras['time_outs'] as the reference publishes it (quirk Q9). `check_termination` builds a NEW time_out_buf tensor every
    step (WG:943-944) but `extras["time_outs"]` is only re-bound inside reset_idx after its early return for an empty env_ids
    (WG:705-706, 753-754): on a step in which no env resets, the learner is handed the mask of the LAST step that had a reset and
    bootstraps those envs' rewards once more (PPO:133-134). Device-side select, no host synchronisation."""
    return torch.where((reset_buf != 0).any(), time_out_buf, prev)


class EpisodeInfo(dict):
    """extras['episode'] (WG:743-750): a dict of 0-dim device tensors and floats, as the reference's. `vector` is the one device
    tensor the tensor entries are views of and `vector_index` maps their keys to its rows, so a logger can average a rollout's
    worth of these with one stack + one host copy instead of one .item() per key (OnPolicyRunner.log)."""
    vector = None
    vector_index = None


def draw_env_params(cfg, n, seed, dt, strip_origins=True, levels=False, gen=None):
    """The per-env constants the reference draws on the host at construction, as numpy arrays keyed by WbcSim.set_env_params'
    arguments (+ 'env_origins' as a torch tensor and 'levels_gen', the generator positioned where the terrain-level draw takes
    it): env origins on the strip in front of the field (WG:207-224), the box's lateral offset (WG:226-227), per-env friction from
    1000 buckets (WG:480-490), base mass / centre of mass / gripper mass (WG:431-456), the box's added mass (WG:458-466), motor
    strengths (WG:402-408), EE-trajectory timing (WG:574-575). Pure: nothing but `cfg` decides the result for a given seed."""
    if gen is None:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
    nprng = np.random.default_rng(int(seed))
    rand = lambda lo, hi, *shape: (hi - lo) * torch.rand(*shape, generator=gen) + lo   # noqa: E731
    t, dr = cfg.terrain, cfg.domain_rand
    origins = torch.zeros(n, 3)
    if strip_origins:                           # WG:207-224: a strip in front of the (Perlin) field
        half_col = t.tot_cols * t.horizontal_scale / 2
        half_row = t.tot_rows * t.horizontal_scale / 2
        origins[:, 0] = rand(-2.5 * half_col / 5, -2 * half_col / 5, n)
        origins[:, 1] = rand(-half_row + 10, half_row - 10, n)
    levels_gen = torch.Generator(device="cpu")
    levels_gen.set_state(gen.get_state())       # (the terrain-level draw of LR:717-731 comes next in the stream)
    if levels:                                  # advance past it exactly as _get_env_origins_levels will
        max_init_level = t.max_init_terrain_level if t.curriculum else t.num_rows - 1
        torch.randint(0, max_init_level + 1, (n,), generator=gen)
    sign = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    box_dy = sign * rand(cfg.box.box_env_origins_y_range[0], cfg.box.box_env_origins_y_range[1], n)
    if dr.randomize_friction:
        buckets = rand(dr.friction_range[0], dr.friction_range[1], 1000)
        friction = buckets[torch.randint(0, 1000, (n,), generator=gen)]
    else:
        friction = torch.ones(n)
    dmass = nprng.uniform(*dr.added_mass_range, size=n) if dr.randomize_base_mass else np.zeros(n)
    gmass = nprng.uniform(*dr.gripper_added_mass_range, size=n) if dr.randomize_gripper_mass else np.zeros(n)
    if dr.randomize_base_com:
        lo = [dr.added_com_range_x[0], dr.added_com_range_y[0], dr.added_com_range_z[0]]
        hi = [dr.added_com_range_x[1], dr.added_com_range_y[1], dr.added_com_range_z[1]]
        dcom = nprng.uniform(lo, hi, size=(n, 3))
    else:
        dcom = np.zeros((n, 3))
    if dr.randomize_motor:
        motor = torch.cat([rand(*dr.leg_motor_strength_range, n, 12), rand(*dr.arm_motor_strength_range, n, 6)], dim=1)
    else:
        motor = torch.ones(n, cfg.env.num_torques)
    box_dmass = nprng.uniform(*cfg.box.added_mass_range, size=n) if cfg.box.randomize_base_mass else np.zeros(n)   # WG:458-466
    traj = rand(cfg.goal_ee.traj_time[0], cfg.goal_ee.traj_time[1], n) / dt
    total = traj + rand(cfg.goal_ee.hold_time[0], cfg.goal_ee.hold_time[1], n) / dt
    return dict(friction=friction.numpy(), base_dmass=dmass, base_dcom=dcom, gripper_dmass=gmass, motor_strength=motor.numpy(),
                env_origins=origins, box_delta_y=box_dy.numpy(), traj_timesteps=traj.numpy(), traj_total_timesteps=total.numpy(),
                box_dmass=box_dmass, levels_gen=levels_gen)


class BaseTask(VecEnv):
    """Buffer/attribute contract of legged_gym/envs/base/base_task.py:41-131 (viewer omitted: headless)."""

    def __init__(self, cfg, sim_params=None, physics_engine=None, sim_device="cuda:0", headless=True):
        self.cfg = cfg
        self.sim_params = sim_params
        self.physics_engine = physics_engine
        self.sim_device = str(sim_device)
        self.device = torch.device(self.sim_device)
        self.headless = headless
        self.num_envs = cfg.env.num_envs
        self.num_obs = cfg.env.num_observations
        self.num_privileged_obs = cfg.env.num_privileged_obs
        self.num_actions = cfg.env.num_actions
        self.privileged_obs_buf = None
        self._obs_output = None
        self._store_output = None
        self.extras = {}
        self.viewer = None
        self.enable_viewer_sync = False

    def get_observations(self):
        return self.obs_buf

    def get_privileged_observations(self):
        return self.privileged_obs_buf

    def reset_idx(self, env_ids):
        raise NotImplementedError

    def reset(self):
        """Reset all robots, then one zero-action step (BT:127-131)."""
        self.reset_idx(torch.arange(self.num_envs, device=self.device), start=True)
        obs, privileged_obs, _, _, _, _ = self.step(torch.zeros(self.num_envs, self.num_actions, device=self.device))
        return obs, privileged_obs

    def render(self, sync_frame_time=True):
        return None


# Methods of the reference's WidowGo1 / LeggedRobot whose work happens INSIDE the fused step (csrc/wbc_step_kernel.hip): a Python
# override in a subclass would never be called, so defining one is an error at class-creation time, not a silent no-op.
FUSED_METHODS = ("compute_observations", "_compute_torques", "check_termination", "compute_reward", "post_physics_step",
                 "_post_physics_step_callback", "_push_robots", "_reset_dofs", "_reset_root_states", "update_curr_ee_goal",
                 "collision_check", "get_body_orientation", "_prepare_reward_function", "_process_rigid_body_props",
                 "_process_rigid_shape_props", "_process_dof_props", "_get_noise_scale_vec")
FUSED_PREFIXES = ("_reward_", "_resample_")


def _fused_overrides(namespace):
    return sorted(n for n in namespace if n in FUSED_METHODS or n.startswith(FUSED_PREFIXES))


class LeggedRobot(BaseTask):
    """Shared pieces of LR:52-77,279-305: config parsing, DoF limits from the URDF, views."""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        bad = _fused_overrides(vars(cls))
        if bad:
            raise TypeError(
                f"{cls.__name__} overrides {', '.join(bad)}: the fused step computes this on the device (csrc/wbc_step_kernel.hip, spec "
                "oracle/wbc_oracle.c) and never calls the Python method. Change a reward through cfg.rewards.scales / arm_scales (every "
                "_reward_* of the reference is a table entry of wbc_curriculum), thresholds and gains through the config (wbc_task_cfg); for "
                "new arithmetic either add it to the kernel and the oracle, or step your own torch code on the C-ABI tensors "
                "(wbc_sim_get_tensor: ROOT_STATES, DOF_STATE, TORQUES, ... are live views) after WidowGo1.step returns.")

    def __init__(self, cfg, sim_params=None, physics_engine=None, sim_device="cuda:0", headless=True,
                 robot_model: Optional[RobotModel] = None, seed: Optional[int] = None):
        super().__init__(cfg, sim_params, physics_engine, sim_device, headless)
        self.debug_viz = False
        self.init_done = False
        self.robot_model = robot_model if robot_model is not None else self._load_model(cfg)
        self._seed = int(seed if seed is not None else getattr(cfg, "seed", 1))
        self._parse_cfg(cfg)
        self.create_sim()
        self._init_buffers()
        self.init_done = True

    @staticmethod
    def _load_model(cfg) -> RobotModel:
        path = cfg.asset.file
        if "{LEGGED_GYM_ROOT_DIR}" not in path and path.endswith(".urdf"):
            return build_model(path)
        return abi.load_default_model()      # the packaged widowGo1 tables (tools/extract_model.py)


class WidowGo1(LeggedRobot):
    def _parse_cfg(self, cfg):                                                     # WG:78-121
        sim_dt = self.sim_params.dt if self.sim_params is not None and hasattr(self.sim_params, "dt") else cfg.sim.dt
        self.num_torques = cfg.env.num_torques
        self.dt = cfg.control.decimation * sim_dt
        self._sim_dt = sim_dt
        self.obs_scales = cfg.normalization.obs_scales
        self.update_counter = 0
        self.max_episode_length_s = cfg.env.episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.dt)
        self.push_interval = np.ceil(cfg.domain_rand.push_interval_s / self.dt)
        self.clip_actions = cfg.normalization.clip_actions
        self.action_delay = cfg.env.action_delay
        if cfg.terrain.mesh_type not in ["heightfield", "trimesh"]:
            cfg.terrain.curriculum = False
        self.collect_episode_stats = True
        # opt-in (OnPolicyRunner.learn sets it): extras['episode'] is computed on a side stream, overlapping the next policy
        # inference; its consumer must synchronise the DEVICE before reading the values (the runner does, at the end of the rollout)
        self.async_episode_stats = False
        self._stats_stream = None
        self._stats_pending = False
        self._track = (None, 0)          # (state, cap) of attach_episode_tracker: advanced by the statistics launch
        # opt-in (OnPolicyRunner.learn sets it): step() does not launch the episode statistics itself but leaves them as a side job
        # (take_stats_job) that the policy inference following every rollout step carries as a few extra workgroups -- one launch
        # and one inter-kernel dependency stall less per env step. extras['episode'] is then complete once that launch has run;
        # a job nobody takes is executed by the next step() / flush_stats_job().
        self.defer_episode_stats = False
        self._stats_job = None
        # cfg.env.reference_stale_time_outs: publish extras['time_outs'] the way the reference does (quirk Q9). The fused step's
        # in-kernel reward bootstrap uses the CURRENT mask, so with the option on the reward / done slots are filled by
        # wbc_rollout_store from the published (possibly stale) mask instead.
        self._stale_time_outs_on = bool(getattr(cfg.env, "reference_stale_time_outs", False))
        self._stale_mask = None

    # ---- construction ----------------------------------------------------------------------
    def create_sim(self):                                                           # WG:230-237, 255-429
        cfg, m, n = self.cfg, self.robot_model, self.num_envs
        # asset.self_collisions is Isaac Gym's collision FILTER: 0 = self-collision enabled (widowGo1_config.py:180)
        self.wmodel = abi.fill_model(m, foot_name=cfg.asset.foot_name, self_collisions=int(getattr(cfg.asset, "self_collisions", 0)) == 0,
                                     box_size=float(cfg.box.box_size), rest_offset=float(abi._get(cfg, "sim.physx.rest_offset", 0.0)))
        self.tcfg = abi.fill_task_cfg(cfg, m, sim_dt=self._sim_dt)
        self.sim = WbcSim(self.wmodel, self.tcfg, n, self.device, seed=self._seed)
        self.num_dofs, self.num_bodies = m.num_dofs, m.num_rigid_bodies
        self.dof_names, self.body_names = list(m.dof_names), list(m.rb_names)
        self.dof_wo_gripper_names = self.dof_names[:-2]
        self.body_names_to_idx = {n_: i for i, n_ in enumerate(self.body_names)}
        self.dof_names_to_idx = {n_: i for i, n_ in enumerate(self.dof_names)}
        self.gripper_idx = self.body_names_to_idx["wx250s/ee_gripper_link"]
        dev = self.device
        feet = [i for i, s in enumerate(self.body_names) if cfg.asset.foot_name in s]
        self.feet_indices = torch.tensor(feet, dtype=torch.long, device=dev)
        pen = [i for name in cfg.asset.penalize_contacts_on for i, s in enumerate(self.body_names) if name in s]
        self.penalized_contact_indices = torch.tensor(pen, dtype=torch.long, device=dev)
        term = [i for name in cfg.asset.terminate_after_contacts_on for i, s in enumerate(self.body_names) if name in s]
        self.termination_contact_indices = torch.tensor(term, dtype=torch.long, device=dev)
        self._terrain_setup()
        self._randomise()

    def _terrain_setup(self):
        """create_sim's terrain part (WG:235-253): mesh_type 'plane' / None is flat ground at z = 0; 'trimesh' or
        'heightfield' with the widowGo1 Perlin parameters (zScale, tot_cols, tot_rows) generates the fractal
        terrain of utils/terrain.py:40-99 and attaches its height grid to the contact kernel."""
        t = self.cfg.terrain
        self.height_samples = None
        self.terrain = None
        if t.mesh_type in ("trimesh", "heightfield") and hasattr(t, "zScale"):
            from .terrain import TerrainPerlin
            self.terrain = TerrainPerlin(t, seed=self._seed)
            self.set_heightfield(self.terrain.heightsamples, self.terrain.horizontal_scale, self.terrain.vertical_scale,
                                 *self.terrain.transform)
        elif t.mesh_type in ("trimesh", "heightfield") and hasattr(t, "terrain_proportions"):
            # the base class's sub-terrain grid (LR:79-95 create_sim -> Terrain(cfg.terrain, num_envs), utils/terrain.py:101-227);
            # np.random is the reference's stream for it (seeded as helpers.set_seed does)
            from .terrain import Terrain
            saved = np.random.get_state()             # building an env must not reseed the process-global numpy stream
            try:
                np.random.seed(self._seed)
                self.terrain = Terrain(t, self.num_envs)
            finally:
                np.random.set_state(saved)
            self.set_heightfield(self.terrain.heightsamples, self.terrain.horizontal_scale, self.terrain.vertical_scale,
                                 *self.terrain.transform)

    def set_heightfield(self, heights_i16: np.ndarray, horizontal_scale, vertical_scale, tx, ty, tz):
        self.sim.set_heightfield(heights_i16, horizontal_scale, vertical_scale, tx, ty, tz)
        self.height_samples = torch.from_numpy(np.asarray(heights_i16)).to(self.device)

    def _randomise(self):
        """Host-side draws of _get_env_origins WG:207-228, _process_rigid_shape_props WG:468-496,
        _process_rigid_body_props WG:431-456, motor strengths WG:402-408, trajectory timing WG:574-575 (draw_env_params)."""
        cfg, n = self.cfg, self.num_envs
        t = cfg.terrain
        gen = torch.Generator(device="cpu")
        gen.manual_seed(self._seed)
        grid = self.terrain is not None and hasattr(self.terrain, "proportions")          # the base class's Terrain
        self._terrain_levels_on = bool(self.terrain is not None and (grid or t.curriculum))
        p = draw_env_params(cfg, n, self._seed, self.dt, strip_origins=not grid, levels=self._terrain_levels_on, gen=gen)
        origins = p.pop("env_origins")
        self.env_origins = origins.to(self.device)
        self.custom_origins = True
        if self._terrain_levels_on:                 # base-class placement on the terrain's (level, type) platforms, LR:717-731
            if not grid:
                self.terrain.level_grid(int(t.num_rows), int(t.num_cols))
            origins = self._get_env_origins_levels(p.pop("levels_gen")).cpu()
        p.pop("levels_gen", None)
        self.sim.set_env_params(env_origins=origins.numpy(), **p)
        self.sim.set_curriculum(make_curriculum(cfg, max(self.update_counter, 0)))

    def _init_buffers(self):
        """Zero-copy views with the attribute names of WG:498-672."""
        s, dev, tc = self.sim, self.device, self.tcfg
        T = s.tensor
        self._root_states = T("ROOT_STATES")
        self.root_states, self.box_root_state = self._root_states[:, 0, :], self._root_states[:, 1, :]
        self.dof_state = T("DOF_STATE").view(self.num_envs * self.num_dofs, 2)
        dv = T("DOF_STATE")
        self.dof_pos, self.dof_vel = dv[..., 0], dv[..., 1]
        self.dof_pos_wo_gripper, self.dof_vel_wo_gripper = self.dof_pos[:, :-2], self.dof_vel[:, :-2]
        self.base_quat = self.root_states[:, 3:7]
        self._contact_forces = T("NET_CONTACT_FORCE")
        self.contact_forces, self.box_contact_force = self._contact_forces[:, :-1, :], self._contact_forces[:, -1, :]
        self._rigid_body_state = T("RIGID_BODY_STATE")
        self.rigid_body_state, self.box_rigid_body_state = self._rigid_body_state[:, :-1, :], self._rigid_body_state[:, -1, :]
        self.force_sensor_tensor = T("FORCE_SENSOR")
        self.ee_pos = self.rigid_body_state[:, self.gripper_idx, :3]
        self.ee_orn = self.rigid_body_state[:, self.gripper_idx, 3:7]
        self.ee_vel = self.rigid_body_state[:, self.gripper_idx, 7:]
        self.box_pos = self.box_root_state[:, 0:3]
        self.obs_buf = T("OBS_BUF")
        self.obs_history_buf = T("OBS_HISTORY")
        self.action_history_buf = T("ACTION_HISTORY")
        self.rew_buf, self.arm_rew_buf = T("REW_BUF"), T("ARM_REW_BUF")
        self.reset_buf = T("RESET_BUF")
        self._episode_length_buf = T("EPISODE_LENGTH")
        self.time_out_buf = T("TIME_OUT_BUF").view(torch.bool)
        self.torques, self.actions, self.last_actions = T("TORQUES"), T("ACTIONS"), T("LAST_ACTIONS")
        self.last_dof_vel, self.last_root_vel = T("LAST_DOF_VEL"), T("LAST_ROOT_VEL")
        self.commands = T("COMMANDS")
        self.base_lin_vel, self.base_ang_vel = T("BASE_LIN_VEL"), T("BASE_ANG_VEL")
        g = T("GOAL_STATE")
        self.ee_start_sphere, self.ee_goal_sphere, self.ee_goal_cart = g[:, 0:3], g[:, 3:6], g[:, 6:9]
        self.curr_ee_goal_sphere, self.curr_ee_goal_cart = g[:, 9:12], g[:, 12:15]
        self.ee_goal_delta_orn_euler, self.ee_goal_orn_euler = g[:, 15:18], g[:, 18:21]
        self.goal_timer, self.traj_timesteps, self.traj_total_timesteps = g[:, 21], g[:, 22], g[:, 23]
        self.curr_ee_goal = self.curr_ee_goal_cart if self.cfg.goal_ee.command_mode == "cart" else self.curr_ee_goal_sphere
        self.mass_params_tensor = T("MASS_PARAMS")
        self.friction_coeffs_tensor = T("FRICTION")
        self.motor_strength = T("MOTOR_STRENGTH")
        self._episode_sums, self._metric_sums = T("EPISODE_SUMS"), T("METRIC_SUMS")
        self._episode_sums_done, self._metric_sums_done = T("EPISODE_SUMS_DONE"), T("METRIC_SUMS_DONE")
        self.episode_sums = {name: self._episode_sums[:, i] for i, name in enumerate(abi.REWARD_TERMS)}
        self.episode_metric_sums = {name: self._metric_sums[:, i] for i, name in enumerate(abi.METRIC_NAMES)}
        f = lambda arr: torch.tensor(list(arr), dtype=torch.float, device=dev)    # noqa: E731
        self.p_gains, self.d_gains = f(tc.p_gains), f(tc.d_gains)
        self.default_dof_pos = f(tc.default_dof_pos)
        self.default_dof_pos_wo_gripper = self.default_dof_pos[:-2]
        self.torque_limits = f(tc.torque_limits)
        self.action_scale = f(tc.action_scale)
        m = self.robot_model
        self.dof_pos_limits = torch.tensor(np.stack([m.dof_lower, m.dof_upper], 1), dtype=torch.float, device=dev)   # LR:294-296
        self.dof_vel_limits = torch.tensor(m.dof_velocity, dtype=torch.float, device=dev)
        self.commands_scale = f(tc.commands_scale)
        # operational-space controller of the torque-supervision path (WG:559-565, 664-670)
        self.arm_osc_kp = torch.tensor(np.asarray(self.cfg.arm.osc_kp, dtype=np.float64), dtype=torch.float, device=dev)
        self.arm_osc_kd = torch.tensor(np.asarray(self.cfg.arm.osc_kd, dtype=np.float64), dtype=torch.float, device=dev)
        self.ee_orn_des = torch.tensor([0, 0.7071068, 0, 0.7071068], device=dev).repeat((self.num_envs, 1))
        self.z_invariant_offset = torch.full((self.num_envs, 1), float(tc.z_invariant_offset), device=dev)
        self._arm_link_rb = list(range(m.num_rigid_bodies - 9, m.num_rigid_bodies))
        self.link_mass = torch.tensor(m.rb_mass[-9:], dtype=torch.float, device=dev).unsqueeze(0).repeat((self.num_envs, 1))
        self.common_step_counter = 0
        self.extras = {"episode": {}}
        self._active_terms = None
        self._reset_travel = T("RESET_TRAVEL")
        self._sim_env_origins = T("ENV_ORIGINS")                                     # what the kernel's resets read
        if self.cfg.terrain.measure_heights:                                         # WG:637-639
            self.height_points = self._init_height_points()
        self.measured_heights = 0
        self._refresh_ranges()

    @property
    def episode_length_buf(self):
        return self._episode_length_buf

    @episode_length_buf.setter
    def episode_length_buf(self, value):          # OnPolicyRunner.learn re-binds this attribute (OPR:107-108)
        self._episode_length_buf.copy_(value)

    # ---- curriculum ------------------------------------------------------------------------
    def _refresh_ranges(self):
        cur = make_curriculum(self.cfg, self.update_counter)
        self._cur = cur
        self.lin_vel_x_ranges = np.array(list(cur.lin_vel_x_range))
        self.ang_vel_yaw_ranges = np.array(list(cur.ang_vel_yaw_range))
        self.goal_ee_l_ranges = np.array(list(cur.goal_l_range))
        self.goal_ee_p_ranges = np.array(list(cur.goal_p_range))
        self.goal_ee_y_ranges = np.array(list(cur.goal_y_range))
        # keys = the config's non-zero scales, fixed at construction (WG:128-157); values = the current (scheduled) scales
        self.reward_scales = {n: cur.leg_reward_scale[i] for i, n in enumerate(abi.REWARD_TERMS) if (cur.leg_active_mask >> i) & 1}
        self.arm_reward_scales = {n: cur.arm_reward_scale[i] for i, n in enumerate(abi.REWARD_TERMS) if (cur.arm_active_mask >> i) & 1}
        if self._active_terms is None:     # episode_sums keys = the config's non-zero scales, fixed at construction (WG:128-163)
            from .curriculum import _scales
            cfg_leg, cfg_arm = _scales(self.cfg.rewards.scales), _scales(self.cfg.rewards.arm_scales)
            self._active_terms = [(i, n) for i, n in enumerate(abi.REWARD_TERMS) if cfg_leg.get(n, 0) != 0 or cfg_arm.get(n, 0) != 0]
            self._episode_vector_index = {"rew_" + n: i for i, n in self._active_terms}
            self._episode_vector_index.update({"metric_" + n: abi.NREW + i for i, n in enumerate(abi.METRIC_NAMES)})
        return cur

    def update_command_curriculum(self):                                            # WG:678-692
        self.update_counter += 1
        self.sim.set_curriculum(self._refresh_ranges())

    # ---- stepping --------------------------------------------------------------------------
    def reset_idx(self, env_ids, start=False):
        if len(env_ids) == 0:
            return
        if not start or len(env_ids) != self.num_envs:
            raise NotImplementedError("per-env resets happen inside the fused step; only reset_idx(all, start=True) is exposed")
        self.sim.reset_all()
        self._fill_extras(start=True)

    def _fill_extras(self, start=False):
        """extras['episode'] / extras['time_outs'] of WG:743-754, 902-906, without host syncs."""
        if self.collect_episode_stats:
            scale = 1.0 / self.max_episode_length_s
            self.flush_stats_job()                       # a deferred job nobody took: its inputs are about to be overwritten
            if self.defer_episode_stats and not start:   # the launch is left to whoever takes the job (the next policy inference)
                stv, self._stats_job = self.sim.episode_stats_job(scale, *self._track)
            elif self.async_episode_stats and self.device.type == "cuda":
                if self._stats_stream is None:
                    self._stats_stream = torch.cuda.Stream(self.device)
                side = self._stats_stream
                side.wait_stream(torch.cuda.current_stream(self.device))                # after the step kernel's writes
                with torch.cuda.stream(side):
                    stv = self.sim.episode_stats(scale, *self._track)
                self._stats_pending = True                                              # the next step() waits for it (it rewrites the inputs)
            else:
                stv = self.sim.episode_stats(scale, *self._track)
            st = stv.unbind(0)                                                           # one launch (or side job), 32 scalar views
            ep = EpisodeInfo()
            ep.vector, ep.vector_index = stv, self._episode_vector_index                 # the same numbers as ONE device tensor
            for i, name in self._active_terms:
                ep["rew_" + name] = st[i]
            for i, name in enumerate(abi.METRIC_NAMES):
                ep["metric_" + name] = st[abi.NREW + i]
            ep["coeff_lin_vel_x_upper_bound"] = self.lin_vel_x_ranges[1]
            ep["coeff_lin_vel_x_lower_bound"] = self.lin_vel_x_ranges[0]
            ep["coeff_ang_vel_yaw_upper_bound"] = self.ang_vel_yaw_ranges[1]
            ep["coeff_ang_vel_yaw_lower_bound"] = self.ang_vel_yaw_ranges[0]
            ep["coeff_tracking_ang_vel_yaw_exp"] = self.reward_scales.get("tracking_ang_vel_yaw_exp", 0.0)
            self.extras["episode"] = ep
        if self.cfg.env.send_timeouts:
            if self._stale_time_outs_on:                 # opt-in quirk Q9; at construction the reference binds the all-False initial mask
                prev = self._stale_mask if self._stale_mask is not None and not start else torch.zeros_like(self.time_out_buf)
                self._stale_mask = stale_time_outs(prev, self.time_out_buf, self.reset_buf) if not start else prev
                self.extras["time_outs"] = self._stale_mask
            else:
                self.extras["time_outs"] = self.time_out_buf

    # ---- whole-body Jacobian / mass matrix (WG:509-510, 517-518, 550-558): created on first use, refreshed only on request ------
    @property
    def jacobian_whole(self) -> torch.Tensor:
        """f32 [N, 27, 6, 26], persistent: views taken of it (the reference's ee_j_eef) follow refresh_jacobian_tensors()."""
        return self.sim.acquire_jacobian_tensor()

    @property
    def mm_whole(self) -> torch.Tensor:
        """f32 [N, 26, 26], persistent: views taken of it (the reference's mm) follow refresh_mass_matrix_tensors()."""
        return self.sim.acquire_mass_matrix_tensor()

    def refresh_jacobian_tensors(self):
        self.sim.refresh_jacobian_tensors()

    def refresh_mass_matrix_tensors(self):
        self.sim.refresh_mass_matrix_tensors()

    # ---- whole-body inverse dynamics (no counterpart in the reference, whose get_g_torques covers nine arm links' weight only) ----
    @property
    def bias_forces(self) -> torch.Tensor:
        """f32 [N, 26], persistent: h = C(q, nu) nu + g(q) in the coordinates of mm_whole; follows refresh_bias_force_tensors()."""
        return self.sim.acquire_bias_force_tensor()

    def refresh_bias_force_tensors(self):
        self.sim.refresh_bias_force_tensors()

    def inverse_dynamics(self, nudot: torch.Tensor = None) -> torch.Tensor:
        """A fresh f32 [N, 26] tau = M nudot + C nu + g of the current state (nudot None: h): rows 0:3 net external force, 3:6 net
        external moment about the root origin (world axes), 6: joint torques (include/wbc_sim.h: wbc_sim_inverse_dynamics)."""
        tau = torch.empty(self.num_envs, 6 + self.num_dofs, dtype=torch.float32, device=self.device)
        self.sim.inverse_dynamics(nudot=nudot, tau=tau)
        return tau

    def gravity_forces(self) -> torch.Tensor:
        """A fresh f32 [N, 26] g(q): what holds the current pose still against sim.gravity."""
        grav = torch.empty(self.num_envs, 6 + self.num_dofs, dtype=torch.float32, device=self.device)
        self.sim.inverse_dynamics(grav=grav)
        return grav

    # ---- M^-1 (no counterpart in the reference, which calls pinv on the gathered arm block): one launch, M never leaves the device ----
    def mass_matrix_solve(self, rhs: torch.Tensor, armature: bool = False) -> torch.Tensor:
        """A fresh f32 M^-1 rhs of the current state, rhs [N, 26] or [N, K, 26] (K <= 32; a strided view such as
        jacobian_whole[:, r] is taken as it stands). armature: with the implicit-PD joint armature on the diagonal, the matrix a
        substep integrates with (include/wbc_sim.h: wbc_sim_mass_solve). Fingers: exactly 0."""
        return self.sim.mass_solve(rhs, armature=armature)

    def forward_dynamics(self, tau: torch.Tensor = None, armature: bool = False) -> torch.Tensor:
        """A fresh f32 [N, 26] nudot = M^-1 (tau - h), the inverse of inverse_dynamics: tau rows 0:3 net external force, 3:6 net
        external moment about the root origin (world axes), 6: joint torques; None: zeros (include/wbc_sim.h:
        wbc_sim_forward_dynamics). Contacts enter as J^T f added to tau by the caller."""
        return self.sim.forward_dynamics(tau, armature=armature)

    def operational_space_inverse_inertia(self, rigid_body: int, armature: bool = False) -> torch.Tensor:
        """f32 [N, 6, 6] inverse operational-space inertia J_r M^-1 J_r^T of rigid body r's origin (rows linear, angular; world
        frame). Refreshes jacobian_whole. It is NOT inverted here: it can be near-singular, and whether and how to invert it is the
        caller's decision."""
        self.sim.refresh_jacobian_tensors()
        J = self.jacobian_whole[:, int(rigid_body)]                                   # [N, 6, 26], env stride 27 * 156
        return torch.bmm(self.sim.mass_solve(J, armature=armature), J.transpose(1, 2))

    # ---- task-space accelerations and stance-constrained forward dynamics (no counterpart in the reference) ------------------------
    def rigid_body_accelerations(self, nudot: torch.Tensor = None) -> torch.Tensor:
        """A fresh f32 [N, 27, 6]: J nudot + Jdot nu of every rigid-body origin in the layout of rigid_body_state[..., 7:13]
        (classical world-frame linear acceleration, angular acceleration). nudot None: zeros, i.e. the task-space bias acceleration
        Jdot nu (include/wbc_sim.h: wbc_sim_body_accelerations)."""
        return self.sim.body_accelerations(nudot)

    def stance_forward_dynamics(self, tau: torch.Tensor = None, stance: torch.Tensor = None, armature: bool = False):
        """(nudot [N, 26], foot_forces [N, 4, 3]): forward dynamics with the origins of the stance feet (feet_indices) held at zero
        linear acceleration. stance: bool [N, 4] such as get_foot_contacts(), None: all four feet. foot_forces are the forces applied
        TO the robot in world axes, exactly 0 for a swing foot (include/wbc_sim.h: wbc_sim_constrained_dynamics)."""
        if self.__dict__.get("_feet_list") is None:
            self._feet_list = [int(i) for i in self.feet_indices.tolist()]
        return self.sim.constrained_dynamics(self._feet_list, tau=tau, active=stance, armature=armature)

    def touchdown_impact(self, stance: torch.Tensor = None, restitution: float = 0.0, push: torch.Tensor = None, apply: bool = False):
        """(nu_plus [N, 26], foot_impulses [N, 4, 3], denergy [N]): the velocity just after the feet in `stance` (bool [N, 4], the feet
        in contact AFTER the event; None: all four) have met the ground with Newton restitution `restitution`, and / or the
        generalised impulse push [N, 26] has acted (rows as tau of forward_dynamics). foot_impulses are in N s, applied TO the robot in
        world axes, exactly 0 for a foot that is not in stance; denergy is the kinetic energy gained (<= 0 for a pure impact).
        apply=True writes nu_plus into the root and DoF velocities (set_root_state / set_dof_state; positions and the locked fingers
        untouched); by default the sim is left as it is (include/wbc_sim.h: wbc_sim_impulse_dynamics)."""
        if self.__dict__.get("_feet_list") is None:
            self._feet_list = [int(i) for i in self.feet_indices.tolist()]
        r = self.sim.impulse_dynamics(self._feet_list, active=stance, restitution=restitution if restitution else None, impulse_ext=push,
                                      want_energy=True)
        if apply:
            root, dof = self.sim.tensor("ROOT_STATES").clone(), self.sim.tensor("DOF_STATE").clone()
            root[:, 0, 7:13] = r["nu_plus"][:, :6]
            dof[:, :-2, 1] = r["nu_plus"][:, 6:-2]
            self.sim.set_root_state(root.contiguous())
            self.sim.set_dof_state(dof.contiguous())
        return r["nu_plus"], r["impulse"], r["denergy"]

    def impact_map(self, stance: torch.Tensor = None, restitution: float = 0.0) -> torch.Tensor:
        """f32 [N, 26, 26]: d nu+ / d nu of touchdown_impact, the exact linear map of the velocity across the event (nu+ = P nu without
        a push); finger rows and columns exactly 0."""
        if self.__dict__.get("_feet_list") is None:
            self._feet_list = [int(i) for i in self.feet_indices.tolist()]
        return self.sim.impulse_dynamics(self._feet_list, active=stance, restitution=restitution if restitution else None,
                                         want_map=True)["dnu_dnu"]

    def stance_forward_dynamics_derivatives(self, tau: torch.Tensor = None, stance: torch.Tensor = None, armature: bool = False):
        """stance_forward_dynamics linearised: (nudot [N, 26], foot_forces [N, 4, 3], dnudot_dq, dnudot_dnu, dnudot_dtau [N, 26, 26],
        dforces_dq, dforces_dnu, dforces_dtau [N, 12, 26]) with [e, i, j] = d (.)_i / d x_j, in the tangent convention of
        inverse_dynamics_derivatives; the rows of a swing foot are exactly 0 (include/wbc_sim.h:
        wbc_sim_constrained_dynamics_derivatives)."""
        if self.__dict__.get("_feet_list") is None:
            self._feet_list = [int(i) for i in self.feet_indices.tolist()]
        r = self.sim.constrained_dynamics_derivatives(self._feet_list, tau=tau, active=stance, armature=armature)
        return (r["nudot"], r["lambda"]) + tuple(r[k] for k in self.sim.CDD_OUTPUTS)

    def whole_body_inverse_dynamics(self, base_acc: torch.Tensor = None, ee_acc: torch.Tensor = None, swing_acc: torch.Tensor = None,
                                    stance: torch.Tensor = None, qdd_ref: torch.Tensor = None, weights: dict = None,
                                    armature: bool = False):
        """The classical whole-body controller as one call (include/wbc_sim.h: wbc_sim_task_inverse_dynamics): the joint torques that
        give the trunk the acceleration base_acc [N, 6], the gripper ee_acc [N, 6] (linear, angular; world axes) and the swing feet
        the linear accelerations swing_acc [N, 4, 3], while the stance feet (stance bool [N, 4] such as get_foot_contacts(), None: all
        four) stay put. A task that is None carries no weight; a foot's task weight is 0 where it stands, so swing_acc needs a
        stance mask (it is refused with stance=None, where every foot stands). qdd_ref [N, 26]: the
        posture term's target for nudot (None: zeros). weights: dict with any of base, ee, swing (task weights, default 1), posture,
        force, torque, damping (defaults of WbcSim.task_inverse_dynamics). No friction cones or torque limits: clamp the result, or
        call whole_body_controller, which solves with them.
        Returns (torques [N, 20] for sim.set_dof_forces, nudot [N, 26], foot_forces [N, 4, 3])."""
        acc, w, scalars = self._whole_body_tasks(base_acc, ee_acc, swing_acc, stance, weights)
        tau, nudot, lam = self.sim.task_inverse_dynamics(self._feet_list, [0, int(self.gripper_idx)] + self._feet_list, acc, w,
                                                         active=stance, nudot_ref=qdd_ref, armature=armature, **scalars)
        return tau[:, 6:].contiguous(), nudot, lam

    def _whole_body_tasks(self, base_acc, ee_acc, swing_acc, stance, weights):
        """(acc [N, 6, 6], w [N, 6, 6], scalar weights) of the trunk, gripper and four foot tasks of the whole-body calls."""
        if self.__dict__.get("_feet_list") is None:
            self._feet_list = [int(i) for i in self.feet_indices.tolist()]
        n, dev = self.num_envs, self.device
        wts = dict(base=1.0, ee=1.0, swing=1.0)
        wts.update(weights or {})
        acc = torch.zeros((n, 6, 6), dtype=torch.float32, device=dev)
        w = torch.zeros((n, 6, 6), dtype=torch.float32, device=dev)
        if base_acc is not None:
            acc[:, 0], w[:, 0] = base_acc, float(wts["base"])
        if ee_acc is not None:
            acc[:, 1], w[:, 1] = ee_acc, float(wts["ee"])
        if swing_acc is not None:
            assert stance is not None, "swing_acc needs a stance mask: with stance=None all four feet stand and no foot has a swing task"
            acc[:, 2:, 0:3] = swing_acc
            w[:, 2:, 0:3] = float(wts["swing"]) * (~stance.bool()).float().unsqueeze(-1)
        return acc, w, {k: float(wts[k]) for k in ("posture", "force", "torque", "damping") if k in wts}

    def whole_body_controller(self, base_acc: torch.Tensor = None, ee_acc: torch.Tensor = None, swing_acc: torch.Tensor = None,
                              stance: torch.Tensor = None, qdd_ref: torch.Tensor = None, weights: dict = None, armature: bool = False,
                              mu=0.5, fn_min: float = 0.0, tau_limit: torch.Tensor = None, normal: torch.Tensor = None, max_iter: int = 0):
        """whole_body_inverse_dynamics with the limits a robot has (include/wbc_sim.h: wbc_sim_task_inverse_dynamics_qp): the same tasks
        and weights, solved subject to |torque| <= tau_limit [N, 18] (None: the config's torque_limits) and, for every stance foot, a
        normal force of at least fn_min and a friction pyramid of coefficient mu (a float or [N, 4]) about normal [N, 4, 3] (None: world
        z). Returns (torques [N, 20] for sim.set_dof_forces, nudot [N, 26], foot_forces [N, 4, 3], info) with info["status"] (0 optimal;
        1, 2: the unconstrained optimum clamped to the torque limits), info["active_set"] and info["iterations"]."""
        acc, w, scalars = self._whole_body_tasks(base_acc, ee_acc, swing_acc, stance, weights)
        tau, nudot, lam, info = self.sim.task_inverse_dynamics_qp(self._feet_list, [0, int(self.gripper_idx)] + self._feet_list, acc, w,
                                                                  active=stance, nudot_ref=qdd_ref, armature=armature, mu=mu, fn_min=fn_min,
                                                                  tau_limit=tau_limit, normal=normal, max_iter=max_iter, **scalars)
        return tau[:, 6:].contiguous(), nudot, lam, info

    # ---- whole-body inverse kinematics (no counterpart in the reference): one launch, include/wbc_sim.h: wbc_sim_inverse_kinematics ----
    def reach_configuration(self, ee_pos: torch.Tensor, ee_quat: torch.Tensor = None, stance: torch.Tensor = None,
                            base_height: torch.Tensor = None, apply: bool = False, refine: int = 2, refine_posture: float = 1e-5,
                            refine_step_tol: float = 1e-5, **opts):
        """(root_pose [N, 7], dof_pos [N, 20], info): the configuration near the current one, inside the joint limits, that keeps the
        feet in `stance` (bool [N, 4]; None: all four) where they are now and puts the gripper at ee_pos [N, 3] (world) and, if given,
        at the orientation ee_quat [N, 4] (xyzw); base_height [N] asks for that world height of the trunk's origin as well.
        The first solve regularises the posture towards default_dof_pos (opts: posture, damping, step_tol, max_iter of
        WbcSim.inverse_kinematics). Its posture term trades against the targets (it misses them by about posture * dq / lever:
        centimetres at the default weight where the joints end 1 rad from default_dof_pos), so `refine` further solves follow, each
        from the last answer with q_ref that answer itself and the small weight refine_posture (a proximal step: the posture term
        vanishes at its start and only picks among the configurations that meet the targets the one nearest to the last answer).
        Over the tests' family the targets are then met to 3e-5 m after one and 1e-7 m after two such solves, each of a few
        iterations; refine=0 returns the first solve's trade-off. A goal out of reach keeps its residual through every solve.
        apply=True writes the result into the root and DoF states with zero velocities (set_root_state / set_dof_state); by default
        the sim is left as it is. info is the last solve's (rows: the four feet, the gripper, then the trunk), its "iterations" the
        sum over the solves."""
        if self.__dict__.get("_feet_list") is None:
            self._feet_list = [int(i) for i in self.feet_indices.tolist()]
        n, dev = self.num_envs, self.device
        self.sim.refresh_rigid_body_state()
        bodies = self._feet_list + [int(self.gripper_idx)] + ([0] if base_height is not None else [])
        k = len(bodies)
        pos = torch.zeros(n, k, 3, dtype=torch.float32, device=dev)
        w = torch.zeros(n, k, 3, dtype=torch.float32, device=dev)
        pos[:, :4] = self.rigid_body_state[:, self.feet_indices, :3]
        w[:, :4] = 1.0 if stance is None else stance.bool().float().unsqueeze(-1)
        pos[:, 4], w[:, 4] = ee_pos, 1.0
        if base_height is not None:
            pos[:, 5, 2], w[:, 5, 2] = base_height, 1.0
        quat = w_ori = None
        if ee_quat is not None:
            quat = torch.zeros(n, k, 4, dtype=torch.float32, device=dev)
            quat[..., 3] = 1.0
            quat[:, 4] = ee_quat
            w_ori = torch.zeros(n, k, dtype=torch.float32, device=dev)
            w_ori[:, 4] = 1.0
        q_ref = self.default_dof_pos.to(torch.float32).expand(n, -1).contiguous()
        root, dof, info = self.sim.inverse_kinematics(bodies, pos, quat, w, w_ori, q_ref=q_ref, **opts)
        total = info["iterations"]
        for _ in range(int(refine)):
            root, dof, info = self.sim.inverse_kinematics(bodies, pos, quat, w, w_ori, root_init=root, dof_init=dof, posture=refine_posture,
                                                          damping=opts.get("damping", 1e-3), step_tol=refine_step_tol,
                                                          max_iter=opts.get("max_iter", 0))
            total = total + info["iterations"]
        info = dict(info, iterations=total)
        if apply:
            rs, ds = self.sim.tensor("ROOT_STATES").clone(), self.sim.tensor("DOF_STATE").clone()
            rs[:, 0, :7], rs[:, 0, 7:13] = root, 0.0
            ds[..., 0], ds[..., 1] = dof, 0.0
            self.sim.set_root_state(rs.contiguous())
            self.sim.set_dof_state(ds.contiguous())
        return root, dof, info

    def ee_goal_reachable(self, ee_pos: torch.Tensor, tol: float = 1e-3, **opts) -> torch.Tensor:
        """bool [N]: the gripper can reach ee_pos [N, 3] (world) with all four feet where they are and every joint inside its limits:
        reach_configuration's last solve converged (status 0) and left the gripper within `tol` metres of the goal. The root and DoF
        states are left untouched. opts: reach_configuration's."""
        _, _, info = self.reach_configuration(ee_pos, **opts)
        return (info["status"] == 0) & (info["residual"][:, 4, :3].norm(dim=-1) <= tol)

    # ---- centre of mass and centroidal momentum (no counterpart in the reference): one launch, include/wbc_sim.h: wbc_sim_centroidal ----
    def centre_of_mass(self):
        """(position [N, 3], velocity [N, 3]) of the robot's centre of mass in the world frame: the root position plus the kernel's
        offset from the root origin (the kernel itself never reads the position), and v_com."""
        com = self.sim.centroidal()[0]
        return self.root_states[:, 0:3] + com[:, 0:3], com[:, 3:6]

    def centroidal_momentum(self, nudot: torch.Tensor = None):
        """(h_G [N, 6], hdot_G [N, 6]): linear momentum and angular momentum about the centre of mass (world axes), and their rate
        A_G nudot + Adot_G nu -- the net external wrench about the centre of mass, weight included. nudot None: zeros (Adot_G nu)."""
        mom = self.sim.centroidal(nudot)[1]
        return mom[:, 0:6], mom[:, 6:12]

    def centroidal_momentum_matrix(self) -> torch.Tensor:
        """A fresh f32 [N, 6, 26] A_G with h_G = A_G nu in the coordinates of mm_whole; A_G[:, 0:3] / mass is the centre-of-mass Jacobian."""
        return self.sim.centroidal()[2]

    def centroidal_inertia(self):
        """(mass [N], I_G [N, 3, 3]): the total mass and the locked centroidal inertia in world axes."""
        inr = self.sim.centroidal()[3]
        return inr[:, 0], inr[:, [1, 4, 5, 4, 2, 6, 5, 6, 3]].view(-1, 3, 3)

    # ---- Coriolis matrix and momentum observer (no counterpart in the reference): include/wbc_sim.h: wbc_sim_coriolis ----
    def coriolis_matrix(self) -> torch.Tensor:
        """A fresh f32 [N, 26, 26] C(q, nu) of M nudot + C nu + g = tau in the coordinates of mm_whole, in the factorisation with
        C + C^T = dM/dt: C nu == bias_forces - gravity_forces. One launch."""
        return self.sim.coriolis(cmat=torch.empty((self.num_envs, 26, 26), dtype=torch.float32, device=self.device))[0]

    def mass_matrix_rate(self) -> torch.Tensor:
        """A fresh f32 [N, 26, 26] dM/dt of mm_whole along the current velocity, bit-symmetric. One launch."""
        return self.sim.coriolis(mdot=torch.empty((self.num_envs, 26, 26), dtype=torch.float32, device=self.device))[0]

    def generalized_momentum(self) -> torch.Tensor:
        """A fresh f32 [N, 26] p = mm_whole nu, without forming the matrix. One launch of the vector kernel."""
        return self.sim.coriolis(vec=torch.empty((self.num_envs, 2, 26), dtype=torch.float32, device=self.device))[0][:, 0]

    def external_torque_estimate(self, gain: float, reset: bool = False) -> torch.Tensor:
        """The momentum observer's residual f32 [N, 26] after one update at the current state with the env's own joint torques
        (`torques`, rows 6:; no known wrench on the root) and control step `dt`: a first-order low-pass, of bandwidth `gain` (1/s,
        gain dt < 1), of the generalised forces the model does not explain -- contacts, pushes, a payload. Call it once per step();
        the first call, and any call with reset, starts the observer at the current momentum with residual 0."""
        tau = torch.zeros((self.num_envs, 26), dtype=torch.float32, device=self.device)
        tau[:, 6:] = self.torques
        return self.sim.momentum_observer(tau, gain, self.dt, reset=reset)[:, 1]

    # ---- first-order layer (no counterpart in the reference): include/wbc_sim.h: wbc_sim_inverse_dynamics_derivatives ----
    def inverse_dynamics_derivatives(self, nudot: torch.Tensor = None):
        """(dtau_dq, dtau_dnu), fresh f32 [N, 26, 26] indexed [N, i, j] = d tau_i / d x_j of inverse_dynamics(nudot) at the current
        state: one launch. dq is the configuration tangent with "qdot = nu" (root translation, WORLD-frame rotation vector, joint
        increments); the world components of nu and nudot are held fixed."""
        return self.sim.inverse_dynamics_derivatives(nudot)

    def forward_dynamics_derivatives(self, tau: torch.Tensor = None, armature: bool = False):
        """(nudot [N, 26], dnudot_dq, dnudot_dnu, minv [N, 26, 26]), fresh tensors indexed [N, i, j]: forward_dynamics(tau) with its
        partial derivatives -M^-1 dtau/dq, -M^-1 dtau/dnu (taken at that nudot) and d nudot / d tau = M^-1, the linearisation
        d nudot = dnudot_dq dq + dnudot_dnu dnu + minv dtau a trajectory optimiser needs."""
        return self.sim.forward_dynamics_derivatives(tau, armature=armature)

    # ---- body parameters (no counterpart in the reference): include/wbc_sim.h: wbc_sim_inverse_dynamics_regressor ----
    def body_parameter_regressor(self, nudot: torch.Tensor = None) -> torch.Tensor:
        """Y, a fresh f32 [N, 26, 19, 10]: inverse_dynamics(nudot) == sum_b Y[:, :, b] @ pi_b with pi_b = (m, m c, inertia about the
        body origin) of every moving body (abi.linear_body_params(robot_model, body_params)); Y holds no body parameter. One launch:
        the rows of logged (state, torque) pairs for identifying a payload by least squares."""
        return self.sim.inverse_dynamics_regressor(nudot=nudot)

    def randomised_parameter_sensitivity(self, nudot: torch.Tensor = None) -> torch.Tensor:
        """A fresh f32 [N, 26, 20]: d inverse_dynamics(nudot) / d BODY_PARAMS, column for column (root composite (m, com, inertia about
        the centre of mass) at 0:10, gripper body at 10:20), at every env's own randomised values. One launch."""
        bodies = (0, int(self.robot_model.gripper_piece["body"]))
        return self.sim.inverse_dynamics_regressor(bodies, nudot=nudot, native=True).view(self.num_envs, 6 + abi.NDOF, 20)

    # ---- recursive identification (no counterpart in the reference): include/wbc_sim.h: wbc_sim_identification_accumulate ----
    def generalised_force(self, tau: torch.Tensor, foot_forces: torch.Tensor = None, feet=None) -> torch.Tensor:
        """A fresh f32 [N, 26] tau + sum_f J_f^T f_f: the net generalised force of applied forces tau [N, 26] (rows as inverse_dynamics)
        and the world-frame forces foot_forces [N, K, 3] acting on the origins of the rigid bodies `feet` (None: feet_indices), through
        the translational rows of jacobian_whole, which is refreshed. With (nudot, foot_forces) of stance_forward_dynamics(tau) this is
        inverse_dynamics(nudot); with logged torques and force-sensor readings, the tau_gen a parameter_identifier takes."""
        out = tau.to(torch.float32).clone()
        if foot_forces is not None:
            feet = self.feet_indices if feet is None else torch.as_tensor(feet, dtype=torch.long, device=self.device)
            self.sim.refresh_jacobian_tensors()
            J = self.jacobian_whole[:, feet, 0:3, :]                                      # [N, K, 3, 26]
            out += torch.einsum("nkic,nki->nc", J, foot_forces.to(torch.float32))
        return out

    def parameter_identifier(self, bodies=None, forget: float = 1.0) -> "ParameterIdentifier":
        """A recursive least-squares estimator of the linear inertial parameters of `bodies` (1..3 moving-body indices; None: the root
        composite and the gripper body, the two that BODY_PARAMS randomises): see ParameterIdentifier."""
        return ParameterIdentifier(self, bodies, forget)

    # ---- state estimation (no counterpart in the reference): include/wbc_sim.h: wbc_sim_leg_odometry ----
    def base_state_estimator(self, **cfg) -> "BaseStateEstimator":
        """A leg-odometry Kalman filter for the base's linear velocity and position from what the robot can sense, the classical
        counterpart of what the policy has to infer: see BaseStateEstimator (cfg: its noise parameters and dt, default env.dt)."""
        return BaseStateEstimator(self, **cfg)

    # ---- force planning (no counterpart in the reference): include/wbc_sim.h: wbc_sim_centroidal_mpc ----
    def centroidal_mpc(self, horizon: int = 10, dt: float = None, **cfg) -> "CentroidalMPC":
        """The convex model-predictive controller of the foot forces on the single-rigid-body model, the layer that produces the
        base_acc whole_body_controller takes: see CentroidalMPC (cfg: the fields of wbc_mpc_cfg; dt None: env.dt)."""
        return CentroidalMPC(self, horizon, dt, **cfg)

    # ---- gait layer (no counterpart in the reference): include/wbc_sim.h: wbc_sim_footstep_plan ----
    def gait_planner(self, gait="trot", period: float = 0.5, duty: float = 0.5, horizon: int = 10, mpc_dt: float = None, **cfg) -> "FootstepPlanner":
        """The gait clock, the terrain-aware footholds and the swing-foot references that tie base_state_estimator, centroidal_mpc and
        whole_body_controller into a controller: see FootstepPlanner (gait: stand, trot, pace, bound, walk or four phase offsets; cfg:
        the other fields of wbc_footstep_cfg; mpc_dt None: env.dt)."""
        return FootstepPlanner(self, gait, period, duty, horizon, mpc_dt, **cfg)

    # ---- contact detection (no counterpart in the reference): include/wbc_sim.h: wbc_sim_contact_detect ----
    def contact_detector(self, planner: "FootstepPlanner" = None, gain: float = 50.0, **cfg) -> "ContactDetector":
        """The probabilistic contact detector: which feet are on the ground, from the momentum observer's external joint torques, the
        feet's heights and the gait clock of `planner` (None: no gait prior), without the simulator's force sensors: see ContactDetector
        (gain: the observer's bandwidth in 1/s, capped at 0.9 / dt; cfg: the fields of wbc_contact_cfg; dt None: env.dt)."""
        return ContactDetector(self, planner, gain, **cfg)

    # ---- leg controller (no counterpart in the reference): include/wbc_sim.h: wbc_sim_leg_control ----
    def leg_controller(self, **cfg) -> "LegController":
        """The controller below the MPC: stance legs push with the planned foot forces (tau = -J^T f), swing legs follow the planner's
        references by a Cartesian impedance with the acceleration feed-forward, the arm holds a posture: see LegController (cfg: the
        fields of wbc_leg_control_cfg, plus bias, tau_limit and clip)."""
        return LegController(self, **cfg)

    # ---- attitude estimation (no counterpart in the reference): include/wbc_sim.h: wbc_sim_attitude_filter ----
    def attitude_estimator(self, **cfg) -> "AttitudeEstimator":
        """The attitude filter: the trunk's orientation and the gyro's bias from the gyro, the accelerometer and optional heading
        vectors, the estimate of what the other layers take as quat and gyro: see AttitudeEstimator (cfg: the fields of
        wbc_attitude_cfg; dt None: env.dt)."""
        return AttitudeEstimator(self, **cfg)

    # ---- terrain estimation (no counterpart in the reference): include/wbc_sim.h: wbc_sim_ground_estimate ----
    def ground_estimator(self, **cfg) -> "GroundEstimator":
        """The blind terrain estimate: a plane through the most recent footholds, the estimate of what the other layers take as ground,
        foot_height, normal and height: see GroundEstimator (cfg: the fields of wbc_ground_cfg; dt None: env.dt)."""
        return GroundEstimator(self, **cfg)

    # ---- slip detection and friction estimate (no counterpart in the reference): include/wbc_sim.h: wbc_sim_slip_detect ----
    def slip_detector(self, **cfg) -> "SlipDetector":
        """The foot slip detector and friction estimate: which standing feet slide, how far a standing foot can be trusted, and the
        friction coefficient from the force ratio while sliding: see SlipDetector (cfg: the fields of wbc_slip_cfg; dt None: env.dt)."""
        return SlipDetector(self, **cfg)

    def imu(self, gyro_bias=0.0, gyro_noise: float = 0.0, accel_noise: float = 0.0, heading_noise: float = None, seed: int = 0) -> "ImuModel":
        """A small IMU model on the sim's state: gyro, accelerometer and (with heading_noise not None) a heading vector in trunk axes,
        with a constant gyro bias and seeded Gaussian noise: see ImuModel."""
        return ImuModel(self, gyro_bias, gyro_noise, accel_noise, heading_noise, seed)

    # ---- torque supervision (WG:1178-1181, 1201-1242): default off (WGC:173) ------------------------------------
    def _refresh_arm_dynamics(self):
        self.mm, self.ee_j_eef, self._g_torque = self.sim.arm_dynamics(self._arm_link_rb, self.robot_model.rb_mass[-9:])

    def get_g_torques(self):                                                        # WG:1201-1207
        self._refresh_arm_dynamics()
        return self._g_torque

    def get_arm_mm(self):                                                           # WG:1209-1211
        self._refresh_arm_dynamics()
        return self.mm

    def get_ee_jac(self):                                                           # WG:1213-1215
        self._refresh_arm_dynamics()
        return self.ee_j_eef

    def get_arm_ee_control_torques(self):
        """Operational-space control torques of the arm, the supervision target (WG:1217-1242), line by line; the
        mass matrix, the Jacobian and the gravity torques come from wbc_sim_arm_dynamics instead of Isaac Gym."""
        self._refresh_arm_dynamics()
        m_inv = torch.linalg.pinv(self.mm)
        m_eef = torch.linalg.pinv(self.ee_j_eef @ m_inv @ torch.transpose(self.ee_j_eef, 1, 2))
        ee_orn_normalized = self.ee_orn / torch.norm(self.ee_orn, dim=-1).unsqueeze(-1)
        orn_err = _orientation_error(self.ee_orn_des, ee_orn_normalized)
        yaw = _yaw_quat(self.base_quat)
        pos_err = (torch.cat([self.root_states[:, :2], self.z_invariant_offset], dim=1) + _quat_apply(yaw, self.curr_ee_goal_cart) - self.ee_pos)
        dpose = torch.cat([pos_err, orn_err], -1)
        u = (torch.transpose(self.ee_j_eef, 1, 2) @ m_eef @ (self.arm_osc_kp * dpose - self.arm_osc_kd * self.ee_vel)[:, :6].unsqueeze(-1)).squeeze(-1)
        return u + self._g_torque

    def step(self, actions):
        """WG:1156-1199 as one kernel launch; returns the reference's 6-tuple (views, overwritten by the
        next step)."""
        a = actions.to(self.device, dtype=torch.float32)
        if not a.is_contiguous():
            a = a.contiguous()
        if self.cfg.control.torque_supervision:                                     # WG:1178-1181: state at t = 0 of the step
            self.arm_ee_control_torques = self.get_arm_ee_control_torques()
            self.extras["target_arm_torques"] = self.arm_ee_control_torques
            self.extras["current_arm_dof_pos"] = self.dof_pos[:, -8:-2].clone()
            self.extras["current_arm_dof_vel"] = self.dof_vel[:, -8:-2].clone()
        out, self._obs_output = self._obs_output, None
        store, self._store_output = self._store_output, None
        if self._stale_time_outs_on:
            store = None                              # the learner's process_env_step bootstraps from extras['time_outs']
        self.flush_stats_job()                        # deferred statistics of the previous step that nobody carried
        if self._stats_pending:                       # the side-stream statistics of the previous step read what this step overwrites
            torch.cuda.current_stream(self.device).wait_stream(self._stats_stream)
            self._stats_pending = False
        self.sim.step(a, out, store)
        self.extras["rollout_stored"] = store[2].data_ptr() if store is not None else None
        self.common_step_counter += 1
        if self._terrain_levels_on and self.cfg.terrain.curriculum:                  # WG:708-709 (reset_idx -> _update_terrain_curriculum)
            self._apply_terrain_curriculum()
        if self.cfg.terrain.measure_heights:                                         # WG:932-933
            self.measured_heights = self._get_heights()
        self._fill_extras()
        return (self.obs_buf if out is None else out), self.privileged_obs_buf, self.rew_buf, self.arm_rew_buf, self.reset_buf, self.extras

    # ---- the base class's terrain bookkeeping (legged_robot.py:421-441, 717-731, 777-829) --------------
    def _init_height_points(self):                                                   # LR:777-791
        """Points (base frame) at which the terrain height is sampled: [num_envs, num_height_points, 3]."""
        y = torch.tensor(self.cfg.terrain.measured_points_y, device=self.device, requires_grad=False)
        x = torch.tensor(self.cfg.terrain.measured_points_x, device=self.device, requires_grad=False)
        grid_x, grid_y = torch.meshgrid(x, y, indexing="ij")
        self.num_height_points = grid_x.numel()
        points = torch.zeros(self.num_envs, self.num_height_points, 3, device=self.device, requires_grad=False)
        points[:, :, 0] = grid_x.flatten()
        points[:, :, 1] = grid_y.flatten()
        return points

    def _get_heights(self, env_ids=None):                                            # LR:793-829
        """Terrain heights under the height points of each robot (rotated by the base yaw, offset by the base position):
        one launch of wbc_get_heights (csrc/wbc_terrain_kernel.hip), bit-exact against oracle/terrain_oracle.py.
        `height_samples` is the [x, y] grid the contact kernel uses (the reference views its array with the two dimensions
        swapped, quirk Q3, which only stays harmless while measure_heights is False)."""
        t = self.cfg.terrain
        if t.mesh_type == "plane":
            return torch.zeros(self.num_envs, self.num_height_points, device=self.device, requires_grad=False)
        elif t.mesh_type == "none":
            raise NameError("Can't measure height with terrain mesh type 'none'")
        if self.height_samples is None:
            raise RuntimeError("no height samples attached (set_heightfield)")
        quat, pos, pts = self.base_quat, self.root_states, self.height_points
        if env_ids is not None and len(env_ids) > 0:                                 # (the reference: `if env_ids:`)
            ids = torch.as_tensor(env_ids, dtype=torch.long, device=self.device)
            quat, pos, pts = quat[ids].contiguous(), pos[ids].contiguous(), pts[ids]
        pts = pts.contiguous()
        n, npts = pts.shape[0], pts.shape[1]
        hs = self.height_samples
        assert hs.dtype == torch.int16 and hs.is_contiguous() and quat.stride(1) == 1 and pos.stride(1) == 1
        out = torch.empty(n, npts, dtype=torch.float32, device=self.device)
        from .native import check, lib
        check(lib().wbc_get_heights(quat.data_ptr(), quat.stride(0), pos.data_ptr(), pos.stride(0), pts.data_ptr(), hs.data_ptr(),
                                    hs.shape[0], hs.shape[1], float(t.border_size), float(t.horizontal_scale), float(t.vertical_scale),
                                    out.data_ptr(), n, npts, torch.cuda.current_stream(self.device).cuda_stream), "wbc_get_heights")
        return out

    def _get_env_origins_levels(self, gen=None):                                     # LR:717-731, the terrain-level branch
        """terrain_levels / terrain_types / terrain_origins and env_origins on the terrain's platforms."""
        t, n, dev = self.cfg.terrain, self.num_envs, self.device
        max_init_level = t.max_init_terrain_level
        if not t.curriculum:
            max_init_level = t.num_rows - 1
        self.terrain_levels = torch.randint(0, max_init_level + 1, (n,), generator=gen).to(dev)
        self.terrain_types = torch.div(torch.arange(n, device=dev), (n / t.num_cols), rounding_mode="floor").to(torch.long)
        self.max_terrain_level = t.num_rows
        self.terrain_origins = torch.from_numpy(self.terrain.env_origins).to(dev).to(torch.float)
        self.env_origins = torch.zeros(n, 3, device=dev, requires_grad=False)
        self.env_origins[:] = self.terrain_origins[self.terrain_levels, self.terrain_types]
        return self.env_origins

    def _update_terrain_curriculum(self, env_ids):                                   # LR:421-441
        """The game-inspired curriculum for the envs being reset. `distance` and the command norm are the finished episode's
        (WBC_T_RESET_TRAVEL: the fused step has already re-placed these robots and may have resampled their commands)."""
        if not self.init_done:
            return                                                                   # don't change on the initial reset
        travel = self._reset_travel[env_ids]
        distance = travel[:, 0]
        move_up = distance > self.terrain.env_length / 2                             # walked far enough: harder terrain
        move_down = (distance < travel[:, 1] * self.max_episode_length_s * 0.5) * ~move_up   # less than half the commanded distance
        self.terrain_levels[env_ids] += 1 * move_up - 1 * move_down
        self.terrain_levels[env_ids] = torch.where(self.terrain_levels[env_ids] >= self.max_terrain_level,    # solved the last level:
                                                   torch.randint_like(self.terrain_levels[env_ids], self.max_terrain_level),   # a random one
                                                   torch.clip(self.terrain_levels[env_ids], 0))
        self.env_origins[env_ids] = self.terrain_origins[self.terrain_levels[env_ids], self.terrain_types[env_ids]]

    def _apply_terrain_curriculum(self):
        """reset_idx's call of _update_terrain_curriculum (WG:708-709) for the envs the fused step has just reset, without a
        host synchronisation: the rule of LR:431-441 over all envs under the reset mask (same arithmetic as
        _update_terrain_curriculum on reset_buf.nonzero()), then those robots (and their boxes, WG:769-771) move from the old
        platform to the new one -- the in-kernel reset placed them relative to the old origin."""
        if not self.init_done:
            return
        m = self.reset_buf.bool()
        distance, cmd_norm = self._reset_travel[:, 0], self._reset_travel[:, 1]
        move_up = m & (distance > self.terrain.env_length / 2)
        move_down = m & (distance < cmd_norm * self.max_episode_length_s * 0.5) & ~move_up
        lv = self.terrain_levels + (1 * move_up - 1 * move_down)
        lv = torch.where(m & (lv >= self.max_terrain_level), torch.randint_like(lv, self.max_terrain_level), torch.clip(lv, 0))
        self.terrain_levels.copy_(lv)
        new = self.terrain_origins[lv, self.terrain_types]
        delta = new - self._sim_env_origins                            # zero for the envs that did not reset
        self.env_origins.copy_(new)
        self._sim_env_origins.copy_(new)
        self.root_states[:, :3] += delta
        self.box_root_state[:, 1] += delta[:, 1]

    def take_stats_job(self):
        """The deferred statistics of the last step (sim.SideJob) or None; the taker executes it before the next step()."""
        job, self._stats_job = self._stats_job, None
        return job

    def flush_stats_job(self):
        job = self.take_stats_job()
        if job is not None:
            job.run(torch.cuda.current_stream(self.device).cuda_stream)

    def attach_episode_tracker(self, state, cap):
        """The training loop's episode deques (OnPolicyRunner.learn, OPR:140-154) ride on the per-step statistics launch as one
        extra workgroup (wbc_sim_episode_stats_track): `state` = wbc_runner_track_state_floats(num_envs, cap) zeroed floats on the
        sim device, or None to detach. Needs collect_episode_stats (the launch it rides on). Effective from the next step():
        returns the value common_step_counter will have after the first step this env accounts for (steps before it are the caller's)."""
        self._track = (state, int(cap)) if state is not None else (None, 0)
        return int(self.common_step_counter) + 1

    def restore_terrain_levels(self, levels, arena_restored=False):
        """Checkpoint resume (OnPolicyRunner.load): adopt saved terrain levels. env_origins and the sim's ENV_ORIGINS are
        re-derived from terrain_origins[level, type]; unless the whole sim arena came back with them (then every robot already
        stands where it stood), all robots are re-placed by a full reset on their restored platforms -- the next
        _apply_terrain_curriculum must see a zero origin delta for every env that did not just reset."""
        if not self._terrain_levels_on:
            return
        self.terrain_levels.copy_(levels.to(self.terrain_levels.device, self.terrain_levels.dtype))
        new = self.terrain_origins[self.terrain_levels, self.terrain_types]
        self.env_origins.copy_(new)
        if not arena_restored:
            self._sim_env_origins.copy_(new)
            self.sim.reset_all()                      # in-kernel reset: places robot + box relative to ENV_ORIGINS
            self._fill_extras(start=True)

    def set_rollout_output(self, values, gamma, rewards, dones):
        """The NEXT step() also writes this transition's rollout-storage slots (PPO.process_env_step's tensor work, ppo.py:129-141):
        rewards [N,2] = (rew, arm_rew) + gamma * values * time_outs, dones [N,1] u8 = reset_buf != 0; `values` = the critic's
        [N,2] output PPO.act stored for the acting observation. One-shot; extras['rollout_stored'] = rewards.data_ptr() tells
        the learner the slots are filled."""
        self._store_output = (values, float(gamma), rewards, dones)

    def set_obs_output(self, tensor):
        """The NEXT step() writes its observations into `tensor` (f32 [num_envs, 860], contiguous, on the sim device) and
        returns it instead of obs_buf -- the rollout loop passes the storage slot of the next transition, which saves the
        14 MB copy `observations[step].copy_(obs)` per step. One-shot; obs_buf keeps the last observation written to it."""
        self._obs_output = tensor

    # gym-tensor-API style helpers some callers of the reference use
    def get_foot_contacts(self):                                                    # WG:1090-1098
        return self.force_sensor_tensor.norm(dim=-1) > 1.5


class ParameterIdentifier:
    """Recursive least squares for the linear inertial parameters (m, m c, inertia about the body origin) of up to three moving bodies
    of every env, the classical baseline to the learned adaptation module: it owns the per-env normal equations A [N, P, P], b [N, P]
    and stat [N, 2] and feeds them one wbc_sim_identification_accumulate launch per update; estimate() is one
    wbc_sim_identification_solve launch. The other bodies' parameters are taken as the sim holds them."""

    def __init__(self, env, bodies=None, forget: float = 1.0):
        m = env.robot_model
        self.env, self.forget = env, float(forget)
        self.bodies = [int(b) for b in ((0, m.gripper_piece["body"]) if bodies is None else bodies)]
        n, p = env.num_envs, abi.NPARAM * len(self.bodies)
        self.info_mat = torch.zeros((n, p, p), dtype=torch.float32, device=env.device)
        self.info_vec = torch.zeros((n, p), dtype=torch.float32, device=env.device)
        self.stat = torch.zeros((n, 2), dtype=torch.float32, device=env.device)
        nominal = abi.body_params_from_randomisation(m, np.zeros(1), np.zeros((1, 3)), np.zeros(1))
        pi0 = abi.linear_body_params(m, nominal)[0, self.bodies]                          # the nominal model, no randomisation
        self.prior = torch.tensor(pi0, dtype=torch.float32, device=env.device).expand(n, -1, -1).contiguous()
        self.last_target = None

    def update(self, tau_gen: torch.Tensor, nudot: torch.Tensor = None, row_weight: torch.Tensor = None) -> None:
        """One observation per env at the sim's current state: tau_gen [N, 26] (env.generalised_force), the acceleration nudot [N, 26]
        (None: zeros) and the rows' weights [N, 26] (None: 1; an env whose weights are all 0 is left as it is, without decay)."""
        self.last_target = self.env.sim.identification_accumulate(self.bodies, tau_gen, nudot=nudot, row_weight=row_weight,
                                                                  forget=self.forget, info_mat=self.info_mat, info_vec=self.info_vec,
                                                                  stat=self.stat, target=self.last_target)[3]

    def reset(self, env_ids=None) -> None:
        """Forget everything (env_ids None), or everything the listed envs have seen."""
        for t in (self.info_mat, self.info_vec, self.stat):
            if env_ids is None:
                t.zero_()
            else:
                t[env_ids] = 0.0

    def solve(self, prior_weight=None, pivot_tol: float = 1e-5, want=WbcSim.IDENT_OUTPUTS) -> dict:
        """WbcSim.identification_solve on the owned buffers with the nominal model as the prior; prior_weight: None (no prior term),
        a float, or f32 [N, len(bodies), 10]."""
        if prior_weight is not None and not isinstance(prior_weight, torch.Tensor):
            prior_weight = torch.full_like(self.prior, float(prior_weight))
        return self.env.sim.identification_solve(self.info_mat, self.info_vec, self.stat, prior=self.prior, prior_weight=prior_weight,
                                                 pivot_tol=pivot_tol, want=want)

    def estimate(self, prior_weight=None):
        """(body_params_hat f32 [N, 10 len(bodies)], status int32 [N, len(bodies)]): every listed body's (m, c, I_c) -- column for column
        BODY_PARAMS when the bodies are the root and the gripper body -- and the flags of wbc_sim_identification_solve. An env that
        cannot be solved yet (status bit 0) returns the nominal model's parameters."""
        r = self.solve(prior_weight, want=("theta_hat", "status"))
        return r["theta_hat"].view(self.env.num_envs, -1), r["status"]

    def payload(self, prior_weight=None) -> torch.Tensor:
        """f32 [N]: the estimated mass of the gripper body less its nominal mass (the gripper body must be listed)."""
        s = self.bodies.index(int(self.env.robot_model.gripper_piece["body"]))
        return self.estimate(prior_weight)[0][:, abi.NPARAM * s] - self.prior[:, s, 0]



class BaseStateEstimator:
    """The leg-odometry Kalman filter of wbc_sim_leg_odometry for every env: it owns the state x [N, 18] = (p, v, four foot origins) and
    its covariance P [N, 18, 18] and advances them by one launch per update(). Keyword arguments are the fields of wbc_estimator_cfg
    (include/wbc_sim.h); dt defaults to env.dt. The estimator starts reset at the true root position."""

    DEFAULTS = dict(sigma_p=0.02, sigma_v=0.5, sigma_f=0.02, sigma_r=0.005, sigma_rdot=0.1, sigma_z=0.005, kappa=1000.0,
                    p0_p=1e-4, p0_v=0.25, p0_f=1e-4)

    def __init__(self, env, dt: float = None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown estimator parameters: {sorted(unknown)}"
        values = dict(self.DEFAULTS, **cfg)
        self.env = env
        self.cfg = abi.WbcEstimatorCfg(float(env.dt if dt is None else dt), *[float(values[k]) for k in self.DEFAULTS])
        n, dev = env.num_envs, env.device
        self.x = torch.zeros((n, abi.ESTIMATOR_NX), dtype=torch.float32, device=dev)
        self.P = torch.zeros((n, abi.ESTIMATOR_NX, abi.ESTIMATOR_NX), dtype=torch.float32, device=dev)
        self.base_lin_vel = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        self.nis = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.status = torch.zeros((n,), dtype=torch.int32, device=dev)
        self._gravity = torch.tensor(list(env.tcfg.gravity), dtype=torch.float32, device=dev)
        self._plane_height = torch.zeros((n, 4), dtype=torch.float32, device=dev) if env.cfg.terrain.mesh_type in ("plane", None) else None
        self._last_root_vel = env.root_states[:, 7:10].clone()
        self.last_inputs = None
        self.reset()

    @property
    def position(self) -> torch.Tensor:
        """f32 [N, 3]: the estimated position of the trunk's origin, world axes (a view of x)."""
        return self.x[:, 0:3]

    @property
    def velocity(self) -> torch.Tensor:
        """f32 [N, 3]: the estimated velocity of the trunk's origin, world axes (a view of x); base_lin_vel is the same in trunk axes."""
        return self.x[:, 3:6]

    @property
    def foot_positions(self) -> torch.Tensor:
        """f32 [N, 4, 3]: the estimated foot origins, world axes, in feet_indices order (a view of x)."""
        return self.x[:, 6:].view(-1, 4, 3)

    def _launch(self, contact, reset_mask=None, reset=False, **inputs):
        p_init = self.env.root_states[:, 0:3].contiguous() if (reset or reset_mask is not None) else None
        self.last_inputs = dict(inputs, contact=contact, reset_mask=reset_mask, p_init=p_init, reset=reset)
        self.env.sim.leg_odometry(self.cfg, self.x, self.P, contact, reset_mask=reset_mask, p_init=p_init, reset=reset,
                                  vel_body=self.base_lin_vel, nis=self.nis, status=self.status, **inputs)

    def reset(self, env_ids=None) -> None:
        """Reset every env (env_ids None) or the listed ones to their true root position, zero velocity, the feet where the leg
        kinematics put them and the initial covariance. One launch; the other envs are left as they are."""
        env = self.env
        contact = env.get_foot_contacts().to(torch.float32)
        if env_ids is None:
            self._last_root_vel.copy_(env.root_states[:, 7:10])
            self._launch(contact, reset=True)
            return
        ids = torch.as_tensor(env_ids, dtype=torch.long, device=env.device)
        self._last_root_vel[ids] = env.root_states[ids, 7:10]
        keep = (self.x.clone(), self.P.clone(), self.base_lin_vel.clone(), self.nis.clone(), self.status.clone())
        mask = torch.zeros((env.num_envs,), dtype=torch.int32, device=env.device)
        mask[ids] = 1
        self._launch(contact, reset_mask=mask)
        rest = mask == 0                                                            # the launch also advanced the others: put them back
        for t, k in zip((self.x, self.P, self.base_lin_vel, self.nis, self.status), keep):
            t[rest] = k[rest]

    def update(self, contact=None, accel=None, quat=None, gyro=None, dof=None, foot_height=None) -> torch.Tensor:
        """One update over env.dt at the sim's current state, to be called once after every env.step(); returns base_lin_vel [N, 3].
        Defaults: contact = env.get_foot_contacts(), the four flags the policy observes; accel = the specific force in trunk axes from
        the finite difference of the root's world velocity since the previous update; quat, gyro, dof = the sim's state; foot_height =
        0 on the plane and none (no height rows) on other terrain (the rows hold the foot ORIGINS to that height: pass the ground height plus
        the foot sphere's radius to account for it). Pass tensors to put sensor noise in. Envs flagged in env.reset_buf
        are reset at their true root position instead. The tensors handed to the kernel are kept in last_inputs."""
        env = self.env
        if contact is None:
            contact = env.get_foot_contacts()
        contact = contact.to(torch.float32).contiguous()
        vel = env.root_states[:, 7:10]
        if accel is None:
            a_world = (vel - self._last_root_vel) / self.cfg.dt - self._gravity
            accel = _quat_rotate_inverse(env.base_quat if quat is None else quat, a_world).contiguous()
        self._last_root_vel.copy_(vel)
        if foot_height is None:
            foot_height = self._plane_height
        self._launch(contact, reset_mask=env.reset_buf.to(torch.int32), accel=accel, quat=quat, gyro=gyro, dof=dof, foot_height=foot_height)
        return self.base_lin_vel


def trot_schedule(phase: torch.Tensor, period: float, duty: float, horizon: int, dt: float) -> torch.Tensor:
    """u8 [N, horizon, 4]: the contact schedule of a diagonal-pair trot for wbc_sim_centroidal_mpc. phase f32 [N] in [0, 1) is where
    each env's gait cycle of `period` seconds stands now; feet 0 and 3 (one diagonal, in feet_indices order) are in stance while the
    cycle's fraction is below `duty`, feet 1 and 2 half a cycle later. Stage k is judged at its middle, (k + 1/2) dt. Torch ops only."""
    k = torch.arange(horizon, dtype=torch.float32, device=phase.device)
    frac = phase.to(torch.float32).unsqueeze(1) + (k + 0.5).unsqueeze(0) * (float(dt) / float(period))           # [N, H]
    first = torch.remainder(frac, 1.0) < float(duty)
    second = torch.remainder(frac + 0.5, 1.0) < float(duty)
    return torch.stack([first, second, second, first], dim=-1).to(torch.uint8).contiguous()


class CentroidalMPC:
    """The convex MPC of wbc_sim_centroidal_mpc for every env: it owns the cfg and the warm-start buffer (z and y of the ADMM
    iteration) and runs one launch per solve(). Keyword arguments are the fields of wbc_mpc_cfg (include/wbc_sim.h); q takes 12 and r
    takes 3 numbers. Not covered: terrain normals other than world z, a friction coefficient per env, the gyroscopic term, foothold
    optimisation, a force-reference term in the whole-body QP (whole_body_controller takes base_acc, not the forces)."""

    DEFAULTS = dict(iters=40, rho=2.5e-6, mu=0.5, fz_min=0.0, fz_max=250.0,
                    q=(25.0, 25.0, 10.0, 2.0, 2.0, 50.0, 0.0, 0.0, 0.3, 0.2, 0.2, 0.1), r=(1e-6, 1e-6, 1e-6), tol=1e-2)

    def __init__(self, env, horizon: int = 10, dt: float = None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown MPC parameters: {sorted(unknown)}"
        v = dict(self.DEFAULTS, **cfg)
        self.env = env
        self.cfg = abi.WbcMpcCfg(int(horizon), int(v["iters"]), float(env.dt if dt is None else dt), float(v["rho"]), float(v["mu"]),
                                 float(v["fz_min"]), float(v["fz_max"]), (abi.f32 * 12)(*[float(t) for t in v["q"]]),
                                 (abi.f32 * 3)(*[float(t) for t in v["r"]]), float(v["tol"]))
        n, dev, H = env.num_envs, env.device, int(horizon)
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)
        self.warm = z(n, 2, H, abi.MPC_NZ)
        self.forces, self.u, self.predicted, self.base_acc, self.residuals = z(n, 4, 3), z(n, H, 12), z(n, H, 12), z(n, 6), z(n, 2)
        self.status = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.x_ref = z(n, H, 12)
        self._com = z(n, 9)
        self._workspace = z(int(env.sim.L.wbc_sim_centroidal_mpc_workspace_floats(n)))
        self._started = False
        self.last_inputs = None

    def reset(self, env_ids=None) -> None:
        """Forget the warm start of every env (env_ids None) or of the listed ones: their next solve starts from zeros."""
        if env_ids is None:
            self.warm.zero_()
            self._started = False
        else:
            self.warm[torch.as_tensor(env_ids, dtype=torch.long, device=self.env.device)] = 0.0

    def reference(self, p0: torch.Tensor, yaw: torch.Tensor, vel_cmd=None, yaw_rate=None, height=None) -> torch.Tensor:
        """x_ref f32 [N, H, 12] for stages 1..H from the centre of mass p0 [N, 3] and the heading yaw [N] now: the planar velocity
        vel_cmd [N, 2] (heading frame; None: 0) turned to world axes, the yaw rate [N] (None: 0) about z and the height [N] or a float
        (None: the current one) of the centre of mass; theta is relative to the heading at the call, so its reference is
        (0, 0, yaw_rate k dt)."""
        n, dev, H, dt = self.env.num_envs, self.env.device, int(self.cfg.horizon), float(self.cfg.dt)
        t = torch.arange(1, H + 1, dtype=torch.float32, device=dev) * dt                                      # [H]
        vc = torch.zeros((n, 2), dtype=torch.float32, device=dev) if vel_cmd is None else vel_cmd.to(torch.float32)
        wz = torch.zeros((n,), dtype=torch.float32, device=dev) if yaw_rate is None else yaw_rate.to(torch.float32)
        c, s = torch.cos(yaw), torch.sin(yaw)
        vw = torch.stack([c * vc[:, 0] - s * vc[:, 1], s * vc[:, 0] + c * vc[:, 1]], dim=-1)                  # [N, 2]
        x = self.x_ref
        x.zero_()
        x[:, :, 2] = wz[:, None] * t[None]
        x[:, :, 3:5] = p0[:, None, 0:2] + vw[:, None] * t[None, :, None]
        x[:, :, 5] = p0[:, None, 2] if height is None else torch.as_tensor(height, dtype=torch.float32, device=dev).expand(n)[:, None]
        x[:, :, 8] = wz[:, None]
        x[:, :, 9:11] = vw[:, None]
        return x

    def solve(self, contact_schedule: torch.Tensor, vel_cmd=None, yaw_rate=None, height=None, x_ref=None, foot_positions=None,
              state=None, shift: bool = False) -> torch.Tensor:
        """One MPC launch at the sim's current state; returns forces [N, 4, 3]. contact_schedule u8 (or bool) [N, H, 4], e.g.
        trot_schedule(...). The reference is x_ref [N, H, 12] if given, else reference(...) from vel_cmd, yaw_rate and height (torch
        ops and one wbc_sim_centroidal launch for the centre of mass). state: None for the sim's own state; a BaseStateEstimator, whose
        position and velocity of the trunk's origin replace the sim's (the centre of mass's offset and relative velocity, the
        orientation and the angular velocity stay the sim's) and whose foot_positions are used unless foot_positions is given; or an
        x0 tensor [N, 12]. foot_positions [N, 4, 3] or [N, H, 4, 3] (world), None: the feet's current origins. The first solve
        after a reset() is cold; later ones start from the last z and y, shifted by one stage with shift=True (one solve per
        stage length). Results: .forces, .base_acc (for whole_body_controller(base_acc=...)), .u, .predicted, .residuals, .status."""
        env = self.env
        n, H = env.num_envs, int(self.cfg.horizon)
        contact = contact_schedule.to(torch.uint8).contiguous()
        x0 = None
        if isinstance(state, BaseStateEstimator):
            env.sim.centroidal(com=self._com)
            root = env.root_states
            yaw = self._yaw(env.base_quat)
            x0 = torch.cat([self._heading_rotvec(env.base_quat, yaw), state.position + self._com[:, 0:3], root[:, 10:13],
                            state.velocity + (self._com[:, 3:6] - root[:, 7:10])], dim=-1).contiguous()
            if foot_positions is None:
                foot_positions = state.foot_positions
        elif state is not None:
            x0 = state.to(torch.float32).contiguous()
        if x_ref is None:
            if x0 is None:
                env.sim.centroidal(com=self._com)
                p0, yaw = env.root_states[:, 0:3] + self._com[:, 0:3], self._yaw(env.base_quat)
            else:
                p0, yaw = x0[:, 3:6], self._yaw(env.base_quat)
            x_ref = self.reference(p0, yaw, vel_cmd, yaw_rate, height)
        x_ref = x_ref.to(torch.float32).contiguous()
        fp = None
        if foot_positions is not None:
            fp = foot_positions.to(torch.float32).reshape(n, -1, 4, 3).contiguous()
        self.last_inputs = dict(contact=contact, x_ref=x_ref, x0=x0, foot_pos=fp, cold=not self._started, shift=bool(shift and self._started))
        env.sim.centroidal_mpc(self.cfg, contact, x_ref, x0=x0, foot_pos=fp, warm=self.warm, cold=not self._started,
                               shift=bool(shift and self._started), forces=self.forces, u=self.u, x_pred=self.predicted,
                               base_acc=self.base_acc, res=self.residuals, status=self.status, workspace=self._workspace)
        self._started = True
        return self.forces

    @staticmethod
    def _yaw(q: torch.Tensor) -> torch.Tensor:
        """The yaw of R(q)'s x axis, q xyzw [N, 4]."""
        x, y, z, w = q.unbind(-1)
        return torch.atan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))

    @staticmethod
    def _heading_rotvec(q: torch.Tensor, yaw: torch.Tensor) -> torch.Tensor:
        """log(R(q) Rz(yaw)^T) as a rotation vector: q times the conjugate of the yaw quaternion, then the quaternion's logarithm."""
        h = 0.5 * yaw
        qz = torch.stack([torch.zeros_like(h), torch.zeros_like(h), -torch.sin(h), torch.cos(h)], dim=-1)
        qr = _quat_mul(q, qz)
        qr = qr * torch.where(qr[:, 3:] < 0, -1.0, 1.0)
        sn = qr[:, :3].norm(dim=-1, keepdim=True)
        ang = 2 * torch.atan2(sn, qr[:, 3:])
        return qr[:, :3] * torch.where(sn > 1e-6, ang / sn.clamp_min(1e-12), torch.full_like(sn, 2.0))


class FootstepPlanner:
    """The gait layer of wbc_sim_footstep_plan for every env: it owns the cfg, the state [N, 32] (phase, and per foot the lift-off
    position, the target foothold and a swing flag) and every output, and advances them by one launch per update(). gait is a name in
    GAITS or four phase offsets in feet_indices order (FL, FR, RL, RR); keyword arguments are the other fields of wbc_footstep_cfg
    (include/wbc_sim.h); dt defaults to env.dt, mpc_dt to env.dt, stance_offset [4, 2] to the feet's xy under the trunk at the default
    joint angles. The planner starts reset at phase 0. Use it as
        planner.update(vel_cmd, yaw_rate, state=estimator)
        mpc.solve(planner.contact_schedule, vel_cmd, yaw_rate, foot_positions=planner.foot_positions, state=estimator)
        env.whole_body_controller(base_acc=mpc.base_acc, swing_acc=planner.swing_acc, stance=planner.stance)
    Not covered: early / late contact adaptation, a duty per foot, footholds searched for standing feet, collision of the swing path with
    the terrain."""

    GAITS = {"stand": (0.0, 0.0, 0.0, 0.0), "trot": (0.0, 0.5, 0.5, 0.0), "pace": (0.0, 0.5, 0.0, 0.5), "bound": (0.0, 0.0, 0.5, 0.5),
             "walk": (0.0, 0.5, 0.75, 0.25)}
    DEFAULTS = dict(k_v=0.03, com_height=0.3, max_reach=0.25, swing_height=0.08, latch=0.8, kp=400.0, kd=40.0, search_radius=2,
                    search_step=0.04, probe_radius=0.03, w_dist=1.0, w_rough=10.0, w_slope=0.1, rough_max=0.03, nz_min=0.85)

    def __init__(self, env, gait="trot", period: float = 0.5, duty: float = 0.5, horizon: int = 10, mpc_dt: float = None, dt: float = None,
                 stance_offset=None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown planner parameters: {sorted(unknown)}"
        v = dict(self.DEFAULTS, **cfg)
        self.env = env
        if isinstance(gait, str):
            assert gait in self.GAITS, f"gait must be one of {sorted(self.GAITS)} or four offsets"
            offsets = self.GAITS[gait]
            if gait == "stand":
                duty = 1.0
        else:
            offsets = tuple(float(o) for o in gait)
            assert len(offsets) == 4
        if stance_offset is None:
            stance_offset = self.default_stance_offset(env)
        so = [[float(stance_offset[i][j]) for j in range(2)] for i in range(4)]
        self.cfg = abi.WbcFootstepCfg(float(env.dt if dt is None else dt), float(period), float(duty), (abi.f32 * 4)(*offsets), int(horizon),
                                      float(env.dt if mpc_dt is None else mpc_dt), ((abi.f32 * 2) * 4)(*[(abi.f32 * 2)(*r) for r in so]),
                                      float(v["k_v"]), float(v["com_height"]), float(v["max_reach"]), float(v["swing_height"]),
                                      float(v["latch"]), float(v["kp"]), float(v["kd"]), int(v["search_radius"]), float(v["search_step"]),
                                      float(v["probe_radius"]), float(v["w_dist"]), float(v["w_rough"]), float(v["w_slope"]),
                                      float(v["rough_max"]), float(v["nz_min"]))
        n, dev, H = env.num_envs, env.device, int(horizon)
        z = lambda *sh, dtype=torch.float32: torch.zeros(sh, dtype=dtype, device=dev)
        self.state = z(n, abi.FOOTSTEP_NS)
        self.stance, self.contact = z(n, 4, dtype=torch.uint8), z(n, 4)
        self.contact_schedule, self.foot_positions = z(n, H, 4, dtype=torch.uint8), z(n, H, 4, 3)
        self.footholds, self.swing_ref, self.swing_acc = z(n, 4, 3), z(n, 4, 9), z(n, 4, 3)
        self.info = z(n, dtype=torch.int32)
        self.reset()

    @staticmethod
    def default_stance_offset(env):
        """[4][2]: the xy of the four foot origins relative to the trunk's origin, trunk axes, at the default joint angles (a walk down
        each leg of the robot model)."""
        m = env.robot_model
        q = env.default_dof_pos.detach().cpu().numpy().reshape(-1).astype(np.float64)
        out = []
        for rb in [int(i) for i in env.feet_indices.tolist()]:
            chain, b = [], int(m.rb_body[rb])
            while b > 0:
                chain.append(b)
                b = int(m.parent[b])
            E, p = np.eye(3), np.zeros(3)
            for b in chain[::-1]:
                p = p + E @ np.asarray(m.joint_xyz[b], dtype=np.float64)
                ax, ang = int(m.axis[b]), q[int(m.body_dof[b])]
                c, s_ = np.cos(ang), np.sin(ang)
                Q = np.eye(3)
                j, k = (ax + 1) % 3, (ax + 2) % 3
                Q[j, j], Q[j, k], Q[k, j], Q[k, k] = c, -s_, s_, c
                E = E @ Q
            p = p + E @ np.asarray(m.rb_offset[rb], dtype=np.float64)
            out.append([float(p[0]), float(p[1])])
        return out

    # the outputs under the names their consumers use
    @property
    def phase(self) -> torch.Tensor:
        """f32 [N]: where each env's gait cycle stands (a view of state)."""
        return self.state[:, 0]

    @property
    def swing_pos(self) -> torch.Tensor:
        return self.swing_ref[:, :, 0:3]

    @property
    def swing_vel(self) -> torch.Tensor:
        return self.swing_ref[:, :, 3:6]

    @property
    def swing_acc_ref(self) -> torch.Tensor:
        """f32 [N, 4, 3]: the reference's own acceleration (swing_acc adds the PD on the tracking error to it)."""
        return self.swing_ref[:, :, 6:9]

    def _launch(self, **kw):
        self.env.sim.footstep_plan(self.cfg, self.state, stance=self.stance, contact=self.contact, schedule=self.contact_schedule,
                                   foot_pos=self.foot_positions, foothold=self.footholds, swing_ref=self.swing_ref, swing_acc=self.swing_acc,
                                   info=self.info, **kw)

    def reset(self, env_ids=None, phase=None) -> None:
        """Reset every env (env_ids None) or the listed ones: phase = `phase` (a float or [N]; None: 0), no foot in swing, lift-off and
        target at the feet's current origins. One launch with the clock held; the other envs' state is left as it is."""
        env = self.env
        n, dev = env.num_envs, env.device
        p0 = None if phase is None else torch.as_tensor(phase, dtype=torch.float32, device=dev).expand(n).contiguous()
        if env_ids is None:
            self._launch(reset=True, hold=True, phase_init=p0)
            return
        mask = torch.zeros((n,), dtype=torch.int32, device=dev)
        mask[torch.as_tensor(env_ids, dtype=torch.long, device=dev)] = 1
        self._launch(reset_mask=mask, hold=True, phase_init=p0)

    def update(self, vel_cmd=None, yaw_rate=None, state=None, hold: bool = False) -> torch.Tensor:
        """One control step at the sim's current state; returns stance u8 [N, 4]. vel_cmd [N, 2] (heading frame) and yaw_rate [N], None:
        0. state: None for the sim's own base position and velocity, or a BaseStateEstimator, whose position and velocity replace them
        (orientation, angular velocity and joints stay the sim's). hold=True leaves the clock where it is. Envs flagged in env.reset_buf
        are reset at phase 0. Results: .stance, .contact, .contact_schedule, .foot_positions, .footholds, .swing_pos / .swing_vel /
        .swing_acc_ref, .swing_acc, .info."""
        env = self.env
        kw = {}
        if isinstance(state, BaseStateEstimator):
            kw = dict(base_pos=state.position.contiguous(), base_vel=state.velocity.contiguous())
        else:
            assert state is None, "state is a BaseStateEstimator or None"
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        self._launch(vel_cmd=f(vel_cmd), yaw_rate=f(yaw_rate), reset_mask=env.reset_buf.to(torch.int32), hold=hold, **kw)
        return self.stance


class ContactDetector:
    """The probabilistic contact detector of wbc_sim_contact_detect for every env (Bledt et al., ICRA 2018): it owns the cfg, the detector
    state [N, 16] = (p, c, t, 0) per foot, a momentum-observer state [N, 2, 26] of its own (not the sim's shared one) and every output, and
    advances them by one observer update and one detector launch per update(). planner: a FootstepPlanner whose duty, offsets and phase
    give the gait prior and the EARLY / LATE events (None: neither); gain: the observer's bandwidth in 1/s, capped at 0.9 / dt (the observer's
    explicit update needs gain dt < 1; .gain holds the value in use); keyword arguments
    are the other fields of wbc_contact_cfg (include/wbc_sim.h); dt defaults to env.dt. The detector starts reset with every foot in
    contact. Use it as
        det.update(torques=tau)                          # after the simulate calls that applied tau
        est.update(contact=det.prob)
        env.whole_body_controller(..., stance=det.stance)
    Not covered: feeding the events back into the planner's clock, contacts on links other than the feet. ground and
    normal can come from a GroundEstimator (det.update(ground=gnd.ground, normal=gnd.normal))."""

    DEFAULTS = dict(sigma_phase=0.05, mu_z=0.01, sigma_z=0.01, mu_f=15.0, sigma_f=8.0, var_phase=0.25, var_z=0.05, var_f=0.05, alpha=0.5,
                    p_on=0.6, p_off=0.4, t_dwell=0.04, early_min=0.5, late_min=0.2, damping=0.02)

    def __init__(self, env, planner: "FootstepPlanner" = None, gain: float = 50.0, dt: float = None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown detector parameters: {sorted(unknown)}"
        v = dict(self.DEFAULTS, **cfg)
        self.env, self.planner = env, planner
        duty = float(planner.cfg.duty) if planner is not None else 1.0
        offsets = [float(o) for o in planner.cfg.offset] if planner is not None else [0.0] * 4
        self.gain = min(float(gain), 0.9 / float(env.dt if dt is None else dt))       # wbc_sim_momentum_observer asks for gain dt < 1
        self.cfg = abi.WbcContactCfg(float(env.dt if dt is None else dt), duty, (abi.f32 * 4)(*offsets), *[float(v[k]) for k in self.DEFAULTS])
        n, dev = env.num_envs, env.device
        z = lambda *sh, dtype=torch.float32: torch.zeros(sh, dtype=dtype, device=dev)
        self.state = z(n, abi.CONTACT_NS)
        self.observer_state, self._observer_fresh = z(n, 2, 6 + abi.NDOF), z(n, 2, 6 + abi.NDOF)
        self._tau = z(n, 6 + abi.NDOF)
        self.prob, self.contact, self.stance = z(n, 4), z(n, 4, dtype=torch.uint8), z(n, 4, dtype=torch.uint8)
        self.foot_forces, self.terms, self.info = z(n, 4, 3), z(n, 4, 4), z(n, dtype=torch.int32)
        self._plane_ground = (torch.full((n, 4), float(abi.FOOT_RADIUS), dtype=torch.float32, device=dev)
                              if env.cfg.terrain.mesh_type in ("plane", None) else None)
        self.last_inputs = None
        self.reset()

    @property
    def tau_ext(self) -> torch.Tensor:
        """f32 [N, 26]: the observer's residual, the estimate of the external generalised forces (a strided view of observer_state)."""
        return self.observer_state[:, 1]

    def _observe(self, torques, reset_mask=None, reset=False) -> None:
        """One observer update with the joint torques `torques` [N, 20] (None: env.torques); the envs in reset_mask (all with reset) restart
        at the current momentum with residual 0."""
        env = self.env
        self._tau[:, 6:] = env.torques if torques is None else torques.to(torch.float32)
        dt = float(self.cfg.dt)
        env.sim.momentum_observer(self._tau, self.gain, dt, state=self.observer_state, reset=reset)
        if reset_mask is not None and not reset:
            env.sim.momentum_observer(self._tau, self.gain, dt, state=self._observer_fresh, reset=True)
            self.observer_state.copy_(torch.where((reset_mask != 0)[:, None, None], self._observer_fresh, self.observer_state))

    def _launch(self, foot_force=None, ground=None, base_pos=None, reset_mask=None, reset=False, normal=None) -> None:
        phase = self.planner.state[:, 0] if self.planner is not None else None
        tau_ext = None if foot_force is not None else self.tau_ext
        self.last_inputs = dict(tau_ext=tau_ext, foot_force=foot_force, ground=ground, base_pos=base_pos, phase=phase, reset_mask=reset_mask, reset=reset)
        if normal is not None:
            self.last_inputs["normal"] = normal
        self.env.sim.contact_detect(self.cfg, self.state, base_pos=base_pos, tau_ext=tau_ext, foot_force=foot_force, normal=normal, ground=ground,
                                    phase=phase, reset_mask=reset_mask, reset=reset, prob=self.prob, contact=self.contact, stance=self.stance,
                                    force=self.foot_forces, terms=self.terms, info=self.info)

    def reset(self, env_ids=None) -> None:
        """Reset every env (env_ids None) or the listed ones: p = 1, every foot in contact, the dwell time served, the observer at the
        current momentum with residual 0. The other envs' states are left as they are."""
        env = self.env
        if env_ids is None:
            self._observe(None, reset=True)
            self._launch(ground=self._plane_ground, reset=True)
            return
        mask = torch.zeros((env.num_envs,), dtype=torch.int32, device=env.device)
        mask[torch.as_tensor(env_ids, dtype=torch.long, device=env.device)] = 1
        tensors = (self.state, self.observer_state, self.prob, self.contact, self.stance, self.foot_forces, self.terms, self.info)
        keep = [t.clone() for t in tensors]
        self._observe(None, reset_mask=mask)
        self._launch(ground=self._plane_ground, reset_mask=mask)
        rest = mask == 0                                                            # the launches also advanced the others: put them back
        for t, k in zip(tensors, keep):
            t[rest] = k[rest]

    def update(self, torques=None, foot_force=None, ground=None, base_pos=None, normal=None) -> torch.Tensor:
        """One observer update and one detector launch at the sim's current state, to be called once per control step after the simulate
        calls; returns prob [N, 4]. torques [N, 20]: the joint torques that were applied, what set_dof_forces takes (None: env.torques).
        foot_force [N, 4, 3] (world): a measured foot force, used instead of the observer's estimate. ground [N, 4]: the height of a
        resting foot's origin; None: the foot sphere's radius above z = 0 on the plane, no height term on other terrain. base_pos
        [N, 3]: the trunk's position (a BaseStateEstimator's), None: the sim's. normal [N, 4, 3]: the ground's normal under each foot (a
        GroundEstimator's), None: world z. duty, offsets and phase are the planner's. Envs flagged
        in env.reset_buf are reset. Results: .prob, .contact, .stance, .foot_forces, .terms, .info; the tensors handed to the kernel are
        kept in last_inputs."""
        env = self.env
        mask = env.reset_buf.to(torch.int32)
        self._observe(torques, reset_mask=mask)
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        self._launch(foot_force=f(foot_force), ground=self._plane_ground if ground is None else f(ground), base_pos=f(base_pos), reset_mask=mask,
                     normal=f(normal))
        return self.prob


class LegController:
    """The leg controller of wbc_sim_leg_control for every env (Di Carlo et al. and Bledt et al., IROS 2018): it owns the cfg and every
    output and turns foot forces and swing references into joint torques by one launch per update(), after one inverse-dynamics launch
    for the bias torques and, with the feed-forward, the mass-matrix refresh and one body-accelerations launch. Keyword arguments are the
    fields of wbc_leg_control_cfg (include/wbc_sim.h): kp, kd (three numbers each, or one for all axes), kd_stance, damping, fz_min,
    fz_max, mu, kp_arm, kd_arm, arm_q_default (six numbers each); and bias ("h": Coriolis and gravity torques, "g": gravity alone, None:
    none), tau_limit ([N, 18], [18] or None for the config's torque limits; False: no clamp) and clip (clip the forces to the pyramid
    of fz_min, fz_max and mu). The swing gains are UNTUNED placeholders; the arm's gains default to the task config's PD stiffness and
    damping of its joints, its targets to the default posture. Use it as
        mpc.solve(planner.contact_schedule, ..., state=est)
        tau = ctl.update(forces=mpc.forces, swing_ref=planner.swing_ref, stance=planner.contact, state=est)
        env.sim.set_dof_forces(tau)
    Not covered: normals other than world z in the clip, the base's acceleration in the feed-forward, joint-space position targets for
    the legs, a task-space arm."""

    DEFAULTS = dict(kp=(400.0, 400.0, 400.0), kd=(8.0, 8.0, 8.0), kd_stance=0.2, damping=0.02, fz_min=0.0, fz_max=250.0, mu=0.5,
                    kp_arm=None, kd_arm=None, arm_q_default=None)

    def __init__(self, env, bias="h", tau_limit=None, clip: bool = False, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown leg-controller parameters: {sorted(unknown)}"
        assert bias in ("h", "g", None), "bias is 'h', 'g' or None"
        v = dict(self.DEFAULTS, **cfg)
        self.env, self.bias, self.clip = env, bias, bool(clip)
        n, dev = env.num_envs, env.device
        self.leg_dofs, self.arm_dofs = self.dof_groups(env)
        arm = self.arm_dofs
        three = lambda t: tuple(float(x) for x in (t if hasattr(t, "__len__") else (t,) * 3))
        six = lambda t, default: tuple(float(x) for x in (default if t is None else t))
        kp_arm = six(v["kp_arm"], [float(env.p_gains[d]) for d in arm])
        kd_arm = six(v["kd_arm"], [float(env.d_gains[d]) for d in arm])
        q_arm = six(v["arm_q_default"], [float(env.default_dof_pos[d]) for d in arm])
        assert len(kp_arm) == len(kd_arm) == len(q_arm) == 6
        self.cfg = abi.WbcLegControlCfg((abi.f32 * 3)(*three(v["kp"])), (abi.f32 * 3)(*three(v["kd"])), float(v["kd_stance"]), float(v["damping"]),
                                        float(v["fz_min"]), float(v["fz_max"]), float(v["mu"]), (abi.f32 * 6)(*kp_arm), (abi.f32 * 6)(*kd_arm),
                                        (abi.f32 * 6)(*q_arm))
        if tau_limit is False:
            self.tau_limit = None
        elif tau_limit is None:
            live = sorted([d for leg in self.leg_dofs for d in leg] + list(arm))        # the 18 revolute joints in DoF order
            self.tau_limit = env.torque_limits[live].to(torch.float32).expand(n, -1).contiguous()
        else:
            self.tau_limit = torch.as_tensor(tau_limit, dtype=torch.float32, device=dev).expand(n, 18).contiguous()
        z = lambda *sh, dtype=torch.float32: torch.zeros(sh, dtype=dtype, device=dev)
        self.tau, self.leg_force, self.foot, self.info = z(n, abi.NDOF), z(n, 4, 3), z(n, 4, 6), z(n, dtype=torch.int32)
        self._bias, self._acc = z(n, 6 + abi.NDOF), z(n, abi.NRB, 6)
        self.last_inputs = None

    @staticmethod
    def dof_groups(env):
        """(legs, arm): the DoFs of each leg's three joints from the trunk down, in feet_indices order, and the six DoFs that drive a
        body but are in no leg, in DoF order (a walk up the robot model from each foot)."""
        m = env.robot_model
        legs = []
        for rb in [int(i) for i in env.feet_indices.tolist()]:
            chain, b = [], int(m.rb_body[rb])
            while b > 0:
                chain.append(int(m.body_dof[b]))
                b = int(m.parent[b])
            legs.append(tuple(chain[::-1]))
        in_leg = {d for leg in legs for d in leg}
        driven = sorted({int(m.body_dof[b]) for b in range(1, len(m.parent))})
        return legs, [d for d in driven if d not in in_leg]

    def update(self, forces=None, swing_ref=None, stance=None, state=None, arm_q_des=None, feedforward: bool = True) -> torch.Tensor:
        """One control step at the sim's current state; returns tau [N, 20] for sim.set_dof_forces. forces [N, 4, 3] (world; a
        CentroidalMPC's .forces; None: 0), swing_ref [N, 4, 9] (a FootstepPlanner's; None: no swing term), stance [N, 4] (the planner's
        .contact or a ContactDetector's .prob, any dtype; None: every foot stands). state: None for the sim's own base position and
        velocity, or a BaseStateEstimator, whose position and velocity replace them. arm_q_des [N, 6]: the arm's targets (None: the
        cfg's). feedforward (with swing_ref only): the swing legs' J^T Lambda (a_ref - Jdot nu), from the refreshed env.mm_whole and one
        body-accelerations launch. Results: .tau, .leg_force (what each leg pushes with), .foot (p, pd) and .info; the tensors handed
        to the kernel are kept in last_inputs."""
        env = self.env
        kw = {}
        if isinstance(state, BaseStateEstimator):
            kw = dict(base_pos=state.position.contiguous(), base_vel=state.velocity.contiguous())
        else:
            assert state is None, "state is a BaseStateEstimator or None"
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        tau_bias = None
        if self.bias == "h":
            env.sim.inverse_dynamics(tau=self._bias)
            tau_bias = self._bias
        elif self.bias == "g":
            env.sim.inverse_dynamics(grav=self._bias)
            tau_bias = self._bias
        mm = acc = None
        if feedforward and swing_ref is not None:
            env.refresh_mass_matrix_tensors()
            mm = env.mm_whole
            acc = env.sim.body_accelerations(None, out=self._acc)
        kw.update(forces=f(forces), swing_ref=f(swing_ref), stance=f(stance), tau_bias=tau_bias, mass_matrix=mm, acc_bias=acc,
                  arm_q_des=f(arm_q_des), tau_limit=self.tau_limit, clip=self.clip)
        self.last_inputs = dict(kw)
        env.sim.leg_control(self.cfg, tau=self.tau, leg_force=self.leg_force, foot=self.foot, info=self.info, **kw)
        return self.tau


class AttitudeEstimator:
    """The attitude filter of wbc_sim_attitude_filter for every env (a multiplicative extended Kalman filter; Markley, JGCD 2003): it owns
    the orientation quat [N, 4] (xyzw), the gyro bias [N, 3], the covariance P [N, 6, 6] of (dtheta, db) and every output, and advances
    them by one launch per update(). Keyword arguments are the fields of wbc_attitude_cfg (include/wbc_sim.h); dt defaults to env.dt. The
    defaults are UNTUNED. The estimator starts reset at the sim's quaternion. Use it as
        gyro, accel, heading = imu.read()                # after env.step() or the simulate calls
        att.update(gyro=gyro, accel=accel, aux=(heading, imu.heading_world, 0.05))
        est.update(quat=att.quat, gyro=att.gyro, accel=accel)
    Not covered: yaw from the leg kinematics (without an aux vector the heading drifts with the gyro's bias about gravity), the covariance
    reset after the multiplicative update, an accelerometer bias, the lever arm of an IMU away from the trunk's origin, and a quat argument
    for the planner, the detector and the leg controller classes, which keep reading the sim's quaternion."""

    DEFAULTS = dict(sigma_g=0.005, sigma_b=1e-4, sigma_a=0.02, kappa_a=100.0, p0_theta=0.25, p0_b=1e-3)

    def __init__(self, env, dt: float = None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown attitude parameters: {sorted(unknown)}"
        v = dict(self.DEFAULTS, **cfg)
        self.env = env
        self.cfg = abi.WbcAttitudeCfg(float(env.dt if dt is None else dt), *[float(v[k]) for k in self.DEFAULTS])
        n, dev = env.num_envs, env.device
        z = lambda *sh, dtype=torch.float32: torch.zeros(sh, dtype=dtype, device=dev)
        self.quat, self.bias, self.P = z(n, 4), z(n, 3), z(n, 6, 6)
        self.quat[:, 3] = 1.0
        self.gyro, self.gravity_body, self.status = z(n, 3), z(n, 3), z(n, dtype=torch.int32)
        self.nis = z(n, 1)
        self.last_inputs = None
        self.reset()

    def _launch(self, gyro=None, accel=None, aux=None, reset_mask=None, q_init=None, reset=False) -> None:
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        n, dev = self.env.num_envs, self.env.device
        body = world = sigma = None
        if aux is not None:
            body, world, sigma = aux
            body = f(body).reshape(n, -1, 3)
            k = body.shape[1]
            world = f(torch.as_tensor(world, dtype=torch.float32, device=dev)).expand(n, k, 3).contiguous()
            sigma = f(torch.as_tensor(sigma, dtype=torch.float32, device=dev)).expand(n, k).contiguous()
        k = 0 if body is None else int(body.shape[1])
        if tuple(self.nis.shape) != (n, 1 + k):
            self.nis = torch.zeros((n, 1 + k), dtype=torch.float32, device=dev)
        kw = dict(gyro=f(gyro), accel=f(accel), aux_body=body, aux_world=world, aux_sigma=sigma, reset_mask=reset_mask, q_init=f(q_init), reset=reset)
        self.last_inputs = dict(kw)
        self.env.sim.attitude_filter(self.cfg, self.quat, self.bias, self.P, gyro_out=self.gyro, gravity_body=self.gravity_body, nis=self.nis,
                                     status=self.status, **kw)

    def reset(self, env_ids=None, quat=None, from_accel: bool = False, accel=None) -> None:
        """Reset every env (env_ids None) or the listed ones: zero bias, the initial covariance, and the orientation quat [N, 4] (None: the
        sim's quaternion; with from_accel the tilt of accel [N, 3] -- None: the identity -- and zero yaw). One launch; the other envs are
        left as they are."""
        env = self.env
        q_init = None if from_accel else (env.base_quat if quat is None else quat)
        if env_ids is None:
            self._launch(accel=accel if from_accel else None, q_init=q_init, reset=True)
            return
        mask = torch.zeros((env.num_envs,), dtype=torch.int32, device=env.device)
        mask[torch.as_tensor(env_ids, dtype=torch.long, device=env.device)] = 1
        tensors = (self.quat, self.bias, self.P, self.gyro, self.gravity_body, self.status)
        keep = [t.clone() for t in tensors]
        self._launch(accel=accel if from_accel else None, q_init=q_init, reset_mask=mask)
        rest = mask == 0                                                            # the launch also advanced the others: put them back
        for t, k in zip(tensors, keep):
            t[rest] = k[rest]

    def update(self, gyro=None, accel=None, aux=None) -> torch.Tensor:
        """One update over env.dt at the sim's current state, to be called once per control step; returns quat [N, 4]. gyro [N, 3] and
        accel [N, 3] in trunk axes, what ImuModel.read() returns (gyro None: the sim's angular velocity, no bias; accel None: no
        gravity row); aux: (body [N, K, 3] or [N, 3], world [K, 3] or [3], sigma [K] or a number) direction measurements, K <= 4. Envs
        flagged in env.reset_buf are reset at the sim's quaternion. Results: .quat, .bias, .P, .gyro (= gyro - bias), .gravity_body,
        .nis, .status; the tensors handed to the kernel are kept in last_inputs."""
        env = self.env
        self._launch(gyro=gyro, accel=accel, aux=aux, reset_mask=env.reset_buf.to(torch.int32), q_init=env.base_quat)
        return self.quat


class GroundEstimator:
    """The blind terrain estimate of wbc_sim_ground_estimate for every env (the terrain-slope estimate of Bledt et al., IROS 2018): a plane
    through the most recent footholds, weighted by their age and regularised towards the previous slope. It owns the cfg, the state
    [N, 32] (per foot the last contact point, its age and a 0; the anchor at 20, the plane (a0, a1, a2) at 22) and every output, and
    advances them by one launch per update(). Keyword arguments are the fields of wbc_ground_cfg (include/wbc_sim.h), `lambda_` for
    lambda; dt defaults to env.dt. The defaults are UNTUNED. The estimator starts reset with every contact point at its foot. Use it as
        gnd.update(det.prob, base_pos=est.position)      # or a flag, or planner.contact
        est.update(foot_height=gnd.ground)
        det.update(ground=gnd.ground, normal=gnd.normal)
        env.whole_body_controller(..., normal=gnd.normal[:, stance_idx])
        mpc.solve(..., height=gnd.trunk[:, 0] + h_nominal)
    Nothing takes it by default. Not covered: per-foot local patches, normals inside the MPC's cone or the leg controller's clip,
    the planner's foothold search (which keeps reading the heightfield)."""

    DEFAULTS = dict(c_on=0.5, tau_age=0.5, lambda_=0.01, slope_max=0.7, tilt_gain=1.0)

    def __init__(self, env, dt: float = None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown ground-estimator parameters: {sorted(unknown)}"
        v = dict(self.DEFAULTS, **cfg)
        self.env = env
        self.cfg = abi.WbcGroundCfg(float(env.dt if dt is None else dt), *[float(v[k]) for k in self.DEFAULTS])
        n, dev = env.num_envs, env.device
        z = lambda *sh, dtype=torch.float32: torch.zeros(sh, dtype=dtype, device=dev)
        self.state = z(n, abi.GROUND_NS)
        self.normal, self.ground, self.residual, self.trunk, self.theta_ref = z(n, 4, 3), z(n, 4), z(n, 4), z(n, 6), z(n, 3)
        self.query_z, self.info = z(n, 0), z(n, dtype=torch.int32)
        self._all = torch.ones((n, 4), dtype=torch.float32, device=dev)
        self.last_inputs = None
        self.reset()

    @property
    def plane(self) -> torch.Tensor:
        """f32 [N, 5]: (c_x, c_y, a0, a1, a2) with z(x, y) = a0 + a1 (x - c_x) + a2 (y - c_y) (a view of the state)."""
        return self.state[:, 20:25]

    def _launch(self, contact, base_pos=None, quat=None, query_xy=None, reset_mask=None, reset=False) -> None:
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        n, dev = self.env.num_envs, self.env.device
        q = f(query_xy)
        if q is not None:
            q = q.reshape(n, -1, 2)
        nq = 0 if q is None else int(q.shape[1])
        if tuple(self.query_z.shape) != (n, nq):
            self.query_z = torch.zeros((n, nq), dtype=torch.float32, device=dev)
        kw = dict(contact=f(contact), base_pos=f(base_pos), quat=f(quat), query_xy=q if nq > 0 else None, reset_mask=reset_mask, reset=reset)
        self.last_inputs = dict(kw)
        self.env.sim.ground_estimate(self.cfg, self.state, normal=self.normal, ground=self.ground, residual=self.residual, trunk=self.trunk,
                                     theta_ref=self.theta_ref, query_z=self.query_z, info=self.info, **kw)

    def reset(self, env_ids=None) -> None:
        """Reset every env (env_ids None) or the listed ones: every contact point at its foot's current position, zero slope. One launch;
        the other envs are left as they are."""
        env = self.env
        if env_ids is None:
            self._launch(self._all, reset=True)
            return
        mask = torch.zeros((env.num_envs,), dtype=torch.int32, device=env.device)
        mask[torch.as_tensor(env_ids, dtype=torch.long, device=env.device)] = 1
        if tuple(self.query_z.shape) != (env.num_envs, 0):
            self.query_z = torch.zeros((env.num_envs, 0), dtype=torch.float32, device=env.device)
        tensors = (self.state, self.normal, self.ground, self.residual, self.trunk, self.theta_ref, self.info)
        keep = [t.clone() for t in tensors]
        self._launch(self._all, reset_mask=mask)
        rest = mask == 0                                                            # the launch also advanced the others: put them back
        for t, k in zip(tensors, keep):
            t[rest] = k[rest]

    def update(self, contact, base_pos=None, quat=None, query_xy=None) -> torch.Tensor:
        """One launch at the sim's current joint state, to be called once per control step; returns ground [N, 4]. contact [N, 4]: a
        ContactDetector's prob, a flag such as get_foot_contacts() or a FootstepPlanner's contact; a foot stands iff its entry is >=
        c_on. base_pos [N, 3] and quat [N, 4] (xyzw): the trunk's estimated position and orientation (a BaseStateEstimator's, an
        AttitudeEstimator's), None: the sim's. query_xy [N, Q, 2]: world points at which the plane is evaluated into .query_z [N, Q].
        Envs flagged in env.reset_buf are reset. Results: .normal, .ground, .residual, .trunk, .theta_ref, .query_z, .info, .plane;
        the tensors handed to the kernel are kept in last_inputs."""
        env = self.env
        self._launch(contact, base_pos=base_pos, quat=quat, query_xy=query_xy, reset_mask=env.reset_buf.to(torch.int32))
        return self.ground


class SlipDetector:
    """The foot slip detector and friction estimate of wbc_sim_slip_detect for every env (after Focchi et al., "Slip Detection and
    Recovery for Quadruped Robots"): per foot a test of the foot origin's tangential world velocity with hysteresis and a dwell time,
    and a friction coefficient from the ratio of tangential to normal force while the foot slides, fused per env, next to a lower bound
    from the feet that stick. It owns the cfg, the state [N, 4, 8] (per foot p, s, t, c_prev, d, mu_i, w_i, m_i) and every output, and
    advances them by one launch per update(). Keyword arguments are the fields of wbc_slip_cfg (include/wbc_sim.h); dt defaults to
    env.dt. The defaults are UNTUNED. The detector starts reset. Use it as
        slip.update(det.prob, foot_force=det.foot_forces, state=est, gyro=att.gyro)     # or a flag, or planner.contact
        est.update(contact=slip.weight)
        gnd.update(contact=slip.weight)
        env.whole_body_controller(..., mu=slip.mu)
    Nothing takes it by default. Not covered: slip recovery (re-planning the force or the foothold), a friction coefficient per env
    inside the MPC, estimating the normal from the slip direction, tuning of any default."""

    DEFAULTS = dict(c_on=0.5, v_slip=0.15, sigma_v=0.05, alpha=0.5, p_on=0.6, p_off=0.3, t_dwell=0.02, common_mode=0.0, fn_min=10.0,
                    gamma=0.995, w_min=1.0, mu_prior=0.5, mu_min=0.1, mu_max=1.5, mu_scale=0.9)

    def __init__(self, env, dt: float = None, **cfg):
        unknown = set(cfg) - set(self.DEFAULTS)
        assert not unknown, f"unknown slip-detector parameters: {sorted(unknown)}"
        v = dict(self.DEFAULTS, **cfg)
        self.env = env
        self.cfg = abi.WbcSlipCfg(float(env.dt if dt is None else dt), *[float(v[k]) for k in self.DEFAULTS])
        n, dev = env.num_envs, env.device
        z = lambda *sh, dtype=torch.float32: torch.zeros(sh, dtype=dtype, device=dev)
        self.state = z(n, 4, abi.SLIP_NS)
        self.prob, self.slip, self.weight, self.foot_vel = z(n, 4), z(n, 4, dtype=torch.uint8), z(n, 4), z(n, 4, 3)
        self.speed, self.distance, self.mu, self.mu_lower, self.mu_env = z(n, 4), z(n, 4), z(n, 4), z(n, 4), z(n, 2)
        self.info = z(n, dtype=torch.int32)
        self._none = z(n, 4)
        self.last_inputs = None
        self.reset()

    def _outputs(self):
        return (self.state, self.prob, self.slip, self.weight, self.foot_vel, self.speed, self.distance, self.mu, self.mu_lower, self.mu_env,
                self.info)

    def _launch(self, contact, foot_force=None, normal=None, base_vel=None, ang_vel=None, reset_mask=None, reset=False) -> None:
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        kw = dict(contact=f(contact), foot_force=f(foot_force), normal=f(normal), base_vel=f(base_vel), ang_vel=f(ang_vel), reset_mask=reset_mask,
                  reset=reset)
        self.last_inputs = dict(kw)
        self.env.sim.slip_detect(self.cfg, self.state, prob=self.prob, slip=self.slip, weight=self.weight, foot_vel=self.foot_vel,
                                 speed=self.speed, distance=self.distance, mu=self.mu, mu_lower=self.mu_lower, mu_env=self.mu_env,
                                 info=self.info, **kw)

    def reset(self, env_ids=None) -> None:
        """Reset every env (env_ids None) or the listed ones: no slip, zero distance, mu_i = mu_prior with no weight. One launch with no
        foot standing; the other envs are left as they are."""
        env = self.env
        if env_ids is None:
            self._launch(self._none, reset=True)
            return
        mask = torch.zeros((env.num_envs,), dtype=torch.int32, device=env.device)
        mask[torch.as_tensor(env_ids, dtype=torch.long, device=env.device)] = 1
        tensors = self._outputs()
        keep = [t.clone() for t in tensors]
        self._launch(self._none, reset_mask=mask)
        rest = mask == 0                                                            # the launch also advanced the others: put them back
        for t, k in zip(tensors, keep):
            t[rest] = k[rest]

    def update(self, contact, foot_force=None, normal=None, state=None, gyro=None) -> torch.Tensor:
        """One launch at the sim's current joint state, to be called once per control step; returns slip u8 [N, 4]. contact [N, 4]: a
        ContactDetector's prob, a flag such as get_foot_contacts() or a FootstepPlanner's contact. foot_force [N, 4, 3] (world): the
        force of the ground on each foot (a ContactDetector's foot_forces), None: no friction update. normal [N, 4, 3]: the ground's
        normal under each foot (a GroundEstimator's), None: world z. state: a BaseStateEstimator, whose velocity is taken as the
        trunk's, None: the sim's. gyro [N, 3]: the angular velocity in trunk axes (an AttitudeEstimator's gyro), None: the sim's. Envs
        flagged in env.reset_buf are reset. Results: .slip, .prob, .weight, .foot_vel, .speed, .distance, .mu, .mu_lower, .mu_env,
        .info; the tensors handed to the kernel are kept in last_inputs."""
        env = self.env
        base_vel = None if state is None else state.velocity
        self._launch(contact, foot_force=foot_force, normal=normal, base_vel=base_vel, ang_vel=gyro, reset_mask=env.reset_buf.to(torch.int32))
        return self.slip


class ImuModel:
    """An IMU on the trunk's origin read from the sim's state, torch ops only: read() returns (gyro, accel, heading) in trunk axes.
    gyro = R^T omega + bias + noise, with a constant per-env bias (gyro_bias: a number, three numbers or [N, 3]); accel = the specific
    force R^T ((v - v_prev) / dt - g) + noise from the finite difference of the root's world velocity between two reads (what
    BaseStateEstimator.update computes inline); heading = R^T heading_world + noise, the world x axis (None without heading_noise). The
    noises are standard deviations per component and sample, drawn from a torch.Generator on the device seeded with `seed`."""

    def __init__(self, env, gyro_bias=0.0, gyro_noise: float = 0.0, accel_noise: float = 0.0, heading_noise: float = None, seed: int = 0):
        self.env = env
        n, dev = env.num_envs, env.device
        self.gyro_bias = torch.as_tensor(gyro_bias, dtype=torch.float32, device=dev).expand(n, 3).clone() if hasattr(gyro_bias, "__len__") \
            else torch.full((n, 3), float(gyro_bias), dtype=torch.float32, device=dev)
        self.gyro_noise, self.accel_noise, self.heading_noise = float(gyro_noise), float(accel_noise), heading_noise
        self.heading_world = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(int(seed))
        self._gravity = torch.tensor(list(env.tcfg.gravity), dtype=torch.float32, device=dev)
        self._last_root_vel = env.root_states[:, 7:10].clone()

    def _noise(self, std: float) -> torch.Tensor:
        n, dev = self.env.num_envs, self.env.device
        return std * torch.randn((n, 3), dtype=torch.float32, device=dev, generator=self.generator)

    def reset(self) -> None:
        """Forget the previous velocity: the next read's acceleration is that of a trunk at rest."""
        self._last_root_vel.copy_(self.env.root_states[:, 7:10])

    def read(self, dt: float = None):
        """(gyro [N, 3], accel [N, 3], heading [N, 3] or None) at the sim's current state; dt: the time since the previous read (None:
        env.dt). Envs flagged in env.reset_buf read the acceleration of a trunk at rest."""
        env = self.env
        dt = float(env.dt if dt is None else dt)
        quat, vel = env.base_quat, env.root_states[:, 7:10]
        last = torch.where(env.reset_buf.bool()[:, None], vel, self._last_root_vel)
        a_world = (vel - last) / dt - self._gravity
        self._last_root_vel.copy_(vel)
        gyro = _quat_rotate_inverse(quat, env.root_states[:, 10:13]) + self.gyro_bias + self._noise(self.gyro_noise)
        accel = _quat_rotate_inverse(quat, a_world) + self._noise(self.accel_noise)
        heading = None
        if self.heading_noise is not None:
            heading = _quat_rotate_inverse(quat, self.heading_world.expand(env.num_envs, 3)) + self._noise(float(self.heading_noise))
        return gyro.contiguous(), accel.contiguous(), heading
