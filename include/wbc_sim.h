/*
 * wbc_sim.h -- C-ABI of libwbc_amd.so: the MI355X-native replacement for the part of
 * the widowGo1 hot path that the reference delegates to Isaac Gym (closed source) and
 * to ~150 eager PyTorch ops per policy step.
 *
 * Every entry point names the reference interface it stands in for (paths relative to
 * the reference root; WG = legged_gym/legged_gym/envs/widowGo1/widowGo1.py,
 * BT = legged_gym/legged_gym/envs/base/base_task.py,
 * LR = legged_gym/legged_gym/envs/base/legged_robot.py,
 * RS = rsl_rl/rsl_rl/storage/rollout_storage.py).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative error code (text via wbc_last_error()); no exceptions cross the boundary; device
 * pointers are HIP device pointers on the device given at creation; `stream` is a
 * hipStream_t passed as void* (NULL = the legacy default stream) and all work is
 * asynchronous on that stream; the library creates no hidden streams or threads.
 * Quaternions are xyzw, float tensors are fp32, reset/episode-length buffers are int64,
 * as in the reference (BT:71-80).
 */
#ifndef WBC_SIM_H
#define WBC_SIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fixed sizes of the widowGo1 articulation ---- */
#define WBC_NB 19        /* moving bodies: floating root + 18 revolute joints */
#define WBC_NJ 18        /* revolute joints */
#define WBC_NDOF 20      /* simulator DoFs: 18 revolute + 2 locked prismatic fingers */
#define WBC_NACT 18      /* num_actions = num_torques (widowGo1_config.py:118-119) */
#define WBC_NRB 27       /* robot rigid bodies as the importer lists them */
#define WBC_NRB_ENV 28   /* + the free box actor (WG:384,542,546) */
#define WBC_NFEET 4
#define WBC_NCP 64       /* contact slots per env (one wavefront lane each): robot spheres vs terrain, box corners vs terrain,
                            the static pairs (arm spheres vs the trunk box, robot spheres vs the free box) and the DYNAMIC slots
                            that the self-collision broad phase promotes its hits into */
#define WBC_NSPH 28      /* the robot's contact spheres (their centres in frame F are cached once per substep) */
#define WBC_NLIMB 11     /* capsules of the self-collision broad phase: 4 thighs, 4 calves, upper arm, forearm, hand */
#define WBC_LIMB_RSUM_MAX 0.060f   /* an upper bound of (largest radius of limb a) + (largest radius of limb b) over all candidate pairs (second
                                      stage of the broad phase: the distance between the two shafts' segments against this + rest + margin) */
#define WBC_BOX_BODY WBC_NB   /* pseudo body index of the free box actor (WG:321-325,384) in cp_body / cp_body2 */
#define WBC_BOX_RB WBC_NRB    /* its row in the [N,28,...] rigid-body tensors (WG:544-548: the last one) */
#define WBC_NPROP 76     /* num_proprio (widowGo1_config.py:122) */
#define WBC_NPRIV 24     /* num_priv */
#define WBC_HIST 10      /* history_len */
#define WBC_NOBS 860     /* num_observations */
#define WBC_ADELAY_LEN 4 /* action_delay + 2 (WG:540) */
#define WBC_NREW 37      /* reward terms implemented (enum wbc_reward_term) */
#define WBC_NMETRIC 10   /* episode_metric_sums (WG:165) */
#define WBC_MAX_DEPTH 6

/* Articulated-body model, produced on the host from the URDF (replaces gym.load_asset +
 * get_asset_* getters, WG:285-294). All joint frames are unrotated (URDF rpy = 0). */
typedef struct {
  int32_t parent[WBC_NB];       /* parent moving body, -1 for the root */
  int32_t axis[WBC_NB];         /* 0/1/2 = x/y/z, -1 root */
  int32_t dof[WBC_NB];          /* simulator DoF index of joint i, -1 root */
  float joint_xyz[WBC_NB][3];   /* joint origin in the parent body frame */
  float mass[WBC_NB];
  float com[WBC_NB][3];
  float inertia[WBC_NB][6];     /* xx,yy,zz,xy,xz,yz about the com, body axes */
  float q_lower[WBC_NDOF], q_upper[WBC_NDOF];   /* URDF limits; lower==upper==0: unlimited */
  float qd_limit[WBC_NDOF];     /* URDF velocity limit */
  float effort[WBC_NDOF];       /* URDF effort limit -> torque_limits (LR:294-299) */
  int32_t rb_body[WBC_NRB];     /* moving body each importer rigid body rides on */
  float rb_offset[WBC_NRB][3];
  int32_t feet_rb[WBC_NFEET];   /* rigid-body indices of the feet, importer order FL,FR,RL,RR */
  int32_t gripper_rb;           /* wx250s/ee_gripper_link (WG:318) */
  /* Collision set (the URDF's <collision> blocks as sphere-swept primitives): ncp contacts in use.
   * Every contact has a sphere (centre cp_pos in the frame of moving body cp_body, radius cp_radius, riding on importer
   * rigid body cp_rb) and a partner selected by cp_kind:
   *   WBC_CP_TERRAIN  the terrain (plane or height grid);
   *   WBC_CP_BOX      a box fixed to moving body cp_body2 (rigid body cp_rb2): centre cp_a, half extents cp_b, its frame;
   * Pairs are two-body contacts (the robot's self-collision, asset.self_collisions = 0 = enabled, widowGo1_config.py:180; the robot
   * against the free box): the impulse acts on both bodies with opposite signs. Terrain contacts come first (the force sensors read contacts 0..3).
   * The free box actor (WG:321-325: a cube, density 1000) takes part under the pseudo body index WBC_BOX_BODY / rigid-body row
   * WBC_BOX_RB: its eight corner spheres against the terrain (cp_body = WBC_BOX_BODY, cp_pos in the box frame) and robot spheres
   * against it (kind WBC_CP_BOX with cp_body2 = WBC_BOX_BODY, cp_a = 0, cp_b = box_half).
   * Slots 0 .. ncp-1 are in use except those marked WBC_CP_NONE. The step kernel's layout rules (checked at wbc_sim_create): every
   * contact that involves the free box sits in slots 32..47 (one 16-lane row: their wrenches on the box are summed by a row
   * reduction) and nothing else does; keep what a walking robot normally touches with (feet, knees, trunk, arm) below 32 -- the
   * per-body loops walk the slots below 32 and those from 48 separately.
   *
   * Self-collision as configured (asset.self_collisions = 0: every pair of non-adjacent links collides): the pairs that can touch
   * inside the URDF's joint limits (tools/self_collision_reach.py: 44 limb pairs and 12 robot spheres against the free box; the legs
   * never reach the trunk box, the front and rear thighs never meet) are too many for one lane each, and almost never active. They are CANDIDATES: every lane carries one
   * pair descriptor (pr_*) -- its own pair for a static pair slot, otherwise a candidate -- and tests it against bounding spheres
   * in the same instructions (the broad phase; a limb pair that passes -- two legs standing side by side always do -- is then tested
   * segment against segment with the generous radius WBC_LIMB_RSUM_MAX before it counts as a hit). A candidate that passes is promoted into a free DYNAMIC slot (kind
   * WBC_CP_DYNAMIC: robot-vs-robot hits into the dynamic slots outside 32..47, in ascending order of candidate and slot;
   * robot-vs-free-box hits into the dynamic slots of the box row), where the exact test runs and, if the gap is inside the contact
   * margin, the contact is solved like any other pair. Hits beyond the free slots (17 outside the box row + 3 inside it) are dropped
   * and COUNTED (tensor WBC_T_DROPPED_HITS: per env, accumulated over the substeps; the tests assert it stays 0).
   * Primitives of the candidates, all in frame F from the cached sphere centres (cp_sph: the compact index of a robot sphere):
   *   limbs -- capsules between two sphere centres (thigh: hip-side end to knee, r 0.017; calf: knee to foot, r 0.008, with its end
   *   spheres knee r 0.02 / foot r 0.02; upper arm: shoulder joint to elbow, forearm: elbow to wrist, hand: wrist to gripper tip, with
   *   the radii fitted to the arm's meshes that wbc_amd/assets/arm_primitives.json records (r 0.040 / 0.025 / 0.0275; that file is the
   *   single source); equal end indices would make a single sphere); kind WBC_PR_LIMBS tests limb pr_a against
   *   limb pr_b as the union of shaft and end spheres (deepest feature pair wins: one contact per limb pair);
   *   kind WBC_PR_SPHERE_BOX tests robot sphere pr_a against the free box (knees, shins, trunk corners, wrist, elbow). */
  int32_t ncp;
  int32_t cp_body[WBC_NCP];
  float cp_pos[WBC_NCP][3];
  float cp_radius[WBC_NCP];
  int32_t cp_rb[WBC_NCP];       /* rigid body whose net_contact_force row receives the force */
  int32_t cp_kind[WBC_NCP];
  int32_t cp_body2[WBC_NCP];    /* -1 for terrain contacts */
  int32_t cp_rb2[WBC_NCP];      /* rigid body that receives the opposite force, -1 for terrain contacts */
  float cp_a[WBC_NCP][3], cp_b[WBC_NCP][3];
  float cp_radius2[WBC_NCP];
  int32_t cp_sph[WBC_NCP];      /* compact index (0 .. WBC_NSPH-1) of the robot sphere of a terrain slot / of a static pair's sphere; -1 otherwise */
  /* pair descriptor of every lane (broad phase): kind, operands, bounding reach (sum of the two bounding radii + contact margin) */
  int32_t pr_kind[WBC_NCP];     /* enum wbc_pair_kind */
  int32_t pr_a[WBC_NCP], pr_b[WBC_NCP];   /* WBC_PR_LIMBS: limb ids; WBC_PR_SPHERE_BOX / WBC_PR_STATIC: pr_a = robot sphere (compact index) */
  float pr_reach[WBC_NCP];
  int32_t nlimb;
  int32_t limb_s0[WBC_NLIMB], limb_s1[WBC_NLIMB];   /* compact sphere indices of the segment's ends (equal: a sphere) */
  float limb_radius[WBC_NLIMB], limb_cap0[WBC_NLIMB], limb_cap1[WBC_NLIMB];   /* shaft radius; end-sphere radii (0: none) */
  int32_t limb_body[WBC_NLIMB];                     /* moving body */
  int32_t limb_rb[WBC_NLIMB], limb_rb0[WBC_NLIMB], limb_rb1[WBC_NLIMB];   /* rigid body reported for a touch on the shaft / end sphere 0 / 1 */
  float pair_rest_offset;                           /* sim.physx.rest_offset for limb pairs (sphere radii already carry it) */
  /* pieces for per-env mass randomisation (WG:431-456) */
  float base_piece_mass, base_piece_com[3], base_piece_inertia[6];
  float base_rest_mass, base_rest_com[3], base_rest_inertia[6];
  int32_t gripper_body;
  float grip_piece_mass, grip_piece_com[3], grip_piece_inertia[6];
  float grip_rest_mass, grip_rest_com[3], grip_rest_inertia[6];
  /* the free box actor: half edge of the cube (box.box_size / 2, widowGo1_config.py:186), nominal mass (density 1000 x size^3,
   * WG:322; the per-env total is WBC_T_BOX_MASS), friction of its material (Isaac Gym's shape default 1.0) */
  float box_half, box_mass, box_friction;
  /* Sleeping (as PhysX puts resting actors to sleep: sleep threshold + wake counter): while the box's speed and (spin x half edge)
   * are below box_sleep_speed, at least three of its corners are within the contact offset of the terrain and no robot sphere is
   * within the contact offset of it, a per-env timer (WBC_T_BOX_SLEEP_TIMER) runs, otherwise it is zero; once it has reached
   * box_sleep_time the box is frozen -- no contacts, no gravity, zero velocity -- until a robot sphere touches it or it loses
   * its support (reset_idx re-places it in the air). box_sleep_speed <= 0: never sleeps. */
  float box_sleep_speed, box_sleep_time;
} wbc_model;

enum wbc_contact_kind { WBC_CP_NONE = -1 /* unused slot */, WBC_CP_TERRAIN = 0, WBC_CP_BOX = 1,
                        WBC_CP_LIMBS = 2 /* run time only: a dynamic slot holding a promoted limb pair */,
                        WBC_CP_DYNAMIC = 3 /* a free slot of the dynamic pool */ };
enum wbc_pair_kind { WBC_PR_NONE = 0, WBC_PR_STATIC = 1 /* the lane's own static pair (kind WBC_CP_BOX) */, WBC_PR_LIMBS = 2, WBC_PR_SPHERE_BOX = 3 };

enum wbc_reward_term {   /* the _reward_* methods WG defines (WG:1352-1469), then the base class's (LR = envs/base/legged_robot.py:832-922)
                            that work in the widowGo1 task. Not offered: orientation (LR:841-843 reads self.projected_gravity, which
                            WidowGo1 never creates: AttributeError in the reference, profiles/r04_reference_switches.txt), arm_orientation
                            (no such method), feet_stumble (the config key names no method; the method is _reward_stumble) */
  WBC_REW_ENERGY_SQUARE = 0, WBC_REW_SURVIVE, WBC_REW_TRACKING_LIN_VEL_X_L1,
  WBC_REW_TRACKING_ANG_VEL_YAW_EXP, WBC_REW_HIP_ACTION_L2, WBC_REW_FOOT_CONTACTS_Z,
  WBC_REW_TRACKING_EE_SPHERE, WBC_REW_ARM_ENERGY_ABS_SUM,
  WBC_REW_TRACKING_EE_CART, WBC_REW_TRACKING_EE_ORN, WBC_REW_TRACKING_EE_ORN_RY,
  WBC_REW_LEG_ENERGY_ABS_SUM, WBC_REW_LEG_ENERGY_SUM_ABS, WBC_REW_LEG_ACTION_L2,
  WBC_REW_LEG_ENERGY, WBC_REW_TRACKING_LIN_VEL, WBC_REW_TRACKING_LIN_VEL_X_EXP,
  WBC_REW_TRACKING_ANG_VEL_YAW_L1, WBC_REW_TRACKING_LIN_VEL_Y_L2,
  WBC_REW_TRACKING_LIN_VEL_Z_L2, WBC_REW_TORQUES, WBC_REW_COLLISION,
  /* base class */
  WBC_REW_LIN_VEL_Z, WBC_REW_ANG_VEL_XY, WBC_REW_DOF_VEL, WBC_REW_DOF_ACC, WBC_REW_ACTION_RATE,
  WBC_REW_TERMINATION,   /* added AFTER the only_positive_rewards clip (WG:184-188, 200-203) */
  WBC_REW_DOF_POS_LIMITS, WBC_REW_DOF_VEL_LIMITS, WBC_REW_TORQUE_LIMITS, WBC_REW_TRACKING_ANG_VEL,
  WBC_REW_FEET_AIR_TIME, /* stateful: WBC_T_FEET_AIR_TIME / WBC_T_LAST_CONTACTS, advanced only while the term is active */
  WBC_REW_STUMBLE, WBC_REW_STAND_STILL, WBC_REW_FEET_CONTACT_FORCES,
  WBC_REW_BASE_HEIGHT    /* with terrain.measure_heights = False (measured_heights = 0, WG:639): (z - base_height_target)^2 */
};

enum wbc_metric {        /* WG:165 order */
  WBC_MET_LEG_ENERGY_ABS_SUM = 0, WBC_MET_TRACKING_LIN_VEL_X_L1, WBC_MET_TRACKING_ANG_VEL_YAW_EXP,
  WBC_MET_TRACKING_EE_CART, WBC_MET_TRACKING_EE_SPHERE, WBC_MET_TRACKING_EE_ORN,
  WBC_MET_LEG_ACTION_L2, WBC_MET_TORQUE, WBC_MET_ENERGY_SQUARE, WBC_MET_FOOT_CONTACTS_Z
};

/* Task constants: WidowGo1RoughCfg + LeggedRobotCfg.sim resolved to numbers. */
typedef struct {
  /* sim (legged_robot_config.py:182-199) */
  float sim_dt;                 /* 0.005 */
  int32_t decimation;           /* 4 */
  float gravity[3];
  /* contact / limit model of THIS framework's physics spec */
  float contact_margin;         /* physx.contact_offset 0.01 */
  float contact_erp;            /* fraction of penetration removed per step */
  float max_depenetration_vel;  /* physx.max_depenetration_velocity 1.0 */
  float terrain_friction;       /* terrain.static_friction 1.0 */
  float limit_kappa, limit_delta; /* joint-limit stop gains, in units of D/dt^2 and D/dt */
  int32_t contact_iters;
  float joint_armature[WBC_NACT]; /* added to each joint's articulated inertia D: dt*Kd + dt^2*Kp makes
                                     the task's PD law (WG:1281) linearly implicit */
  /* control (WG:1262-1295, widowGo1_config.py:163-173) */
  float clip_actions;
  float action_scale[WBC_NACT];
  float p_gains[WBC_NACT], d_gains[WBC_NACT];
  float default_dof_pos[WBC_NDOF];
  float torque_limits[WBC_NDOF];
  int32_t action_delay;         /* 2; -1 disables the FIFO */
  /* observations (WG:966-1001) */
  float obs_scale_ang_vel, obs_scale_dof_pos, obs_scale_dof_vel, clip_obs;
  float commands_scale[3];
  /* episode, termination (WG:937-963) */
  int32_t max_episode_length;   /* 500 */
  float term_rp_threshold;      /* 0.2, hard-coded at WG:945-946 */
  float term_z_threshold;       /* 0.325 */
  uint32_t term_contact_rb_mask;     /* bit rb: rigid body rb is in asset.terminate_after_contacts_on (WG:305-306,940: |net force| > 1 N
                                        ends the episode); shipped config: empty */
  uint32_t penalize_contact_rb_mask; /* asset.penalize_contacts_on (WG:299-300; _reward_collision counts |net force| > 0.1 N, LR:865-867) */
  int32_t resample_interval;    /* int(3.0/0.02)=150 (WG:922) */
  int32_t push_interval;        /* 150 (WG:119); <=0 disables */
  float max_push_vel;
  float lin_vel_x_clip, ang_vel_yaw_clip;
  /* EE goal sampler (WG:1297-1350, widowGo1_config.py:46-85) */
  float goal_collision_lower[3], goal_collision_upper[3];
  float goal_underground_limit;
  int32_t goal_collision_samples;     /* 10 */
  float goal_delta_orn_range[3][2];
  float sphere_error_scale[3], orn_error_scale[3];
  float z_invariant_offset;           /* 0.53 (WG:597) */
  int32_t goal_command_cart;          /* goal_ee.command_mode == 'cart' (WG:589-593): curr_ee_goal is the Cartesian goal -- observation
                                         entries 70..72 (WG:980) and the sign tests of the roll / pitch termination (WG:945-946) read it
                                         instead of the spherical one; 0 = 'sphere' (the shipped config) */
  /* rewards */
  float tracking_sigma, tracking_ee_sigma;
  int32_t only_positive_rewards;
  /* the base class's terms: soft joint limits (LR:301-304: centre +- half range * rewards.soft_dof_pos_limit), velocity limits
   * * soft_dof_vel_limit (LR:882), torque limits * soft_torque_limit (LR:886), rewards.max_contact_force, base_height_target */
  float soft_dof_lower[WBC_NDOF], soft_dof_upper[WBC_NDOF], soft_dof_vel_limit[WBC_NDOF], soft_torque_limit[WBC_NDOF];
  float max_contact_force, base_height_target;
  /* resets (WG:757-828) */
  float base_init_state[13];
  float origin_perturb_range, init_vel_perturb_range;
  float dof_reset_lo, dof_reset_hi;   /* 0.8, 1.2 */
  float box_origin_x, box_origin_z;
  /* flat ground height unless a heightfield is attached */
  float ground_z;
} wbc_task_cfg;

/* Host scalars the reference recomputes in update_command_curriculum (WG:678-692). */
typedef struct {
  float lin_vel_x_range[2], ang_vel_yaw_range[2];
  float goal_l_range[2], goal_p_range[2], goal_y_range[2];
  float leg_reward_scale[WBC_NREW];   /* rewards.scales: CURRENT value of each term's scale (WG:176-178) */
  float arm_reward_scale[WBC_NREW];   /* rewards.arm_scales */
  /* bit t set = term t's _reward_ function is in the list built at construction from the config's non-zero scales
   * (_prepare_reward_function, WG:128-157): it is evaluated every step -- episode sum += term * current scale, metric side
   * effect applied -- even while a scheduled scale is 0 */
  uint64_t leg_active_mask, arm_active_mask;
} wbc_curriculum;

/* Device tensors owned by the sim; ids for wbc_sim_get_tensor. Shapes at N envs. */
enum wbc_tensor_id {
  WBC_T_ROOT_STATES = 0,   /* f32 [N,2,13]  acquire_actor_root_state_tensor  (WG:505,523) */
  WBC_T_DOF_STATE,         /* f32 [N,20,2]  acquire_dof_state_tensor         (WG:506,526) */
  WBC_T_NET_CONTACT_FORCE, /* f32 [N,28,3]  acquire_net_contact_force_tensor (WG:507,542) */
  WBC_T_RIGID_BODY_STATE,  /* f32 [N,28,13] acquire_rigid_body_state_tensor  (WG:508,546) */
  WBC_T_FORCE_SENSOR,      /* f32 [N,4,6]   acquire_force_sensor_tensor      (WG:511,522) */
  WBC_T_TORQUES,           /* f32 [N,20]    self.torques                     (WG:619,1176) */
  WBC_T_OBS_BUF,           /* f32 [N,860]   obs_buf                          (WG:992,1196) */
  WBC_T_OBS_HISTORY,       /* f32 [N,10,76] obs_history_buf                  (WG:539,994) */
  WBC_T_ACTION_HISTORY,    /* f32 [N,4,18]  action_history_buf               (WG:540,1167) */
  WBC_T_ACTIONS,           /* f32 [N,18]    self.actions (delayed, sim order)(WG:1173) */
  WBC_T_LAST_ACTIONS,      /* f32 [N,18]                                     (WG:623,908) */
  WBC_T_LAST_DOF_VEL,      /* f32 [N,20]                                     (WG:624,909) */
  WBC_T_LAST_ROOT_VEL,     /* f32 [N,6]                                      (WG:625,910) */
  WBC_T_COMMANDS,          /* f32 [N,3]                                      (WG:627) */
  WBC_T_GOAL_STATE,        /* f32 [N,24]  ee_start_sphere,ee_goal_sphere,ee_goal_cart,
                              curr_ee_goal_sphere,curr_ee_goal_cart,ee_goal_delta_orn_euler,
                              ee_goal_orn_euler (3 each), goal_timer, traj_timesteps,
                              traj_total_timesteps                           (WG:574-583) */
  WBC_T_REW_BUF,           /* f32 [N]                                        (BT:72) */
  WBC_T_ARM_REW_BUF,       /* f32 [N] */
  WBC_T_RESET_BUF,         /* i64 [N]                                        (BT:74) */
  WBC_T_TIME_OUT_BUF,      /* u8  [N]  (bool)                                (BT:76) */
  WBC_T_EPISODE_LENGTH,    /* i64 [N]                                        (BT:75) */
  WBC_T_EPISODE_SUMS,      /* f32 [N,37] per-term sums (WBC_NREW), zeroed on reset (WG:162) */
  WBC_T_METRIC_SUMS,       /* f32 [N,10]                                     (WG:166) */
  WBC_T_EPISODE_SUMS_DONE, /* f32 [N,37] sums at the moment of reset (for extras) (WG:743-746) */
  WBC_T_METRIC_SUMS_DONE,  /* f32 [N,10]                                     (WG:748-750) */
  WBC_T_BASE_LIN_VEL,      /* f32 [N,3]                                      (WG:880) */
  WBC_T_BASE_ANG_VEL,      /* f32 [N,3]                                      (WG:881) */
  WBC_T_MASS_PARAMS,       /* f32 [N,5]  mass_params_tensor                  (WG:354,455) */
  WBC_T_FRICTION,          /* f32 [N]    friction_coeffs_tensor              (WG:400) */
  WBC_T_MOTOR_STRENGTH,    /* f32 [N,18]                                     (WG:403) */
  WBC_T_ENV_ORIGINS,       /* f32 [N,3]                                      (WG:212) */
  WBC_T_BOX_DELTA_Y,       /* f32 [N]                                        (WG:226) */
  WBC_T_BODY_PARAMS,       /* f32 [N,20] per-env composite root + gripper (mass, com, inertia6) */
  WBC_T_RESET_TRAVEL,      /* f32 [N,2]  at the moment of an env's reset: ||root_xy - env_origin_xy|| and ||commands[:2]||,
                              the two quantities _update_terrain_curriculum reads before reset_idx overwrites them (LR:431-435) */
  WBC_T_BOX_MASS,          /* f32 [N]    total mass of the env's box actor: nominal + box.added_mass_range draw (WG:458-466) */
  WBC_T_BOX_SLEEP_TIMER,   /* f32 [N]    substeps the box actor has been at rest (asleep from box_sleep_time / sim_dt on) */
  WBC_T_FEET_AIR_TIME,     /* f32 [N,4]  feet_air_time (WG:633, LR:898-909), zeroed on reset (WG:734) */
  WBC_T_LAST_CONTACTS,     /* f32 [N,4]  last_contacts as 0 / 1 (WG:626, LR:902-903) */
  WBC_T_DROPPED_HITS,      /* f32 [N]    broad-phase hits that found no free dynamic contact slot, accumulated over all substeps since the sim was
                              created (diagnostic: a non-zero value means a self-collision / box contact was not simulated) */
  WBC_T_COUNT
};
enum wbc_dtype { WBC_F32 = 0, WBC_I64 = 1, WBC_U8 = 2 };

typedef struct wbc_sim wbc_sim;

const char* wbc_last_error(void);

/* ---- asset: what gym.load_asset + the get_asset_* getters (WG:268-294) and the config resolution of WidowGo1._parse_cfg /
 * _init_buffers (WG:78-121, 498-672) hand to the reference, as ONE binary file -- so that a binding in any language can create a
 * sim without this repository's Python: wbc_asset_load -> wbc_asset_model / _task_cfg / _curriculum -> (edit the documented fields
 * of its own copies: gains, thresholds, reward scales ...) -> wbc_sim_create. The packaged widowGo1 asset with the shipped config is
 * deep-whole-body-control_amd/wbc_amd/assets/widowgo1_default.wbcasset (written by tools/make_asset.py from the URDF tables and
 * WidowGo1RoughCfg; a test keeps it equal to what the Python host path builds). File layout: magic "WBCASSET1", the three struct
 * sizes (checked against this library's: -3 on a mismatch = another ABI version), dof / rigid-body counts, the structs (wbc_model,
 * wbc_task_cfg, wbc_curriculum before and after the first update_command_curriculum call), then the names (64-byte fields). */
typedef struct wbc_asset wbc_asset;
int wbc_asset_load(const char* path, wbc_asset** out);
void wbc_asset_free(wbc_asset* asset);
int wbc_asset_dof_count(const wbc_asset* asset);                       /* gym.get_asset_dof_count (WG:287) */
int wbc_asset_rigid_body_count(const wbc_asset* asset);                /* gym.get_asset_rigid_body_count (WG:288) */
const char* wbc_asset_dof_name(const wbc_asset* asset, int i);         /* gym.get_asset_dof_names (WG:293) */
const char* wbc_asset_rigid_body_name(const wbc_asset* asset, int i);  /* gym.get_asset_rigid_body_names (WG:292) */
/* gym.get_asset_dof_properties (WG:289, LR:279-305): lower / upper / velocity / effort, each dof_count floats (NULL: skipped) */
int wbc_asset_dof_properties(const wbc_asset* asset, float* lower, float* upper, float* velocity, float* effort);
const wbc_model* wbc_asset_model(const wbc_asset* asset);
const wbc_task_cfg* wbc_asset_task_cfg(const wbc_asset* asset);
/* which = 0: as the task object carries them before the first update_command_curriculum call; 1: after it (the shipped schedules
 * saturate on the first call, WG:678-692) */
const wbc_curriculum* wbc_asset_curriculum(const wbc_asset* asset, int which);

/* ---- asset from the URDF itself: gym.load_asset(sim, root, file, AssetOptions) (WG:268-285). A host-only loader
 * (deep-whole-body-control_amd/csrc/wbc_urdf.h: a small XML reader, no meshes opened) restates what the Python host path does
 * (urdf_model.build_model + abi.collision_set + abi.fill_model): inertial origins rotated (R I R^T), children depth-first in
 * alphabetical order of the child link (quirk Q1), collapse_fixed_joints honouring dont_collapse, prismatic joints whose URDF
 * friction is >= lock_friction_above as locked DoFs, composite inertias, the randomised base / gripper pieces and their rests,
 * the collision slots, limbs and candidates, rest_offset. On the shipped URDF the wbc_model is byte-identical to the packaged
 * asset's. The kernels are compiled for one topology, so the loader REFUSES (-4, wbc_last_error() names the element) joint
 * types other than revolute / fixed / locked prismatic (a prismatic joint whose friction is below lock_friction_above is refused
 * at the joint), a link tree deeper than 64 levels, axes other than +x/+y/+z, a non-zero joint rpy, counts other than
 * WBC_NB / WBC_NDOF / WBC_NRB, a missing foot / gripper / trunk / arm link, a limb pair over WBC_LIMB_RSUM_MAX, a reach beyond
 * the pair descriptor's 3 bits, and the options abi.UNSUPPORTED_SWITCHES refuses (asset.*). Unreadable or malformed XML and a
 * joint naming an unknown link are -2. On any error *out is left untouched. */
typedef struct wbc_asset_opts {
  uint32_t struct_size;                /* sizeof(wbc_asset_opts): set by wbc_asset_opts_default; another value is -1 */
  /* gymapi.AssetOptions as WG:268-282 sets them from cfg.asset */
  int32_t default_dof_drive_mode;      /* 3 = effort (WG:1183); anything else -4 */
  int32_t collapse_fixed_joints;       /* 1; 0 is -4 (the 27-body list is the collapsed one) */
  int32_t replace_cylinder_with_capsule, flip_visual_attachments;   /* accepted, no effect (no meshes / visuals here) */
  int32_t fix_base_link;               /* 0; 1 is -4 (floating base) */
  int32_t disable_gravity;             /* 0; 1 is -4 (set wbc_task_cfg.gravity instead) */
  double density;                      /* accepted, no effect: the URDF gives every link its mass */
  double angular_damping, linear_damping;                /* 0; anything else -4 (body damping is not modelled) */
  double max_angular_velocity, max_linear_velocity;      /* accepted, never reached */
  double armature;                     /* reported in wbc_dof_props.armature (a template's joint_armature already holds it) */
  double thickness;                    /* accepted, no effect */
  int32_t self_collisions;             /* Isaac Gym's meaning: 0 = self-collision ON (widowGo1_config.py:180) */
  char root_link[64];                  /* "base": the floating root, and the randomised base piece (WG:431-441) */
  char foot_name[64];                  /* "foot": rigid bodies whose name contains it are the feet (WG:297) */
  char gripper_name[64];               /* "wx250s/ee_gripper_link" (WG:318) */
  double lock_friction_above;          /* 100: a prismatic joint with URDF friction >= this is a locked DoF (the fingers: 1000) */
  double box_size;                     /* box.box_size (widowGo1_config.py:186): the free box actor's edge */
  double rest_offset;                  /* sim.physx.rest_offset (LRC:194) */
  double arm_limb_fit[3][3];           /* upper arm, forearm, hand: {radius, cap0, cap1} (abi.ARM_LIMB_FIT, assets/arm_primitives.json) */
  double soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit;   /* cfg.rewards (LR:294-304), 1.0 as shipped: used with a template */
} wbc_asset_opts;
void wbc_asset_opts_default(wbc_asset_opts* opts);   /* the shipped WidowGo1RoughCfg values */

/* `opts` NULL = defaults. cfg_template NULL: wbc_asset_task_cfg / wbc_asset_curriculum return NULL (gym.load_asset carries no task
 * config). With a template (e.g. the packaged asset): its task cfg and both curricula are copied, then the fields that come from the
 * model are recomputed from the URDF -- torque_limits (LR:294-299) and soft_dof_lower / _upper / soft_dof_vel_limit /
 * soft_torque_limit (LR:294-304). A template whose DoF or rigid-body names differ from the URDF's is -4; a template without a task
 * cfg (itself a URDF asset loaded without a template) is -1. */
int wbc_asset_load_urdf(const char* urdf_path, const wbc_asset_opts* opts, const wbc_asset* cfg_template, wbc_asset** out);

/* gym.get_asset_dof_properties (WG:289) with every DofProperties field, plus `locked` (a prismatic joint held by its friction) */
typedef struct wbc_dof_props {
  int32_t has_limits;                  /* 0 when the URDF gives lower == upper == 0 (widow_waist) */
  float lower, upper;
  int32_t drive_mode;                  /* AssetOptions.default_dof_drive_mode */
  float velocity, effort;
  float stiffness, damping;            /* 0 and the URDF's <dynamics damping> */
  float friction;                      /* URDF <dynamics friction> (the fingers: 1000) */
  float armature;                      /* AssetOptions.armature */
  int32_t locked;
} wbc_dof_props;
/* `out`: dof_count entries. A .wbcasset has no such table: -5. */
int wbc_asset_dof_properties_ex(const wbc_asset* asset, wbc_dof_props* out);
/* get_asset_rigid_body_dict / get_asset_dof_dict / find_actor_rigid_body_handle (WG:291,294,318): index, or -1 (either asset kind) */
int wbc_asset_find_rigid_body(const wbc_asset* asset, const char* name);
int wbc_asset_find_dof(const wbc_asset* asset, const char* name);
/* create_asset_force_sensor on the feet (WG:310-315): the rigid body behind each row of WBC_T_FORCE_SENSOR (either asset kind) */
int wbc_asset_force_sensor_bodies(const wbc_asset* asset, int32_t out[4]);

/* Bytes of device memory a sim of `num_envs` needs. */
size_t wbc_sim_arena_bytes(int num_envs);

/* gymapi.acquire_gym + create_sim + load_asset + the create_env/create_actor loop +
 * prepare_sim (BT:42,86-87; WG:234,285,355-392). `arena` is caller-provided device memory
 * of >= wbc_sim_arena_bytes(num_envs) bytes (e.g. a torch allocation, so that the tensors
 * below are zero-copy views of it); NULL lets the library hipMalloc its own. 1 <= num_envs <= 2^22 (the kernels index a tensor's
 * rows with 32-bit element offsets); anything else is -1 with a message in wbc_last_error(). */
int wbc_sim_create(const wbc_model* model, const wbc_task_cfg* cfg, int num_envs, int hip_device,
                   uint64_t seed, void* arena, size_t arena_bytes, wbc_sim** out);
int wbc_sim_destroy(wbc_sim* sim);

/* acquire_*_tensor + gymtorch.wrap_tensor (WG:505-551): device pointer, shape, dtype. */
int wbc_sim_get_tensor(wbc_sim* sim, int id, void** dev_ptr, int64_t shape[4], int* ndim, int* dtype);

/* Batched replacement for the O(N) per-env Python loop that sets shape friction and
 * randomised rigid-body properties (WG:365-389, 431-496) and motor strengths (WG:402-408).
 * Host pointers, N entries each (motor_strength N*18, base_dcom N*3, env_origins N*3); box_dmass = the box actor's added
 * mass (_box_process_rigid_body_props, WG:458-466), NULL = 0. */
int wbc_sim_set_env_params(wbc_sim* sim, const float* friction, const float* base_dmass,
                           const float* base_dcom, const float* gripper_dmass,
                           const float* motor_strength, const float* env_origins,
                           const float* box_delta_y, const float* traj_timesteps,
                           const float* traj_total_timesteps, const float* box_dmass);

/* gym.add_triangle_mesh for the regular-grid terrain (WG:242-252): the int16 height samples
 * the trimesh is built from, host pointer, rows*cols; NULL restores the flat plane. */
int wbc_sim_set_heightfield(wbc_sim* sim, const int16_t* heights, int rows, int cols,
                            float horizontal_scale, float vertical_scale,
                            float tx, float ty, float tz);

/* update_command_curriculum results (WG:678-692). */
int wbc_sim_set_curriculum(wbc_sim* sim, const wbc_curriculum* cur);

/* WidowGo1.step (WG:1156-1199) as ONE launch: action reorder/clip/delay FIFO, 4x
 * {_compute_torques, simulate}, post_physics_step (EE goal, commands, pushes, termination,
 * rewards, resets, observations), obs clipping. actions: device f32 [N,18], policy order. */
int wbc_sim_step(wbc_sim* sim, const float* actions_dev, void* stream);
/* The same step with the observation rows written to obs_out_dev (f32 [N,860], e.g. the rollout storage slot of the next
 * transition: what `self.observations[self.step].copy_(transition.observations)`, rollout_storage.py:66, would copy)
 * instead of WBC_T_OBS_BUF; obs_out_dev == NULL is wbc_sim_step. */
int wbc_sim_step_to(wbc_sim* sim, const float* actions_dev, float* obs_out_dev, void* stream);
/* The step with PPO.process_env_step's tensor work folded in (rsl_rl/algorithms/ppo.py:129-141, rollout_storage.py:70-72; what
 * wbc_rollout_store does as a separate launch): out_rewards[n] = (rew[n], arm_rew[n]) + gamma * values[n] * time_out[n],
 * out_dones[n] = reset_buf[n] != 0, written to the rollout storage's slots of this transition. values_dev: f32 [N,2], the
 * critic's output for the observation the actions were computed from. obs_out_dev as in wbc_sim_step_to; any of the two
 * groups may be NULL. */
int wbc_sim_step_rollout(wbc_sim* sim, const float* actions_dev, float* obs_out_dev, const float* values_dev, float gamma,
                         float* out_rewards_dev, uint8_t* out_dones_dev, void* stream);

/* BaseTask.reset() first half: reset_idx(all envs, start=True) (BT:127-131, WG:695-754). */
int wbc_sim_reset_all(wbc_sim* sim, void* stream);

/* gym.set_dof_actuation_force_tensor (WG:1183): device f32 [N,20]. */
int wbc_sim_set_dof_forces(wbc_sim* sim, const float* torques_dev, void* stream);
/* gym.simulate (WG:1184): one physics substep with the torques currently set. */
int wbc_sim_simulate(wbc_sim* sim, void* stream);
/* gym.set_actor_root_state_tensor / set_dof_state_tensor (WG:787,814,827): device pointers
 * with the layouts of WBC_T_ROOT_STATES / WBC_T_DOF_STATE; passing the sim's own tensor is a
 * no-op copy. The _indexed forms (LR:389-391,410-412) take int32 env ids on the device. */
int wbc_sim_set_root_state(wbc_sim* sim, const float* root_dev, void* stream);
int wbc_sim_set_dof_state(wbc_sim* sim, const float* dof_dev, void* stream);
int wbc_sim_set_root_state_indexed(wbc_sim* sim, const float* root_dev, const int32_t* env_ids_dev, int n, void* stream);
int wbc_sim_set_dof_state_indexed(wbc_sim* sim, const float* dof_dev, const int32_t* env_ids_dev, int n, void* stream);
/* gym.refresh_*_tensor (WG:513-519,870-873,1187-1191): state is resident, these return 0;
 * refresh_rigid_body_state recomputes forward kinematics after a state write. */
int wbc_sim_refresh_dof_state(wbc_sim* sim);
int wbc_sim_refresh_root_state(wbc_sim* sim);
int wbc_sim_refresh_net_contact_force(wbc_sim* sim);
int wbc_sim_refresh_force_sensor(wbc_sim* sim);
int wbc_sim_refresh_rigid_body_state(wbc_sim* sim, void* stream);

/* Step counter (common_step_counter, WG:613,876) get/set, for checkpoint/resume and tests. */
int wbc_sim_get_step_counter(wbc_sim* sim, int64_t* out);
int wbc_sim_set_step_counter(wbc_sim* sim, int64_t value);

/* RolloutStorage.compute_returns (RS:136-150) as one launch: reverse-time GAE over both
 * reward channels with shared dones, then advantages = returns - values. Device pointers:
 * rewards, values, returns, advantages f32 [T,N,2]; dones u8 [T,N]; last_values f32 [N,2].
 * stats_dev (f64 [wbc_gae_workspace_doubles(N)]; the first three entries receive count, sum and
 * sum of squares of the raw advantages) is filled for the joint normalisation (RS:150), which
 * wbc_gae_normalize applies with the (optionally all-reduced) statistics. */
int wbc_gae_compute(const float* rewards, const float* values, const uint8_t* dones,
                    const float* last_values, float* returns, float* advantages, double* stats_dev,
                    int T, int N, float gamma, float lam, void* stream);
/* (advantages - mean) / (std + 1e-8) over `total` = T*N*2 elements with the statistics in stats_dev[0..2]. */
int wbc_gae_normalize(float* advantages, const double* stats_dev, int64_t total, void* stream);
/* Number of doubles stats_dev must hold for N envs (3 statistics + per-block partials). */
int wbc_gae_workspace_doubles(int N);

/* Side jobs: a small per-step reduction that ANOTHER launch carries as a few extra workgroups instead of being a launch (and an
 * inter-kernel dependency stall) of its own. wbc_sim_episode_stats_job describes the work of wbc_sim_episode_stats_track without
 * launching it; wbc_policy_act_job (the policy inference that follows every env step in a rollout anyway) executes it next to
 * its own workgroups, wbc_side_job_run executes it stand-alone. The job holds device pointers into the sim's tensors: it must be
 * executed before the sim's next step. */
typedef struct {
  const float* ep_done; const float* met_done; const int64_t* reset_buf; const float* prev; const float* rew; const float* arm_rew;
  float* out; float* track_state;
  int32_t n, track_cap, nblocks;     /* nblocks: workgroups the job needs (one per statistics column + 1 with a tracker state) */
  float scale;
} wbc_side_job;
int wbc_sim_episode_stats_job(wbc_sim* sim, float scale, const float* prev, float* out, float* track_state, int track_cap,
                              wbc_side_job* job);
int wbc_side_job_run(const wbc_side_job* job, void* stream);

/* The policy side of one rollout step, PPO.act (rsl_rl/algorithms/ppo.py:115-127) with the privileged
 * latent: Actor.forward (actor_critic.py:204-221), Critic.forward (:281-286), the action sample
 * mean + std * eps (Normal.sample, :337-339) and get_actions_log_prob (:341-345) in ONE launch on fp32
 * MFMA. `params`: 33 device pointers in state_dict order of the layers used (struct PolicyParams in
 * csrc/wbc_mlp.h: priv_encoder.{0,2}, actor_backbone.0, leg head {0,2,4}, arm head {0,2,4},
 * critic_backbone.0, critic leg head {0,2,4}, critic arm head {0,2,4}, each weight then bias, then std).
 * `wpack`: wbc_policy_pack_floats() floats holding the weights in MFMA-fragment order; refresh it with
 * wbc_policy_pack whenever the parameters changed. obs f32 [rows,860]; eps f32 [rows,18] standard
 * normals (NULL: act on the mean); outputs actions/mean f32 [rows,18], logp/values f32 [rows,2].
 * `latent` f32 [rows,20] or NULL: if given (student path, hist_encoding=True, actor_critic.py:206-209) it replaces
 * the privileged encoder's output (e.g. the result of wbc_hist_latent). */
int wbc_policy_pack_floats(void);
int wbc_policy_pack(const void* const* params, float* wpack, void* stream);
int wbc_policy_act(const void* const* params, const float* wpack, const float* obs, const float* latent,
                   const float* eps, float* actions, float* mean, float* logp, float* values, int num_rows,
                   void* stream);
/* wbc_policy_act + a side job (may be NULL) executed by extra workgroups of the same launch. */
int wbc_policy_act_job(const void* const* params, const float* wpack, const float* obs, const float* latent,
                       const float* eps, float* actions, float* mean, float* logp, float* values, int num_rows,
                       const wbc_side_job* job, void* stream);

/* StateHistoryEncoder forward without gradient (rsl_rl/modules/actor_critic.py:39-84, tsteps = 10), the regulariser
 * target of PPO.update (ppo.py:174-176). params: 8 device pointers (encoder.0.weight [30,76], .bias,
 * conv_layers.0.weight [20,30,4], .bias, conv_layers.2.weight [10,20,2], .bias, linear_output.0.weight [20,30],
 * .bias); reads obs[:, 100:860] of f32 [rows,860]; writes out f32 [rows,20]. ELU activations. */
int wbc_hist_latent(const void* const* params, const float* obs, float* out, int rows, void* stream);

/* One PPO.update() minibatch (rsl_rl/algorithms/ppo.py:163-246, teacher path, no torque supervision): gathers
 * the rows `idx` of the flat [T*N, ...] rollout tensors, runs actor + critic forward, the clipped surrogate
 * with Advantage Mixing (:199-206), the (clipped) value loss (:209-216) and the ROA regulariser (:174-179),
 * and back-propagates; writes into `grad` (wbc_ppo_grad_floats() floats) the gradient of
 * surrogate + value_coef*value_loss + roa_coef*priv_reg in the order: for each of the 16 layers of
 * `params` (same table as wbc_policy_act) weight then bias; std[18]; then the three loss SUMS (surrogate and
 * value over B*2 entries, priv_reg over B). `hist_latent` f32 [T*N,20]: history-encoder latent of every
 * stored row (constant during update()). `workspace`: wbc_ppo_workspace_floats(B) floats. `loss_accum` (device, 3 floats,
 * or NULL): the three loss sums are also ADDED to it (an update's running totals without a launch of its own).
 * Also leaves, at workspace + wbc_ppo_sq_partials_offset(B), partial sums of squares of the gradient it wrote
 * (wbc_ppo_clip_adam's `sq_partials`). Deterministic. B < 338 000 rows (32-bit offsets into the workspace); -3 beyond. */
int wbc_ppo_minibatch_grad(const void* const* params, const float* obs, const float* actions,
                           const float* old_values, const float* advantages, const float* returns,
                           const float* old_logp, const float* hist_latent, const int64_t* idx, int B,
                           float clip, float value_coef, float mixing, float roa_coef,
                           int use_clipped_value_loss, float* workspace, float* grad, float* loss_accum, void* stream);
/* The same call without its weight-pack launch (5.9 us + a launch gap of every minibatch): valid while `workspace` still holds the
 * weight streams that a wbc_ppo_minibatch_grad call for the same B packed into it and every change of the parameters since then
 * was a wbc_ppo_clip_adam_packed(..., workspace, B) step (which keeps the streams current). The library keeps a record per workspace
 * (B, params[0]) of which streams are current: a call whose (workspace, B, params[0]) does not match it -- a different B, a
 * reallocated workspace, another parameter set, a plain wbc_ppo_clip_adam step in between -- packs afresh instead of computing
 * gradients against stale weights. What the library cannot see is a write to the parameters by other code (a checkpoint load, a
 * broadcast): follow it with wbc_ppo_minibatch_grad (or wbc_ppo_pack_invalidate(workspace); NULL drops every record). */
int wbc_ppo_minibatch_grad_packed(const void* const* params, const float* obs, const float* actions,
                                  const float* old_values, const float* advantages, const float* returns,
                                  const float* old_logp, const float* hist_latent, const int64_t* idx, int B,
                                  float clip, float value_coef, float mixing, float roa_coef,
                                  int use_clipped_value_loss, float* workspace, float* grad, float* loss_accum, void* stream);
int wbc_ppo_pack_invalidate(const float* workspace);
size_t wbc_ppo_sq_partials_offset(int B);
/* nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.Adam.step() (ppo.py:243-246) for the 33 parameters of
 * `params`, reading their gradients from grad[0 : wbc_ppo_grad_floats()-3] (scaled in place by the clip factor);
 * exp_avg / exp_avg_sq are flat Adam moments in the same layout. step_size = lr/(1-beta1^t), bc2_sqrt =
 * sqrt(1-beta2^t). max_norm <= 0 disables the clip. grad_scale (> 0) multiplies the gradient before the clip: 1 on one GPU,
 * 1 / world_size after the SUM all-reduce of the sharded learner (the mean over ranks without a separate launch).
 * sq_partials: the partial sums of squares wbc_ppo_minibatch_grad left for THIS gradient (pass them only while grad is
 * exactly what that call wrote -- not after an all-reduce), or NULL: the same partials are then recomputed from grad (same
 * blocks, same order: the two ways give the same bits for the same gradient).
 * workspace: >= wbc_ppo_clip_adam_workspace_floats() floats. Deterministic. */
int wbc_ppo_clip_adam_workspace_floats(void);
int wbc_ppo_clip_adam(const void* const* params, float* grad, float* exp_avg, float* exp_avg_sq, float max_norm,
                      float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float grad_scale,
                      const float* sq_partials, float* workspace, void* stream);
/* wbc_ppo_clip_adam, and every updated parameter is also written to its copies in the weight streams inside `mb_workspace` (the
 * wbc_ppo_minibatch_grad workspace for B rows): see wbc_ppo_minibatch_grad_packed. A workspace whose streams were not packed from
 * these parameters for this B is left alone (the step is then a plain wbc_ppo_clip_adam). -4: the scatter table could not be built. */
int wbc_ppo_clip_adam_packed(const void* const* params, float* grad, float* exp_avg, float* exp_avg_sq, float max_norm,
                             float beta1, float beta2, float eps, float step_size, float bc2_sqrt, float grad_scale,
                             const float* sq_partials, float* workspace, float* mb_workspace, int B, void* stream);
/* One minibatch of PPO.update_dagger (rsl_rl/algorithms/ppo.py:265-291): the history encoder's forward
 * (rsl_rl/modules/actor_critic.py:39-84), loss = mean over rows of ||target - latent||_2, backward and weight gradients
 * for the `rows` rows obs[idx[r]] (obs f32 [batch, 860], target f32 [batch, 20] = the privileged latents, idx i64 [rows]).
 * params: the 8 tensors of wbc_hist_latent. grad (out): wbc_hist_train_grad_floats() floats = the flat gradient in
 * history_encoder.parameters() order (5760) followed by the minibatch's SUM of row norms (divide by rows for the loss).
 * workspace: wbc_hist_train_workspace_floats() floats. Deterministic (fixed-order reduction). */
int wbc_hist_train_grad(const void* const* params, const float* obs, const float* target, const long long* idx, int rows,
                        float* workspace, float* grad, void* stream);
int wbc_hist_train_grad_floats(void);
size_t wbc_hist_train_workspace_floats(void);
/* clip_grad_norm_ + Adam.step (ppo.py:283-284) of the history encoder on the flat buffers, as wbc_ppo_clip_adam.
 * grad_was_reduced != 0: grad was changed since wbc_hist_train_grad (all-reduce over ranks); the squares of the reduced
 * gradient are re-derived by a launch of their own BEFORE the one that rescales grad in place (every block of the Adam
 * launch sees the same norm). workspace: the one passed to wbc_hist_train_grad (its squared-gradient tail is rewritten). */
int wbc_hist_clip_adam(const void* const* params, float* grad, float* exp_avg, float* exp_avg_sq, float max_norm, float beta1,
                       float beta2, float eps, float step_size, float bc2_sqrt, float grad_scale, int grad_was_reduced,
                       float* workspace, void* stream);
/* Actor.infer_priv_latent (actor_critic.py:219-221) for every row: params = priv_encoder.{0,2}.{weight,bias} ([64,24], [64],
 * [20,64], [20]); obs f32 [rows, 860]; out f32 [rows, 20]. */
int wbc_priv_latent(const void* const* params, const float* obs, float* out, int rows, void* stream);
int wbc_ppo_grad_floats(void);
int wbc_ppo_num_splits(void);
size_t wbc_ppo_workspace_floats(int B);

/* What Isaac Gym's mass-matrix / Jacobian tensors give the torque-supervision path (widowGo1.py:550-558, 1201-1242):
 * mm f32 [N,6,6] = joint-space inertia block of the 6 arm joints, jac f32 [N,6,6] = world-frame Jacobian of the
 * end-effector rigid body w.r.t. them (rows linear xyz, angular xyz), gtorque f32 [N,6] = sum over the rigid bodies
 * link_rb9 (the actor's last 9) of J_body^T (0,0,9.81 m,0,0,0) with the host masses link_mass9 (+ env 0's gripper mass
 * delta, as the reference reads env 0's properties). Computed from the sim's current root / DoF state. */
int wbc_sim_arm_dynamics(wbc_sim* sim, const int* link_rb9, const float* link_mass9, float* mm, float* jac,
                         float* gtorque, void* stream);

/* Isaac Gym's whole-body tensors of the robot actor (acquire_jacobian_tensor / acquire_mass_matrix_tensor, widowGo1.py:509-510,
 * 517-518, 550-558), from the sim's current root / DoF state and per-env body parameters (WBC_T_BODY_PARAMS).
 * Generalised velocity nu = (v_root, omega_root, qd[0..WBC_NDOF-1]), WBC_NCOL = 6 + WBC_NDOF = 26 columns:
 *   v_root, omega_root  the root origin's linear and the root's angular velocity, world frame (WBC_T_ROOT_STATES[:, 0, 7:13]);
 *   qd                  simulator DoF order (WBC_T_DOF_STATE[..., 1]); column 6 + d is DoF d.
 * jac f32 [N, WBC_NRB, 6, 26]: rows 0:3 the world-frame linear velocity of rigid body r's ORIGIN (rb_offset), rows 3:6 its
 *   angular velocity, as linear maps of nu: J[e, r] @ nu_e == rigid_body_state[e, r, 7:13] (wbc_sim_refresh_rigid_body_state).
 *   A DoF column is non-zero only where that joint is an ancestor of r's moving body.
 * mm f32 [N, 26, 26]: kinetic energy 1/2 nu^T M nu = sum over moving bodies of 1/2 (m |v_com|^2 + omega^T I_world omega) with the
 *   per-env root composite and gripper body of WBC_T_BODY_PARAMS (the inertias the step kernel integrates with).
 * Locked fingers (DoFs 18, 19: prismatic joints the dynamics treats as rigid, see urdf_model.build_model): their columns of J
 * and their rows and columns of M are exactly zero; M restricted to the other 24 coordinates is symmetric positive definite.
 * jac / mm: caller-owned device memory, 16-byte aligned; either may be NULL (that tensor is not written), not both.
 * -1 with a message in wbc_last_error() for a NULL sim, both outputs NULL or a misaligned output. */
#define WBC_NCOL (6 + WBC_NDOF)
int wbc_sim_body_dynamics(wbc_sim* sim, float* jac, float* mm, void* stream);

/* Whole-body inverse dynamics in the coordinates of wbc_sim_body_dynamics: the third term of the equations of motion
 *     M(q) nudot + h(q, nu) = S^T tau_joint + sum J_c^T f_c ,     h = C(q, nu) nu + g(q) ,
 * i.e. tau = M nudot + C nu + g, from the sim's current WBC_T_ROOT_STATES (orientation and nu[0:6]), WBC_T_DOF_STATE (q, qd),
 * per-env WBC_T_BODY_PARAMS (root composite and gripper body, as wbc_sim_body_dynamics uses them) and all three components of
 * wbc_task_cfg.gravity. One launch of a recursive Newton-Euler kernel.
 * nudot  device f32 [N, 26] or NULL (= zeros): d/dt of the WORLD components of nu -- the classical linear acceleration of the root
 *        origin, the angular acceleration of the root, the joint accelerations in simulator DoF order.
 * tau    device f32 [N, 26] or NULL: rows 0:3 the net external force on the robot (world axes), rows 3:6 the net external moment
 *        about the ROOT ORIGIN (world axes), rows 6: the joint torques, such that (q, nu, nudot) is the motion the rigid-body
 *        dynamics produce. With nudot == NULL this is the bias vector h. tau(nudot) - tau(0) == mm @ nudot by definition.
 * grav   device f32 [N, 26] or NULL: g(q) alone (tau at nu = 0, nudot = 0); h - g is the velocity-product term C nu.
 * At least one of tau / grav is non-NULL; all three pointers need 4-byte alignment only.
 * Locked fingers (DoFs 18, 19): their entries of nudot and of qd are ignored, their rows of tau / grav are exactly 0.
 * The root POSITION is never read: the result is bit-identical under a translation of the robot.
 * This is RIGID-BODY dynamics: wbc_task_cfg.joint_armature, the joint-limit stop torques and contacts are not part of it.
 * -1 with a message in wbc_last_error() for a NULL sim, both outputs NULL or a misaligned pointer; -3 for a model whose tree the
 * kernel cannot walk; -2 if the launch fails. Stream / device handling as wbc_sim_body_dynamics. */
int wbc_sim_inverse_dynamics(wbc_sim* sim, const float* nudot, float* tau, float* grav, void* stream);

/* M^-1 in the coordinates of wbc_sim_body_dynamics, M formed from the sim's CURRENT state inside the launch and factorised as
 * L^T D L over the kinematic tree (leaves first: no fill-in); it never goes through memory.
 *     out[e, k, :] = M_e^-1 rhs[e, k, :]   for k < nrhs.
 * rhs    device f32: right-hand side k of env e is the 26 contiguous floats at rhs + e * rhs_env_stride + 26 k.
 *        rhs_env_stride is in floats and >= 26 nrhs, so that the view jac[:, r] of one rigid body's six Jacobian rows (env stride
 *        27 * 156) can be passed as it stands: M is symmetric, the result is then (M^-1 J_r^T)^T and out @ J_r^T the inverse
 *        operational-space inertia J_r M^-1 J_r^T.
 * out    device f32 [N, nrhs, 26], contiguous, not overlapping rhs. Both pointers need 4-byte alignment only.
 * flags  0, or WBC_SOLVE_ARMATURE: solve with M + diag(0_6, wbc_task_cfg.joint_armature[0..]) -- the matrix one airborne substep
 *        of the step kernel integrates with (the implicit-PD armature).
 * Locked fingers (coordinates 24, 25): their entries of rhs are ignored, their entries of out are exactly 0; the other 24
 * coordinates are solved as a symmetric positive definite system. The root POSITION is never read: the result is bit-identical
 * under a translation of the robot.
 * -1 with a message in wbc_last_error() for a NULL sim / rhs / out, nrhs outside 1..WBC_SOLVE_MAX_RHS, a stride below 26 nrhs,
 * unknown flag bits or a misaligned pointer (nothing is written); -3 for a model whose tree the kernel cannot walk; -2 if the
 * launch fails. Stream / device handling as wbc_sim_body_dynamics. */
#define WBC_SOLVE_ARMATURE 1
#define WBC_SOLVE_MAX_RHS 32
int wbc_sim_mass_solve(wbc_sim* sim, const float* rhs, int64_t rhs_env_stride, int nrhs, float* out, int flags, void* stream);

/* Forward dynamics nudot = M^-1 (tau - h), the inverse of wbc_sim_inverse_dynamics: tau device f32 [N, 26] or NULL (= zeros) in
 * that function's conventions (rows 0:3 the net external force, rows 3:6 the net external moment about the root origin, world
 * axes; rows 6: the joint torques; a caller adds J^T f of contacts itself), nudot device f32 [N, 26]. Two launches on `stream`:
 * the inverse-dynamics kernel writes h into a [N, 26] buffer the sim owns (allocated by wbc_sim_create, so the call is safe under stream capture), the solve subtracts it. That buffer
 * is one per sim: calls for the same sim on DIFFERENT streams must be ordered by the caller (events), or they race on h.
 * Without flags this is rigid-body dynamics: wbc_sim_inverse_dynamics(nudot) returns tau up to rounding. With
 * WBC_SOLVE_ARMATURE it is the acceleration one airborne substep of the step kernel applies for the applied torques tau[6:]
 * away from the joint limits. Fingers, translation, alignment and error codes as wbc_sim_mass_solve (NULL nudot: -1). */
int wbc_sim_forward_dynamics(wbc_sim* sim, const float* tau, float* nudot, int flags, void* stream);

/* How every rigid body accelerates: acc[e, r] = J[e, r] @ nudot_e + (Jdot nu)[e, r] with J the matrix of wbc_sim_body_dynamics, so
 * that a task-space law has xddot = J nudot + Jdot nu without differencing two Jacobian refreshes.
 * nudot  device f32 [N, 26] or NULL (= zeros, the result is then Jdot nu), in the convention of wbc_sim_inverse_dynamics:
 *        nudot[0:3] is the classical acceleration of the root origin.
 * acc    device f32 [N, WBC_NRB, 6], the layout of rigid_body_state[..., 7:13]: rows 0:3 the classical world-frame linear
 *        acceleration of rigid body r's ORIGIN (rb_offset), rows 3:6 its angular acceleration.
 * Pure kinematics: no gravity and no inertias (WBC_T_BODY_PARAMS is not read). The fingers' entries of nudot and of qd are
 * ignored. The root POSITION is never read: the result is bit-identical under a translation of the robot. One launch
 * (wbc_body_accel_kernel). Alignment (4 bytes), error codes (-1 NULL sim / acc or misaligned pointer, nothing written; -3; -2)
 * and stream handling as wbc_sim_inverse_dynamics. */
int wbc_sim_body_accelerations(wbc_sim* sim, const float* nudot, float* acc, void* stream);

/* Forward dynamics with the origins of up to WBC_CONSTR_MAX_BODIES rigid bodies held by bilateral constraints on their LINEAR
 * acceleration (the stance feet of the standard whole-body-control model; angular rows are not offered):
 *     M nudot + h = tau + sum_r J_r^T lambda_r ,      J_r nudot + (Jdot nu)_r = a_des_r - damping lambda_r ,
 * J_r the three linear rows of wbc_sim_body_dynamics' Jacobian of listed body r.
 * rigid_bodies  HOST array of nbodies (1..WBC_CONSTR_MAX_BODIES) rigid-body indices, e.g. the four feet, or the feet and the gripper.
 * active   device u8 [N, nbodies] or NULL (= all active): the per-env stance mask. An inactive body contributes no constraint, its
 *          entries of lambda are exactly 0 and its entries of acc_des are never used (a NaN there does not spread).
 * tau      device f32 [N, 26] or NULL (= zeros), as in wbc_sim_forward_dynamics.
 * acc_des  device f32 [N, nbodies, 3] or NULL (= zeros): the prescribed world-frame accelerations of the origins.
 * damping  >= 0, added to the diagonal of the Delassus matrix A = J_c M^-1 J_c^T; 0 gives hard constraints.
 * flags    0 or WBC_SOLVE_ARMATURE (M + armature, as in wbc_sim_mass_solve).
 * nudot    device f32 [N, 26], fingers exactly 0. lambda: device f32 [N, nbodies, 3] or NULL (not written).
 *          lambda_r is the force applied TO the robot at body r's origin in world axes: a standing robot's foot forces point up.
 * workspace  caller-owned device floats, at least wbc_sim_constrained_dynamics_workspace_floats(N, nbodies) of them (0 for a bad
 *          argument). Nothing is allocated in the call, so it is safe under stream capture. The sim's bias-force scratch of
 *          wbc_sim_forward_dynamics is used as well, with the same caveat: one stream at a time per sim.
 * Four launches on `stream`, no host synchronisation: h (wbc_inverse_dynamics_kernel), the right-hand-side block [J_c^T | tau - h]
 * and gamma = Jdot nu (wbc_constraint_rhs_kernel), the mass solve with 3 nbodies + 1 right-hand sides, and
 * wbc_constraint_solve_kernel (A, its Cholesky factorisation, lambda, nudot = a_free + M^-1 J_c^T lambda).
 * -1 with a message in wbc_last_error(), nothing written: NULL sim / rigid_bodies / nudot / workspace; nbodies outside
 * 1..WBC_CONSTR_MAX_BODIES; an index outside 0..WBC_NRB-1; two entries that ride on the same moving body (duplicates included:
 * their rows are linearly dependent); damping negative or not finite; unknown flag bits; a pointer that is not 4-byte aligned.
 * Any other rank deficiency is the caller's to regularise with damping: for an env whose A is not positive definite that env's
 * outputs are unspecified, and no other env is affected. -3 / -2 as wbc_sim_mass_solve. */
#define WBC_CONSTR_MAX_BODIES 5
size_t wbc_sim_constrained_dynamics_workspace_floats(int num_envs, int nbodies);
int wbc_sim_constrained_dynamics(wbc_sim* sim, const int32_t* rigid_bodies /* host */, int nbodies, const uint8_t* active,
                                 const float* tau, const float* acc_des, float damping, int flags, float* nudot, float* lambda,
                                 float* workspace, void* stream);

/* What a change of the contact set does to the velocity: the impulse-level counterpart of wbc_sim_constrained_dynamics. When a swing
 * foot lands (or the robot is pushed while it stands), the generalised velocity jumps from the state's nu to nu+, per env
 *     M (nu+ - nu) = iota + sum_r J_r^T Lambda_r ,      J_r nu+ + damping Lambda_r = vdes_r - e_r (u_r - vdes_r)   for every active r,
 * with u_r = J_r nu the pre-impact world-frame velocity of listed body r's origin (three linear rows). Coordinates, nu, rigid-body
 * indices, the fingers, WBC_T_BODY_PARAMS, WBC_SOLVE_ARMATURE and stream handling are those of wbc_sim_constrained_dynamics.
 * rigid_bodies, nbodies, active: as there. An inactive body contributes no row, its entries of impulse are exactly 0 and its entries of
 *              restitution and vel_des are never loaded into arithmetic (a NaN there does not spread).
 * restitution  device f32 [N, nbodies] or NULL (= zeros, a plastic impact): Newton's coefficient e_r relative to the surface velocity,
 *              used as given (values outside 0..1 are the caller's business).
 * vel_des      device f32 [N, nbodies, 3] or NULL (= zeros): the surface's world-frame velocity at the contact.
 * impulse_ext  device f32 [N, 26] or NULL (= zeros): a generalised impulse iota in the row conventions of tau in
 *              wbc_sim_forward_dynamics (rows 0:3 a linear impulse on the robot, rows 3:6 an angular impulse about the root origin,
 *              rows 6: joint impulses); a push on the trunk, or a J^T p the caller formed. Finger entries are ignored.
 * damping      >= 0, added to the diagonal of the Delassus matrix. flags: 0 or WBC_SOLVE_ARMATURE.
 * nu_plus      device f32 [N, 26], fingers exactly 0. With no active body and impulse_ext NULL it is the state's nu bit for bit on the
 *              live coordinates.
 * impulse      device f32 [N, nbodies, 3] or NULL: Lambda_r in N s, applied TO the robot at body r's origin, world axes.
 * denergy      device f32 [N] or NULL: T(nu+) - T(nu), T = nu^T M nu / 2 with the matrix the solve used, formed as the quadratic form
 *              g^T nu + g^T M^-1 g / 2 of g = iota + J^T Lambda (not as a difference of two energies). Exactly 0 with no active body
 *              and impulse_ext NULL.
 * dnu_dnu      device f32 [N, 26, 26] or NULL, 16-byte aligned: the exact linear map P[e, i, j] = d nu+_i / d nu_j
 *              = 1 - M^-1 J^T (A + damping)^-1 diag(1 + e) J on the live coordinates, finger rows and columns exactly 0. With
 *              impulse_ext and vel_des NULL, nu+ = P nu. The other outputs have the same bits with and without it.
 * workspace    caller-owned device floats, at least wbc_sim_impulse_dynamics_workspace_floats(N, nbodies) of them (0 for a bad
 *              argument). Nothing is allocated in the call and no bias-force scratch is used (no h enters), so the call is safe under
 *              stream capture and calls on different streams need their own workspaces only.
 * The root position is never read: every output is bit-identical under a translation of the robot.
 * Three launches on `stream`, no host synchronisation: wbc_impulse_rhs_kernel ([J_c^T | iota]), the mass solve with
 * 3 nbodies + 1 right-hand sides, wbc_impulse_solve_kernel (u = J nu, A, its Cholesky factorisation, Lambda, nu+; or
 * wbc_impulse_solve_map_kernel where dnu_dnu is given).
 * -1 with a message in wbc_last_error() that names this entry point, nothing written: NULL sim / rigid_bodies / nu_plus / workspace;
 * nbodies outside 1..WBC_CONSTR_MAX_BODIES; an index outside 0..WBC_NRB-1; two entries that ride on the same moving body; damping
 * negative or not finite; unknown flag bits; a pointer that is not 4-byte aligned; dnu_dnu not 16-byte aligned. The checks that need
 * no sim are made first. Rank deficiency, -3 and -2 as wbc_sim_constrained_dynamics. */
size_t wbc_sim_impulse_dynamics_workspace_floats(int num_envs, int nbodies);
int wbc_sim_impulse_dynamics(wbc_sim* sim, const int32_t* rigid_bodies /* host */, int nbodies, const uint8_t* active,
                             const float* restitution, const float* vel_des, const float* impulse_ext, float damping, int flags,
                             float* nu_plus, float* impulse, float* denergy, float* dnu_dnu, float* workspace, void* stream);

/* Whole-body inverse kinematics with joint limits: which configuration puts the listed rigid bodies at the wanted poses. Per env, over
 * the 24 live coordinates (root translation, root rotation, the 18 revolute joints; the fingers stay locked):
 *     minimise  1/2 sum_k sum_{i<3} w_pos[k,i] (target_pos[k,i] - x_k(q)_i)^2 + 1/2 sum_k w_ori[k] |log(R_target,k R_k(q)^T)|^2
 *             + 1/2 posture |q_j - q_ref|^2  (the 18 joints)         subject to  q_lower[j] <= q_j <= q_upper[j]
 * x_k, R_k: world origin (rb_offset) and rotation of rigid body bodies[k], as wbc_sim_refresh_rigid_body_state reports them; limits
 * from wbc_model, lower == upper == 0 meaning unlimited. Tangent: root translation in world axes, a WORLD rotation vector
 * (R <- exp([dtheta]x) R) and joint increments, so the Gauss-Newton Jacobian of target k is rows 0:3 / 3:6 of wbc_sim_body_dynamics'
 * J[bodies[k]]; for the scalar w_ori the orientation term's exact gradient is -w_ori J_ang^T phi.
 * bodies       HOST array of 1..WBC_IK_MAX_TARGETS rigid-body indices; two entries on one moving body are allowed.
 * target_pos   device f32 [N, nt, 3]. target_quat device f32 [N, nt, 4] (xyzw, normalised by the kernel) or NULL: no orientation rows.
 * w_pos        device f32 [N, nt, 3], >= 0, or NULL (= ones). w_ori device f32 [N, nt] or NULL (= ones where target_quat is given);
 *              NULL where target_quat is NULL. A row of weight 0 is skipped: its target is never loaded into arithmetic (a NaN there
 *              does not spread) and its entry of residual is exactly 0.
 * root_init    device f32 [N, 7] (position, xyzw quaternion) or NULL (= WBC_T_ROOT_STATES[:, 0, 0:7]); dof_init device f32 [N, 20] or
 *              NULL (= WBC_T_DOF_STATE[..., 0]); start joints outside their limits are clamped before the first evaluation.
 * q_ref        device f32 [N, 20] or NULL (= the clamped start joints).
 * opts         HOST: posture >= 0; damping > 0, the initial Levenberg-Marquardt factor lambda0 on diag(H); step_tol > 0 (metres and
 *              radians); max_iter 1..WBC_IK_MAX_ITER, 0 = WBC_IK_MAX_ITER.
 * root_out     device f32 [N, 7]: a unit quaternion wherever a step was accepted; where none was (iterations 0, or status 3) the
 *              start's own seven floats bit for bit, its quaternion as given and not re-normalised. dof_out device f32 [N, 20]: the
 *              fingers are the start's bits, limited joints lie inside their limits exactly.
 * residual     device f32 [N, nt, 6] or NULL: target - x and phi at the output. cost device f32 [N, 2] or NULL: the objective at the
 *              start and at the output (cost[:,1] <= cost[:,0] bit-wise).
 * status       device i32 [N] or NULL: 0 converged (the proposed projected step's infinity norm <= step_tol while lambda <= lambda0),
 *              1 iteration cap, 2 no descent before the damping reached its ceiling (stationary to fp32 resolution, or a target out of
 *              reach), 3 a non-finite input of that env (its outputs are the start; no other env is affected).
 * iterations   device i32 [N] or NULL: candidates evaluated.
 * Projected Levenberg-Marquardt: H = J^T W J + posture S^T S and g in LDS; a joint at a limit whose gradient pushes outward gets the
 * identity's row and column; (H + lambda diag H + floor) d = -g; where a free joint's step would leave its limits, that joint goes
 * onto the limit and the others solve once more with its step held; retract, clamp, evaluate; accepted if the cost did not rise
 * (lambda /= 8), else lambda *= 8. The point returned is the last accepted one. Positions are carried relative to the start root
 * position p0: under a translation S of start and targets that is exact in fp32 every output but root_out[:, 0:3] is bit-identical,
 * and root_out[:, 0:3] = fl(p0 + d) with the same bits of the relative position d, so it moves by S to within one ulp of the moved
 * value (fl(p0 + S + d) is not fl(p0 + d) + S in general).
 * The sim's state is read and never written. One launch (wbc_ik_kernel), no workspace, nothing allocated: safe under stream capture and
 * on any stream.
 * -1 with a message in wbc_last_error() that names this entry point, nothing written: NULL sim / bodies / target_pos / opts / root_out /
 * dof_out; ntargets out of range; a body index outside 0..WBC_NRB-1; w_ori without target_quat; an opts field out of range or not
 * finite; a pointer that is not 4-byte aligned. The checks that need no sim are made first. -3 and -2 as wbc_sim_mass_solve. */
#define WBC_IK_MAX_TARGETS 6
#define WBC_IK_MAX_ITER 64
typedef struct { float posture, damping, step_tol; int32_t max_iter; } wbc_ik_opts;
int wbc_sim_inverse_kinematics(wbc_sim* sim, const int32_t* bodies /* host */, int ntargets, const float* target_pos,
                               const float* target_quat, const float* w_pos, const float* w_ori, const float* root_init,
                               const float* dof_init, const float* q_ref, const wbc_ik_opts* opts /* host */, float* root_out,
                               float* dof_out, float* residual, float* cost, int32_t* status, int32_t* iterations, void* stream);

/* Whole-body inverse dynamics for task-space accelerations: the joint torques that produce wanted accelerations of a few rigid bodies
 * while the stance feet stay put. Coordinates, nu, nudot, tau rows and rigid-body indices are those of wbc_sim_body_dynamics /
 * wbc_sim_inverse_dynamics / wbc_sim_constrained_dynamics; state, WBC_T_BODY_PARAMS and all three gravity components as there. Per env:
 *     minimise over (nudot, lambda, tau_j)
 *         1/2 sum_{k<ntasks} sum_{i<6} w[k,i] ((J_k nudot + Jdot_k nu)_i - acc[k,i])^2     origin of task body k: linear 0:3, angular 3:6
 *       + 1/2 posture |nudot - nudot_ref|^2 (24 live coordinates) + 1/2 force |lambda|^2 + 1/2 torque |tau_j|^2
 *     subject to
 *         M nudot + h = S^T tau_j + sum_r J_r^T lambda_r                 (the six root rows carry no actuation)
 *         J_r nudot + (Jdot nu)_r = stance_acc_r - damping lambda_r      for every ACTIVE stance body r (three linear rows)
 * tau_j are the 18 revolute joint torques; the locked fingers' entries are exactly 0 everywhere. torque > 0 makes the solution unique
 * for every stance pattern. NO INEQUALITIES are offered: no friction cones, no unilateral contact and no torque limits -- a caller
 * clamps the result, or raises `force` / `torque`, or calls wbc_sim_task_inverse_dynamics_qp below, which solves with them.
 * stance_bodies  HOST array of nstance (0..WBC_TASKID_MAX_STANCE) rigid-body indices, e.g. the four feet.
 * active      device u8 [N, nstance] or NULL (= all active). An inactive body contributes no constraint, its lambda is exactly 0 and
 *             its stance_acc is never read (a NaN there does not spread).
 * stance_acc  device f32 [N, nstance, 3] or NULL (= zeros).
 * task_bodies HOST array of ntasks (0..WBC_TASKID_MAX_TASKS) rigid-body indices. A body may be both a stance and a task body (a foot
 *             that swings in one env and stands in the next: task weight 0 where it is active).
 * task_acc    device f32 [N, ntasks, 6]; task_weight device f32 [N, ntasks, 6] >= 0 or NULL (= ones). A row of weight 0 is skipped and
 *             its task_acc is never read.
 * nudot_ref   device f32 [N, 26] or NULL (= zeros). weights: HOST struct; damping as in wbc_sim_constrained_dynamics.
 * flags       0 or WBC_SOLVE_ARMATURE (M + armature throughout).
 * tau         device f32 [N, 26]: rows 0:6 and the fingers exactly 0, rows 6: tau_j in DoF order (tau[:, 6:] is what
 *             wbc_sim_set_dof_forces takes). nudot: device f32 [N, 26] or NULL. lambda: device f32 [N, nstance, 3] or NULL; the force
 *             applied TO the robot, as in wbc_sim_constrained_dynamics.
 * workspace   caller-owned device floats, at least wbc_sim_task_inverse_dynamics_workspace_floats(N, nstance, ntasks) of them (0 for a
 *             bad argument). Nothing is allocated in the call, so it is safe under stream capture. The sim's bias-force scratch is used
 *             as well: one stream at a time per sim.
 * Four launches on `stream`, no host synchronisation: h, the right-hand sides [J_c^T | -h | S^T] with the task rows
 * (wbc_taskid_rhs_kernel), the mass solve with 3 nstance + 19 right-hand sides, and wbc_taskid_solve_kernel: the problem reduced to
 * the 18 torques through stance-constrained forward dynamics and solved in square-root form (Householder reflections of the stacked
 * sqrt(weight)-scaled rows, at most 90 x 19); (nudot, lambda) are then those of constrained forward dynamics with tau.
 * The root POSITION is never read: outputs are bit-identical under a translation of the robot.
 * Accuracy (fp32): the equations of motion and the stance rows hold to the rounding of wbc_sim_constrained_dynamics for every call.
 * First-order optimality holds to fp32 rounding of the SIZES of the objective's terms (|J nudot| + |Jdot nu| + |acc|, |nudot| +
 * |nudot_ref|, |lambda|, |tau|). It is NOT held to that level where a term is a small difference of large fp32 quantities that those
 * sizes do not show: with ntasks = 0 and nudot_ref = 0 (or NULL) the posture term pins the light wrist joints' accelerations near 0
 * while a_0 = -M^-1 h and M^-1 S^T tau_j are each tens of rad/s^2 there; the reduced gradient then sits one to two orders above its
 * level with tasks or with a reference of the size of the accelerations at play.
 * -1 with a message in wbc_last_error(), nothing written: NULL sim / tau / workspace / weights; NULL stance_bodies, task_bodies or
 * task_acc with its count above 0; a count out of range; an index outside 0..WBC_NRB-1; two stance entries, or two task entries, on the
 * same moving body; torque <= 0 or not finite; posture, force or damping negative or not finite; unknown flag bits; a pointer that is
 * not 4-byte aligned. -3 / -2 as wbc_sim_mass_solve. */
#define WBC_TASKID_MAX_STANCE 4
#define WBC_TASKID_MAX_TASKS 6
typedef struct { float posture, force, torque, damping; } wbc_taskid_weights;
size_t wbc_sim_task_inverse_dynamics_workspace_floats(int num_envs, int nstance, int ntasks);
int wbc_sim_task_inverse_dynamics(wbc_sim* sim, const int32_t* stance_bodies /* host */, int nstance, const uint8_t* active,
                                  const float* stance_acc, const int32_t* task_bodies /* host */, int ntasks, const float* task_acc,
                                  const float* task_weight, const float* nudot_ref, const wbc_taskid_weights* weights /* host */,
                                  int flags, float* tau, float* nudot, float* lambda, float* workspace, void* stream);

/* wbc_sim_task_inverse_dynamics with torque limits and friction pyramids: the problem, arguments, conventions, launches 1-3 and the
 * workspace rules are that call's (the size comes from wbc_sim_task_inverse_dynamics_qp_workspace_floats); per env the minimisation is
 * further subject to
 *     |tau_j| <= tau_limit[j]                                            the 18 revolute joints, in the order of tau[:, 6:24]
 *     n_k . lambda_k >= fn_min                                           for every ACTIVE stance body k, lambda_k the force applied TO
 *     +-t1_k . lambda_k <= mu_k n_k . lambda_k                           the robot: a friction pyramid, and unilateral contact for
 *     +-t2_k . lambda_k <= mu_k n_k . lambda_k                           fn_min >= 0
 * tau_limit  device f32 [N, 18] or NULL (= wbc_task_cfg.torque_limits of those DoFs).
 * normal     device f32 [N, nstance, 3], normalised by the kernel, or NULL (= world z). mu: device f32 [N, nstance] or NULL (=
 *            limits.mu). TANGENTS: with a NULL normal t1 = world x, t2 = world y; otherwise t1 = normalise(n x e) with e = world x, or
 *            world y where |n_x| > 0.9, and t2 = n x t1. An inactive stance body has no rows; its mu and normal are never read.
 * limits     HOST struct: mu > 0 and finite; fn_min finite; max_iter 1..WBC_TASKQP_MAX_ITER, 0 = the default (100).
 * tau, nudot, lambda  as in the sibling: after the solve (nudot, lambda) are recomputed from tau_j by constrained forward dynamics.
 *            |tau_j| <= tau_limit[j] holds exactly in fp32, and a joint reported at a limit equals that limit bit for bit.
 * status     device i32 [N] or NULL: 0 optimal; 1 the iteration cap was reached; 2 the inequalities admit no point.
 * active_set device i64 [N] or NULL, for status 0: bit j: tau_j at +limit; bit 18 + j: tau_j at -limit; bit 36 + 5 k + {0: the normal
 *            row, 1: +t1, 2: -t1, 3: +t2, 4: -t2} of stance body k. iterations: device i32 [N] or NULL: the steps taken (a row
 *            added, a row dropped, or a dependent candidate set aside).
 * Status 1 or 2: tau_j is the unconstrained optimum clamped to the box (what a caller of the sibling is told to do), (nudot, lambda)
 * are recomputed from it and active_set is 0. Where no row is violated at the unconstrained optimum the outputs are the sibling's bit
 * for bit, status 0, active_set 0, iterations 0.
 * Method (wbc_taskqp_solve_kernel, the fourth launch, one env per 64-lane workgroup): with R, c of the sibling's reflected stack,
 * min 1/2 |R tau_j + c|^2 over the rows above (linear in tau_j through lambda = lambda_0 + G_lambda tau_j) by the dual active-set
 * method of Goldfarb and Idnani started from the unconstrained optimum; the iterate and the multipliers are rebuilt from the working
 * set after every accepted row. Every loop has a compile-time bound.
 * Non-finite or non-positive tau_limit or mu, or a zero normal, of an env: that env's outputs are unspecified, no other env is affected.
 * -1 with a message in wbc_last_error(), nothing written: everything the sibling refuses; a NULL limits; a limits field out of range; a
 * tau_limit / normal / mu / status / iterations that is not 4-byte aligned or an active_set that is not 8-byte aligned.
 * flags: 0 or WBC_SOLVE_ARMATURE. Out of scope: warm starts, second-order cones, a largest normal force, limits on accelerations. */
#define WBC_TASKQP_MAX_ITER 128
typedef struct { float mu, fn_min; int32_t max_iter; } wbc_taskqp_limits;
size_t wbc_sim_task_inverse_dynamics_qp_workspace_floats(int num_envs, int nstance, int ntasks);
int wbc_sim_task_inverse_dynamics_qp(wbc_sim* sim, const int32_t* stance_bodies /* host */, int nstance, const uint8_t* active,
                                     const float* stance_acc, const int32_t* task_bodies /* host */, int ntasks, const float* task_acc,
                                     const float* task_weight, const float* nudot_ref, const wbc_taskid_weights* weights /* host */,
                                     const wbc_taskqp_limits* limits /* host */, const float* tau_limit, const float* normal, const float* mu,
                                     int flags, float* tau, float* nudot, float* lambda, int32_t* status, int64_t* active_set,
                                     int32_t* iterations, float* workspace, void* stream);

/* Centre of mass, centroidal momentum, its rate, the centroidal momentum matrix and the locked centroidal inertia of the robot, in the
 * coordinates of wbc_sim_body_dynamics (nu = (v_root, omega_root, qd), world axes, 26 columns) with the inertias of the per-env
 * WBC_T_BODY_PARAMS, from the sim's current root / DoF state. One launch (wbc_centroidal_kernel).
 * nudot    device f32 [N, 26] or NULL (= zeros), in the convention of wbc_sim_inverse_dynamics: nudot[0:3] is the classical
 *          acceleration of the root origin.
 * com      device f32 [N, 9]: c - p_root, the centre of mass relative to the root origin (world axes; add WBC_T_ROOT_STATES[:, 0, 0:3]
 *          for its world position); v_com; a_com = J_com nudot + Jdot_com nu (NULL nudot: the bias part Jdot_com nu).
 * mom      device f32 [N, 12]: h_G = (m v_com ; k_G), k_G the angular momentum about the centre of mass in world axes; then
 *          hdot_G = A_G nudot + Adot_G nu (NULL nudot: Adot_G nu). hdot_G is kinematics times inertia and reads no gravity: along a
 *          motion of the robot it equals the net external wrench about the centre of mass, the weight included.
 * cmm      device f32 [N, 6, 26] = A_G, h_G = A_G nu: rows 0:3 linear, rows 3:6 angular about the centre of mass. The block
 *          [0:3, 0:3] is exactly m on the diagonal and exactly 0 off it, the block [3:6, 0:3] is exactly 0, and the locked fingers'
 *          columns 24, 25 are exactly 0. The centre-of-mass Jacobian is cmm[:, 0:3, :] / m.
 * inertia  device f32 [N, 7]: the total mass m, then the locked centroidal inertia I_G = A_G[3:6, 3:6] in world axes in the model's
 *          six-value order xx, yy, zz, xy, xz, yz.
 * Any output may be NULL and is then not written; not all four. Every pointer needs 4-byte alignment only. The fingers' entries of
 * nudot and of qd are ignored. The root POSITION is never read: every output is bit-identical under a translation of the robot, and
 * the angular rows hold no term that grows with |v_root| or |nudot[0:3]|. Nothing is allocated in the call, so it is safe under
 * stream capture. Error codes (-1 NULL sim, all outputs NULL or a misaligned pointer, nothing written; -3; -2) and stream handling as
 * wbc_sim_inverse_dynamics. */
int wbc_sim_centroidal(wbc_sim* sim, const float* nudot, float* com, float* mom, float* cmm, float* inertia, void* stream);

/* The Coriolis matrix C(q, nu) of M nudot + C nu + g = tau, dM/dt, the generalised momentum p = M nu and C^T nu, in the coordinates of
 * wbc_sim_body_dynamics / wbc_sim_inverse_dynamics (nu = (v_root, omega_root, qd), world axes, 26 columns; nudot the derivative of nu's
 * world components) with the inertias of the per-env WBC_T_BODY_PARAMS, from the sim's current root / DoF state. The sim's state is
 * read, never written. C is the factorisation of Echeandia and Wensing (Pinocchio's): with S_c the spatial motion vector of coordinate
 * c, v_k the spatial velocity and I_k the spatial inertia of moving body k,
 *     C = sum_k J_k^T (I_k Jdot_k + B_k J_k),    B_k = 1/2 [crf(v_k) I_k + crfbar(I_k v_k) - I_k crm(v_k)],
 * which satisfies C nu = h - g (wbc_sim_inverse_dynamics) and C + C^T = dM/dt EXACTLY; the generalised momentum then obeys
 *     d/dt p = tau + C^T nu - g + tau_ext.
 * cmat  device f32 [N, 26, 26] = C. The whole of columns 0:3 (the root's linear coordinates, the block [0:3, 0:3] included), the locked
 *       fingers' rows and columns 24, 25 and every pair of joints of which neither moves the other are exactly 0.
 * mdot  device f32 [N, 26, 26] = dM/dt along nu: bit-symmetric, and bit-equal to cmat + cmat^T of the same launch.
 * vec   device f32 [N, 2, 26]: p = M nu, then C^T nu; the fingers' entries exactly 0.
 * Any output may be NULL and is then not written; not all three. cmat and mdot need 16-byte alignment, vec 4-byte alignment. One launch:
 * wbc_coriolis_kernel where a matrix is asked for, wbc_momentum_kernel (which forms nothing 26 x 26) for vec alone; vec has the same bits
 * from either. The fingers' qd is ignored. The root POSITION is never read: every output is bit-identical under a translation of the
 * robot. Nothing is allocated and nothing synchronises: safe under stream capture. Error codes (-1 NULL sim, all outputs NULL or a
 * misaligned pointer, nothing written; -3; -2) and stream handling as wbc_sim_inverse_dynamics. */
int wbc_sim_coriolis(wbc_sim* sim, float* cmat, float* mdot, float* vec, void* stream);

/* One update of the generalised-momentum observer, the estimator of external joint torques (contact detection without force sensors):
 * along a motion d/dt p = tau + C^T nu - g + tau_ext, so with the caller-owned
 * state  device f32 [N, 2, 26]: the integral, then the residual r (the estimate of tau_ext, a first-order low-pass of it with the
 *        bandwidth `gain`),
 * evaluated at the sim's current state, the call performs
 *     with WBC_OBSERVER_RESET:  integral = p,                                        r = 0
 *     otherwise:                integral += dt (tau + C^T nu - g + r_old),           r = gain (p - integral).
 * tau    device f32 [N, 26] or NULL (= zeros), rows as wbc_sim_inverse_dynamics: 0:6 the KNOWN external wrench on the root (force, moment
 *        about the root origin, world axes), 6: the joint torques. What is not in tau shows up in r.
 * gain > 0 (1/s), dt > 0 (s), gain dt < 1: the explicit update must not overshoot. flags: 0 or WBC_OBSERVER_RESET.
 * The fingers' entries of state are exactly 0 after every call. g comes with all three gravity components.
 * Two launches on `stream`, no host synchronisation, nothing allocated: wbc_inverse_dynamics_kernel writes g(q) into the sim's [N, 26]
 * bias-force scratch (the one wbc_sim_forward_dynamics uses: one stream at a time per sim among the calls that use it), then
 * wbc_momentum_kernel forms p and C^T nu and updates state in its epilogue. The sim's state is read, never written.
 * -1 with a message in wbc_last_error() that names this entry point, nothing written: NULL sim or state; unknown flag bits; gain or dt not
 * finite or <= 0; gain dt >= 1; a tau or state that is not 4-byte aligned. -3 / -2 as wbc_sim_mass_solve. */
#define WBC_OBSERVER_RESET 1
int wbc_sim_momentum_observer(wbc_sim* sim, const float* tau, float gain, float dt, int flags, float* state, void* stream);

/* Self-collision proximity: the signed gaps of the robot's own collision pairs, their closest points and d gap / d q, from the sim's
 * current root / DoF state in one launch (wbc_proximity_kernel). The sim's state is read, never written.
 * THE PAIRS are those of the model the sim was created with, in a fixed order: first the lanes whose pr_kind is WBC_PR_LIMBS, in lane
 * order (44 in the shipped model), then the static pairs of cp_kind WBC_CP_BOX whose box rides on a robot body (3: the gripper, wrist and
 * elbow spheres against the trunk box); P = 47. Pairs against the free box actor are not listed: the box has no generalised coordinate.
 * wbc_sim_proximity_pair_count returns P (0 for a model built without self-collisions) or a negative error code;
 * wbc_sim_proximity_pairs writes (kind, a, b, 0) per pair into out (host int32 [P][4]) and returns P: kind WBC_PR_LIMBS with the limb ids
 * a, b; kind WBC_PR_STATIC with a = the sphere's compact index (cp_sph) and b = the box's rigid body (cp_rb2). Both run on the host alone (-1 for a NULL sim or out).
 * GEOMETRY, that of the step kernel's exact test: a limb is the union of its shaft capsule (limb_radius about the segment between its end
 * spheres' centres) and its end spheres (limb_cap0 / limb_cap1; 0: none). A limb pair's gap is the smallest over its feature pairs, in the
 * order shaft-shaft, A's end spheres against B's shaft, A's shaft against B's end spheres, end sphere against end sphere (of equal gaps the
 * earlier); for a feature pair with the core points c_a, c_b (the closest points of the two core segments or centres) gap = |c_a - c_b| -
 * r_a - r_b. For a sphere against a box c_b is the box's closest point to the centre c_a, r_b = 0 and r_a = cp_radius; with the centre
 * inside the box gap = -(depth to the nearest face) - r_a and the normal is that face's. pair_rest_offset and contact_margin are NOT
 * subtracted: this is geometry, not the contact law's activation distance. Segments shorter than 1e-5 m count as points; parallel shafts
 * (sin^2 of their angle <= 1e-7) take the first end of A as A's parameter, where gap and normal are unique and the core points are not.
 * gap      device f32 [N, P].
 * normal   device f32 [N, P, 3]: the unit vector n from c_b to c_a of the winning feature pair, world axes ((1, 0, 0) in base axes where
 *          the core points coincide).
 * witness  device f32 [N, P, 2, 3]: the surface points w_a = c_a - r_a n and w_b = c_b + r_b n, world axes, RELATIVE TO THE ROOT'S ORIGIN.
 * jac      device f32 [N, P, 26] = d gap / d q in the coordinates of wbc_sim_body_dynamics: d gap / dt = jac . nu. Entry c is n . (column c
 *          of the linear Jacobian of the point c_a riding on a's moving body minus that of c_b on b's), each lever taken from the joint's
 *          own origin. Columns 0:6 (a self-distance does not see the root), the columns of every joint that moves neither body or both,
 *          and the locked fingers' columns 24, 25 are exactly 0. A limb's moving body is limb_body, a sphere's cp_body, the trunk box's 0.
 * nearest  device int32 [N, k_nearest], 1 <= k_nearest <= 8: the indices of the env's k_nearest smallest gaps in ascending order of
 *          (gap, pair index), decided on the launch's own gap values (-1 beyond P). k_nearest is ignored where nearest is NULL.
 * Any output may be NULL and is then not written; not all five. What is written does not depend on which others are asked for. Every
 * pointer needs 4-byte alignment only. The root POSITION and every velocity are never read: every output is bit-identical under a
 * translation of the robot. Nothing is allocated and nothing synchronises: safe under stream capture. -1 with a message in
 * wbc_last_error() that names the entry point, nothing written: NULL sim; all outputs NULL; a misaligned pointer; k_nearest out of range;
 * a model with P = 0. -3 / -2 and stream handling as wbc_sim_coriolis. */
int wbc_sim_proximity_pair_count(const wbc_sim* sim);
int wbc_sim_proximity_pairs(const wbc_sim* sim, int32_t* out);
int wbc_sim_proximity(wbc_sim* sim, float* gap, float* normal, float* witness, float* jac, int32_t* nearest, int k_nearest, void* stream);

/* One update of the leg-odometry Kalman filter, the classical estimator of what no sensor on the robot measures: the base's linear velocity
 * and its position relative to the footholds, from the IMU and the leg kinematics (a stance foot does not move). One launch
 * (wbc_leg_odometry_kernel); the sim's state is read, never written. Per env the caller owns
 * x      device f32 [N, 18] = (p, v, p_1 .. p_4): position and velocity of the trunk's origin and the origins of the four feet (the rigid
 *        bodies feet_rb, in that order), world axes;
 * P      device f32 [N, 18, 18], its covariance. P is read as a symmetric matrix (its lower triangle is read) and written bit-symmetric.
 * INPUTS of one update over a step cfg->dt that ends now; each of quat, gyro and dof may be NULL, which means the sim's current state:
 * quat   device f32 [N, 4], xyzw: the trunk's orientation R (world <- trunk), normalised in the call. NULL: ROOT_STATES' quaternion.
 * gyro   device f32 [N, 3]: the angular velocity w_b in trunk axes. NULL: ROOT_STATES' world angular velocity rotated by R^T.
 * dof    device f32 [N, 20, 2]: (q, qd) in the layout of DOF_STATE. NULL: DOF_STATE.
 * accel  device f32 [N, 3] or NULL: the specific force in trunk axes over the interval this call advances across; a = R accel + g with
 *        wbc_task_cfg.gravity. NULL: a = 0, the constant-velocity model.
 * contact      device f32 [N, 4], required: c_i, clamped to [0, 1]; 1 a stance foot, 0 a swing foot.
 * foot_height  device f32 [N, 4] or NULL: the world height of the ground under each foot. NULL leaves the four height rows out (m = 24).
 * With r_i = R fk_i(q) and rdot_i = R (w_b x fk_i(q) + J_i(q) qd) from the leg kinematics and s_i = 1 + kappa (1 - c_i):
 *   predict   p <- p + v dt + a dt^2 / 2, v <- v + a dt, the feet unchanged; P- = A P A^T + Q with A = I + dt I_3 in the (p, v) block and
 *             Q = dt diag(sigma_p^2 I_3, sigma_v^2 I_3, sigma_f^2 s_i I_3 per foot);
 *   correct   twelve position rows (foot-major) -r_i - (p - p_i) of variance sigma_r^2 s_i, twelve velocity rows -rdot_i - v of variance
 *             sigma_rdot^2 s_i, four height rows foot_height_i - p_i,z of variance sigma_z^2 s_i; S = C P- C^T + R_m = L L^T,
 *             W = L^-1 C P-, y = L^-1 e: x+ = x- + W^T y, P+ = P- - W^T W, nis = |y|^2.
 * Where a pivot of S fails the env keeps the predicted (x-, P-), nis = 0 and status WBC_ESTIMATOR_STATUS_FAILED; finite inputs give finite outputs.
 * RESET: with WBC_ESTIMATOR_RESET in flags every env, with reset_mask (device int32 [N] or NULL) the envs whose entry is not 0:
 * p = p_init (device f32 [N, 3]; NULL: 0), v = 0, p_i = p + r_i, P = diag(p0_p I_3, p0_v I_3, p0_f I_12), nis = 0, status
 * WBC_ESTIMATOR_STATUS_RESET; such an env is neither predicted nor corrected in that call, and its x and P are not read.
 * OUTPUTS besides x and P, each may be NULL and is then not written; what is written does not depend on which are asked for:
 * vel_body  device f32 [N, 3] = R^T v, the estimate of BASE_LIN_VEL;   nis  device f32 [N];   status  device int32 [N].
 * Every pointer needs 4-byte alignment only. Nothing is allocated and nothing synchronises: safe under stream capture. -1 with a message
 * in wbc_last_error() that names the entry point, nothing written: NULL sim, cfg, contact, x or P; unknown flag bits; dt, a sigma or an
 * initial variance that is not finite and > 0; kappa not finite or < 0; a misaligned pointer. -3 / -2 and stream handling as
 * wbc_sim_coriolis. */
typedef struct {
  float dt;                                  /* s */
  float sigma_p, sigma_v, sigma_f;           /* process noise densities of p, v and a stance foot's origin */
  float sigma_r, sigma_rdot, sigma_z;        /* standard deviations of the position, velocity and height rows of a stance foot */
  float kappa;                               /* swing inflation: variances of foot i times 1 + kappa (1 - c_i) */
  float p0_p, p0_v, p0_f;                    /* the variances a reset starts from */
} wbc_estimator_cfg;
#define WBC_ESTIMATOR_RESET 1
#define WBC_ESTIMATOR_STATUS_OK 0
#define WBC_ESTIMATOR_STATUS_RESET 1
#define WBC_ESTIMATOR_STATUS_FAILED 2
int wbc_sim_leg_odometry(wbc_sim* sim, const wbc_estimator_cfg* cfg, const float* quat, const float* gyro, const float* dof, const float* accel,
                         const float* contact, const float* foot_height, const int32_t* reset_mask, const float* p_init, int flags,
                         float* x, float* P, float* vel_body, float* nis, int32_t* status, void* stream);

/* Convex model-predictive control of the foot forces on the single-rigid-body model (Di Carlo et al., IROS 2018), the layer that hands
 * base_acc to the whole-body controller: one QP per env, one launch (wbc_centroidal_mpc_kernel) with a fixed iteration count, so that it
 * takes the same time for every env and replays under graph capture. The sim's state is read, never written.
 * PROBLEM per env, world axes, H = cfg->horizon stages of cfg->dt:
 *   x = (theta, p, omega, v) in R^12: theta = log(R Rz(psi)^T) the rotation vector from the heading frame to the trunk (psi the yaw of R's
 *       x axis at the call), p and v the centre of mass and its velocity, omega the angular velocity;
 *   u_k = (f_1 .. f_4) in R^12, the forces on the four feet (feet_rb order), constant over stage k = 0 .. H-1;
 *   x_{k+1} = A x_k + B_k u_k + d: A = I + dt (theta <- omega, p <- v), d = (0, dt^2/2 g, 0, dt g), foot i's block of B_k with
 *       W = I_G^-1 [r_ki]x: rows theta, p, omega, v = dt^2/2 W, dt^2/(2m) 1, dt W, dt/m 1 where contact[k][i] != 0 and zero elsewhere
 *       (the exact zero-order hold of the time-varying linear model without the gyroscopic term); r_ki = foot_pos_ki - pbar_k, pbar_0 = p
 *       of x0, pbar_k = the position part of x_ref_k for k >= 1;
 *   cost  sum_{k=1..H} 1/2 (x_k - x_ref_k)^T diag(q) (x_k - x_ref_k) + sum_{k=0..H-1} 1/2 u_k^T diag(r, r, r, r) u_k;
 *   for every stance foot five rows lo <= C f <= hi: C = [[-1,0,mu],[1,0,mu],[0,-1,mu],[0,1,mu],[0,0,1]], lo = (0,0,0,0,fz_min),
 *       hi = (inf,inf,inf,inf,fz_max); a swing foot's force is exactly 0.
 * ALGORITHM (the kernel and tests/mpc_reference.py implement exactly this): ADMM on z = C u (20 rows per stage), scaled dual y.
 *   Factor once per call: Rt = diag(r ..) + rho C^T C (diagonal: (2, 2, 4 mu^2 + 1) per foot); P_H = Q; for k = H-1 .. 0:
 *       G_k = Rt + B_k^T P_{k+1} B_k = L L^T, K_k = G_k^-1 B_k^T P_{k+1} A and G_k^-1 itself by substitution on [B_k^T P_{k+1} A | 1],
 *       P_k = Q_k + A^T P_{k+1} (A - B_k K_k) symmetrised (Q_0 = 0), and P_{k+1} d is kept.
 *   Iterate cfg->iters times, no early exit:
 *     1. rt_k = -rho C^T (z_k - y_k);
 *     2. backward from p_H = -Q x_ref_H: s = p_{k+1} + P_{k+1} d, v = B_k^T s + rt_k, kappa_k = G_k^-1 v, p_k = -Q_k x_ref_k + A^T s - K_k^T v;
 *     3. forward: u_k = -K_k x_k - kappa_k, x_{k+1} = A x_k + B_k u_k + d;
 *     4. z_k <- clip(C u_k + y_k, lo, hi), y_k <- y_k + C u_k - z_k; the rows of swing feet are held at 0.
 *   After the last iteration res = (max |C u - z| over stance rows, rho max |C^T (z - z_prev)|); forces = stage 0's u with f_z clipped to
 *   [fz_min, fz_max] and then f_x, f_y to +-mu f_z (always feasible, u_0 where the residual is 0; a swing foot's is 0).
 * INPUTS (device; every float pointer f32, 4-byte alignment):
 *   contact  u8 [N,H,4], required;   x_ref  [N,H,12], stages 1 .. H, required;
 *   x0       [N,12] or NULL: p = root position + wbc_sim_centroidal's offset, v = v_com, omega = the root's world angular velocity, theta as above;
 *   mass [N], inertia [N,3,3] (world axes, about the centre of mass) or NULL: what wbc_sim_centroidal produces. When x0, mass or inertia
 *       is NULL the entry point launches wbc_centroidal_kernel into workspace (wbc_sim_centroidal_mpc_workspace_floats(N) floats) first;
 *   foot_pos [N,S,4,3], S = foot_pos_stages in {1, H} (1: one set for every stage), or NULL: the current origins of the four feet;
 *   warm     [N,2,H,20] or NULL: z then y, read and written. WBC_MPC_COLD starts from zeros (implied by NULL), WBC_MPC_SHIFT shifts both
 *       left by one stage and repeats the last before starting.
 * OUTPUTS, each may be NULL; what is written never depends on which are asked for: forces [N,4,3], u [N,H,12], x_pred [N,H,12]
 *   (x_1 .. x_H), base_acc [N,6] = (sum forces / m + g ; I_G^-1 sum r_0i x forces_i), linear then angular, world axes (what
 *   wbc_sim_task_inverse_dynamics_qp's base task takes), res [N,2], status int32 [N]: WBC_MPC_STATUS_OK both residuals <= cfg->tol,
 *   WBC_MPC_STATUS_ITERATIONS the iterate after cfg->iters iterations is above it (the outputs are the iterate's), WBC_MPC_STATUS_FAILED an input
 *   of that env is not finite, m or det I_G is not positive or a pivot failed: every float output of the env and its warm entries are 0.
 * Nothing is allocated, nothing synchronises. -1 with a message in wbc_last_error() that names the entry point, nothing written, checked
 * BEFORE the sim: NULL cfg, contact or x_ref; unknown flag bits; horizon outside 1..WBC_MPC_MAX_HORIZON or iters outside 1..1000; dt, rho, mu,
 * an r entry or tol not finite and > 0; a q entry not finite or < 0; fz_min not finite or < 0; fz_max not finite or < fz_min;
 * foot_pos_stages other than 1 or H; a misaligned pointer; NULL workspace when x0, mass or inertia is NULL. Then NULL sim; -3 / -2 and
 * stream handling as wbc_sim_coriolis. Not covered: terrain normals other than world z, per-env mu, the gyroscopic term, foothold
 * optimisation. */
#define WBC_MPC_MAX_HORIZON 16
typedef struct {
  int32_t horizon;                           /* H, 1..16 */
  int32_t iters;                             /* 1..1000 */
  float dt, rho, mu, fz_min, fz_max;
  float q[12];                               /* >= 0 */
  float r[3];                                /* > 0 */
  float tol;                                 /* > 0: status only */
} wbc_mpc_cfg;
#define WBC_MPC_COLD 1
#define WBC_MPC_SHIFT 2
#define WBC_MPC_STATUS_OK 0
#define WBC_MPC_STATUS_ITERATIONS 1
#define WBC_MPC_STATUS_FAILED 2
int wbc_sim_centroidal_mpc(wbc_sim* sim, const wbc_mpc_cfg* cfg, const float* x0, const float* mass, const float* inertia,
                           const float* foot_pos, int foot_pos_stages, const uint8_t* contact, const float* x_ref, float* warm, int flags,
                           float* forces, float* u, float* x_pred, float* base_acc, float* res, int32_t* status, float* workspace,
                           void* stream);
size_t wbc_sim_centroidal_mpc_workspace_floats(int num_envs);

/* One control step of the gait layer that ties the estimator, the MPC and the whole-body controller into a loop: a gait clock that decides
 * which feet stand, Raibert footholds moved to safe terrain by a search over the heightfield, and minimum-jerk swing-foot references. One
 * launch (wbc_footstep_plan_kernel); the sim's state is read, never written. Per env the caller owns
 * state  device f32 [N, WBC_FOOTSTEP_NS = 32], read and written: [0] the phase in [0, 1); [1..3] reserved, written as 0; then per foot
 *        (feet_rb order FL, FR, RL, RR) seven floats at 4 + 7 i: the lift-off position (3), the target foothold (3), a swing flag (0 or 1).
 * INPUTS (device f32 unless said otherwise; each may be NULL):
 * base_pos, base_vel  [N, 3]: position b and velocity v of the trunk's origin, world axes. NULL: ROOT_STATES' (a BaseStateEstimator's
 *        position / velocity fit here).   quat [N, 4] xyzw, normalised in the call: R (world <- trunk). NULL: ROOT_STATES'.
 * dof    [N, 20, 2] in the layout of DOF_STATE. NULL: DOF_STATE.   vel_cmd [N, 2]: the commanded planar velocity in the heading frame,
 *        NULL: 0.   yaw_rate [N]: w_z, NULL: 0.   reset_mask int32 [N].   phase_init [N], NULL: 0.
 * The foot origins and their velocities come from the leg kinematics of wbc_sim_leg_odometry: r_i = R fk_i(q), rdot_i = R (w_b x fk_i +
 * J_i qd) with w_b = R^T (ROOT_STATES' world angular velocity): p_i = b + r_i, pd_i = v + rdot_i.
 * PER ENV, in this order (T_st = duty period, T_sw = (1 - duty) period, frac(x) = x - floor(x)):
 * 1 RESET (WBC_FOOTSTEP_RESET in flags: every env; otherwise the envs whose reset_mask entry is not 0; the env's state is then not read):
 *   phase = phase_init, every swing flag 0, lift-off = target = p_i; info bit WBC_FOOTSTEP_INFO_RESET.
 * 2 CLOCK  phi_i = frac(phase + offset_i). Foot i stands iff duty >= 1 or phi_i < duty; otherwise it swings with the swing fraction
 *   s_i = (phi_i - duty) / (1 - duty). A foot whose flag is 0 and that swings now lifts off: lift-off <- p_i, flag <- 1 (info bit
 *   WBC_FOOTSTEP_INFO_LIFT << i). A foot whose flag is 1 and that stands now touches down: flag <- 0, target <- p_i.
 * 3 NOMINAL FOOTHOLD of the touchdown t seconds from now: t = (1 - s_i) T_sw for a swinging foot, t = (duty - phi_i) period + T_sw for a
 *   standing one (duty >= 1: t = 0). With (c, s) = (R_00, R_10) / |(R_00, R_10)| the heading psi of R's x axis ((1, 0) where that axis is
 *   vertical), Rz(psi_t) = Rz(psi) Rz(w_z t),
 *   v_c = Rz(psi) vel_cmd:   hip = b_xy + v_c t + Rz(psi_t) stance_offset_i,
 *   add = (T_st / 2) v_xy + k_v (v_xy - v_c) + (1/2) sqrt(com_height / |g|) (v_y w_z, -v_x w_z)     [Raibert; the last term (v x (0, 0, w_z))_xy]
 *   scaled down to length max_reach where it is longer; nom = hip + add. g is wbc_task_cfg.gravity; with |g| = 0 the last term is left out.
 * 4 TERRAIN SEARCH, only for a foot that swings now with s_i < latch (a swinging foot past the latch keeps the stored target): the
 *   candidates c_ab = nom + (a, b) search_step, a, b in [-R, R], index (a + R)(2R + 1) + (b + R). h(x, y) and n(x, y) are the terrain's
 *   surface height and unit normal exactly as the step kernel's contacts see them (terrain_query: the cell's triangle with u >= v or u < v,
 *   indices clamped to the grid, the plane z = ground_z without a heightfield). Per candidate rough = the largest of |h(c +- probe_radius
 *   e_x) - h(c)| and |h(c +- probe_radius e_y) - h(c)|, slope = 1 - n_z(c); it is rejected where rough > rough_max or n_z < nz_min;
 *   cost = w_dist |c - nom|^2 + w_rough rough^2 + w_slope slope. target = the accepted candidate of least cost (the lowest index on a
 *   tie) with z = h(c); all rejected: target = (nom, h(nom)) and info bit WBC_FOOTSTEP_INFO_NO_SAFE << i.
 * 5 SWING REFERENCE of a swinging foot, b(s) = s^3 (10 - 15 s + 6 s^2), sdot = 1 / T_sw: xy = lift + (target - lift) b(s); with the apex
 *   z_a = max(lift_z, target_z) + swing_height, z = lift_z + (z_a - lift_z) b(2 s) for s < 1/2 and z_a + (target_z - z_a) b(2 s - 1) otherwise;
 *   velocity and acceleration are the analytic time derivatives (b' sdot, b'' sdot^2; in z with 2 sdot).     [the MIT Cheetah 3 swing shape]
 * OUTPUTS, each may be NULL and is then not written; what is written never depends on which are asked for; they belong to the phase BEFORE step 6:
 * stance u8 [N, 4], contact f32 [N, 4] (1.0 / 0.0);   swing_ref [N, 4, 9] = (pos, vel, acc), a standing foot (p_i, 0, 0);
 * swing_acc [N, 4, 3] = acc + kp (pos - p_i) + kd (vel - pd_i), 0 for a standing foot (what the whole-body calls take as the feet's task);
 * foothold [N, 4, 3]: a swinging foot's target; a standing foot's (nom, h(nom)) of step 3, one query and no search;
 * schedule u8 [N, H, 4]: with x_ik = (phase + (k + 1/2) (mpc_dt / period)) + offset_i foot i stands in stage k iff duty >= 1 or
 *   frac(x_ik) < duty (the fp32 statements of the Python trot_schedule, which trot offsets reproduce);
 * foot_pos [N, H, 4, 3] (the MPC's foot_pos with foot_pos_stages = H): with m_ik = floor(x_ik) - floor(phase + offset_i) the number of
 *   lift-offs between now and stage k, a stance stage with m = 0 (or duty >= 1) gets p_i, one with m >= 1 gets foothold_i + (m - 1) period
 *   (v_c, 0); a swing stage gets the value of the foot's next stance stage in the horizon, failing that of its last one, failing that foothold_i;
 * info int32 [N]: the bits below.
 * 6 ADVANCE  phase <- frac(phase + dt / period) unless WBC_FOOTSTEP_HOLD is set.
 * An env with a non-finite input (b, v, quat, the root's angular velocity, a leg joint's q or qd, vel_cmd, yaw_rate, the state it reads or
 * its phase_init) writes zeros to every output but info = WBC_FOOTSTEP_INFO_FAILED and leaves its state as it was.
 * Every pointer needs 4-byte alignment only (the u8 outputs none). Nothing is allocated and nothing synchronises: safe under stream capture.
 * -1 with a message in wbc_last_error() that names the entry point, nothing written, checked BEFORE the sim: NULL cfg or state; unknown
 * flag bits; dt, period, mpc_dt (when horizon > 0), search_step or probe_radius not finite and > 0; duty not finite or <= 0; an offset
 * outside [0, 1); horizon outside 0..WBC_MPC_MAX_HORIZON; search_radius outside 0..WBC_FOOTSTEP_MAX_RADIUS; a stance_offset entry not
 * finite; k_v, com_height, max_reach, swing_height, kp, kd, w_dist, w_rough, w_slope, rough_max or nz_min not finite or < 0; latch outside
 * [0, 1]; a misaligned pointer. Then NULL sim; -3 / -2 and stream handling as wbc_sim_coriolis. Not covered: early / late contact
 * adaptation, a duty per foot, footholds searched for standing feet, collision of the swing path with the terrain. */
#define WBC_FOOTSTEP_NS 32          /* floats of state per env */
#define WBC_FOOTSTEP_MAX_RADIUS 3   /* (2*3+1)^2 = 49 candidates <= 64 lanes */
typedef struct {
  float dt;                 /* control step, s */
  float period, duty;       /* gait cycle s; stance fraction; duty >= 1: every foot always stands */
  float offset[4];          /* per-foot phase offset in [0,1), feet_rb order FL,FR,RL,RR; trot = (0, .5, .5, 0) */
  int32_t horizon;          /* H of the MPC outputs, 0..WBC_MPC_MAX_HORIZON (0: no per-stage outputs) */
  float mpc_dt;             /* stage length of those outputs */
  float stance_offset[4][2];/* nominal foot xy relative to the trunk origin, heading frame */
  float k_v, com_height, max_reach;   /* Raibert feedback gain; h of the centrifugal term; clamp on |nominal - hip| */
  float swing_height, latch;          /* apex clearance; swing fraction after which the target is frozen */
  float kp, kd;                       /* swing PD on the reference */
  int32_t search_radius;    /* R in 0..3: (2R+1)^2 candidates; 0: the nominal alone */
  float search_step, probe_radius;
  float w_dist, w_rough, w_slope, rough_max, nz_min;
} wbc_footstep_cfg;
#define WBC_FOOTSTEP_RESET 1
#define WBC_FOOTSTEP_HOLD  2        /* do not advance the clock */
#define WBC_FOOTSTEP_INFO_RESET 1
#define WBC_FOOTSTEP_INFO_FAILED 2
#define WBC_FOOTSTEP_INFO_NO_SAFE 16   /* << foot */
#define WBC_FOOTSTEP_INFO_LIFT 256     /* << foot: the foot lifted off in this call */
int wbc_sim_footstep_plan(wbc_sim* sim, const wbc_footstep_cfg* cfg, const float* base_pos, const float* base_vel, const float* quat,
                          const float* dof, const float* vel_cmd, const float* yaw_rate, const int32_t* reset_mask,
                          const float* phase_init, int flags, float* state,
                          uint8_t* stance, float* contact, uint8_t* schedule, float* foot_pos, float* foothold,
                          float* swing_ref, float* swing_acc, int32_t* info, void* stream);

/* One control step of the probabilistic contact detector (Bledt, Wensing, Ingersoll, Kim, "Contact Model Fusion for Event-Based Locomotion
 * in Unstructured Terrains", ICRA 2018): which feet are on the ground, from proprioception alone. Per foot a force term (from the
 * momentum observer's external joint torques or from a measured foot force), a height term and the gait clock's prior are fused into a
 * contact probability, low-passed, and turned into a flag with hysteresis and a dwell time, and into touchdown / lift-off / early / late
 * events. One launch (wbc_contact_detect_kernel); the sim's state is read, never written. Per env the caller owns
 * state  device f32 [N, WBC_CONTACT_NS = 16], read and written: four floats per foot (feet_rb order FL, FR, RL, RR) at 4 i: the filtered
 *        probability p_i, the flag c_i (0.0 or 1.0; read as c_i != 0), the seconds t_i since the flag last switched, a reserved 0 (written
 *        as 0, never read).
 * INPUTS (device f32 unless said otherwise; each may be NULL):
 * quat [N, 4] xyzw, normalised in the call: R (world <- trunk). NULL: ROOT_STATES'.   dof [N, 20, 2] in the layout of DOF_STATE (the
 *        velocities are not read). NULL: DOF_STATE.   base_pos [N, 3]: the trunk origin b, world axes. NULL: ROOT_STATES' (a
 *        BaseStateEstimator's position fits here). It is read whether or not `ground` is given.
 * tau_ext with tau_ext_stride (floats between envs, >= 26): the estimate of the external generalised forces in the 26 coordinates of
 *        wbc_sim_body_dynamics; row 6 + d belongs to DoF d. The stride lets the residual plane of wbc_sim_momentum_observer's [N, 2, 26]
 *        state be passed as it stands (state + 26, stride 52). Rows 0:6 are never read, nor the rows of joints that are in no leg.
 * foot_force [N, 4, 3], world axes: a measured foot force, which replaces the estimate. tau_ext and foot_force together are refused;
 *        with neither the force term is left out.
 * normal [N, 4, 3]: the ground's normal under each foot, normalised in the call. NULL: world z.
 * ground [N, 4]: the world height of a foot ORIGIN at rest on the ground under it (the convention of foot_height in
 *        wbc_sim_leg_odometry). NULL leaves the height term out.
 * phase [N] with phase_stride (floats between envs, >= 1): the gait clock; element 0 of wbc_sim_footstep_plan's state fits (stride
 *        WBC_FOOTSTEP_NS). NULL leaves the gait prior and step 7's EARLY / LATE out.
 * reset_mask int32 [N].   p_init [N, 4], NULL: 1.
 * At least one of {tau_ext or foot_force, ground, phase} must be given.
 * PER ENV AND FOOT i, in this order (frac(x) = x - floor(x); Phi(x) = (1/2) (1 + erf(x / sqrt 2))):
 * 1 RESET (WBC_CONTACT_RESET in flags: every env; otherwise the envs whose reset_mask entry is not 0; the env's state is then not read):
 *   p = p_init_i, c = 1 if p >= 1/2 else 0, t = t_dwell; info bit WBC_CONTACT_INFO_RESET. The env then goes through steps 2 .. 7 of this
 *   very call with that state.
 * 2 KINEMATICS  the leg walk of wbc_sim_leg_odometry from the trunk to the foot: fk_i(q) in trunk axes, the foot origin P_i = b + R fk_i,
 *   and the 3 x 3 leg Jacobian J_i in world axes: column k = R (a_k x (fk_i - o_k)), a_k the axis and o_k the origin of the leg's k-th
 *   actuated joint (k = 0, 1, 2 from the trunk down), both in trunk axes. These are the columns of the whole-body Jacobian's linear rows
 *   for that foot and those DoFs.
 * 3 FORCE  with tau_i = the three rows of tau_ext that belong to the leg's joints and delta = damping,
 *   f_i = J_i (J_i^T J_i + delta^2 I)^-1 tau_i, which is J_i^-T tau_i where J_i is regular and delta = 0, and stays bounded (by
 *   |tau_i| / (2 delta)) at a straight knee. A = J_i^T J_i + delta^2 I = L L^T is factorised row by row (l00 = sqrt(a00), l10 = a10 / l00,
 *   d1 = a11 - l10^2, l11 = sqrt(d1), l20 = a20 / l00, l21 = (a21 - l20 l10) / l11, d2 = a22 - l20^2 - l21^2, l22 = sqrt(d2)), L z = tau_i
 *   forwards, L^T y = z backwards, f_i = (J_0 y_0 + J_1 y_1) + J_2 y_2 over the columns. Where a pivot (a00, d1, d2) is not a positive
 *   finite number, or f_i comes out not finite, f_i = 0 and info bit WBC_CONTACT_INFO_FORCE_SINGULAR << i. With foot_force, f_i is that
 *   input. n_i = normal_i / |normal_i| (NULL: (0, 0, 1)), f_n = f_i . n_i.
 * 4 TERMS
 *   height  P_z = Phi((mu_z - (P_i,z - ground_i)) / sigma_z);
 *   force   P_f = Phi((f_n - mu_f) / sigma_f);
 *   prior   phi_i = frac(phase + offset_i). Foot i is scheduled to stand iff duty >= 1 or phi_i < duty (wbc_sim_footstep_plan's rule).
 *           With k = sigma_phase sqrt 2 and G(s) = (1/2) [erf(s / k) + erf((1 - s) / k)]:
 *           scheduled stance, s = phi_i / duty (the stance fraction):                 P_phi = G(s);
 *           scheduled swing,  s = (phi_i - duty) / (1 - duty) (the swing fraction):   P_phi = 1 - G(s).
 * 5 FUSION  the one-step Kalman fusion of the paper with A = 0, an inverse-variance mean over the terms present, summed in the order
 *   prior, height, force:  P = (sum_k P_k / var_k) / (sum_k 1 / var_k);  then  p <- p + alpha (P - p).
 * 6 FLAG  t <- t + dt. If c = 0, p >= p_on and t >= t_dwell: c <- 1, t <- 0, info bit WBC_CONTACT_INFO_TOUCHDOWN << i. Else if c = 1,
 *   p <= p_off and t >= t_dwell: c <- 0, t <- 0, info bit WBC_CONTACT_INFO_LIFTOFF << i.
 * 7 EVENTS (with phase only), on the c of step 6: WBC_CONTACT_INFO_EARLY << i while the foot is scheduled to swing with s >= early_min
 *   and c = 1; WBC_CONTACT_INFO_LATE << i while it is scheduled to stand with s >= late_min and c = 0.
 * OUTPUTS, each may be NULL and is then not written; what is written never depends on which are asked for:
 * prob f32 [N, 4] = p (what wbc_sim_leg_odometry takes as contact);   contact u8 [N, 4] = c;
 * stance u8 [N, 4]: what the whole-body calls take: (scheduled stance or EARLY) and not LATE; without phase it equals c;
 * force f32 [N, 4, 3] = f_i (the input where foot_force was given, 0 without a force input);
 * terms f32 [N, 4, 4] = (P_phi, P_z, P_f, P), 0 where a term is absent;   info int32 [N]: the bits below.
 * An env with a non-finite input (quat, b, a leg joint's q, the rows of tau_ext it reads, foot_force, normal (or a zero normal), ground,
 * phase, the p, c, t of the state it reads or its p_init) writes zeros to every output but info = WBC_CONTACT_INFO_FAILED and leaves its
 * state as it was.
 * Every pointer needs 4-byte alignment only (the u8 outputs none). Nothing is allocated and nothing synchronises: safe under stream capture.
 * -1 with a message in wbc_last_error() that names the entry point, nothing written, checked BEFORE the sim: NULL cfg or state; unknown
 * flag bits; dt, duty, sigma_phase, sigma_z, sigma_f, var_phase, var_z or var_f not finite and > 0; an offset outside [0, 1); mu_z or mu_f
 * not finite; alpha outside (0, 1]; p_on or p_off not finite, or p_on <= p_off; t_dwell or damping not finite or < 0; early_min or
 * late_min outside [0, 1]; no measurement source; both force inputs; tau_ext_stride < 26 or phase_stride < 1 where the pointer is given; a
 * misaligned pointer. Then NULL sim; -3 (also: a foot whose leg does not have exactly three joints) / -2 and stream handling as
 * wbc_sim_coriolis. Not covered: feeding the events back into the planner's clock, contacts on links other
 * than the feet. `ground` and `normal` can be estimated rather than given: wbc_sim_ground_estimate below writes both in this layout. */
#define WBC_CONTACT_NS 16           /* floats of state per env */
typedef struct {
  float dt;                         /* control step, s */
  float duty;                       /* the planner's stance fraction; duty >= 1: every foot is always scheduled to stand */
  float offset[4];                  /* the planner's per-foot phase offsets in [0, 1) */
  float sigma_phase;                /* width of the gait prior, in units of the stance / swing fraction */
  float mu_z, sigma_z;              /* height term: mean and width of the foot origin's height above `ground`, m */
  float mu_f, sigma_f;              /* force term: mean and width of the normal force, N */
  float var_phase, var_z, var_f;    /* fusion variances */
  float alpha;                      /* low-pass weight of the filtered probability, (0, 1] */
  float p_on, p_off;                /* hysteresis thresholds, p_on > p_off */
  float t_dwell;                    /* minimum seconds between flag switches, >= 0 */
  float early_min, late_min;        /* swing / stance fractions from which EARLY / LATE are judged, [0, 1] */
  float damping;                    /* delta of the damped force solve, >= 0 */
} wbc_contact_cfg;
#define WBC_CONTACT_RESET 1
#define WBC_CONTACT_INFO_RESET 1
#define WBC_CONTACT_INFO_FAILED 2
#define WBC_CONTACT_INFO_TOUCHDOWN 16            /* << foot */
#define WBC_CONTACT_INFO_LIFTOFF 256             /* << foot */
#define WBC_CONTACT_INFO_EARLY 4096              /* << foot */
#define WBC_CONTACT_INFO_LATE 65536              /* << foot */
#define WBC_CONTACT_INFO_FORCE_SINGULAR 1048576  /* << foot */
int wbc_sim_contact_detect(wbc_sim* sim, const wbc_contact_cfg* cfg, const float* quat, const float* dof, const float* base_pos,
                           const float* tau_ext, int tau_ext_stride, const float* foot_force, const float* normal, const float* ground,
                           const float* phase, int phase_stride, const int32_t* reset_mask, const float* p_init, int flags, float* state,
                           float* prob, uint8_t* contact, uint8_t* stance, float* force, float* terms, int32_t* info, void* stream);

/* One control step of the leg controller that turns the MPC's foot forces and the planner's swing references into joint torques, the
 * layer that Di Carlo et al. ("Dynamic Locomotion in the MIT Cheetah 3 Through Convex Model-Predictive Control", IROS 2018) and Bledt et
 * al. ("MIT Cheetah 3: Design and Control of a Robust, Dynamic Quadruped Robot", IROS 2018) run below their force planner: a stance leg
 * maps its planned force through the leg Jacobian (tau = -J^T f), a swing leg runs a Cartesian impedance on its reference with the
 * feed-forward J^T Lambda (a_ref - Jdot qd) + C qd + g, the arm holds a posture by a joint PD. One launch (wbc_leg_control_kernel); the
 * sim's state is read, never written; the call keeps no state of its own.
 * INPUTS (device f32; each may be NULL):
 * quat [N, 4] xyzw, normalised in the call: R (world <- trunk).   dof [N, 20, 2] in the layout of DOF_STATE.   base_pos, base_vel [N, 3]:
 *        position b and velocity v of the trunk's origin.   ang_vel [N, 3]: the trunk's angular velocity. All in world axes; NULL:
 *        ROOT_STATES' / DOF_STATE's, as in wbc_sim_footstep_plan (a BaseStateEstimator's position and velocity fit base_pos / base_vel).
 * forces [N, 4, 3]: the force ON each foot, world axes, as wbc_sim_centroidal_mpc writes it (feet_rb order FL, FR, RL, RR). NULL: 0.
 * swing_ref [N, 4, 9] = (pos, vel, acc) per foot, as wbc_sim_footstep_plan writes it. NULL: no swing term (F_i = 0 in step 4); acc is
 *        read only where mass_matrix is given.
 * stance [N, 4]: the stance weight of each foot, clamped to [0, 1] in the call (wbc_sim_footstep_plan's contact and
 *        wbc_sim_contact_detect's prob fit). NULL: 1.
 * tau_bias with tau_bias_stride (floats between envs, >= 26): row 6 + d is added to DoF d's torque; the tau of wbc_sim_inverse_dynamics
 *        fits (h with nudot NULL, or its grav output g). NULL: 0. Rows 0:6 and the fingers' rows are never read.
 * mass_matrix with mass_matrix_stride (>= 676): the [N, 26, 26] tensor of wbc_sim_body_dynamics as it stands; of each env only the
 *        3 x 3 block M_i (rows and columns 6 + the leg's own three DoFs) of every leg is read. NULL: no acceleration feed-forward (step 6
 *        is left out). mass_matrix without swing_ref is refused.
 * acc_bias with acc_bias_stride (>= 162): the [N, 27, 6] tensor of wbc_sim_body_accelerations(nudot = NULL) as it stands, Jdot nu of
 *        every rigid-body origin; only rows 0:3 of rigid body feet_rb[i] are read, and only where mass_matrix is given. NULL: 0.
 * arm_q_des [N, 6]: the arm's joint targets, the arm's DoFs in DoF order. NULL: cfg.arm_q_default.
 * tau_limit [N, 18]: in the layout wbc_sim_task_inverse_dynamics_qp takes (the 18 revolute joints in DoF order), >= 0. NULL: no clamp.
 * Entries that are never read may hold NaN.
 * PER ENV AND FOOT i (feet_rb order), in this order; d_0, d_1, d_2 are the DoFs of the leg's joints from the trunk down:
 * 1 KINEMATICS  the leg walk of wbc_sim_contact_detect step 2: fk_i(q) in trunk axes, the columns c_k = a_k x (fk_i - o_k) of the leg
 *   Jacobian in trunk axes (a_k the axis, o_k the origin of the leg's k-th joint), p_i = b + R fk_i and J_i = R [c_0 c_1 c_2] in world
 *   axes; the foot's velocity in the planner's convention, pd_i = v + R (w_b x fk_i + ((c_0 qd_0 + c_1 qd_1) + c_2 qd_2)) with
 *   w_b = R^T ang_vel.
 * 2 WEIGHT  w_i = min(max(stance_i, 0), 1).
 * 3 STANCE FORCE  f_i = forces_i. With WBC_LEGCTL_CLIP in flags the output rule of wbc_sim_centroidal_mpc applies: f_z <- min(max(f_z,
 *   fz_min), fz_max), then f_x <- min(max(f_x, -mu f_z), mu f_z) and the same for f_y; info bit WBC_LEGCTL_INFO_FORCE_CLIPPED << i where
 *   w_i > 0 and a component changed.
 * 4 SWING FORCE  F_i = kp o (pos_ref - p_i) + kd o (vel_ref - pd_i), o the product per world axis (kp[3], kd[3]); 0 without swing_ref.
 * 5 FEEDBACK TORQUE  G_i = (1 - w_i) F_i - w_i f_i, the force the leg is to push the foot with; tau_fb,k = J_i[:, k] . G_i.
 * 6 FEED-FORWARD (with mass_matrix only)  a = acc_ref - acc_bias_i (the foot's commanded acceleration less Jdot nu), delta = damping,
 *   A = J_i^T J_i + delta^2 I = L L^T factorised row by row as in wbc_sim_contact_detect step 3 (l00 = sqrt(a00), l10 = a10 / l00,
 *   d1 = a11 - l10^2, l11 = sqrt(d1), l20 = a20 / l00, l21 = (a21 - l20 l10) / l11, d2 = a22 - l20^2 - l21^2, l22 = sqrt(d2)), L z = J_i^T a
 *   forwards, L^T qdd = z backwards: qdd = A^-1 J_i^T a, the joint accelerations that give the foot the acceleration a while the trunk's
 *   own acceleration is taken as ZERO; |qdd| <= |a| / (2 delta) at a straight knee. tau_ff,k = (1 - w_i) ((M_i[k,0] qdd_0 + M_i[k,1] qdd_1)
 *   + M_i[k,2] qdd_2). For a regular J_i and delta = 0 this is Cheetah 3's J_i^T Lambda_i (a_ref - Jdot qd), Lambda_i = (J_i M_i^-1
 *   J_i^T)^-1. Where a pivot (a00, d1, d2) is not a positive finite number or qdd is not finite: tau_ff = 0 and info bit
 *   WBC_LEGCTL_INFO_FF_SINGULAR << i.
 * 7 LEG JOINTS  tau_dk = ((tau_fb,k + tau_ff,k) + tau_bias[6 + d_k]) - (w_i kd_stance) qd_dk.
 * 8 ARM, once per env, for the six DoFs d that are in no leg and are not the locked fingers, j = 0 .. 5 in DoF order:
 *   tau_d = (tau_bias[6 + d] + kp_arm[j] (q_des,j - q_d)) - kd_arm[j] qd_d.
 * 9 LIMIT (with tau_limit only)  every torque tau <- min(max(tau, -limit), limit); info bit WBC_LEGCTL_INFO_SATURATED << i for leg i and
 *   << 4 for the arm where one changed. The fingers' entries of tau are exactly 0.
 * OUTPUTS, each may be NULL and is then not written (not all four); what is written never depends on which are asked for:
 * tau f32 [N, 20], what wbc_sim_set_dof_forces takes;   leg_force f32 [N, 4, 3] = G_i;   foot f32 [N, 4, 6] = (p_i, pd_i);
 * info int32 [N]: the bits below.
 * An env with a non-finite input that it reads (a tau_limit entry that is negative counts as one), or with an output that comes out
 * not finite, writes zeros to every output but info = WBC_LEGCTL_INFO_FAILED.
 * Every pointer needs 4-byte alignment only. Nothing is allocated and nothing synchronises: safe under stream capture.
 * -1 with a message in wbc_last_error() that names the entry point, nothing written, checked BEFORE the sim: NULL cfg; unknown flag bits;
 * a kp, kd, kd_stance, kp_arm, kd_arm or damping entry not finite or < 0; fz_min not finite or < 0, fz_max not finite or < fz_min, mu not
 * finite or < 0; an arm_q_default entry not finite; a stride below its minimum where its pointer is given; a misaligned pointer;
 * mass_matrix without swing_ref; every output NULL. Then NULL sim; -3 (also: a foot whose leg does not have exactly three joints, or an
 * arm DoF count other than six) / -2 and stream handling as wbc_sim_coriolis. Not covered: normals other than world z in the clip, the
 * base's acceleration in the feed-forward, joint-space position targets for the legs, a task-space arm. */
typedef struct {
  float kp[3], kd[3];               /* swing impedance per world axis, N/m and N s/m, >= 0 */
  float kd_stance;                  /* joint damping of a stance leg, N m s/rad, >= 0 */
  float damping;                    /* delta of the damped feed-forward solve, >= 0 */
  float fz_min, fz_max, mu;         /* the clip of WBC_LEGCTL_CLIP: 0 <= fz_min <= fz_max, mu >= 0 */
  float kp_arm[6], kd_arm[6];       /* the arm's joint PD, the arm's DoFs in DoF order, >= 0 */
  float arm_q_default[6];           /* the arm's targets where arm_q_des is NULL */
} wbc_leg_control_cfg;
#define WBC_LEGCTL_CLIP 1
#define WBC_LEGCTL_INFO_FAILED 2
#define WBC_LEGCTL_INFO_FORCE_CLIPPED 16         /* << foot */
#define WBC_LEGCTL_INFO_FF_SINGULAR 256          /* << foot */
#define WBC_LEGCTL_INFO_SATURATED 4096           /* << foot; << 4: the arm */
int wbc_sim_leg_control(wbc_sim* sim, const wbc_leg_control_cfg* cfg, const float* quat, const float* dof, const float* base_pos,
                        const float* base_vel, const float* ang_vel, const float* forces, const float* swing_ref, const float* stance,
                        const float* tau_bias, int tau_bias_stride, const float* mass_matrix, int mass_matrix_stride,
                        const float* acc_bias, int acc_bias_stride, const float* arm_q_des, const float* tau_limit, int flags,
                        float* tau, float* leg_force, float* foot, int32_t* info, void* stream);

/* One update of the attitude filter, the estimator of what wbc_sim_leg_odometry, wbc_sim_footstep_plan, wbc_sim_contact_detect and
 * wbc_sim_leg_control take as `quat` and `gyro`: the trunk's orientation and the gyro's bias from the gyro, the accelerometer's gravity
 * direction and up to WBC_ATTITUDE_MAX_AUX further direction measurements (a compass, say). A multiplicative extended Kalman filter on
 * the unit quaternion (Markley, "Attitude error representations for Kalman filtering", JGCD 2003; the error-state algebra of Trawny and
 * Roumeliotis, "Indirect Kalman filter for 3D attitude estimation", 2005). OURS, not the papers': quaternions are xyzw (Hamilton product,
 * scalar last) and R(q) maps trunk axes to world axes as everywhere in this header (Trawny and Roumeliotis use the JPL product and the
 * opposite map); the error is a rotation vector in TRUNK axes applied on the right, R_true = R(q) exp([dtheta]x) (Markley applies his
 * on the other side); the bias error is db = b_true - b; the correction runs as sequential 3-row updates in square-root form (W = L^-1 H P),
 * not with one gain matrix. One launch (wbc_attitude_filter_kernel); the sim's state is read, never written. Per env the caller owns
 * q      device f32 [N, 4], xyzw, unit: taken as stored (not normalised on reading), written normalised;
 * b      device f32 [N, 3], the gyro's bias in trunk axes, rad/s;
 * P      device f32 [N, 6, 6], the covariance of the error state (dtheta, db). P is read as a symmetric matrix (its lower triangle is
 *        read) and written bit-symmetric.
 * INPUTS of one update over a step cfg->dt that ends now:
 * gyro   device f32 [N, 3] or NULL: the measured angular velocity in trunk axes. NULL: ROOT_STATES' world angular velocity rotated by
 *        R^T of ROOT_STATES' quaternion, normalised (wbc_sim_leg_odometry's rule).
 * accel  device f32 [N, 3] or NULL: the specific force in trunk axes, wbc_sim_leg_odometry's convention (a = R accel + g with
 *        wbc_task_cfg.gravity, which must not be zero). NULL: no gravity row.
 * aux_body, aux_world  device f32 [N, K, 3], aux_sigma device f32 [N, K], K = num_aux in 0 .. WBC_ATTITUDE_MAX_AUX (all three NULL or
 *        unread with K = 0): a direction measured in trunk axes, the same direction known in world axes (both normalised in the call)
 *        and the standard deviation of each component of the normalised measurement. An entry whose sigma is <= 0 is skipped and its
 *        vectors are never read.
 * With exp(phi) = (phi / |phi| sin(|phi| / 2), cos(|phi| / 2)), and for |phi| < 1e-4 the series (phi / 2 (1 - |phi|^2 / 24), 1 - |phi|^2 / 8)
 * (so that exp(0) = (0, 0, 0, 1) exactly and q (x) exp(0) has q's bits), normalise(q) = q / sqrt(q . q) and gn = |gravity|:
 *   predict   w = gyro - b, dq = exp(w dt), q- = normalise(q (x) dq); with A = R(dq)^T and G = A P_tb:
 *             P-_tt = A P_tt A^T - dt (G + G^T) + dt^2 P_bb + dt sigma_g^2 I, P-_tb = G - dt P_bb, P-_bb = P_bb + dt sigma_b^2 I
 *             (= Phi P Phi^T + Q with Phi = [[A, -dt I], [0, I]], Q = dt diag(sigma_g^2 I, sigma_b^2 I));
 *   correct   one 3-row update per measurement j, the accelerometer (j = 0) first, then aux 0 .. K-1 (j = 1 + k), each on the result
 *             of the one before: world unit vector w_j (the accelerometer's: -gravity / gn; aux: aux_world / |aux_world|), measured
 *             u (accel; aux_body), m = u / |u|, mh = R(q)^T w_j, e = m - mh, H = [[mh]x, 0] (d mh / d dtheta = [mh]x), per-component
 *             variance r = sigma^2; the accelerometer's r = sigma_a^2 (1 + kappa_a ((|accel| - gn) / gn)^2): a trunk that accelerates
 *             or falls is trusted less, continuously, with no gate. S = H P H^T + r I = L L^T row by row as in wbc_sim_contact_detect
 *             step 3; W = L^-1 H P, y = L^-1 e, dx = W^T y; q <- normalise(q (x) exp(dx[0:3])), b <- b + dx[3:6], P <- P - W^T W,
 *             nis_j = |y|^2. The reset of the covariance after the multiplicative update (its Jacobian I - [dx_theta / 2]x) is
 *             first order in the correction and left out.
 *             A measurement with u . u = 0 (in fp32) is skipped: nis_j = 0 and status bit WBC_ATTITUDE_INFO_ZERO << j (an aux
 *             entry whose aux_world has zero length likewise). One where a pivot of S is not a positive finite number is skipped and the
 *             state from before it is kept: nis_j = 0, bit WBC_ATTITUDE_INFO_PIVOT << j, status code WBC_ATTITUDE_STATUS_FAILED_PIVOT.
 * RESET: with WBC_ATTITUDE_RESET in flags every env, with reset_mask (device int32 [N] or NULL) the envs whose entry is not 0:
 * b = 0, P = diag(p0_theta I_3, p0_b I_3), nis = 0, status code WBC_ATTITUDE_STATUS_RESET, and
 *   q = normalise(q_init) with q_init (device f32 [N, 4] or NULL) given;
 *   else, with accel given and accel . accel != 0, the shortest rotation with R(q) m = w_0: q = normalise((m x w_0, 1 + m . w_0)), which
 *   fixes the tilt and turns about no vertical axis (zero yaw); where 1 + m . w_0 < WBC_ATTITUDE_ANTIPARALLEL (the trunk upside down, the
 *   shortest rotation undefined) q = (h, 0), a half turn about h = normalise(c x w_0), c the world x axis where |w_0,x| <= 0.9 and the
 *   world y axis otherwise, with bit WBC_ATTITUDE_INFO_HALF_TURN;
 *   else q = (0, 0, 0, 1) (a zero accel with bit WBC_ATTITUDE_INFO_ZERO).
 * Such an env is neither predicted nor corrected in that call; its q, b, P and the aux inputs are not read.
 * An env that reads a value that is not finite (gyro and accel are read by every env; the aux vectors and sigma of an entry that is not
 * skipped, q, b and P's lower triangle by an env that is not reset; q_init by one that is) or whose new state comes out not finite keeps
 * its state, gets zeros in every float output and status WBC_ATTITUDE_STATUS_FAILED alone; no other env is affected.
 * OUTPUTS besides q, b and P, each may be NULL and is then not written; what is written does not depend on which are asked for:
 * gyro_out      device f32 [N, 3] = gyro - b with the b that leaves: what wbc_sim_leg_odometry takes as gyro;
 * gravity_body  device f32 [N, 3] = R(q)^T gravity / gn with the q that leaves: the estimate of the policy's projected gravity;
 * nis           device f32 [N, 1 + K], 0 for a row that was skipped or not given;
 * status        device int32 [N]: a code in the bits WBC_ATTITUDE_STATUS_MASK, OR'ed with the WBC_ATTITUDE_INFO_* bits.
 * Every pointer needs 4-byte alignment only. Nothing is allocated and nothing synchronises: safe under stream capture. -1 with a message
 * in wbc_last_error() that names the entry point, nothing written, checked before the sim: NULL cfg, q, b or P; num_aux out of range or
 * > 0 with a NULL aux pointer; unknown flag bits; dt, a sigma or an initial variance that is not finite and > 0; kappa_a not finite or
 * < 0; a misaligned pointer. Then NULL sim; zero gravity. -3 / -2 and stream handling as wbc_sim_coriolis. */
#define WBC_ATTITUDE_MAX_AUX 4
typedef struct {
  float dt;                                  /* s */
  float sigma_g, sigma_b;                    /* noise densities of the gyro (rad/s/sqrt(Hz)) and of the bias's random walk */
  float sigma_a;                             /* standard deviation of each component of the normalised accelerometer direction */
  float kappa_a;                             /* inflation of sigma_a^2 by the squared relative excess of |accel| over |gravity| */
  float p0_theta, p0_b;                      /* the variances a reset starts from */
} wbc_attitude_cfg;
#define WBC_ATTITUDE_RESET 1
#define WBC_ATTITUDE_ANTIPARALLEL 1e-6f
#define WBC_ATTITUDE_STATUS_MASK 15
#define WBC_ATTITUDE_STATUS_OK 0
#define WBC_ATTITUDE_STATUS_RESET 1
#define WBC_ATTITUDE_STATUS_FAILED 2
#define WBC_ATTITUDE_STATUS_FAILED_PIVOT 3
#define WBC_ATTITUDE_INFO_ZERO 16                /* << j: measurement j (0 the accelerometer, 1 + k aux k) had zero length */
#define WBC_ATTITUDE_INFO_PIVOT 512              /* << j: measurement j's innovation matrix had a failed pivot */
#define WBC_ATTITUDE_INFO_HALF_TURN 16384        /* the reset from the accelerometer took the half turn */
int wbc_sim_attitude_filter(wbc_sim* sim, const wbc_attitude_cfg* cfg, const float* gyro, const float* accel, const float* aux_body,
                            const float* aux_world, const float* aux_sigma, int num_aux, const int32_t* reset_mask, const float* q_init,
                            int flags, float* q, float* b, float* P, float* gyro_out, float* gravity_body, float* nis, int32_t* status,
                            void* stream);

/* One control step of the blind terrain estimate, the layer that gives wbc_sim_leg_odometry its foot_height, wbc_sim_contact_detect its
 * ground and normal, wbc_sim_task_inverse_dynamics_qp its normal and the MPC's reference its height and tilt without the simulator's
 * heightfield: a plane through the most recent footholds (Bledt et al., "MIT Cheetah 3: Design and Control of a Robust, Dynamic Quadruped
 * Robot", IROS 2018, the terrain-slope estimate). OURS, not the paper's: the footholds are weighted by their age, the fit is regularised
 * towards the previous slope (which is its only memory), and the plane is kept relative to an anchor at the footholds' weighted mean, so
 * that nothing is squared in world coordinates. One launch (wbc_ground_estimate_kernel); the sim's state is read, never written. Per env
 * the caller owns
 * state  device f32 [N, WBC_GROUND_NS = 32], read and written. Per foot (feet_rb order FL, FR, RL, RR) five floats at 5 i: the last contact
 *        point m_i (the foot ORIGIN, world axes), its age t_i in seconds, a reserved 0. At 20: the anchor (c_x, c_y). At 22: the plane
 *        (a0, a1, a2), z(x, y) = a0 + a1 (x - c_x) + a2 (y - c_y): the height of a foot origin at rest on the ground at (x, y). 25 .. 31
 *        are written as 0. Only m_i, t_i, a1 and a2 are ever read.
 * INPUTS (device f32 unless said otherwise; each but contact may be NULL):
 * quat [N, 4] xyzw, normalised in the call: R (world <- trunk). NULL: ROOT_STATES'.   dof [N, 20, 2] in the layout of DOF_STATE (the
 *        velocities are not read). NULL: DOF_STATE.   base_pos [N, 3]: the trunk origin b, world axes. NULL: ROOT_STATES' (a
 *        BaseStateEstimator's position fits here).
 * contact [N, 4], required: wbc_sim_contact_detect's prob, a 0 / 1 flag or wbc_sim_footstep_plan's contact. Foot i counts as standing iff
 *        contact_i >= c_on.
 * reset_mask int32 [N].   query_xy [N, Q, 2], Q = num_query >= 0: world points at which the plane is evaluated (the planner's footholds,
 *        the positions of x_ref's stages). NULL: no query, whatever Q.
 * PER ENV, in this order. A sum over the four feet is taken pairwise, (s_0 + s_1) + (s_2 + s_3).
 * 1 KINEMATICS  the leg walk of wbc_sim_leg_odometry: the foot origins p_i = b + R fk_i(q).
 * 2 RESET (WBC_GROUND_RESET in flags: every env; otherwise the envs whose reset_mask entry is not 0; the env's state is then not read):
 *   m_i = p_i and t_i = 0 for every foot, (a1, a2) = 0; info bit WBC_GROUND_INFO_RESET. The env then goes through steps 3 .. 6 of this very
 *   call with that state.
 * 3 LATCH  a standing foot: m_i <- p_i, t_i <- 0, info bit WBC_GROUND_INFO_LATCHED << i. Any other foot: t_i <- t_i + dt. Weights
 *   w_i = exp(-(t_i - t_min) / tau_age) with t_min the smallest of the four ages, W = sum w_i. The fit below is homogeneous in the weights,
 *   so this is the fit with w_i = exp(-t_i / tau_age), a foot that stays in the air loses weight against the others at that rate, and
 *   W >= 1 however old the footholds are.
 * 4 FIT  relative to foot 0's point, e_i = m_i - m_0: r = (sum w_i e_i) / W, the anchor cbar = m_0 + r (the weighted mean of the m_i, all
 *   three coordinates) and d_i = e_i - r = m_i - cbar, formed without rounding cbar and before anything is squared. With lw = lambda W and
 *   a_prev the stored slope (0 after a reset):
 *     [Sxx + lw, Sxy; Sxy, Syy + lw] a = (Sxz + lw a_prev,1, Syz + lw a_prev,2),   Suv = sum_i (w_i d_i,u) d_i,v.
 *   The lambda term is the only memory of the slope; it keeps the system regular when the weighted footholds are collinear (a long trot
 *   stance on one diagonal): the slope along the line is fitted, the slope across it stays a_prev. The system is solved by the written-out
 *   Cholesky factorisation of wbc_sim_contact_detect step 3 (l00 = sqrt(A00), l10 = A10 / l00, d1 = A11 - l10^2, l11 = sqrt(d1), forwards,
 *   backwards). Where a pivot (A00, d1) is not a positive finite number, or a comes out not finite, a = a_prev: info bit
 *   WBC_GROUND_INFO_DEGENERATE (anchor and a0 still move). Then, where |a| > slope_max, a <- a (slope_max / |a|): info bit
 *   WBC_GROUND_INFO_CLAMPED. Stored: (c_x, c_y) = m_0,xy + r_xy, a0 = m_0,z + r_z, (a1, a2) = a. A point (x, y) enters the plane as
 *   g = ((x, y) - m_0,xy) - r_xy, z = a0 + (a1 g_x + a2 g_y): relative to the anchor before it was rounded into the state.
 * 5 OUTPUTS, each may be NULL and is then not written; what is written never depends on which are asked for:
 *   normal f32 [N, 4, 3]: n = (-a1, -a2, 1) / sqrt(1 + a1^2 + a2^2), the same for every foot: the layout wbc_sim_contact_detect and
 *          wbc_sim_task_inverse_dynamics_qp take.
 *   ground f32 [N, 4] = z(p_i,xy) for every foot, standing or not: the foot-ORIGIN convention of wbc_sim_contact_detect's ground and
 *          wbc_sim_leg_odometry's foot_height. A standing foot does not get its own height back (the detector's height term would be
 *          circular).
 *   residual f32 [N, 4] = m_i,z - z(m_i,xy) = d_i,z - (a1 d_i,x + a2 d_i,y): the fit's own roughness measure.
 *   trunk f32 [N, 6]: z(b_xy); the clearance (b_z - z(b_xy)) n_z along the normal; the slopes along and across the heading,
 *          s_f = a1 c + a2 s and s_l = -a1 s + a2 c with (c, s) wbc_sim_footstep_plan's heading rule on R; two reserved zeros.
 *   theta_ref f32 [N, 3] = tilt_gain g(s) (a2, -a1, 0), s = |a|, g(s) = atan(s) / s, and for s < WBC_GROUND_SERIES the series 1 - s^2 / 3
 *          (a = 0 gives exactly 0): the world-axes rotation vector of the shortest rotation from world z to n, scaled by tilt_gain: what
 *          the theta block of the MPC's x_ref holds.
 *   query_z f32 [N, Q]: the plane at the query points (nothing is written with Q = 0 or without query_xy).
 *   info int32 [N]: the bits below.
 * 6 FAILURE  an env that reads a value that is not finite (quat, or a zero quat; b; a leg joint's q; contact; its query points; and,
 *   unless it is reset, its m_i, t_i, a1, a2) writes zeros to every float output, info = WBC_GROUND_INFO_FAILED alone, and leaves its state
 *   as it was; no other env is affected.
 * Every pointer needs 4-byte alignment only. Nothing is allocated and nothing synchronises: safe under stream capture. -1 with a message
 * in wbc_last_error() that names the entry point, nothing written, checked BEFORE the sim: NULL cfg, state or contact; unknown flag bits;
 * dt, tau_age, lambda or slope_max not finite and > 0; c_on not finite; tilt_gain outside [0, 1]; num_query < 0, or query_xy given with
 * num_query = 0; a misaligned pointer. Then NULL sim; -3 (also: a foot whose leg does not have exactly three joints) / -2 and stream
 * handling as wbc_sim_coriolis. Not covered: per-foot local patches, normals inside the MPC's cone or the leg controller's clip,
 * feeding the plane to wbc_sim_footstep_plan (which keeps reading the heightfield). */
#define WBC_GROUND_NS 32            /* floats of state per env */
#define WBC_GROUND_SERIES 1e-4f     /* below this |a|, atan(s) / s is taken from its series */
typedef struct {
  float dt;                         /* control step, s */
  float c_on;                       /* a foot stands iff contact >= c_on */
  float tau_age;                    /* time constant of a foothold's weight, s */
  float lambda;                     /* weight of the previous slope in the fit, m^2 */
  float slope_max;                  /* largest |a| */
  float tilt_gain;                  /* share of the plane's tilt that theta_ref asks of the trunk, [0, 1] */
} wbc_ground_cfg;
#define WBC_GROUND_RESET 1
#define WBC_GROUND_INFO_RESET 1
#define WBC_GROUND_INFO_FAILED 2
#define WBC_GROUND_INFO_DEGENERATE 4
#define WBC_GROUND_INFO_CLAMPED 8
#define WBC_GROUND_INFO_LATCHED 16               /* << foot */
int wbc_sim_ground_estimate(wbc_sim* sim, const wbc_ground_cfg* cfg, const float* quat, const float* dof, const float* base_pos,
                            const float* contact, const int32_t* reset_mask, const float* query_xy, int num_query, int flags, float* state,
                            float* normal, float* ground, float* residual, float* trunk, float* theta_ref, float* query_z, int32_t* info,
                            void* stream);

/* One control step of the foot slip detector and friction estimate, the layer that tells wbc_sim_leg_odometry and
 * wbc_sim_ground_estimate how far a standing foot can be trusted to stand still, and wbc_sim_task_inverse_dynamics_qp which friction
 * coefficient its pyramid should take: a per-foot velocity test with hysteresis, and a friction estimate from the force ratio while the
 * foot slides (Focchi, Barasuol, Frigerio, Caldwell, Semini, "Slip Detection and Recovery for Quadruped Robots", ISRR 2015). OURS, not
 * the paper's: the evidence is a probability Phi of the tangential speed, low-passed, with hysteresis and a dwell time (the paper
 * compares each foot's speed with the median of the feet's); the common mode is a contact-weighted mean with a gain; the estimate is a
 * weighted running mean with forgetting per foot, fused per env, next to a lower bound from the feet that stick; a foot in the air cannot
 * start slipping. One launch (wbc_slip_detect_kernel); the sim's state is read, never written. The base POSITION is never read (there is
 * no such argument): every output is bit-identical under a translation of the robot. Per env the caller owns
 * state  device f32 [N, 4, WBC_SLIP_NS = 8], read and written; per foot (feet_rb order FL, FR, RL, RR): 0 p the filtered slip
 *        probability; 1 s the slip flag (0.0 or 1.0; read as != 0); 2 t the dwell timer, s; 3 c_prev, whether the foot stood in the last
 *        call (0.0 or 1.0; read as != 0); 4 d the distance slid in this stance, m; 5 mu_i this foot's friction estimate; 6 w_i the weight
 *        of mu_i; 7 m_i the sticking bound: the largest force ratio seen while not slipping, forgotten at rate gamma.
 * INPUTS (device f32 unless said otherwise; each but contact may be NULL):
 * quat [N, 4] xyzw, normalised in the call: R (world <- trunk). NULL: ROOT_STATES'.   dof [N, 20, 2] in the layout of DOF_STATE; the
 *        positions q and the velocities qd of the leg joints are read. NULL: DOF_STATE.
 * base_vel [N, 3]: the world linear velocity v of the trunk origin (a BaseStateEstimator's v fits). NULL: ROOT_STATES'.
 * ang_vel [N, 3]: the trunk's angular velocity w in TRUNK axes (wbc_sim_attitude_filter's gyro_out fits). NULL: R^T times ROOT_STATES'
 *        (which is in world axes).
 * contact [N, 4], required: wbc_sim_contact_detect's prob, a 0 / 1 flag or wbc_sim_footstep_plan's contact.
 * foot_force [N, 4, 3], world axes: the force of the ground on the foot (wbc_sim_contact_detect's force). NULL: step 7 is left out, slots
 *        5 .. 7 of the state keep their values, info bit WBC_SLIP_INFO_NO_FORCE.
 * normal [N, 4, 3]: the ground's normal under each foot, normalised in the call: n_i = normal_i / |normal_i|. NULL: world z.
 * reset_mask int32 [N].   mu_init [N, 4], NULL: mu_prior.
 * PER ENV AND FOOT i, in this order (Phi(x) = (1/2) (1 + erf(x / sqrt 2)), wbc_sim_contact_detect's). A sum over the four feet is taken
 * pairwise, (x_0 + x_1) + (x_2 + x_3).
 * 1 KINEMATICS  the leg walk of wbc_sim_contact_detect step 2: fk_i(q) in trunk axes, a_k the axis and o_k the origin of the leg's k-th
 *   actuated joint (k = 0, 1, 2 from the trunk down), c_k = a_k x (fk_i - o_k). The foot origin's world velocity is
 *     u_i = v + R (w x fk_i + ((qd_0 c_0 + qd_1 c_1) + qd_2 c_2)).
 * 2 RESET (WBC_SLIP_RESET in flags: every env; otherwise the envs whose reset_mask entry is not 0; the env's state is then not read):
 *   p = 0, s = 0, t = t_dwell, c_prev = 0, d = 0, w_i = 0, m_i = 0, mu_i = mu_init_i (NULL: mu_prior); info bit WBC_SLIP_INFO_RESET. The
 *   env then goes through steps 3 .. 9 of this very call with that state.
 * 3 STANDING  c_i = min(max(contact_i, 0), 1), stand_i = c_i >= c_on. A touchdown (stand_i and c_prev = 0) sets d = 0.
 * 4 COMMON MODE  a wrong base_vel moves every foot alike, so it can be taken out. With cw_j = c_j where foot j stands and 0 elsewhere,
 *   S = sum_j cw_j: where at least two feet stand and S > 0, ubar = (sum_j cw_j u_j) / S per coordinate, otherwise ubar = 0.
 *   g_i = u_i - common_mode ubar, its tangential part gt_i = g_i - n_i (n_i . g_i), the slip speed s_i = |gt_i|.
 * 5 EVIDENCE  P_i = c_i Phi((s_i - v_slip) / sigma_v) where foot i stands, 0 elsewhere;  p <- p + alpha (P_i - p).
 * 6 FLAG  t <- t + dt. If the foot does not stand and s = 1: s <- 0, t <- 0, info bit WBC_SLIP_INFO_END << i. Else if it stands, s = 0,
 *   p >= p_on and t >= t_dwell: s <- 1, t <- 0, info bit WBC_SLIP_INFO_START << i. Else if s = 1, p <= p_off and t >= t_dwell: s <- 0,
 *   t <- 0, info bit WBC_SLIP_INFO_END << i. Then d <- d + s_i dt where s = 1, c_prev <- stand_i, and info bit
 *   WBC_SLIP_INFO_SLIPPING << i where s = 1.
 * 7 FRICTION (with foot_force only)  fn = n_i . f_i, ft = |f_i - n_i fn|, valid = stand_i and fn >= fn_min, rho = ft / fn.
 *   m_i <- gamma m_i, and where valid and s = 0: m_i <- max(m_i, rho). w_i <- gamma w_i, and where valid, s = 1 and p > 0:
 *   w_i <- w_i + p, then mu_i <- mu_i + (p / w_i) (rho - mu_i). A sticking foot bounds the coefficient from below; a sliding foot measures
 *   it. Info bit WBC_SLIP_INFO_MU_VALID << i where w_i >= w_min (with or without foot_force).
 * 8 FUSE, per env: W = sum_i w_i; mu_env = (sum_i w_i mu_i) / W where W >= w_min, mu_prior elsewhere. Per foot mu_raw = mu_i where
 *   w_i >= w_min, mu_env elsewhere.
 * 9 OUTPUTS, each may be NULL and is then not written; what is written never depends on which are asked for:
 *   prob f32 [N, 4] = p;   slip u8 [N, 4] = s;   weight f32 [N, 4] = c_i (1 - p): what wbc_sim_leg_odometry and wbc_sim_ground_estimate
 *   should take as contact;   foot_vel f32 [N, 4, 3] = u_i;   speed f32 [N, 4] = s_i;   distance f32 [N, 4] = d;
 *   mu f32 [N, 4] = min(max(mu_scale mu_raw, mu_min), mu_max): the layout wbc_sim_task_inverse_dynamics_qp takes;
 *   mu_lower f32 [N, 4] = m_i;   mu_env f32 [N, 2] = (mu_env, W);   info int32 [N]: the bits below.
 * 10 FAILURE  an env that reads a value that is not finite (quat, or a zero quat; v; w; a leg joint's q or qd; contact; foot_force; normal,
 *   or a zero normal; mu_init where it is reset; unless it is reset, the eight floats of state of any foot), or whose u_i or new p, t, d,
 *   mu_i, w_i or m_i comes out not finite, writes zeros to every float and byte output, info = WBC_SLIP_INFO_FAILED alone, and leaves its
 *   state as it was; no other env is affected.
 * Every pointer needs 4-byte alignment only (the u8 output none). No workspace; nothing is allocated and nothing synchronises: safe under
 * stream capture. -1 with a message in wbc_last_error() that names the entry point, nothing written, checked BEFORE the sim: NULL cfg,
 * state or contact; unknown flag bits; dt, sigma_v, fn_min, w_min or mu_scale not finite and > 0; c_on not finite; v_slip, t_dwell,
 * mu_prior or mu_min not finite or < 0; alpha or gamma outside (0, 1]; p_on or p_off not finite, or p_on <= p_off; common_mode outside
 * [0, 1]; mu_max not finite or < mu_min; a misaligned pointer. Then NULL sim; -3 (also: a foot whose leg does not have exactly three
 * joints) / -2 and stream handling as wbc_sim_coriolis. Not covered: slip recovery (re-planning the force or the foothold), a friction
 * coefficient per env inside the MPC, estimating the normal from the slip direction, tuning of any default. */
#define WBC_SLIP_NS 8               /* floats of state per foot */
typedef struct {
  float dt;                         /* control step, s */
  float c_on;                       /* a foot stands iff its clamped contact >= c_on */
  float v_slip, sigma_v;            /* mean and width of the slip speed's evidence, m/s */
  float alpha;                      /* low-pass weight of the filtered probability, (0, 1] */
  float p_on, p_off;                /* hysteresis thresholds, p_on > p_off */
  float t_dwell;                    /* minimum seconds between flag switches, >= 0 */
  float common_mode;                /* share of the standing feet's mean velocity that is taken out, [0, 1] */
  float fn_min;                     /* smallest normal force at which the force ratio is used, N, > 0 */
  float gamma;                      /* forgetting factor per call of w_i and m_i, (0, 1] */
  float w_min;                      /* weight from which an estimate counts, > 0 */
  float mu_prior;                   /* the coefficient where nothing has been measured */
  float mu_min, mu_max;             /* clamp of the mu output */
  float mu_scale;                   /* safety factor of the mu output, > 0 */
} wbc_slip_cfg;
#define WBC_SLIP_RESET 1
#define WBC_SLIP_INFO_RESET 1
#define WBC_SLIP_INFO_FAILED 2
#define WBC_SLIP_INFO_NO_FORCE 4
#define WBC_SLIP_INFO_START 16                /* << foot */
#define WBC_SLIP_INFO_END 256                 /* << foot */
#define WBC_SLIP_INFO_SLIPPING 4096           /* << foot */
#define WBC_SLIP_INFO_MU_VALID 65536          /* << foot */
int wbc_sim_slip_detect(wbc_sim* sim, const wbc_slip_cfg* cfg, const float* quat, const float* dof, const float* base_vel,
                        const float* ang_vel, const float* contact, const float* foot_force, const float* normal,
                        const int32_t* reset_mask, const float* mu_init, int flags, float* state, float* prob, uint8_t* slip, float* weight,
                        float* foot_vel, float* speed, float* distance, float* mu, float* mu_lower, float* mu_env, int32_t* info,
                        void* stream);

/* First-order layer of wbc_sim_inverse_dynamics / wbc_sim_forward_dynamics: the analytic partial derivatives of tau(q, nu, nudot) and
 * of nudot(q, nu, tau) in the coordinates of wbc_sim_body_dynamics, from the sim's current root / DoF state, WBC_T_BODY_PARAMS and all
 * three gravity components. The sim's state is read, never written.
 * Configuration tangent dq in R^26, chosen so that "qdot = nu":
 *   dq[0:3]  translates the root origin, world axes;
 *   dq[3:6]  is a WORLD-frame rotation vector, R <- exp([dtheta]x) R;
 *   dq[6+d]  increments DoF d.
 * Partial derivatives with respect to dq hold the WORLD components of nu and nudot fixed; the rows of tau are those of
 * wbc_sim_inverse_dynamics (0:3 net external force, 3:6 net external moment about the root origin, world axes, 6: joint torques).
 * With this choice, along any motion d tau / dt = (dtau/dq) nu + (dtau/dnu) nudot + M d(nudot)/dt.
 *
 * wbc_sim_inverse_dynamics_derivatives: ONE launch (wbc_dynamics_derivatives_kernel).
 * nudot     device f32 [N, 26] or NULL (= zeros), in the convention of wbc_sim_inverse_dynamics.
 * dtau_dq, dtau_dnu   device f32 [N, 26, 26], [e, i, j] = d tau_i / d x_j; either may be NULL (not written), not both. With
 *           WBC_DERIV_TRANSPOSED in flags the layout is [e, j, i]: one direction's 26 values are contiguous, the right-hand-side
 *           layout wbc_sim_mass_solve reads (rhs_env_stride 676, nrhs 26).
 * Exact structure, written as literal zeros: dtau_dq[:, :, 0:3] (the root position is never read: every output is bit-identical under
 * a translation of the robot), dtau_dnu[:, :, 0:3] (Galilean invariance: v_root does not enter the arithmetic), rows and columns
 * 24, 25 (locked fingers; their entries of nudot and of qd are ignored) and every joint-row x joint-column entry whose two joints lie
 * on different chains.
 * RIGID-BODY dynamics only, exactly as wbc_sim_inverse_dynamics: no armature, no limit stops, no contacts. Nothing is allocated, so
 * the call is safe under stream capture. Every pointer needs 4-byte alignment only.
 *
 * wbc_sim_forward_dynamics_derivatives:
 * tau       device f32 [N, 26] or NULL (= zeros), nudot device f32 [N, 26] (required): nudot = M^-1 (tau - h), the bits of
 *           wbc_sim_forward_dynamics.
 * dnudot_dq   = -M^-1 dtau/dq taken at that nudot;  dnudot_dnu = -M^-1 dtau/dnu;  minv = d nudot / d tau = M^-1. Device f32
 *           [N, 26, 26] in the layout rules above ([e, i, j] = d nudot_i / d x_j, or [e, j, i] with WBC_DERIV_TRANSPOSED); each may be
 *           NULL, not all three. The zero columns 0:3 of the first two and the fingers' rows and columns are exactly zero.
 * flags     any of WBC_SOLVE_ARMATURE (M + diag(0_6, joint_armature) throughout; the armature is constant, so the formula is
 *           unchanged) and WBC_DERIV_TRANSPOSED.
 * workspace caller-owned device floats, at least wbc_sim_forward_dynamics_derivatives_workspace_floats(N) of them (0 for a bad
 *           argument). Nothing is allocated in the call. The sim's bias-force scratch of wbc_sim_forward_dynamics is used as well,
 *           with the same caveat: one stream at a time per sim.
 * Launches on `stream`, no host synchronisation: h (wbc_inverse_dynamics_kernel) and the solve for nudot (the two launches of
 * wbc_sim_forward_dynamics); wbc_dynamics_derivatives_kernel at that nudot, writing -dtau/dq and -dtau/dnu transposed into the
 * workspace (and a 26 x 26 identity when minv is wanted); one wbc_mass_solve_kernel launch of 26 right-hand sides per requested
 * output, which leaves the transposed layout -- straight in the caller's tensors with WBC_DERIV_TRANSPOSED; otherwise one
 * wbc_derivatives_transpose_kernel launch moves all of them to [e, i, j]. Seven launches for everything in the conventional layout,
 * six transposed.
 * Both: -1 with a message in wbc_last_error(), nothing written, for a NULL sim (/ nudot / workspace), all outputs NULL, unknown flag
 * bits or a pointer that is not 4-byte aligned; -3 for a model whose tree the kernel cannot walk; -2 if a launch fails. Stream / device
 * handling as wbc_sim_centroidal. */
#define WBC_DERIV_TRANSPOSED 2   /* distinct from WBC_SOLVE_ARMATURE (1): the two functions share `flags` */
int wbc_sim_inverse_dynamics_derivatives(wbc_sim* sim, const float* nudot, float* dtau_dq, float* dtau_dnu, int flags, void* stream);
size_t wbc_sim_forward_dynamics_derivatives_workspace_floats(int num_envs);
int wbc_sim_forward_dynamics_derivatives(wbc_sim* sim, const float* tau, float* nudot, float* dnudot_dq, float* dnudot_dnu, float* minv,
                                         int flags, float* workspace, void* stream);

/* How wbc_sim_inverse_dynamics depends on the bodies' inertial parameters. Inverse dynamics is LINEAR in every moving body's ten
 * parameters: tau = sum_b Y_b(q, nu, nudot) pi_b. One launch (wbc_inverse_dynamics_regressor_kernel) writes Y from the state sources of
 * wbc_sim_inverse_dynamics: the sim's current root / DoF state, all three gravity components, nudot. The sim's state is read, never
 * written.
 * bodies  HOST array of nbodies distinct moving-body indices in 0..WBC_NB-1 (1..WBC_NB of them), the order of the output's body axis;
 *         NULL with nbodies == 0: all nineteen, in order.
 * nudot   device f32 [N, 26] or NULL (= zeros: the regressor of the bias vector h), in the convention of wbc_sim_inverse_dynamics.
 * Y       device f32 [N, 26, nbodies, 10], caller-owned, 16-byte aligned: [e, i, b, k] = d tau_i / d (parameter k of bodies[b]); rows as
 *         the rows of tau (0:3 net external force, 3:6 net external moment about the root origin, world axes, 6: joint torques). With
 *         WBC_DERIV_TRANSPOSED the layout is [N, nbodies * 10, 26]: one parameter's 26 values are contiguous, the right-hand-side
 *         layout wbc_sim_mass_solve reads.
 * flags   any of WBC_DERIV_TRANSPOSED and WBC_REGRESSOR_NATIVE.
 * Columns, default: the linear parameters pi_b = (m, m c_x, m c_y, m c_z, Ibar_xx, Ibar_yy, Ibar_zz, Ibar_xy, Ibar_xz, Ibar_yz), c the
 *         centre of mass in body axes and Ibar the rotational inertia about the body's own ORIGIN in body axes,
 *         Ibar = I_c + m (|c|^2 1 - c c^T). Then sum_b Y[:, :, b] pi_b equals tau of wbc_sim_inverse_dynamics(nudot) up to rounding,
 *         with pi of the root and the gripper body formed from WBC_T_BODY_PARAMS and pi of the other bodies from wbc_model. Y itself does
 *         not depend on any body parameter.
 * Columns, WBC_REGRESSOR_NATIVE: d tau / d theta_b with theta_b = (m, c_x, c_y, c_z, I_c xx, yy, zz, xy, xz, yz), the parametrisation
 *         of WBC_T_BODY_PARAMS and of wbc_model, with the inertia about the centre of mass, by the chain rule in the kernel at the body's
 *         CURRENT theta (per env for the root composite and the gripper body). With bodies = (0, wbc_model.gripper_body) the output
 *         [N, 26, 20] lines up column for column with WBC_T_BODY_PARAMS.
 * Exact structure, written as literal zeros: the entries of joint row i for a body that is not in the subtree joint i moves, the
 * fingers' rows 24, 25 (their entries of nudot and of qd are ignored) and the inertia columns of the force rows 0:3.
 * The root POSITION is never read: the result is bit-identical under a translation of the robot. RIGID-BODY dynamics only, exactly as
 * wbc_sim_inverse_dynamics. Nothing is allocated, so the call is safe under stream capture.
 *
 * wbc_sim_forward_dynamics_sensitivity: nudot = M^-1 (tau - h), the bits of wbc_sim_forward_dynamics, and how it depends on the same
 * parameters, d nudot / d (parameter) = -M^-1 Y(q, nu, nudot) (M nudot + h = tau at fixed tau, differentiated).
 * bodies, nbodies   as above.  tau device f32 [N, 26] or NULL (= zeros), nudot device f32 [N, 26] (required).
 * dnudot_dpi  device f32 [N, nbodies * 10, 26], parameter-major ([e, b * 10 + k, i]): the solve's own layout.
 * workspace   caller-owned device f32 of the same size, 16-byte aligned. nudot, dnudot_dpi and workspace share no bytes (an overlap is
 *             refused; tau is only read, by the launches that write nudot). Nothing is allocated in the call,
 *             so it is safe under stream capture on a single stream. The sim's bias-force scratch of wbc_sim_forward_dynamics is used
 *             as well, with the same caveat: one stream at a time per sim.
 * flags       any of WBC_SOLVE_ARMATURE (M + diag(0_6, joint_armature) in every solve; the armature is no body parameter) and
 *             WBC_REGRESSOR_NATIVE (columns as above).
 * Launches on `stream`, no host synchronisation: the two of wbc_sim_forward_dynamics; the regressor kernel at that nudot, writing -Y
 * transposed into the workspace; one wbc_mass_solve_kernel launch per WBC_SOLVE_MAX_RHS columns (1 for two bodies, 6 for all nineteen).
 * The fingers' entries are exactly 0.
 * Both: -1 with a message in wbc_last_error(), nothing written, for a NULL sim / Y (/ nudot / dnudot_dpi / workspace), a bad `bodies`
 * (NULL with nbodies != 0, nbodies outside 1..WBC_NB, an index out of range or repeated), unknown flag bits, a misaligned pointer or
 * overlapping nudot / dnudot_dpi / workspace; -3 for a model whose tree the kernel cannot walk; -2 if a launch fails. Stream / device handling as
 * wbc_sim_centroidal. */
#define WBC_REGRESSOR_NATIVE 4   /* distinct from WBC_SOLVE_ARMATURE (1) and WBC_DERIV_TRANSPOSED (2): the functions share `flags` */
int wbc_sim_inverse_dynamics_regressor(wbc_sim* sim, const int32_t* bodies /* host */, int nbodies, const float* nudot, float* Y, int flags,
                                       void* stream);
int wbc_sim_forward_dynamics_sensitivity(wbc_sim* sim, const int32_t* bodies /* host */, int nbodies, const float* tau, float* nudot,
                                         float* dnudot_dpi, float* workspace, int flags, void* stream);

/* Recursive least-squares identification of the listed bodies' linear parameters (the columns of wbc_sim_inverse_dynamics_regressor),
 * the classical baseline to the learned adaptation module: per env the P x P normal equations, P = 10 nbodies <= 30,
 *     A <- forget A + Phi^T W Phi,   b <- forget b + Phi^T W z,   stat <- forget stat + (sum_c w_c z_c^2, number of rows with w_c > 0),
 * updated by ONE launch per control step (wbc_identification_accumulate_kernel) at the sim's current state (the state sources of the
 * regressor; read, never written). Phi [26, P] is the regressor's linear-parameter columns of the listed bodies, column s * 10 + k for
 * bodies[s]; z = tau_gen - sum over the bodies NOT listed of Y_b pi_b, with pi_b their current linear parameters (the root's and the
 * gripper body's from that env's WBC_T_BODY_PARAMS, the others' from wbc_model). Both come from the same closed-form entries inside the
 * kernel: Y is never formed in HBM, and z is not formed as tau - Phi pi, so nothing cancels.
 * bodies      HOST array of 1..WBC_IDENT_MAX_BODIES distinct moving-body indices (NULL is refused).
 * nudot       device f32 [N, 26] or NULL (= zeros).
 * tau_gen     device f32 [N, 26], required: the net generalised force in the rows of wbc_sim_inverse_dynamics, S^T tau + sum J^T f.
 * row_weight  device f32 [N, 26], entries >= 0, or NULL (= 1 on the 24 live rows). The fingers' rows 24, 25 never count.
 * forget      HOST float in (0, 1].
 * info_mat    device f32 [N, P, P] (A), info_vec device f32 [N, P] (b), stat device f32 [N, 2]: read and written.
 * target      device f32 [N, 26] or NULL: z (the fingers' rows: tau_gen).
 * flags       WBC_IDENT_RESET: the incoming A, b and stat are taken as zero and never read (NaN-poisoned buffers are fine).
 * A is written in full and is bit-symmetric. An env without a row of positive weight keeps its A, b and stat bit for bit, without
 * decay (with WBC_IDENT_RESET they become zeros); its target is still written. Every sum has a fixed order and there are no atomics: the
 * result is bitwise reproducible. The root POSITION is never read. All buffers are caller-owned, 16-byte aligned and share no bytes with
 * an output. Nothing is allocated, so the call is safe under stream capture. HBM traffic per env: the state, the three [26] rows and one
 * read and one write of A, b and stat.
 *
 * wbc_sim_identification_solve (wbc_identification_solve_kernel, one launch): (A + Lambda) pi_hat = b + Lambda pi_0 per env, Lambda =
 * diag(prior_weight) >= 0. The matrix is equilibrated to a unit diagonal, D = diag(A + Lambda)^-1/2, then factorised and solved by the
 * fp32 Cholesky core the contact kernels share.
 * nbodies       1..WBC_IDENT_MAX_BODIES, as in the accumulate calls that built A, b and stat (device f32, read only).
 * prior, prior_weight  device f32 [N, nbodies, 10] (pi_0 in the linear parameters; Lambda's diagonal) or NULL (weight NULL: 0; a NULL
 *               prior with a weight is refused).
 * pivot_tol     HOST float > 0.
 * pi_hat        device f32 [N, nbodies, 10], required.
 * theta_hat     device f32 [N, nbodies, 10] or NULL: (m, c = h / m, I_c = Ibar - m (|c|^2 1 - c c^T)), the parametrisation of
 *               WBC_T_BODY_PARAMS.
 * cov_diag      device f32 [N, nbodies, 10] or NULL: diag((A + Lambda)^-1).
 * sse           device f32 [N] or NULL (needs stat): stat_0 - 2 pi_hat^T b + pi_hat^T A pi_hat, clamped at 0. Three fp32 numbers of the
 *               size of stat_0 cancel here: it resolves no better than a few 2^-24 stat_0, whatever the true residual.
 * status        device int32 [N, nbodies] or NULL. Bit 0, the same for all bodies of an env: a diagonal entry of A + Lambda that is not
 *               positive and finite, or a squared pivot of the equilibrated factor <= pivot_tol; pi_hat is then the prior (zeros without
 *               one), theta_hat its map (zeros without one), cov_diag +inf, sse the formula at that pi_hat, and status exactly 1.
 *               Otherwise bit 1: m_hat <= 0; bit 2: I_c_hat not positive definite; bit 3: the triangle inequality of its principal
 *               moments violated. Only the flags are built: the estimate is not projected.
 * Both: -1 with a message in wbc_last_error(), nothing written, for a NULL sim or required buffer, a bad `bodies` / nbodies, forget
 * outside (0, 1], pivot_tol not positive, unknown flag bits, a buffer that is not 16-byte aligned or an output that overlaps another
 * buffer; -3 for a model whose tree the kernel cannot walk; -2 if a launch fails. Stream / device handling as wbc_sim_centroidal.
 * OUT OF SCOPE: the step kernel's own substep (implicit PD, armature, contact impulses) as the source of tau_gen; a physically
 * consistent projection; more than three bodies or a base-parameter reduction. */
#define WBC_IDENT_MAX_BODIES 3   /* P = 10 * nbodies <= 30: fits the m <= 32 Cholesky core */
#define WBC_IDENT_RESET 8        /* distinct from WBC_SOLVE_ARMATURE (1), WBC_DERIV_TRANSPOSED (2), WBC_REGRESSOR_NATIVE (4) */
int wbc_sim_identification_accumulate(wbc_sim* sim, const int32_t* bodies /* host */, int nbodies, const float* nudot,
                                      const float* tau_gen, const float* row_weight, float forget, float* info_mat, float* info_vec,
                                      float* stat, float* target, int flags, void* stream);
int wbc_sim_identification_solve(wbc_sim* sim, int nbodies, const float* info_mat, const float* info_vec, const float* stat,
                                 const float* prior, const float* prior_weight, float pivot_tol, float* pi_hat, float* theta_hat,
                                 float* cov_diag, float* sse, int32_t* status, void* stream);

/* First-order layer of wbc_sim_constrained_dynamics: the analytic partial derivatives of its solution (nudot, lambda) with respect to
 * the configuration, the velocity and the applied force, in the tangent convention of wbc_sim_inverse_dynamics_derivatives above (dq =
 * root translation, WORLD rotation vector, joint increments; the world components of nu, nudot, tau (all 26 rows), acc_des and lambda
 * held fixed). The solution satisfies, with m = 3 nbodies,
 *     r1 = ID(q, nu, nudot) [+ armature nudot] - Jc^T lambda - tau = 0        (26 rows; ID = wbc_sim_inverse_dynamics)
 *     r2 = Jc nudot + (Jdot nu)_c - acc_des + damping lambda    = 0        (m rows: the classical acceleration of the listed origins)
 * and with A = Jc M^-1 Jc^T, Y = M^-1 Jc^T and x one of the 26 directions of q or of nu
 *     X = -M^-1 dr1/dx,   dlambda/dx = -(A + damping I)^-1 (Jc X + dr2/dx),   dnudot/dx = X + Y dlambda/dx,
 *     dr1/dq = dtau_ID/dq (at the solution's nudot) - d(Jc^T lambda)/dq,   dr1/dnu = dtau_ID/dnu,
 *     dr2/dq, dr2/dnu = the partials of the listed origins' classical acceleration at fixed nudot,
 *     dnudot/dtau = M^-1 - Y (A + damping I)^-1 Y^T,   dlambda/dtau = -(A + damping I)^-1 Y^T.
 * The armature is constant, so it changes M only. Along any motion with tau(t): d nudot / dt = (dnudot/dq) nu + (dnudot/dnu) nudot +
 * (dnudot/dtau) dtau/dt at fixed acc_des, and likewise for lambda.
 * rigid_bodies, nbodies (1..WBC_CONSTR_MAX_BODIES), active, tau, acc_des, damping: exactly as in wbc_sim_constrained_dynamics.
 * flags     any of WBC_SOLVE_ARMATURE and WBC_DERIV_TRANSPOSED.
 * nudot     device f32 [N, 26] (required), lambda device f32 [N, nbodies, 3] or NULL: the bits wbc_sim_constrained_dynamics writes for
 *           the same arguments.
 * dnudot_dq, dnudot_dnu, dnudot_dtau    device f32 [N, 26, 26], [e, i, j] = d nudot_i / d x_j;
 * dlambda_dq, dlambda_dnu, dlambda_dtau device f32 [N, 3 nbodies, 26], [e, i, j] = d lambda_i / d x_j. With WBC_DERIV_TRANSPOSED the
 *           layouts are [e, j, i]: [N, 26, 26] and [N, 26, 3 nbodies]. Any of the six may be NULL (not written, and neither its walks
 *           nor its solves are run), not all six.
 * Exact structure, written as literal zeros: columns 0:3 of the four q / nu outputs (the root position and linear velocity are never
 * read: every output is bit-identical under a translation of the robot), the fingers' rows and columns 24, 25 everywhere, and the
 * three rows of an inactive body in every dlambda_*. For an env with no active body the dnudot_* are the free robot's partials
 * (wbc_sim_forward_dynamics_derivatives' formulas).
 * workspace caller-owned device floats, at least wbc_sim_constrained_dynamics_derivatives_workspace_floats(N, nbodies) of them (0 for a
 *           bad argument). Nothing is allocated in the call, so it is safe under stream capture on a single stream. The sim's
 *           bias-force scratch is used as in wbc_sim_constrained_dynamics, with the same caveat: one stream at a time per sim. The
 *           sim's state is read and never written.
 * Launches on `stream`, no host synchronisation: the four of wbc_sim_constrained_dynamics; wbc_dynamics_derivatives_kernel at that
 * nudot (-dtau_ID/dq, -dtau_ID/dnu, an identity if dnudot_dtau is wanted); wbc_constraint_tangent_kernel (dr2/dq, dr2/dnu and
 * + d(Jc^T lambda)/dq) if a q or nu output is wanted; one wbc_mass_solve_kernel launch of 26 right-hand sides per requested group;
 * wbc_constraint_derivatives_solve_kernel, which factorises A + damping I again and stores either layout directly. Ten launches for
 * everything.
 * -1 with a message in wbc_last_error(), nothing written, for everything wbc_sim_constrained_dynamics refuses, all six derivative
 * outputs NULL, unknown flag bits or a pointer that is not 4-byte aligned; -3 / -2 as there.
 * OUT OF SCOPE: the derivatives of wbc_sim_task_inverse_dynamics and wbc_sim_task_inverse_dynamics_qp (with or without an active set);
 * angular constraint rows; partials with respect to acc_des (they are Y (A + damping I)^-1 for nudot and (A + damping I)^-1 for lambda:
 * a caller with a Baumgarte law chains them itself); partials with respect to body parameters; second order. */
size_t wbc_sim_constrained_dynamics_derivatives_workspace_floats(int num_envs, int nbodies);
int wbc_sim_constrained_dynamics_derivatives(wbc_sim* sim, const int32_t* rigid_bodies /* host */, int nbodies, const uint8_t* active,
                                             const float* tau, const float* acc_des, float damping, int flags,
                                             float* nudot, float* lambda,
                                             float* dnudot_dq, float* dnudot_dnu, float* dnudot_dtau,
                                             float* dlambda_dq, float* dlambda_dnu, float* dlambda_dtau,
                                             float* workspace, void* stream);

/* extras["episode"] of reset_idx (widowGo1.py:743-754): out[0:WBC_NREW] = mean over the envs that reset in the last
 * step of their finished episode's reward sums, out[WBC_NREW:+WBC_NMETRIC] the same for the metric sums, both
 * times `scale` (1 / max_episode_length_s). `out`: device, WBC_NREW + WBC_NMETRIC floats. On a step in which no env reset
 * the reference does not touch extras["episode"] (reset_idx returns early, widowGo1.py:705-706), i.e. the previous values
 * stay published: out = prev then (prev: the previous call's output, or NULL = zeros). */
int wbc_sim_episode_stats(wbc_sim* sim, float scale, const float* prev, float* out, void* stream);
/* The same launch with one more workgroup that does wbc_runner_track_episodes' work (below) on this sim's reward / reset
 * buffers: the logged training loop's episode bookkeeping at no launch of its own. track_state == NULL: wbc_sim_episode_stats. */
int wbc_sim_episode_stats_track(wbc_sim* sim, float scale, const float* prev, float* out, float* track_state, int track_cap,
                                void* stream);

/* PPO.process_env_step's tensor work (rsl_rl/algorithms/ppo.py:129-141 + rollout_storage.py:70-72) in one launch:
 * out_rewards[n] = (rew[n], arm_rew[n]) + gamma * values[n] * time_outs[n], out_dones[n] = dones[n] != 0.
 * time_outs may be NULL (no bootstrap). All pointers device; out_* are the rollout-storage slots of this step. */
int wbc_rollout_store(const float* rew, const float* arm_rew, const int64_t* dones, const uint8_t* time_outs,
                      const float* values, float gamma, float* out_rewards, uint8_t* out_dones, int n, void* stream);

/* OnPolicyRunner.learn's per-step episode bookkeeping (rsl_rl/runners/on_policy_runner.py:140-154: cur_reward_sum +=
 * rewards, cur_episode_length += 1, new_ids = (dones > 0).nonzero(), rewbuffer / armrewbuffer / lenbuffer.extend(...),
 * donebuffer.append(len(new_ids) / N), the sums of new_ids zeroed) in one launch and without the reference's three host
 * copies per env step. `state` (device f32, wbc_runner_track_state_floats(n, cap), zero-initialised by the caller):
 *   cur[n][3] running (reward, arm reward, length) | ring[cap][3] the last `cap` finished episodes in the order the
 *   reference's deques receive them (step by step, ascending env index) | done_ring[cap] the last `cap` per-step done
 *   fractions | 4 int32: ring head, ring fill (<= cap), done_ring head, done_ring fill.
 * cap = the deques' maxlen (100). The host reads ring / done_ring once per iteration. */
int wbc_runner_track_episodes(const float* rew, const float* arm_rew, const int64_t* dones, int n, int cap, float* state,
                              void* stream);
size_t wbc_runner_track_state_floats(int n, int cap);

/* Per-env shape (up to 3 dims; the leading N is implied), ndim and dtype (0 f32, 1 i64, 2 u8) of tensor `id`, without a sim. */
int wbc_tensor_spec(int id, int64_t* dims3, int* ndim, int* dtype);

/* sizeof(wbc_model), sizeof(wbc_task_cfg), sizeof(wbc_curriculum): lets a binding check its mirrors. */
void wbc_abi_sizes(int* out3);

/* LeggedRobot._get_heights (legged_gym/envs/base/legged_robot.py:793-829): terrain height under num_points points around
 * every robot -- points rotated by the base yaw (utils/math.py:38-42) and offset by the base position, `+= border_size`,
 * `(p / horizontal_scale).long()` (toward zero), clip to [0, dim-2], min of the three corner samples, * vertical_scale.
 * Bit-exact against oracle/terrain_oracle.py (integer / index work; the divisor is applied as PyTorch's CUDA kernel does:
 * multiplication by the fp32 reciprocal). base_quat: device f32 rows of (x,y,z,w), quat_stride floats apart; root_pos:
 * device f32 rows starting with (x,y), pos_stride floats apart (root_states: 13); height_points: device f32 [N,P,3];
 * height_samples: device int16 [rows,cols]; out: device f32 [N,P]. */
int wbc_get_heights(const float* base_quat, int quat_stride, const float* root_pos, int pos_stride, const float* height_points,
                    const int16_t* height_samples, int rows, int cols, float border_size, float horizontal_scale,
                    float vertical_scale, float* out, int num_envs, int num_points, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WBC_SIM_H */
