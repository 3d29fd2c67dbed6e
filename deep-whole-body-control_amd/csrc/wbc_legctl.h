// wbc_legctl.h -- what the host side of wbc_sim_leg_control (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_legctl_kernel.hip) share: the kernel's argument struct and its launcher.
#pragma once
#include "wbc_estimator.h"

#define LC_EPW 16                               // envs per wavefront: lane = (env, foot), the contact kernel's layout
#define LC_LPE (64 / LC_EPW)                    // lanes per env
#define LC_LEG_JOINTS 3                         // actuated joints between the trunk and a foot (the host refuses any other model)
#define LC_ARM_DOFS 6                           // DoFs that are in no leg and are not locked (the host refuses any other count)
#define LC_NLIMIT 18                            // entries per env of tau_limit

// The legs as the estimator walks them: EstConst (TreeWalk, foot_body, foot_off; gravity is not read).
// dofs / quat / pos / vel / ang: the caller's tensors or the sim's, with their strides in floats; every other pointer as
// wbc_sim_leg_control's (NULL: as documented there).
struct LcArgs {
  const float *dofs, *quat, *pos, *vel, *ang, *forces, *swing_ref, *stance, *tau_bias, *mass_matrix, *acc_bias, *arm_q_des, *tau_limit;
  int32_t quat_stride, pos_stride, vel_stride, ang_stride, bias_stride, mm_stride, acc_stride, clip, n;
  int32_t foot_rb[WBC_NFEET];                   // the rigid body of each foot: its row of acc_bias
  int32_t arm_dof[LC_ARM_DOFS];                 // the arm's DoFs in DoF order
  int32_t finger_dof[WBC_NDOF - WBC_NFEET * LC_LEG_JOINTS - LC_ARM_DOFS];   // the DoFs left over: their torque is written as 0
  int32_t limit_col[WBC_NDOF];                  // DoF -> its column of tau_limit, -1: none
  float *tau, *leg_force, *foot;
  int32_t* info;
};

// One launch of wbc_leg_control_kernel on `stream`, LC_EPW envs per 64-lane workgroup.
void wbc_legctl_launch(const EstConst& K, const wbc_leg_control_cfg& cfg, const LcArgs& a, void* stream);
