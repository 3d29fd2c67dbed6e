// wbc_slip.h -- what the host side of wbc_sim_slip_detect (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_slip_kernel.hip) share: the kernel's argument struct and its launcher.
#pragma once
#include "wbc_estimator.h"

#ifndef SL_EPW
#define SL_EPW 16                               // envs per wavefront: 16: lane = (env, foot), the contact detector's mapping; 64 builds the
#endif                                          // variant it was measured against: lane = env, the four legs walked in sequence
#define SL_LPE (64 / SL_EPW)                    // lanes per env: 4 or 1
#define SL_FPL (WBC_NFEET / SL_LPE)             // feet per lane: 1 or 4
#define SL_LEG_JOINTS 3                         // actuated joints between the trunk and a foot (the host refuses any other model)
static_assert(SL_EPW == 16 || SL_EPW == 64, "SL_EPW is 16 (lane = (env, foot)) or 64 (lane = env)");

// The legs as the estimator walks them: EstConst (TreeWalk, foot_body, foot_off; gravity is not read).
// dofs / quat / vel / ang: the caller's tensors or the sim's, with their strides in floats; ang_world: ang is in world axes (the sim's)
// and is turned into trunk axes in the kernel. Every other pointer as wbc_sim_slip_detect's (NULL: as documented there).
struct SlArgs {
  const float *dofs, *quat, *vel, *ang, *contact, *foot_force, *normal, *mu_init;
  const int32_t* reset_mask;
  int32_t quat_stride, vel_stride, ang_stride, ang_world, reset_all, n;
  float *state, *prob;
  uint8_t* slip;
  float *weight, *foot_vel, *speed, *distance, *mu, *mu_lower, *mu_env;
  int32_t* info;
};

// One launch of wbc_slip_detect_kernel on `stream`, SL_EPW envs per 64-lane workgroup.
void wbc_slip_launch(const EstConst& K, const wbc_slip_cfg& cfg, const SlArgs& a, void* stream);
