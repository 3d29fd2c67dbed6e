// wbc_ground.h -- what the host side of wbc_sim_ground_estimate (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_ground_kernel.hip) share: the kernel's argument struct and its launcher.
#pragma once
#include "wbc_estimator.h"

#ifndef GE_EPW
#define GE_EPW 16                               // envs per wavefront: 16: lane = (env, foot), the contact detector's mapping; 64 builds the
#endif                                          // variant it was measured against: lane = env, the four legs walked in sequence
#define GE_LPE (64 / GE_EPW)                    // lanes per env: 4 or 1
#define GE_FPL (WBC_NFEET / GE_LPE)             // feet per lane: 1 or 4
#define GE_LEG_JOINTS 3                         // actuated joints between the trunk and a foot (the host refuses any other model)
static_assert(GE_EPW == 16 || GE_EPW == 64, "GE_EPW is 16 (lane = (env, foot)) or 64 (lane = env)");

// The legs as the estimator walks them: EstConst (TreeWalk, foot_body, foot_off; gravity is not read).
// dofs / quat / pos: the caller's tensors or the sim's, with their strides in floats; every other pointer as wbc_sim_ground_estimate's
// (NULL: as documented there). nq is 0 where query_xy is NULL.
struct GeArgs {
  const float *dofs, *quat, *pos, *contact, *query_xy;
  const int32_t* reset_mask;
  int32_t quat_stride, pos_stride, reset_all, nq, n;
  float *state, *normal, *ground, *residual, *trunk, *theta_ref, *query_z;
  int32_t* info;
};

// One launch of wbc_ground_estimate_kernel on `stream`, GE_EPW envs per 64-lane workgroup.
void wbc_ground_launch(const EstConst& K, const wbc_ground_cfg& cfg, const GeArgs& a, void* stream);
