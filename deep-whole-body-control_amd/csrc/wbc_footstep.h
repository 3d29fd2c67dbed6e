// wbc_footstep.h -- what the host side of wbc_sim_footstep_plan (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_footstep_kernel.hip) share: the kernel's argument structs and its launcher.
#pragma once
#include "wbc_estimator.h"

#ifndef FS_LPF
#define FS_LPF 0                                // lanes per foot in the terrain search. 0: by the candidate count (16 lanes per foot and the four feet at
#endif                                          // once up to 16 candidates, else 64 and the feet in sequence); 16 / 64 build the variants it was measured against

// The legs as the estimator walks them (EstConst: TreeWalk, foot_body, foot_off, gravity) and the terrain as the step kernel queries it.
struct FsConst : EstConst {
  const int16_t* hf;                            // NULL: the plane z = ground_z
  int32_t hf_rows, hf_cols;
  float hf_hs, hf_vs, hf_t[3], ground_z;
  float k_c;                                    // (1/2) sqrt(com_height / |g|), 0 where |g| = 0
};
// root / dofs: the sim's tensors; every other pointer as wbc_sim_footstep_plan's (NULL: as documented there), pos / vel / quat with their
// strides in floats.
struct FsArgs {
  const float *root, *dofs, *pos, *vel, *quat, *vel_cmd, *yaw_rate, *phase_init;
  const int32_t* reset_mask;
  int32_t pos_stride, vel_stride, quat_stride, reset_all, hold, n;
  float* state;
  uint8_t *stance, *schedule;
  float *contact, *foot_pos, *foothold, *swing_ref, *swing_acc;
  int32_t* info;
};

// One launch of wbc_footstep_plan_kernel on `stream`, one env per 64-lane workgroup.
void wbc_footstep_launch(const FsConst& K, const wbc_footstep_cfg& cfg, const FsArgs& a, void* stream);
