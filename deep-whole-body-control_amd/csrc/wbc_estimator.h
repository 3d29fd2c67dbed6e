// wbc_estimator.h -- what the host side of wbc_sim_leg_odometry (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_estimator_kernel.hip) share: the kernel's argument structs and its launcher.
#pragma once
#include "wbc_tree.h"

#define EST_NX 18                               // p, v and the four foot origins
#define EST_MAXM 28                             // 12 position rows, 12 velocity rows, 4 height rows
#ifndef EST_EPW
#define EST_EPW 2                               // envs per wavefront: one per 32-lane group; 1 builds the variant it was measured against
#endif
#define EST_LPE (64 / EST_EPW)
// LDS pitches in floats, odd: lane = row reads of a column and lane = column reads of a row both meet 32 distinct banks
#define EST_PP 19                               // P
#define EST_PW 19                               // C P- and then W, 18 columns, with the residual and then L^-1 e as column 18
#define EST_PS 29                               // S and then its factor L

struct EstConst : TreeWalk {
  int32_t foot_body[WBC_NFEET];                 // the moving body each foot rides on
  float foot_off[WBC_NFEET][3];                 // the foot's origin in that body's frame
  float gravity[3];
};
// root / dofs: the sim's tensors; every other input as wbc_sim_leg_odometry's (NULL: as documented there), quat with its stride in floats.
struct EstArgs {
  const float *root, *dofs, *quat, *gyro, *accel, *contact, *foot_height, *p_init;
  const int32_t* reset_mask;
  int32_t quat_stride, reset_all, n;
  float *x, *P, *vel_body, *nis;
  int32_t* status;
};

// One launch of wbc_leg_odometry_kernel on `stream`, EST_EPW envs per 64-lane workgroup.
void wbc_estimator_launch(const EstConst& K, const wbc_estimator_cfg& cfg, const EstArgs& a, void* stream);
