// wbc_attitude.h -- what the host side of wbc_sim_attitude_filter (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_attitude_kernel.hip) share: the kernel's argument struct and its launcher.
#pragma once
#include "wbc_device.h"

#ifndef AT_EPW
#define AT_EPW 64                               // envs per wavefront: lane = env. 16 builds the variant it was measured against: the same lane
#endif                                          // = env code on lanes 0..15 of four times as many wavefronts, 48 lanes idle
#define AT_NM (1 + WBC_ATTITUDE_MAX_AUX)        // measurements of one call: the accelerometer and the aux entries

// root: the sim's ROOT_STATES (read only where gyro is NULL); up = -gravity / |gravity| and half, the half turn's axis, from the host;
// every other pointer as wbc_sim_attitude_filter's (NULL: as documented there).
struct AtArgs {
  const float *root, *gyro, *accel, *aux_body, *aux_world, *aux_sigma, *q_init;
  const int32_t* reset_mask;
  int32_t naux, reset_all, n;
  float up[3], half[3], gnorm;
  float *q, *b, *P, *gyro_out, *gravity_body, *nis;
  int32_t* status;
};

// One launch of wbc_attitude_filter_kernel on `stream`, AT_EPW envs per 64-lane workgroup.
void wbc_attitude_launch(const wbc_attitude_cfg& cfg, const AtArgs& a, void* stream);
