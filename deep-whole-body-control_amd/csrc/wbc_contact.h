// wbc_contact.h -- what the host side of wbc_sim_contact_detect (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_contact_kernel.hip) share: the kernel's argument struct and its launcher.
#pragma once
#include "wbc_estimator.h"

#ifndef CT_EPW
#define CT_EPW 16                               // envs per wavefront: lane = (env, foot). 2 builds the variant it was measured against, the
#endif                                          // estimator's layout: the feet on lanes 0..3 of each 32-lane group
#define CT_LPE (64 / CT_EPW)                    // lanes per env
#define CT_LEG_JOINTS 3                         // actuated joints between the trunk and a foot (the host refuses any other model)

// The legs as the estimator walks them: EstConst (TreeWalk, foot_body, foot_off; gravity is not read).
// dofs / quat / pos: the caller's tensors or the sim's, with their strides in floats; every other pointer as wbc_sim_contact_detect's
// (NULL: as documented there).
struct CtArgs {
  const float *dofs, *quat, *pos, *tau_ext, *foot_force, *normal, *ground, *phase, *p_init;
  const int32_t* reset_mask;
  int32_t quat_stride, pos_stride, tau_stride, phase_stride, reset_all, n;
  float *state, *prob;
  uint8_t *contact, *stance;
  float *force, *terms;
  int32_t* info;
};

// One launch of wbc_contact_detect_kernel on `stream`, CT_EPW envs per 64-lane workgroup.
void wbc_contact_launch(const EstConst& K, const wbc_contact_cfg& cfg, const CtArgs& a, void* stream);
