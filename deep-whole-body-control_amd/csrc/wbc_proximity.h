// wbc_proximity.h -- what the host side of wbc_sim_proximity (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_proximity_kernel.hip) share: the kernel's argument struct and its launcher.
#pragma once
#include "wbc_tree.h"

#define PX_MAXP 64                              // pairs per env: one lane each
#define PX_MAXBOX 8                             // sphere-box pairs among them
#define PX_FT 16                                // floats per body: E 0..8, p 9..11, axis 12..14
struct ProxConst : TreeWalk {
  uint32_t anc[WBC_NB];
  int32_t npairs;
  int32_t pair[PX_MAXP];                        // kind | a << 8 | b << 16: WBC_PR_LIMBS (limb ids) or WBC_PR_STATIC (a: index into the sb_ tables)
  int32_t limb_body[WBC_NLIMB], end_body[WBC_NLIMB][2];
  // how an end's body hangs on its limb's body, kind | k << 4: 0 the same body; 1 an ancestor, path[limb_body][k]; 2 a descendant with
  // path[end_body][k] = limb_body; 3 neither (the difference of the two origins)
  int32_t end_link[WBC_NLIMB][2];
  float end_pos[WBC_NLIMB][2][3], limb_rad[WBC_NLIMB][3];   // the ends in their own bodies' frames; shaft, end-0 and end-1 radii
  int32_t sb_body[PX_MAXBOX];
  float sb_pos[PX_MAXBOX][3], sb_rad[PX_MAXBOX], sb_centre[PX_MAXBOX][3], sb_half[PX_MAXBOX][3];
};

// One launch of wbc_proximity_kernel on `stream`, one workgroup per env; outputs as wbc_sim_proximity's, NULL: not written.
void wbc_proximity_launch(const ProxConst& K, const float* root, const float* dofs, int n, float* gap, float* normal, float* witness, float* jac,
                          int32_t* nearest, int k_nearest, void* stream);
