// wbc_mpc.h -- what the host side of wbc_sim_centroidal_mpc (wbc_arm_kernel.hip, with the other whole-body entry points) and its kernel
// (wbc_mpc_kernel.hip) share: the kernel's argument structs and its launcher.
#pragma once
#include "wbc_tree.h"

#define MPC_NX 12                               // (theta, p, omega, v)
#define MPC_NU 12                               // four foot forces
#define MPC_NZ 20                               // five cone rows per foot
#define MPC_HMAX WBC_MPC_MAX_HORIZON
#ifndef MPC_EPW
#define MPC_EPW 1                               // envs per wavefront; 2 (one per 32-lane group) builds the variant it was measured against
#endif
#define MPC_LPE (64 / MPC_EPW)
// LDS pitches in floats, odd: lane = row reads of a column and lane = column reads of a row both meet distinct banks
#define MPC_PM 13                               // the 12 x 12 work matrices
#define MPC_PK 25                               // [K_k | G_k^-1], 12 x 24
#define MPC_STAGE_BYTES 1780                    // dynamic LDS per env and stage (wbc_mpc_kernel.hip: MpcStage)
#define MPC_CM_COM 9                            // wbc_centroidal_kernel's com and inertia rows, as they lie in the workspace
#define MPC_CM_INR 7

struct MpcConst : TreeWalk {
  int32_t foot_body[WBC_NFEET];                 // the moving body each foot rides on
  float foot_off[WBC_NFEET][3];                 // the foot's origin in that body's frame
  float gravity[3];
};
// root / dofs: the sim's tensors; com / inr: wbc_centroidal_kernel's outputs in the workspace (NULL where not needed); every other pointer as
// wbc_sim_centroidal_mpc's.
struct MpcArgs {
  const float *root, *dofs, *com, *inr, *x0, *mass, *inertia, *foot_pos, *x_ref;
  const uint8_t* contact;
  float *warm, *forces, *u, *x_pred, *base_acc, *res;
  int32_t* status;
  int32_t foot_pos_stages, flags, n;
};

// One launch of wbc_centroidal_mpc_kernel on `stream`, MPC_EPW envs per 64-lane workgroup.
void wbc_mpc_launch(const MpcConst& K, const wbc_mpc_cfg& cfg, const MpcArgs& a, void* stream);
