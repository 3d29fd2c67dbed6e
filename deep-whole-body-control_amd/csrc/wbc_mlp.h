// wbc_mlp.h -- what the fused ActorCritic kernels share about the network itself (gfx950, fp32 MFMA): the parameter pointer
// table and the layer shapes, used by the rollout inference kernel (wbc_policy_kernel.hip) and the PPO update kernels
// (wbc_ppo_kernel.hip). How a layer chain is run on the matrix pipe is in wbc_chain_fwd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PT_THREADS 256
#define PT_NPROP 76
#define PT_NPRIV 24
#define PT_NOBS 860
#define PT_NLEG 12
#define PT_NARM 6
#define NLAYERS 16
#define R16 16              // rows of a tile (v_mfma_f32_16x16x4_f32)

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct PolicyParams {       // device pointers to the torch parameters (weight [out,in] row-major, bias [out])
  const float *priv0_w, *priv0_b, *priv2_w, *priv2_b;
  const float *bb_w, *bb_b;
  const float *leg0_w, *leg0_b, *leg2_w, *leg2_b, *leg4_w, *leg4_b;
  const float *arm0_w, *arm0_b, *arm2_w, *arm2_b, *arm4_w, *arm4_b;
  const float *cbb_w, *cbb_b;
  const float *cleg0_w, *cleg0_b, *cleg2_w, *cleg2_b, *cleg4_w, *cleg4_b;
  const float *carm0_w, *carm0_b, *carm2_w, *carm2_b, *carm4_w, *carm4_b;
  const float* std;         // [18]
};

// layer order = PolicyParams order
enum { L_PRIV0 = 0, L_PRIV2, L_BB, L_LEG0, L_LEG2, L_LEG4, L_ARM0, L_ARM2, L_ARM4, L_CBB, L_CLEG0, L_CLEG2, L_CLEG4, L_CARM0, L_CARM2, L_CARM4 };
__host__ __device__ constexpr int layer_out(int l) {
  return l == L_PRIV0 ? 64 : l == L_PRIV2 ? 20 : l == L_LEG4 ? 12 : l == L_ARM4 ? 6 : (l == L_CLEG4 || l == L_CARM4) ? 1 : 128;
}
__host__ __device__ constexpr int layer_in(int l) { return l == L_PRIV0 ? 24 : l == L_PRIV2 ? 64 : l == L_BB ? 96 : l == L_CBB ? 100 : 128; }
