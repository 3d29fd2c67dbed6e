// wbc_policy_kernel.hip -- fused ActorCritic inference for the rollout (gfx950, fp32 MFMA).
//
// Replaces, per policy step, the ~60 eager launches of PPO.act (reference rsl_rl/algorithms/ppo.py:115-127:
// Actor.forward AC:204-217 with the privileged latent, Critic.forward AC:281-286, Normal.sample,
// get_actions_log_prob AC:341-345) by ONE launch on the register-chain layout of wbc_chain_fwd.h (the forward half of the PPO
// update's chain kernel): no LDS, no barrier, every activation of a 16-row tile in the registers of ONE wavefront.
//
// Work unit = (16-row tile, head chain), four kinds:
//   actor-leg   priv0, priv2, backbone, leg0, leg2, leg4      (832 MFMAs)        -> mean / actions [:, 0:12], logp[:, 0]
//   actor-arm   the same trunk, then arm0, arm2, arm4                             -> mean / actions [:, 12:18], logp[:, 1]
//   critic-leg  cbb, cleg0, cleg2, cleg4                        (768 MFMAs)        -> values[:, 0]
//   critic-arm  cbb, carm0, carm2, carm4                                           -> values[:, 1]
// The dependent chain of a wave is six (four) layers deep with no per-layer fixed cost; the price is the trunk computed twice per
// part (19 % more MFMAs than one chain through both heads). A 256-thread workgroup is four consecutive tiles of ONE kind: its
// four waves (one per SIMD) walk the same weight stream side by side, so a 1-KB element is fetched from L2 once per CU and
// found in the vector cache by the other three (tools/micro/l2_stream.hip). 4096 rows = 1024 units = 256 workgroups. The
// actor kinds are dispatched first. The epilogue -- tanh, sampling from pre-drawn standard normals, the log-density sums
// (12 leg / 6 arm dims) -- runs in the registers the head's MFMAs left their results in: lane (g, n) holds features 4 g + r of row n.
//
// Weights: wbc_policy_pack writes four forward-only streams, one per kind, in consumption order (pairs of out-blocks with
// interleaved k-groups, then the two bias quadruples), zero-padded so that the backbone and the head chain start at a multiple
// of the ring depth. With a given latent (the student path) an actor unit starts its ring at the backbone segment.
//
// Summation order: the rollout's numbers are those of the 16-row LDS kernel this one replaced, bit for bit (the env step is
// chaotic: a last-bit change of an action is another trajectory after a few hundred steps). That kernel summed an output over
// its inputs on ONE accumulator from 0, k-step (c, j) = 8 c + j ascending, slot g of a step standing for input 32 c + 8 g + j,
// then added the bias. The register chain is free in two places and both are spent on this: which feature row m of out-block b
// stands for, pol_feat(b, m) = 32 (b >> 1) + 8 (m >> 2) + 4 (b & 1) + (m & 3), makes register i of in-block q on the lane groups
// g = 0..3 exactly the inputs of k-step c = q >> 1, j = 4 (q & 1) + i, so a layer walks its in-blocks and registers in their
// natural order; the observation columns are gathered in the same pattern. Steps whose weights are all zero padding are left
// out (they add +0). The heads run on one accumulator, and the log-density sums follow the old kernel's 16-lane butterfly.
#include "wbc_chain_fwd.h"
#include "wbc_stats.h"
#include "wbc_stream_guard.h"

enum { K_ALEG = 0, K_AARM = 1, K_CLEG = 2, K_CARM = 3, POL_NKIND = 4 };
#define POL_MAXSEG 10
#define POL_PRIV_ELEM 22                        // priv0: 4 blocks x (2 k-groups + bias), priv2: 2 blocks x (4 k-groups + bias)
#define POL_PAD_PRIV ((CH_D - POL_PRIV_ELEM % CH_D) % CH_D)
#define POL_BB_ELEM (POL_PRIV_ELEM + POL_PAD_PRIV)          // stream element an actor kind's backbone starts at (a multiple of CH_D)
static_assert(POL_BB_ELEM % CH_D == 0 && (64 + CH_PAD_BB) % CH_D == 0, "looped bodies start ring-aligned");
// the two actor streams have nelem_a elements each, the two critic streams nelem_c; kind k at float offset pol_base(k)
struct PolStreams { ChainSeg s[POL_NKIND][POL_MAXSEG]; int nseg[POL_NKIND], nelem_a, nelem_c; };

static PolStreams make_pol_streams() {
  PolStreams t;
  for (int k = 0; k < POL_NKIND; ++k) {
    int n = 0, pos = 0;
    auto seg = [&](int layer, int kind, int nblk, int ngrp) {
      t.s[k][n++] = ChainSeg{pos, layer, kind, nblk, ngrp};
      pos += chain_seg_elems(kind, nblk, ngrp);
    };
    const bool critic = k >= K_CLEG, arm = (k & 1) != 0;
    if (!critic) { seg(L_PRIV0, SEG_FWD, 4, 2); seg(L_PRIV2, SEG_FWD, 2, 4); seg(-1, SEG_PAD, POL_PAD_PRIV, 0); }       // 12 + 10 (+ pad)
    seg(critic ? L_CBB : L_BB, SEG_FWD, 8, 7); seg(-1, SEG_PAD, CH_PAD_BB, 0);                                           // 64 (+ pad)
    const int h0 = critic ? (arm ? L_CARM0 : L_CLEG0) : (arm ? L_ARM0 : L_LEG0);
    seg(h0, SEG_FWD, 8, 8); seg(h0 + 1, SEG_FWD, 8, 8); seg(h0 + 2, SEG_FWD, 1, 8);                                      // 153
    seg(-1, SEG_PAD, CH_D, 0);                    // the ring reads CH_D elements past the last one consumed
    t.nseg[k] = n;
    (critic ? t.nelem_c : t.nelem_a) = pos;
  }
  return t;
}
static const PolStreams& pol_streams() { static const PolStreams t = make_pol_streams(); return t; }
static __host__ __device__ __forceinline__ int pol_base(int kind, int nelem_a, int nelem_c) {
  return (kind < K_CLEG ? kind * nelem_a : 2 * nelem_a + (kind - K_CLEG) * nelem_c) * 256;
}

// the feature that row m of out-block b stands for, and the input that slot g of register i of in-block q stands for
static __host__ __device__ __forceinline__ int pol_feat(int b, int m) { return 32 * (b >> 1) + 8 * (m >> 2) + 4 * (b & 1) + (m & 3); }
// output feature of row m of out-block b of `layer` (-1: none). priv2's 20 outputs sit where the backbone wants its inputs
// 76..95 (pol_feat - 76 of the blocks 4 and 5); a head's (one block) in natural order for the epilogue.
static __device__ __forceinline__ int pol_out_feat(int layer, int nblk, int b, int m) {
  const int N = layer_out(layer);
  if (nblk == 1) return m < N ? m : -1;
  if (layer == L_PRIV2) { const int u = pol_feat(4 + b, m) - PT_NPROP; return (u >= 0 && u < N) ? u : -1; }
  return pol_feat(b, m);
}
// float i of lane `lane` of element `rel` of the SEG_FWD segment sg (the element order of chain_fwd_slot_source: pairs of
// out-blocks with alternating elements, a single block in k order, the bias quadruples last)
static __device__ __forceinline__ ChainSrc pol_slot_source(const ChainSeg& sg, int rel, int lane, int i) {
  const int g = lane >> 4, m = lane & 15;
  ChainSrc r{-1, 0, 0, sg.kind};
  const int K = layer_in(sg.layer);
  int blk, kq;
  if (sg.nblk == 1) { blk = 0; kq = rel; }
  else { const int pe = 2 * (sg.ngrp + 1), pr = rel / pe, r2 = rel - pr * pe; blk = 2 * pr + (r2 & 1); kq = r2 >> 1; }
  if (kq == sg.ngrp) {
    const int o = pol_out_feat(sg.layer, sg.nblk, blk, 4 * g + i);
    if (o >= 0) { r.layer = sg.layer; r.bias = 1; r.idx = o; }
  } else {
    const int o = pol_out_feat(sg.layer, sg.nblk, blk, m), c = pol_feat(kq, 4 * g + i);       // priv0's inputs are x[76 + c], the backbone's [prop, latent][c]
    if (o >= 0 && c < K) { r.layer = sg.layer; r.idx = o * K + c; }
  }
  return r;
}

// Head layer (one out-block, no activation) on ONE accumulator in k order. The builtin, not ch_mfma8: the compiler places the
// waits a dependent chain and the read of its result need.
template <int NKG, int POS0>
static __device__ __forceinline__ f32x4 pol_head(ChainRing& R, const f32x4* bin) {
  f32x4 acc = CH_Z4;
#pragma unroll
  for (int kq = 0; kq < NKG; ++kq) {
    const f32x4 w = R.take((POS0 + kq) % CH_D);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], bin[kq][i], acc, 0, 0, 0);
  }
  const f32x4 b = R.take((POS0 + NKG) % CH_D);
  return acc + b;
}

// grid = (blocks, 4 kinds), one thread per (element, lane): a float4 of the stream.
static __global__ void __launch_bounds__(256) policy_pack_kernel(PolicyParams P, PolStreams S, float* __restrict__ pack) {
  const int k = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int el = t >> 6;
  if (el >= (k < K_CLEG ? S.nelem_a : S.nelem_c)) return;
  const ChainSeg sg = chain_find_seg(S.s[k], S.nseg[k], el);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ChainSrc r{-1, 0, 0, sg.kind};
    if (sg.kind == SEG_FWD) r = pol_slot_source(sg, el - sg.start, t & 63, i);
    v[i] = r.layer < 0 ? 0.f : reinterpret_cast<const float* const*>(&P)[2 * r.layer + r.bias][r.idx];
  }
  reinterpret_cast<float4*>(pack + pol_base(k, S.nelem_a, S.nelem_c))[t] = make_float4(v[0], v[1], v[2], v[3]);
}

struct PolLaunch { int nelem_a, nelem_c, groups, tiles, num_rows; };      // groups: workgroups per kind = ceil(tiles / 4)

extern "C" __global__ void __launch_bounds__(PT_THREADS, 2) wbc_policy_act16_kernel(const float* __restrict__ pack, PolLaunch Q, const float* __restrict__ stdp,
                                                                                    const float* __restrict__ obs, const float* __restrict__ latent,
                                                                                    const float* __restrict__ eps, float* __restrict__ actions,
                                                                                    float* __restrict__ mean_out, float* __restrict__ logp_out,
                                                                                    float* __restrict__ value_out, wbc_side_job job) {
  // workgroups past the unit workgroups carry a side job (the env step's episode statistics: wbc_stats.h) next to the inference
  if ((int)blockIdx.x >= POL_NKIND * Q.groups) {
    side_job_block<PT_THREADS>(job, (int)blockIdx.x - POL_NKIND * Q.groups);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int kind = (int)blockIdx.x / Q.groups;                                     // workgroup-uniform
  const int tile = ((int)blockIdx.x - kind * Q.groups) * (PT_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (tile >= Q.tiles) return;                                                      // (no barrier anywhere below: a wave may leave alone)
  const bool critic = kind >= K_CLEG, arm = (kind & 1) != 0, student = latent != nullptr;
  const int g = lane >> 4, n = lane & 15;
  const int row = tile * R16 + n;
  const bool live = row < Q.num_rows;
  const size_t rc = (size_t)(live ? row : Q.num_rows - 1);       // a dead row re-reads the last live one; its MFMA column never reaches another row
  // the ring: an actor unit that is given the latent skips priv0 / priv2 and starts at the backbone
  const int first = (!critic && student) ? POL_BB_ELEM : 0;
  ChainRing R;
  R.init(pack + pol_base(kind, Q.nelem_a, Q.nelem_c) + first * 256, ((critic ? Q.nelem_c : Q.nelem_a) - first) * 1024, lane);
  // x = obs[row, :100]: register i of block q holds column pol_feat(q, 4 g + i) = 32 (q >> 1) + 8 g + 4 (q & 1) + i
  f32x4 zin[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const int c = pol_feat(q, 4 * g);
    f32x4 v = *reinterpret_cast<const f32x4*>(obs + rc * PT_NOBS + (c < 100 ? c : 0));
    if (c >= 100) v = CH_Z4;
    zin[q] = v;
  }
  // the epilogue's per-row inputs, requested a whole chain ahead of their use: lane (g, n) owns the action dims j0 + 4 g + r of row n
  const int w = arm ? PT_NARM : PT_NLEG, j0 = arm ? PT_NLEG : 0;
  float ep[4], sd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + (4 * g + r < w ? 4 * g + r : 0);
    sd[r] = critic ? 1.f : stdp[j];
    ep[r] = (critic || !eps) ? 0.f : eps[rc * 18 + j];
  }
  if (!critic) {
    // the backbone's input is [prop (76), latent (20)]: the columns 76.. of the blocks 4 (lane groups 2, 3) and 5 (1..3) are the
    // latent, block 6 (96..) is zero. Nothing privileged stays in zin: the columns need not be finite on the student path
    f32x4 l0, l1;
    if (!student) {
      f32x4 xp[2], h1[4], lat[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {               // priv0's input: x[76 + pol_feat(q, 4 g + i)], 24 columns (lane group 3: none)
        xp[q] = *reinterpret_cast<const f32x4*>(obs + rc * PT_NOBS + PT_NPROP + (g < 3 ? 8 * g + 4 * q : 0));
        if (g == 3) xp[q] = CH_Z4;
      }
      chain_fwd<4, 2, 0, false>(R, xp, h1, R.rs, 0, 0);
      chain_fwd<2, 4, 12 % CH_D, false>(R, h1, lat, R.rs, 0, 0);
#pragma unroll
      for (int s = 0; s < POL_PAD_PRIV; ++s) (void)R.take((POL_PRIV_ELEM + s) % CH_D);
      l0 = lat[0]; l1 = lat[1];
    } else {
      l0 = *reinterpret_cast<const f32x4*>(latent + rc * 20 + (g >= 2 ? 8 * g - 12 : 0));
      l1 = *reinterpret_cast<const f32x4*>(latent + rc * 20 + (g >= 1 ? 8 * g - 8 : 0));
    }
    if (g >= 2) zin[4] = l0;
    if (g >= 1) zin[5] = l1;
    zin[6] = CH_Z4;
  }
  // backbone (actor: [prop, latent] -> 128; critic: x -> 128): the same code, the stream holds the part's weights
  f32x4 hbb[8];
  chain_fwd<8, 7, 0, false>(R, zin, hbb, R.rs, 0, 0);
#pragma unroll
  for (int s = 0; s < CH_PAD_BB; ++s) (void)R.take((64 + s) % CH_D);
  // the unit's head: 128 -> 128 -> 128 -> (12 | 6 | 1 | 1)
  f32x4 a1[8], a2[8];
  chain_fwd<8, 8, 0, false>(R, hbb, a1, R.rs, 0, 0);
  chain_fwd<8, 8, 72 % CH_D, false>(R, a1, a2, R.rs, 0, 0);
  const f32x4 o = pol_head<8, 144 % CH_D>(R, a2);
  if (critic) {
    if (g == 0 && live) value_out[(size_t)row * 2 + (arm ? 1 : 0)] = o[0];        // the head's single output: feature 0 = (g 0, r 0)
    return;
  }
  // sampling and log-probabilities. The sum over a part's dims is the tree of the old kernel's 16-lane butterfly (lane c = dim c
  // and 16 + c, xor 8, 4, 2, 1): dim 4 g + i first over the lane groups, (g0 + g2) + (g1 + g3), then (i0 + i2) + (i1 + i3).
  float lp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool ok = 4 * g + r < w;
    const float mu = tanhf(o[r]);
    const float a = mu + sd[r] * ep[r];
    const float dd = a - mu;
    const float term = -(dd * dd) / (2.f * sd[r] * sd[r]) - logf(sd[r]) - 0.91893853320467274178f;
    float t = ok ? term : 0.f;
    t += __shfl_xor(t, 32); t += __shfl_xor(t, 16);
    lp[r] = t;
    if (ok && live) {
      const size_t at = (size_t)row * 18 + j0 + 4 * g + r;
      actions[at] = a; mean_out[at] = mu;
    }
  }
  const float lps = (lp[0] + lp[2]) + (lp[1] + lp[3]);
  if (g == 0 && live) logp_out[(size_t)row * 2 + (arm ? 1 : 0)] = lps;
}


static int fill_params(const void* const* params, PolicyParams* P) {
  const float** dst = reinterpret_cast<const float**>(P);
  for (int i = 0; i < 33; ++i) {
    if (!params[i]) return -1;
    dst[i] = static_cast<const float*>(params[i]);
  }
  return 0;
}

// C-ABI. params: 33 device pointers in the order of struct PolicyParams; wpack: wbc_policy_pack_floats() floats.
extern "C" int wbc_policy_pack_floats(void) { return 2 * (pol_streams().nelem_a + pol_streams().nelem_c) * 256; }

// Re-pack the weights into the four streams (call after the parameters changed).
extern "C" int wbc_policy_pack(const void* const* params, float* wpack, void* stream) {
  StreamDeviceGuard sdg(stream);
  PolicyParams P;
  if (!params || !wpack || (reinterpret_cast<uintptr_t>(wpack) & 15) || fill_params(params, &P)) return -1;
  const PolStreams& S = pol_streams();
  hipLaunchKernelGGL(policy_pack_kernel, dim3((S.nelem_a * 64 + 255) / 256, POL_NKIND), dim3(256), 0, (hipStream_t)stream, P, S, wpack);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int wbc_policy_act_job(const void* const* params, const float* wpack, const float* obs, const float* latent, const float* eps,
                                  float* actions, float* mean, float* logp, float* values, int num_rows, const wbc_side_job* job, void* stream) {
  StreamDeviceGuard sdg(stream);
  PolicyParams P;
  if (!params || !wpack || !obs || !actions || !mean || !logp || !values || num_rows <= 0 || fill_params(params, &P)) return -1;
  wbc_side_job J;
  if (job) J = *job; else { J = wbc_side_job(); J.nblocks = 0; }
  if (J.nblocks < 0 || (J.nblocks > 0 && !J.out)) return -1;
  const PolStreams& S = pol_streams();
  const int tiles = (num_rows + R16 - 1) / R16;
  const PolLaunch Q{S.nelem_a, S.nelem_c, (tiles + PT_THREADS / 64 - 1) / (PT_THREADS / 64), tiles, num_rows};
  hipLaunchKernelGGL(wbc_policy_act16_kernel, dim3(POL_NKIND * Q.groups + J.nblocks), dim3(PT_THREADS), 0, (hipStream_t)stream, wpack, Q, P.std, obs,
                     latent, eps, actions, mean, logp, values, J);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int wbc_policy_act(const void* const* params, const float* wpack, const float* obs, const float* latent, const float* eps,
                              float* actions, float* mean, float* logp, float* values, int num_rows, void* stream) {
  return wbc_policy_act_job(params, wpack, obs, latent, eps, actions, mean, logp, values, num_rows, nullptr, stream);
}
