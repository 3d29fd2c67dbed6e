// wbc_chain_fwd.h -- the forward building blocks of the register-chain layout (gfx950, v_mfma_f32_16x16x4_f32), shared by the PPO
// update's chain kernel (wbc_ppo_chain.h: forward + loss + backward) and the rollout's policy inference (wbc_policy_kernel.hip:
// forward only).
//
// One WAVEFRONT owns 16 rows and runs a whole layer chain alone: no LDS, no barrier, nothing shared with the other waves of its
// workgroup. The GEMMs are computed TRANSPOSED: out^T[feature, row] = W[feature, k] * in^T[k, row]. The MFMA's A operand (16 x 4) is
// a weight fragment, its B operand (4 x 16) the activations, and the result D[m = 4 g + r][n] (lane = 16 g + n, register r)
// leaves lane (g, n) with features 16 j + 4 g + r of row n for out-block j. The B operand wants lane (g, n) to supply
// in^T[k-slot g][row n]: register r of out-block j IS a valid B operand for the k-step that stands for the features
// {16 j + 4 g + r : g = 0..3} -- the reduction order is free, the weights are packed to match. A layer's output registers are
// the next layer's input operands as they are: bias + activation happen in place, element-wise.
//
// Weights: one stream per chain, in consumption order, element = 64 lanes x float4 = the A operands of four consecutive MFMAs
// (or a bias quadruple): a wave walks its stream with a CH_D-element register ring, the address is a scalar pointer bumped by
// 1 KB per element.
#pragma once
#include "wbc_mlp.h"

#ifndef CH_D
#define CH_D 9                    // ring depth (stream elements in flight); must divide 153 (a head chain's forward elements)
#endif
// zero elements that bring the stream position back to a multiple of the ring depth in front of the looped bodies
#define CH_PAD_PRIV ((CH_D - 26 % CH_D) % CH_D)
#define CH_PAD_BB ((CH_D - 64 % CH_D) % CH_D)
static_assert(153 % CH_D == 0, "ring depth");

// ---- stream layout ----------------------------------------------------------------------------------------------------
enum { SEG_FWD = 0, SEG_BWD = 1, SEG_PAD = 2 };
struct ChainSeg { int start, layer, kind, nblk, ngrp; };       // SEG_FWD: per block ngrp weight elements + 1 bias element;
                                                                // SEG_BWD: per block ngrp weight elements; SEG_PAD: nblk zero elements
// elements a segment occupies
static inline int chain_seg_elems(int kind, int nblk, int ngrp) { return kind == SEG_FWD ? nblk * (ngrp + 1) : (kind == SEG_BWD ? nblk * ngrp : nblk); }

// which input column of W the k-step (group kq, component i) stands for on lane group g, forward layers (-1: none)
static __device__ __forceinline__ int chain_fwd_kcol(int layer, int kq, int g, int i) {
  const int t = 16 * kq + 4 * g + i;
  if (layer == L_PRIV0) { const int f = t + 64; return (f >= PT_NPROP && f < 100) ? f - PT_NPROP : -1; }      // x blocks 4..6: the privileged part
  if (layer == L_BB) { if (kq < 5) return t < PT_NPROP ? t : -1; const int u = t - 80; return u < 20 ? PT_NPROP + u : -1; }   // proprio from x, then the latent blocks
  return t < layer_in(layer) ? t : -1;
}

// Source of float i of a stream float4: parameter 2 l (weight) / 2 l + 1 (bias) of layer l and the element inside it, or
// layer -1 for a zero of the padding. kind: SEG_FWD / SEG_BWD of its segment.
struct ChainSrc { int layer, bias, idx, kind; };
// the segment of `n` (sorted by start) that holds stream element el
static __device__ __forceinline__ ChainSeg chain_find_seg(const ChainSeg* s, int n, int el) {
  int si = 0;
  while (si + 1 < n && s[si + 1].start <= el) ++si;
  return s[si];
}
// float i of lane `lane` of element `rel` of the SEG_FWD segment sg
static __device__ __forceinline__ ChainSrc chain_fwd_slot_source(const ChainSeg& sg, int rel, int lane, int i) {
  const int g = lane >> 4, m = lane & 15;
  ChainSrc r{-1, 0, 0, sg.kind};
  const int N = layer_out(sg.layer), K = layer_in(sg.layer);
  // blocks come in pairs (2 p, 2 p + 1) whose elements alternate: two independent accumulators per wave (a dependent
  // v_mfma_f32_16x16x4_f32 issues every 40 cycles, an independent one every 32); single-block layers (heads) keep k order
  int blk, kq;
  if (sg.nblk == 1) { blk = 0; kq = rel; }
  else { const int pe = 2 * (sg.ngrp + 1), pr = rel / pe, r2 = rel - pr * pe; blk = 2 * pr + (r2 & 1); kq = r2 >> 1; }
  if (kq == sg.ngrp) {                                   // bias quadruple of lane group g: features 16 blk + 4 g + i
    const int o = 16 * blk + 4 * g + i;
    if (o < N) { r.layer = sg.layer; r.bias = 1; r.idx = o; }
  } else {
    const int o = 16 * blk + m, c = chain_fwd_kcol(sg.layer, kq, g, i);
    if (o < N && c >= 0) { r.layer = sg.layer; r.idx = o * K + c; }
  }
  return r;
}

// ---- the ring ---------------------------------------------------------------------------------------------------------
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
#define CH_RSRC_FLAGS 0x00020000          // raw buffer, 32-bit data format (gfx9 family)
// Ring loads are pinned where they are written (the scheduler otherwise sinks each load to its use, nine elements later)
#define CH_PIN() __builtin_amdgcn_sched_barrier(0)
struct ChainRing {
  f32x4 r[CH_D];
  __amdgpu_buffer_rsrc_t rs;  // the part's stream
  int so;                     // uniform: byte offset of the element the next load fetches
  int loff;                   // lane * 16
  __device__ __forceinline__ void init(const float* stream, int bytes, int lane) {
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(stream), 0, bytes, CH_RSRC_FLAGS);
    so = 0; loff = lane * 16;
#pragma unroll
    for (int s = 0; s < CH_D; ++s) { r[s] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, loff, so, 0)); so += 1024; }
    CH_PIN();
  }
  // the element at ring slot `slot` (a compile-time constant after unrolling); its slot is refilled from the stream head
  __device__ __forceinline__ f32x4 take(int slot) {
    const f32x4 v = r[slot];
    r[slot] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, loff, so, 0));
    so += 1024;
    CH_PIN();
    return v;
  }
};

// stash accesses: buffer resource of the whole stash, per-lane byte offset, uniform slab offset (bytes), small immediate
static __device__ __forceinline__ f32x4 ch_ld4(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
}
static __device__ __forceinline__ void ch_st4(__amdgpu_buffer_rsrc_t rs, int voff, int soff, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, voff, soff, 0);
}
// 8 MFMAs on two independent accumulators, strictly alternating (one asm statement: the compiler neither reorders them nor
// renames an accumulator in mid-chain, which costs hazard nops). A dependent v_mfma_f32_16x16x4_f32 issues every 40 cycles,
// alternating chains every 32. FIRST: the accumulators start from 0. The compiler does not see the matrix pipe's result
// latency through an asm statement: results are read CH_MFMA_SETTLE() or >= 8 further MFMAs later.
template <bool FIRST>
static __device__ __forceinline__ void ch_mfma8(const f32x4 w0, const f32x4 w1, const f32x4 b0, const f32x4 b1, f32x4& a0, f32x4& a1) {
  if (FIRST)
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %2, %10, 0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %6, %14, 0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %3, %11, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %7, %15, %1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %4, %12, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %8, %16, %1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %5, %13, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %9, %17, %1"
                 : "=&v"(a0), "=&v"(a1)
                 : "v"(w0[0]), "v"(w0[1]), "v"(w0[2]), "v"(w0[3]), "v"(w1[0]), "v"(w1[1]), "v"(w1[2]), "v"(w1[3]),
                   "v"(b0[0]), "v"(b0[1]), "v"(b0[2]), "v"(b0[3]), "v"(b1[0]), "v"(b1[1]), "v"(b1[2]), "v"(b1[3]));
  else
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %2, %10, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %6, %14, %1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %3, %11, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %7, %15, %1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %4, %12, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %8, %16, %1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %5, %13, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %1, %9, %17, %1"
                 : "+v"(a0), "+v"(a1)
                 : "v"(w0[0]), "v"(w0[1]), "v"(w0[2]), "v"(w0[3]), "v"(w1[0]), "v"(w1[1]), "v"(w1[2]), "v"(w1[3]),
                   "v"(b0[0]), "v"(b0[1]), "v"(b0[2]), "v"(b0[3]), "v"(b1[0]), "v"(b1[1]), "v"(b1[2]), "v"(b1[3]));
}
// 16 wait states: an 8-pass MFMA result is readable by the vector ALU / as an MFMA A/B operand 11 states after its issue
#define CH_MFMA_SETTLE() asm volatile("s_nop 7\n\ts_nop 7" ::: "memory")
static __device__ __forceinline__ float ch_elu(float x) {       // branch-free; exp via v_exp_f32 (+inf for large x: not selected)
  const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f) - 1.f;
  return x > 0.f ? x : e;
}
static __device__ __forceinline__ f32x4 ch_elu4(f32x4 a, f32x4 b) {
  return (f32x4){ch_elu(a[0] + b[0]), ch_elu(a[1] + b[1]), ch_elu(a[2] + b[2]), ch_elu(a[3] + b[3])};
}
#define CH_Z4 ((f32x4){0.f, 0.f, 0.f, 0.f})

// Forward layer: out[ob] = ELU(W in + b) for NOB (even) out-blocks over NKG k-groups, two blocks at a time; POS0 = ring
// position (mod CH_D) of its first element. STASH: the output goes to the activation slab at (uniform byte offset soff) +
// (lane offset voff) + 64 ob. The epilogue of a pair runs after the next pair's MFMAs were issued (the matrix pipe's result
// latency is not waited for).
template <int NOB, int NKG, int POS0, bool STASH>
static __device__ __forceinline__ void chain_fwd(ChainRing& R, const f32x4* bin, f32x4* out, __amdgpu_buffer_rsrc_t ars, int voff, int soff) {
  static_assert(NOB % 2 == 0, "pairs of out-blocks");
  constexpr int PE = 2 * (NKG + 1);
  f32x4 bp0 = CH_Z4, bp1 = CH_Z4;
#pragma unroll
  for (int p = 0; p < NOB / 2; ++p) {
    f32x4 a0, a1;
#pragma unroll
    for (int kq = 0; kq < NKG; ++kq) {
      const f32x4 w0 = R.take((POS0 + p * PE + 2 * kq) % CH_D), w1 = R.take((POS0 + p * PE + 2 * kq + 1) % CH_D);
      if (kq == 0) ch_mfma8<true>(w0, w1, bin[kq], bin[kq], a0, a1);
      else ch_mfma8<false>(w0, w1, bin[kq], bin[kq], a0, a1);
    }
    out[2 * p] = a0; out[2 * p + 1] = a1;
    const f32x4 b0 = R.take((POS0 + p * PE + 2 * NKG) % CH_D), b1 = R.take((POS0 + p * PE + 2 * NKG + 1) % CH_D);
    if (p > 0) {
      out[2 * p - 2] = ch_elu4(out[2 * p - 2], bp0);
      out[2 * p - 1] = ch_elu4(out[2 * p - 1], bp1);
      if (STASH) { ch_st4(ars, voff + 64 * (2 * p - 2), soff, out[2 * p - 2]); ch_st4(ars, voff + 64 * (2 * p - 1), soff, out[2 * p - 1]); }
    }
    bp0 = b0; bp1 = b1;
  }
  CH_MFMA_SETTLE();
  out[NOB - 2] = ch_elu4(out[NOB - 2], bp0);
  out[NOB - 1] = ch_elu4(out[NOB - 1], bp1);
  if (STASH) { ch_st4(ars, voff + 64 * (NOB - 2), soff, out[NOB - 2]); ch_st4(ars, voff + 64 * (NOB - 1), soff, out[NOB - 1]); }
}

// Head layer (one out-block, no activation): the k-groups alternate between two accumulators. NKG even, NKG + 1 elements.
template <int NKG, int POS0>
static __device__ __forceinline__ f32x4 chain_head(ChainRing& R, const f32x4* bin) {
  static_assert(NKG % 2 == 0, "pairs of k-groups");
  f32x4 a0, a1;
#pragma unroll
  for (int kq = 0; kq < NKG; kq += 2) {
    const f32x4 w0 = R.take((POS0 + kq) % CH_D), w1 = R.take((POS0 + kq + 1) % CH_D);
    if (kq == 0) ch_mfma8<true>(w0, w1, bin[kq], bin[kq + 1], a0, a1);
    else ch_mfma8<false>(w0, w1, bin[kq], bin[kq + 1], a0, a1);
  }
  const f32x4 b = R.take((POS0 + NKG) % CH_D);
  CH_MFMA_SETTLE();
  return (a0 + a1) + b;
}

static __device__ __forceinline__ float ch_sum_g(float v) { v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); return v; }       // over the 4 lane groups of a row
static __device__ __forceinline__ float ch_sum_n(float v) {                                                                       // over the 16 rows of a lane group
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
  return v;
}
