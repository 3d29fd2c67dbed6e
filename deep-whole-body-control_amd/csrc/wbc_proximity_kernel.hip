// wbc_proximity_kernel.hip -- the kernel of wbc_sim_proximity (include/wbc_sim.h); its entry points, argument checks and the pair list are
// with the other whole-body calls in wbc_arm_kernel.hip. A translation unit of its own: tests/test_identification.py pins the number of
// kernels in wbc_arm_kernel.hip's code object.
#include "wbc_proximity.h"

// ---- self-collision proximity: signed gaps, witness points and gap Jacobians (include/wbc_sim.h: wbc_sim_proximity) --------------------
// The pairs are the model's own: the lanes whose pr_kind is WBC_PR_LIMBS, in lane order, then the static pairs of kind WBC_CP_BOX whose box
// rides on the root body (prox_const_fill). One env per 64-lane workgroup, a single wavefront:
//  1) lane b = moving body b walks root -> b (tree_frame_step per joint) in registers and leaves in LDS its frame E, its origin p (= its
//     joint's origin) and its joint's axis, in F's axes relative to the root's origin, and for every joint j on its path the vector
//     p_b - p_j as the sum of the joint offsets between them (never as a difference of two positions);
//  2) lane p = pair p: the ends of its two limbs RELATIVE TO THEIR LIMB'S BODY from those tables, the feature pairs in the step kernel's
//     order (shafts; A's end spheres against B's shaft; A's shaft against B's end spheres; end sphere against end sphere; of equal gaps the
//     earlier), or the sphere against the box in F; then n, the witnesses and the gap;
//  3) the same lane walks the two paths and writes n . (axis_j x lever) for the joints that move one side only into a zeroed LDS tile
//     [P][26], the lever (p_body - p_j) + (c - p_body) built from the joint's own origin outwards: its rounding scales with the lever, not
//     with the point's distance from the root; the tile leaves in consecutive 4-byte stores of consecutive lanes (normal and witness
//     leave from their lanes: through tiles of their own they were measured no faster);
//  4) nearest: each lane counts the pairs whose (gap, index) precedes its own.
// Nothing depends on which outputs are asked for but the stores. The root position and every velocity are never read.

// A limb's end relative to the origin of the limb's body lb, in F's axes.
__device__ __forceinline__ f3 px_end(const float (*sF)[PX_FT], const float (*sRel)[WBC_MAX_DEPTH][3], int lb, int eb, int link, const float* pos) {
  const int kind = link & 15, k = link >> 4;
  f3 o = mk3(0.f, 0.f, 0.f);
  if (kind == 1) o = o - ld3(sRel[lb][k]);
  else if (kind == 2) o = ld3(sRel[eb][k]);
  else if (kind == 3) o = ld3(sF[eb] + 9) - ld3(sF[lb] + 9);
  return o + mat_mul(sF[eb], mk3(pos[0], pos[1], pos[2]));
}
__device__ __forceinline__ float px_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
// e0 + u (e1 - e0), the ends themselves at u = 0 and u = 1.
__device__ __forceinline__ f3 px_at(f3 e0, f3 e1, float u) { return u <= 0.f ? e0 : (u >= 1.f ? e1 : e0 + (e1 - e0) * u); }
// Parameter of the closest point to q on the segment b0 b1; a segment shorter than 1e-5 m counts as its first end (as the step kernel's).
__device__ __forceinline__ float px_on_segment(f3 q, f3 b0, f3 b1) {
  const f3 d = b1 - b0;
  const float e = dot(d, d);
  return e <= 1e-10f ? 0.f : px_clamp01(dot(q - b0, d) / e);
}
// Parameters of the closest points of two segments (Ericson 5.1.9, the step kernel's branches and thresholds) with the determinant as
// |d1 x d2|^2 and its numerator as (d1 x d2) . (d2 x r): neither is a difference of two products of lengths. Parallel shafts
// (sin^2 <= 1e-7): s = 0.
__device__ __forceinline__ void px_seg_seg(f3 a0, f3 a1, f3 b0, f3 b1, float* ps, float* pt) {
  const f3 d1 = a1 - a0, d2 = b1 - b0, r = a0 - b0;
  const float EPS = 1e-10f;
  const float a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r);
  float s = 0.f, t = 0.f;
  if (a <= EPS && e <= EPS) {
  } else if (a <= EPS) {
    t = px_clamp01(f / e);
  } else {
    const float c = dot(d1, r);
    if (e <= EPS) {
      s = px_clamp01(-c / a);
    } else {
      const f3 x = cross(d1, d2);
      const float b = dot(d1, d2), den = dot(x, x);
      s = den > 1e-7f * a * e ? px_clamp01(dot(x, cross(d2, r)) / den) : 0.f;
      t = (b * s + f) / e;
      if (t < 0.f) { t = 0.f; s = px_clamp01(-c / a); }
      else if (t > 1.f) { t = 1.f; s = px_clamp01((b - c) / a); }
    }
  }
  *ps = s; *pt = t;
}

extern "C" __global__ void __launch_bounds__(64) wbc_proximity_kernel(ProxConst K, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                     int n, float* __restrict__ gap, float* __restrict__ normal,
                                                                     float* __restrict__ witness, float* __restrict__ jac,
                                                                     int32_t* __restrict__ nearest, int k_nearest) {
  __shared__ float sF[WBC_NB][PX_FT];
  __shared__ float sRel[WBC_NB][WBC_MAX_DEPTH][3];             // [b][k]: p_b - p_path[b][k]
  // 9.5 kB in all: the 16 workgroups a CU gets at 4096 envs are resident at once (with 11.8 kB 13 are, and the launch takes half as long again)
  __shared__ float sJ[PX_MAXP * WBC_NCOL];
  __shared__ float sG[PX_MAXP];
  const int lane = threadIdx.x, P = K.npairs;
  const size_t e = blockIdx.x;
  if ((int)e >= n) return;
  for (int t = lane; t < P * WBC_NCOL; t += 64) sJ[t] = 0.f;

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f), S = p;
#pragma nounroll
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int a = K.path[b][k];
      if (a < 0) break;
      const f3 r = mat_mul(E, mk3(K.joint_xyz[a][0], K.joint_xyz[a][1], K.joint_xyz[a][2]));   // this joint's offset: what the step adds to p
#pragma nounroll
      for (int m = 0; m < k; ++m) st3(sRel[b][m], ld3(sRel[b][m]) + r);
      st3(sRel[b][k], mk3(0.f, 0.f, 0.f));
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * K.dof[a]], Q);
      S = tree_frame_step(E, p, Q, K.joint_xyz[a], u);
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) sF[b][j] = E[j];
    st3(sF[b] + 9, p); st3(sF[b] + 12, S);
  }
  __syncthreads();

  float g = 3.0e38f;
  if (lane < P) {
    const int pd = K.pair[lane], kind = pd & 255, ia = (pd >> 8) & 255, ib = (pd >> 16) & 255;
    f3 cal, cbl, pA, pB, nF;                                       // the core points relative to their bodies' origins pA, pB
    float ra, rb, dist;
    int ba, bb;
    if (kind == WBC_PR_LIMBS) {
      ba = K.limb_body[ia]; bb = K.limb_body[ib];
      pA = ld3(sF[ba] + 9); pB = ld3(sF[bb] + 9);
      const f3 a0l = px_end(sF, sRel, ba, K.end_body[ia][0], K.end_link[ia][0], K.end_pos[ia][0]);
      const f3 a1l = px_end(sF, sRel, ba, K.end_body[ia][1], K.end_link[ia][1], K.end_pos[ia][1]);
      const f3 b0l = px_end(sF, sRel, bb, K.end_body[ib][0], K.end_link[ib][0], K.end_pos[ib][0]);
      const f3 b1l = px_end(sF, sRel, bb, K.end_body[ib][1], K.end_link[ib][1], K.end_pos[ib][1]);
      const f3 a0 = pA + a0l, a1 = pA + a1l, b0 = pB + b0l, b1 = pB + b1l;
      const float ra0 = K.limb_rad[ia][0], ra1 = K.limb_rad[ia][1], ra2 = K.limb_rad[ia][2];
      const float rb0 = K.limb_rad[ib][0], rb1 = K.limb_rad[ib][1], rb2 = K.limb_rad[ib][2];
      float s, t;
      px_seg_seg(a0, a1, b0, b1, &s, &t);
      ra = ra0; rb = rb0;
      {
        const f3 d = (pA + px_at(a0l, a1l, s)) - (pB + px_at(b0l, b1l, t));
        dist = sqrtf(dot(d, d)); g = dist - ra - rb;
      }
#pragma nounroll
      for (int f = 1; f < 9; ++f) {
        const int ea = f <= 2 ? f - 1 : (f <= 4 ? -1 : (f - 5) >> 1), eb = f <= 2 ? -1 : (f <= 4 ? f - 3 : (f - 5) & 1);
        const float fra = ea < 0 ? ra0 : (ea == 0 ? ra1 : ra2), frb = eb < 0 ? rb0 : (eb == 0 ? rb1 : rb2);
        if (!(fra > 0.f) || !(frb > 0.f)) continue;               // no such end sphere
        float sf, tf;
        if (ea >= 0) {
          sf = (float)ea;
          tf = eb >= 0 ? (float)eb : px_on_segment(ea == 0 ? a0 : a1, b0, b1);
        } else {
          tf = (float)eb;
          sf = px_on_segment(eb == 0 ? b0 : b1, a0, a1);
        }
        const f3 d = (pA + px_at(a0l, a1l, sf)) - (pB + px_at(b0l, b1l, tf));
        const float dd = sqrtf(dot(d, d)), gf = dd - fra - frb;
        if (gf < g) { g = gf; s = sf; t = tf; ra = fra; rb = frb; dist = dd; }
      }
      cal = px_at(a0l, a1l, s); cbl = px_at(b0l, b1l, t);
      const f3 d = (pA + cal) - (pB + cbl);
      nF = dist > 1e-9f ? mk3(d.x / dist, d.y / dist, d.z / dist) : mk3(1.f, 0.f, 0.f);
    } else {                                                       // a sphere against a box on the root body: the box's axes are F's
      ba = K.sb_body[ia]; bb = 0;
      pA = ld3(sF[ba] + 9); pB = mk3(0.f, 0.f, 0.f);
      cal = mat_mul(sF[ba], mk3(K.sb_pos[ia][0], K.sb_pos[ia][1], K.sb_pos[ia][2]));
      const f3 ca = pA + cal;
      ra = K.sb_rad[ia]; rb = 0.f;
      const float loc[3] = {ca.x - K.sb_centre[ia][0], ca.y - K.sb_centre[ia][1], ca.z - K.sb_centre[ia][2]};
      const float h[3] = {K.sb_half[ia][0], K.sb_half[ia][1], K.sb_half[ia][2]};
      float cl[3], depth = 3.0e38f;
      int face = 0;
      bool inside = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        cl[j] = fminf(fmaxf(loc[j], -h[j]), h[j]);
        inside = inside && fabsf(loc[j]) <= h[j];
        const float dj = h[j] - fabsf(loc[j]);
        if (dj < depth) { depth = dj; face = j; }                  // of equally near faces the first
      }
      if (inside) {                                                // the nearest face: its normal, its point, minus the depth
        const float sgn = loc[face] < 0.f ? -1.f : 1.f;
        nF = mk3(face == 0 ? sgn : 0.f, face == 1 ? sgn : 0.f, face == 2 ? sgn : 0.f);
#pragma unroll
        for (int j = 0; j < 3; ++j) if (j == face) cl[j] = sgn * h[j];
        dist = -depth;
      } else {
        const f3 d = mk3(loc[0] - cl[0], loc[1] - cl[1], loc[2] - cl[2]);
        dist = sqrtf(dot(d, d));
        nF = mk3(d.x / dist, d.y / dist, d.z / dist);
      }
      cbl = mk3(K.sb_centre[ia][0] + cl[0], K.sb_centre[ia][1] + cl[1], K.sb_centre[ia][2] + cl[2]);
      g = dist - ra;
    }
    // the row of the gap Jacobian: the joints that move one side only, each lever from the joint's own origin outwards
    const uint32_t ma = K.anc[ba], mb = K.anc[bb];
#pragma nounroll
    for (int side = 0; side < 2; ++side) {
      const int bs = side ? bb : ba;
      const uint32_t only = (side ? mb & ~ma : ma & ~mb) & ~1u;
      const f3 c = side ? cbl : cal;
#pragma nounroll
      for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
        const int j = K.path[bs][k];
        if (j < 0) break;
        if (!((only >> j) & 1u)) continue;
        const float v = dot(nF, cross(ld3(sF[j] + 12), ld3(sRel[bs][k]) + c));
        sJ[lane * WBC_NCOL + 6 + K.dof[j]] = side ? -v : v;
      }
    }
    sG[lane] = g;
    // world axes: the rotation of the root's quaternion, normalised
    const float* qr = root + e * 26 + 3;
    const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
    const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
    float R[9];
    quat_to_mat(qu, R);
    if (gap) gap[e * P + lane] = g;
    if (normal) {                                                  // normalised again in world axes: |n| = 1 to the rounding of one division
      const f3 nw = mat_mul(R, nF);
      const float nn = sqrtf(dot(nw, nw));
      st3(normal + (e * P + lane) * 3, mk3(nw.x / nn, nw.y / nn, nw.z / nn));
    }
    if (witness) {
      float* w = witness + (e * P + lane) * 6;
      st3(w, mat_mul(R, (pA + cal) - nF * ra)); st3(w + 3, mat_mul(R, (pB + cbl) + nF * rb));
    }
  }
  __syncthreads();
  if (jac) {
    float* out = jac + e * (size_t)(P * WBC_NCOL);
    for (int t = lane; t < P * WBC_NCOL; t += 64) out[t] = sJ[t];
  }
  if (nearest) {
    if (lane < P) {
      int rank = 0;
      for (int q = 0; q < P; ++q) {
        const float gq = sG[q];
        rank += (gq < g || (gq == g && q < lane)) ? 1 : 0;
      }
      if (rank < k_nearest) nearest[e * k_nearest + rank] = lane;
    } else if (lane < k_nearest) {
      nearest[e * k_nearest + lane] = -1;                          // fewer pairs than k_nearest
    }
  }
}

void wbc_proximity_launch(const ProxConst& K, const float* root, const float* dofs, int n, float* gap, float* normal, float* witness, float* jac,
                          int32_t* nearest, int k_nearest, void* stream) {
  hipLaunchKernelGGL(wbc_proximity_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, K, root, dofs, n, gap, normal, witness, jac, nearest, k_nearest);
}
