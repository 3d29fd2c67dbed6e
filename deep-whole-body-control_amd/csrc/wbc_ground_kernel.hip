// wbc_ground_kernel.hip -- the kernel of wbc_sim_ground_estimate (include/wbc_sim.h, whose comment is the text this kernel and
// tests/ground_reference.py both implement); its entry point and argument checks are with the other whole-body calls in wbc_arm_kernel.hip.
// A translation unit of its own: tests/test_identification.py pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_ground.h"

// ---- ground plane from the footholds ---------------------------------------------------------------------------------------------------------
// The leg walk is the one part with real work and it is per foot, so lane = (env, foot): GE_EPW = 16 envs per 64-lane workgroup, a single
// wavefront, env `grp` on lanes 4 grp .. 4 grp + 3 (a launch whose env count is no multiple of GE_EPW repeats the last env on the idle
// groups and stores nothing from them). Each lane walks its own leg and owns its foot's five floats of state; the sums of the fit, the
// smallest age, foot 0's point and the non-finite vote go through xor shuffles inside the 4-lane group, which leave every lane of the
// group with the same bits ((s_0 + s_1) + (s_2 + s_3) whichever lane adds), so every lane solves the same 2 x 2 system and none waits for
// another. The query points, the one part whose work varies from call to call, are dealt over the env's lanes (point k on lane k mod 4):
// the loop count is the same on every lane of the wavefront. No LDS, no barrier, no scratch.
// GE_EPW = 64 is lane = env with the four legs walked in sequence (the same code, the per-foot values in unrolled arrays of four and
// the sums written out), kept for the measurement in DESIGN.md.
// Control flow around the shuffles is uniform; a failed env runs the same instructions and stores zeros. Every store follows the lane's
// last read of the state.

__device__ __forceinline__ bool ge_finite(float v) { return fabsf(v) <= 3.4e38f; }        // false for a NaN
__device__ __forceinline__ bool ge_finite(f3 v) { return ge_finite(v.x) && ge_finite(v.y) && ge_finite(v.z); }
__device__ __forceinline__ bool ge_pivot(float v) { return v > 0.f && v <= 3.4e38f; }

// (s_0 + s_1) + (s_2 + s_3) over the env's four feet, the same bits on every lane of the env
__device__ __forceinline__ float ge_sum(const float (&v)[GE_FPL]) {
#if GE_FPL == 1
  float s = v[0];
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  return s;
#else
  return (v[0] + v[1]) + (v[2] + v[3]);
#endif
}
__device__ __forceinline__ float ge_min(const float (&v)[GE_FPL]) {
#if GE_FPL == 1
  float s = v[0];
  s = fminf(s, __shfl_xor(s, 1));
  s = fminf(s, __shfl_xor(s, 2));
  return s;
#else
  return fminf(fminf(v[0], v[1]), fminf(v[2], v[3]));
#endif
}
__device__ __forceinline__ float ge_foot0(const float (&v)[GE_FPL], int lane) {
#if GE_FPL == 1
  return __shfl(v[0], lane & ~(GE_LPE - 1));
#else
  return v[0];
#endif
}
__device__ __forceinline__ int ge_or(int v) {
#if GE_FPL == 1
  v |= __shfl_xor(v, 1);
  v |= __shfl_xor(v, 2);
#endif
  return v;
}

extern "C" __global__ void __launch_bounds__(64) wbc_ground_estimate_kernel(EstConst K, wbc_ground_cfg cfg, GeArgs a) {
  const int lane = threadIdx.x, grp = lane / GE_LPE, l = lane - grp * GE_LPE;
  const int eu = blockIdx.x * GE_EPW + grp;
  const bool live = eu < a.n;
  const size_t e = live ? eu : a.n - 1;
  const bool reset = a.reset_all || (a.reset_mask && a.reset_mask[e] != 0);
  float* const st = a.state + e * WBC_GROUND_NS;

  // 1 kinematics: the trunk's rotation from the quaternion, normalised; b
  const float* qr = a.quat + e * a.quat_stride;
  const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
  const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
  float R[9];
  quat_to_mat(qu, R);
  const f3 b = ld3(a.pos + e * a.pos_stride);
  const float* dq = a.dofs + e * (2 * WBC_NDOF);

  int bits = 0;
  bool bad = false;
  float ap1 = 0.f, ap2 = 0.f;
  if (!reset) { ap1 = st[23]; ap2 = st[24]; bad = !(ge_finite(ap1) && ge_finite(ap2)); }

  // per foot: the leg walk, 2 reset, 3 latch
  float px[GE_FPL], py[GE_FPL], mx[GE_FPL], my[GE_FPL], mz[GE_FPL], t[GE_FPL];
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) {
    const int f = l + j;
    const int body = K.foot_body[f];
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 o = mk3(0.f, 0.f, 0.f);                                     // in trunk axes, relative to the trunk
#pragma unroll
    for (int k = 0; k < GE_LEG_JOINTS; ++k) {
      const int jn = K.path[body][k];
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[jn], dq[2 * K.dof[jn]], Q);
      tree_frame_step(E, o, Q, K.joint_xyz[jn], u);
    }
    const f3 fk = o + mat_mul(E, mk3(K.foot_off[f][0], K.foot_off[f][1], K.foot_off[f][2]));
    const f3 pw = b + mat_mul(R, fk);
    const float c = a.contact[e * WBC_NFEET + f];
    bad = bad || !ge_finite(pw) || !ge_finite(c);
    f3 m = pw;
    float age = 0.f;
    if (!reset) {
      m = ld3(st + 5 * f);
      age = st[5 * f + 3];
      bad = bad || !ge_finite(m) || !ge_finite(age);
    }
    if (c >= cfg.c_on) { m = pw; age = 0.f; bits |= WBC_GROUND_INFO_LATCHED << f; }
    else age = age + cfg.dt;
    px[j] = pw.x; py[j] = pw.y; mx[j] = m.x; my[j] = m.y; mz[j] = m.z; t[j] = age;
  }

  // the weights and the fit: relative to foot 0's point, nothing squared before the anchor is taken out
  const float tmin = ge_min(t);
  const float m0x = ge_foot0(mx, lane), m0y = ge_foot0(my, lane), m0z = ge_foot0(mz, lane);
  float w[GE_FPL], ex[GE_FPL], ey[GE_FPL], ez[GE_FPL], v[GE_FPL];
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) {
    w[j] = expf(-(t[j] - tmin) / cfg.tau_age);
    ex[j] = mx[j] - m0x; ey[j] = my[j] - m0y; ez[j] = mz[j] - m0z;
  }
  const float W = ge_sum(w);
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = w[j] * ex[j];
  const float rx = ge_sum(v) / W;
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = w[j] * ey[j];
  const float ry = ge_sum(v) / W;
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = w[j] * ez[j];
  const float rz = ge_sum(v) / W;
  float dx[GE_FPL], dy[GE_FPL], dz[GE_FPL];
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) { dx[j] = ex[j] - rx; dy[j] = ey[j] - ry; dz[j] = ez[j] - rz; }
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = (w[j] * dx[j]) * dx[j];
  const float Sxx = ge_sum(v);
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = (w[j] * dx[j]) * dy[j];
  const float Sxy = ge_sum(v);
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = (w[j] * dy[j]) * dy[j];
  const float Syy = ge_sum(v);
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = (w[j] * dx[j]) * dz[j];
  const float Sxz = ge_sum(v);
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) v[j] = (w[j] * dy[j]) * dz[j];
  const float Syz = ge_sum(v);
  const float lw = cfg.lambda * W;
  const float A00 = Sxx + lw, A10 = Sxy, A11 = Syy + lw, b0 = Sxz + lw * ap1, b1 = Syz + lw * ap2;
  const float l00 = sqrtf(A00), l10 = A10 / l00;
  const float d1 = A11 - l10 * l10, l11 = sqrtf(d1);
  const float z0 = b0 / l00, z1 = (b1 - l10 * z0) / l11;
  const float y1 = z1 / l11, y0 = (z0 - l10 * y1) / l00;
  float a1 = y0, a2 = y1;
  if (!(ge_pivot(A00) && ge_pivot(d1) && ge_finite(a1) && ge_finite(a2))) { a1 = ap1; a2 = ap2; bits |= WBC_GROUND_INFO_DEGENERATE; }
  const float sl = sqrtf(a1 * a1 + a2 * a2);
  if (sl > cfg.slope_max) { const float k = cfg.slope_max / sl; a1 *= k; a2 *= k; bits |= WBC_GROUND_INFO_CLAMPED; }
  const float s2 = a1 * a1 + a2 * a2, s = sqrtf(s2);
  const float a0 = m0z + rz;

  // the query points' share of the vote
  const float* qx = a.query_xy + e * (size_t)a.nq * 2;
  for (int k = l; k < a.nq; k += GE_LPE) bad = bad || !(ge_finite(qx[2 * k]) && ge_finite(qx[2 * k + 1]));

  // what the env's feet share
  const bool failed = ge_or(bad ? 1 : 0) != 0;
  bits = ge_or(bits);
  if (!live) return;

  // 5 outputs
  const float ninv = 1.f / sqrtf(1.f + s2);
  const f3 nrm = failed ? mk3(0.f, 0.f, 0.f) : mk3(-a1 * ninv, -a2 * ninv, ninv);
#pragma unroll
  for (int j = 0; j < GE_FPL; ++j) {
    const int f = l + j;
    const size_t ef = e * WBC_NFEET + f;
    if (!failed) {
      float* sf = st + 5 * f;
      sf[0] = mx[j]; sf[1] = my[j]; sf[2] = mz[j]; sf[3] = t[j]; sf[4] = 0.f;
    }
    if (a.normal) st3(a.normal + ef * 3, nrm);
    if (a.ground) a.ground[ef] = failed ? 0.f : a0 + (a1 * ((px[j] - m0x) - rx) + a2 * ((py[j] - m0y) - ry));
    if (a.residual) a.residual[ef] = failed ? 0.f : dz[j] - (a1 * dx[j] + a2 * dy[j]);
  }
  if (a.query_z)
    for (int k = l; k < a.nq; k += GE_LPE)
      a.query_z[e * (size_t)a.nq + k] = failed ? 0.f : a0 + (a1 * ((qx[2 * k] - m0x) - rx) + a2 * ((qx[2 * k + 1] - m0y) - ry));
  if (l != 0) return;
  if (!failed) {
    st[20] = m0x + rx; st[21] = m0y + ry; st[22] = a0; st[23] = a1; st[24] = a2;
#pragma unroll
    for (int k = 25; k < WBC_GROUND_NS; ++k) st[k] = 0.f;
  }
  if (a.trunk) {
    float* tr = a.trunk + e * 6;
    const float zb = a0 + (a1 * ((b.x - m0x) - rx) + a2 * ((b.y - m0y) - ry));
    const float hn = sqrtf(R[0] * R[0] + R[3] * R[3]);
    const float ch = hn > 0.f ? R[0] / hn : 1.f, sh = hn > 0.f ? R[3] / hn : 0.f;
    tr[0] = failed ? 0.f : zb;
    tr[1] = failed ? 0.f : (b.z - zb) * ninv;
    tr[2] = failed ? 0.f : a1 * ch + a2 * sh;
    tr[3] = failed ? 0.f : a2 * ch - a1 * sh;
    tr[4] = 0.f; tr[5] = 0.f;
  }
  if (a.theta_ref) {
    const float g = cfg.tilt_gain * (s < WBC_GROUND_SERIES ? 1.f - s2 / 3.f : atanf(s) / s);
    st3(a.theta_ref + e * 3, failed ? mk3(0.f, 0.f, 0.f) : mk3(g * a2, 0.f - g * a1, 0.f));
  }
  if (a.info) a.info[e] = failed ? WBC_GROUND_INFO_FAILED : ((reset ? WBC_GROUND_INFO_RESET : 0) | bits);
}

void wbc_ground_launch(const EstConst& K, const wbc_ground_cfg& cfg, const GeArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_ground_estimate_kernel, dim3((a.n + GE_EPW - 1) / GE_EPW), dim3(64), 0, (hipStream_t)stream, K, cfg, a);
}
