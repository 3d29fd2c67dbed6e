// wbc_attitude_kernel.hip -- the kernel of wbc_sim_attitude_filter (include/wbc_sim.h, whose comment is the text this kernel and
// tests/attitude_reference.py both implement); its entry point and argument checks are with the other whole-body calls in wbc_arm_kernel.hip.
// A translation unit of its own: tests/test_identification.py pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_attitude.h"

// ---- attitude filter: multiplicative EKF on the unit quaternion and the gyro bias -----------------------------------------------------------
// Per env a few hundred dependent flops on the 21 distinct entries of a 6 x 6 covariance, so lane = env: AT_EPW = 64 envs per 64-lane
// workgroup, a single wavefront (a launch whose env count is no multiple of 64 repeats the last env on the idle lanes and stores nothing
// from them). q, b and P live in registers as a full 6 x 6 with both triangles kept equal; every loop over the 6 x 6 algebra and over the
// AT_NM measurements is unrolled, so no array is indexed dynamically and nothing goes to scratch. No LDS, no barrier, no shuffle: lanes
// diverge freely (a reset lane, a skipped measurement). Every store follows the lane's last read of the state; a failed env stores no state.
// AT_EPW = 16 is the same code on lanes 0..15 of four times as many wavefronts, kept for the measurement in DESIGN.md.

__device__ __forceinline__ bool at_finite(float v) { return fabsf(v) <= 3.4e38f; }        // false for a NaN
__device__ __forceinline__ bool at_finite(f3 v) { return at_finite(v.x) && at_finite(v.y) && at_finite(v.z); }
__device__ __forceinline__ bool at_pivot(float v) { return v > 0.f && v <= 3.4e38f; }

// q <- normalise(q (x) exp(phi))
__device__ __forceinline__ void at_compose(float* q, f3 phi, float* dq) {
  const float n2 = dot(phi, phi), n = sqrtf(n2);
  float s, c;
  if (n < 1e-4f) { s = 0.5f * (1.f - n2 / 24.f); c = 1.f - n2 / 8.f; }
  else { s = sinf(0.5f * n) / n; c = cosf(0.5f * n); }
  dq[0] = phi.x * s; dq[1] = phi.y * s; dq[2] = phi.z * s; dq[3] = c;
  float o[4];
  quat_mul(q, dq, o);
  const float nrm = sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
  q[0] = o[0] / nrm; q[1] = o[1] / nrm; q[2] = o[2] / nrm; q[3] = o[3] / nrm;
}

// One 3-row update with the world unit vector w, the measured trunk vector u and the per-component variance r. 0, or the bit to shift:
// WBC_ATTITUDE_INFO_ZERO (u . u = 0) or WBC_ATTITUDE_INFO_PIVOT; then q, b, p and nis are as they came.
__device__ __forceinline__ int at_update(float* q, float* b, float (*p)[6], f3 w, f3 u, float r, float& nis) {
  const float u2 = dot(u, u);
  if (u2 == 0.f) return WBC_ATTITUDE_INFO_ZERO;
  const f3 m = u * (1.f / sqrtf(u2));
  float R[9];
  quat_to_mat(q, R);
  const f3 mh = matT_mul(R, w);
  const f3 e = m - mh;
  f3 hp[6];                                                        // H P, column c: mh x (the top three rows of P's column c)
#pragma unroll
  for (int c = 0; c < 6; ++c) hp[c] = cross(mh, mk3(p[0][c], p[1][c], p[2][c]));
  // S = H P H^T + r I: row i of (H P)[:, 0:3] [mh]x^T is mh x (that row)
  const f3 s0 = cross(mh, mk3(hp[0].x, hp[1].x, hp[2].x)), s1 = cross(mh, mk3(hp[0].y, hp[1].y, hp[2].y)), s2 = cross(mh, mk3(hp[0].z, hp[1].z, hp[2].z));
  const float a00 = s0.x + r, a10 = s1.x, a11 = s1.y + r, a20 = s2.x, a21 = s2.y, a22 = s2.z + r;
  const float l00 = sqrtf(a00), l10 = a10 / l00;
  const float p1 = a11 - l10 * l10, l11 = sqrtf(p1);
  const float l20 = a20 / l00, l21 = (a21 - l20 * l10) / l11;
  const float p2 = a22 - l20 * l20 - l21 * l21, l22 = sqrtf(p2);
  if (!(at_pivot(a00) && at_pivot(p1) && at_pivot(p2))) return WBC_ATTITUDE_INFO_PIVOT;
  const float y0 = e.x / l00, y1 = (e.y - l10 * y0) / l11, y2 = (e.z - l20 * y0 - l21 * y1) / l22;
  float dx[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {                                    // W = L^-1 H P, in place
    const float w0 = hp[c].x / l00, w1 = (hp[c].y - l10 * w0) / l11, w2 = (hp[c].z - l20 * w0 - l21 * w1) / l22;
    hp[c] = mk3(w0, w1, w2);
    dx[c] = w0 * y0 + w1 * y1 + w2 * y2;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const float v = p[i][j] - dot(hp[i], hp[j]);
      p[i][j] = v; p[j][i] = v;
    }
  float dq[4];
  at_compose(q, mk3(dx[0], dx[1], dx[2]), dq);
  b[0] += dx[3]; b[1] += dx[4]; b[2] += dx[5];
  nis = y0 * y0 + y1 * y1 + y2 * y2;
  return 0;
}

extern "C" __global__ void __launch_bounds__(64) wbc_attitude_filter_kernel(wbc_attitude_cfg cfg, AtArgs a) {
  const int eu = blockIdx.x * AT_EPW + threadIdx.x;
  const bool live = eu < a.n && threadIdx.x < AT_EPW;
  const size_t e = live ? eu : a.n - 1;
  const bool reset = a.reset_all || (a.reset_mask && a.reset_mask[e] != 0);
  const float dt = cfg.dt;
  const f3 up = mk3(a.up[0], a.up[1], a.up[2]);

  // what every env reads: the gyro and the accelerometer
  f3 gyro;
  if (a.gyro) gyro = ld3(a.gyro + e * 3);
  else {
    const float* qr = a.root + e * 26 + 3;
    const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
    const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
    float Rs[9];
    quat_to_mat(qu, Rs);
    gyro = matT_mul(Rs, ld3(a.root + e * 26 + 10));
  }
  f3 acc = mk3(0.f, 0.f, 0.f);
  if (a.accel) acc = ld3(a.accel + e * 3);
  bool bad = !(at_finite(gyro) && at_finite(acc));

  float q[4] = {0.f, 0.f, 0.f, 1.f}, b[3] = {0.f, 0.f, 0.f}, p[6][6], nis[AT_NM];
  int bits = 0, code = WBC_ATTITUDE_STATUS_OK;
#pragma unroll
  for (int j = 0; j < AT_NM; ++j) nis[j] = 0.f;

  if (reset) {
    code = WBC_ATTITUDE_STATUS_RESET;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) p[i][j] = i != j ? 0.f : (i < 3 ? cfg.p0_theta : cfg.p0_b);
    float o[4] = {0.f, 0.f, 0.f, 1.f};
    if (a.q_init) {
      const float* qi = a.q_init + e * 4;
      o[0] = qi[0]; o[1] = qi[1]; o[2] = qi[2]; o[3] = qi[3];
    } else if (a.accel) {
      const float u2 = dot(acc, acc);
      if (u2 == 0.f) bits |= WBC_ATTITUDE_INFO_ZERO;
      else {
        const f3 m = acc * (1.f / sqrtf(u2));
        const float d = 1.f + dot(m, up);
        if (d < WBC_ATTITUDE_ANTIPARALLEL) { o[0] = a.half[0]; o[1] = a.half[1]; o[2] = a.half[2]; o[3] = 0.f; bits |= WBC_ATTITUDE_INFO_HALF_TURN; }
        else { const f3 x = cross(m, up); o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = d; }
      }
    }
    const float nrm = sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    q[0] = o[0] / nrm; q[1] = o[1] / nrm; q[2] = o[2] / nrm; q[3] = o[3] / nrm;
  } else {
    const float* qg = a.q + e * 4;
    const float* bg = a.b + e * 3;
    const float* Pg = a.P + e * 36;
    q[0] = qg[0]; q[1] = qg[1]; q[2] = qg[2]; q[3] = qg[3];
    b[0] = bg[0]; b[1] = bg[1]; b[2] = bg[2];
    bool fin = at_finite(q[0]) && at_finite(q[1]) && at_finite(q[2]) && at_finite(q[3]) && at_finite(b[0]) && at_finite(b[1]) && at_finite(b[2]);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const float v = Pg[i * 6 + j];
        fin = fin && at_finite(v);
        p[i][j] = v; p[j][i] = v;
      }
    bad = bad || !fin;

    // predict
    float dq[4], Rd[9];
    at_compose(q, (gyro - mk3(b[0], b[1], b[2])) * dt, dq);
    quat_to_mat(dq, Rd);                                           // A = Rd^T: A[i][k] = Rd[3 k + i]
    float G[3][3], T[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        G[i][j] = Rd[i] * p[0][3 + j] + Rd[3 + i] * p[1][3 + j] + Rd[6 + i] * p[2][3 + j];
        T[i][j] = Rd[i] * p[0][j] + Rd[3 + i] * p[1][j] + Rd[6 + i] * p[2][j];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        float v = T[i][0] * Rd[j] + T[i][1] * Rd[3 + j] + T[i][2] * Rd[6 + j];
        v = v - dt * (G[i][j] + G[j][i]) + dt * dt * p[3 + i][3 + j];
        if (i == j) v += dt * (cfg.sigma_g * cfg.sigma_g);
        p[i][j] = v; p[j][i] = v;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float v = G[i][j] - dt * p[3 + i][3 + j];
        p[i][3 + j] = v; p[3 + j][i] = v;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i) p[3 + i][3 + i] += dt * (cfg.sigma_b * cfg.sigma_b);

    // correct: the accelerometer, then the aux entries
    if (a.accel && !bad) {
      const float x = (sqrtf(dot(acc, acc)) - a.gnorm) / a.gnorm;
      const int rc = at_update(q, b, p, up, acc, cfg.sigma_a * cfg.sigma_a * (1.f + cfg.kappa_a * (x * x)), nis[0]);
      bits |= rc;
    }
#pragma unroll
    for (int k = 0; k < WBC_ATTITUDE_MAX_AUX; ++k) {
      if (k >= a.naux) continue;
      const size_t ek = e * a.naux + k;
      const float sg = a.aux_sigma[ek];
      if (sg <= 0.f) continue;
      const f3 u = ld3(a.aux_body + ek * 3), ww = ld3(a.aux_world + ek * 3);
      if (!(at_finite(sg) && at_finite(u) && at_finite(ww))) { bad = true; continue; }
      if (bad) continue;
      const float w2 = dot(ww, ww);
      if (w2 == 0.f) { bits |= WBC_ATTITUDE_INFO_ZERO << (1 + k); continue; }
      const int rc = at_update(q, b, p, ww * (1.f / sqrtf(w2)), u, sg * sg, nis[1 + k]);
      bits |= rc << (1 + k);
    }
    if (bits & (WBC_ATTITUDE_INFO_PIVOT * ((1 << AT_NM) - 1))) code = WBC_ATTITUDE_STATUS_FAILED_PIVOT;
  }

  // the state that leaves must be finite
  bool fin = at_finite(q[0]) && at_finite(q[1]) && at_finite(q[2]) && at_finite(q[3]) && at_finite(b[0]) && at_finite(b[1]) && at_finite(b[2]);
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) fin = fin && at_finite(p[i][j]);
  bad = bad || !fin;
  if (!live) return;

  f3 go = mk3(0.f, 0.f, 0.f), gb = go;
  if (bad) {
#pragma unroll
    for (int j = 0; j < AT_NM; ++j) nis[j] = 0.f;
  } else {
    float R[9];
    quat_to_mat(q, R);
    go = gyro - mk3(b[0], b[1], b[2]);
    gb = matT_mul(R, up) * -1.f;
    float* qg = a.q + e * 4;
    float* bg = a.b + e * 3;
    float* Pg = a.P + e * 36;
    qg[0] = q[0]; qg[1] = q[1]; qg[2] = q[2]; qg[3] = q[3];
    bg[0] = b[0]; bg[1] = b[1]; bg[2] = b[2];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) Pg[i * 6 + j] = p[i][j];
  }
  if (a.gyro_out) st3(a.gyro_out + e * 3, go);
  if (a.gravity_body) st3(a.gravity_body + e * 3, gb);
  if (a.nis) {
    float* ng = a.nis + e * (1 + a.naux);
#pragma unroll
    for (int j = 0; j < AT_NM; ++j)
      if (j <= a.naux) ng[j] = nis[j];
  }
  if (a.status) a.status[e] = bad ? WBC_ATTITUDE_STATUS_FAILED : (code | bits);
}

void wbc_attitude_launch(const wbc_attitude_cfg& cfg, const AtArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_attitude_filter_kernel, dim3((a.n + AT_EPW - 1) / AT_EPW), dim3(64), 0, (hipStream_t)stream, cfg, a);
}
