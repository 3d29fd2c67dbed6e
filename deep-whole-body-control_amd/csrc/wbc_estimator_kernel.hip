// wbc_estimator_kernel.hip -- the kernel of wbc_sim_leg_odometry (include/wbc_sim.h); its entry point and argument checks are with the other
// whole-body calls in wbc_arm_kernel.hip. A translation unit of its own: tests/test_identification.py pins the number of kernels in
// wbc_arm_kernel.hip's code object.
#include "wbc_estimator.h"
#include "wbc_delassus.h"

// ---- leg-odometry Kalman filter for the base's position and velocity (include/wbc_sim.h: wbc_sim_leg_odometry) -------------------------
// State x = (p, v, p_1 .. p_4), covariance P [18][18]; the correction's rows: 12 position rows, 12 velocity rows (both foot-major) and, with
// foot heights, 4 height rows. Two envs per 64-lane workgroup, a single wavefront: env `half` on lanes 32 half .. 32 half + 31, `l` the lane
// in its group (a launch with an odd env count repeats the last env on the idle group and stores nothing from it).
//  1) lane l < 4 walks leg l from the trunk to the foot (tree_frame_step per joint) with the angular velocity and the foot origin's velocity
//     relative to the trunk, and leaves r_l = R fk_l and rdot_l = R (w_b x fk_l + J_l qd) and the swing inflation s_l in LDS; lanes l < 18 predict x;
//  2) P- = A P A^T + Q, one lower-triangle entry per lane and round straight from the caller's P (read as symmetric: its lower triangle), mirrored;
//  3) C P- (28 x 18; C is a signed selection matrix: each entry a difference of at most two entries of P-) with the residual as column 18,
//     then the lower triangle of S = C P- C^T + R_m from it; S = L L^T by delassus_cholesky, lane = row;
//  4) lane c <= 18 forward-substitutes column c: W = L^-1 C P- and y = L^-1 e;
//  5) x+ = x- + W^T y, P+ = P- - W^T W (lower triangle, mirrored: bit-symmetric), NIS = |y|^2; a failed pivot (1 / sqrt of it not a positive
//     finite number) keeps (x-, P-); a reset env leaves with the reset values. Every store happens after the last read of x and P.
// Nothing depends on which outputs are asked for but the stores; control flow around the barriers is uniform (a reset or failed env runs the
// same instructions on values that are then discarded).

__device__ __forceinline__ float est_sel(f3 v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : v.z); }

// Row k of the correction: C has +1 at column c1 and -1 at column c2 (c2 < 0: none); its foot and its group (0 position, 1 velocity, 2 height).
__device__ __forceinline__ void est_row(int k, int& c1, int& c2, int& foot, int& group) {
  if (k < 12) { foot = k / 3; group = 0; c1 = k - 3 * foot; c2 = 6 + k; }
  else if (k < 24) { foot = (k - 12) / 3; group = 1; c1 = 3 + (k - 12) - 3 * foot; c2 = -1; }
  else { foot = k - 24; group = 2; c1 = 6 + 3 * foot + 2; c2 = -1; }
}

extern "C" __global__ void __launch_bounds__(64) wbc_leg_odometry_kernel(EstConst K, wbc_estimator_cfg cfg, EstArgs a) {
  __shared__ float sP[EST_EPW][EST_NX][EST_PP];
  __shared__ float sW[EST_EPW][EST_MAXM][EST_PW];
  __shared__ float sS[EST_EPW][EST_MAXM][EST_PS];
  __shared__ float sD[EST_EPW][32];
  __shared__ float sX[EST_EPW][EST_NX];
  __shared__ float sK[EST_EPW][WBC_NFEET][6];                      // r_f, rdot_f in world axes
  __shared__ float sC[EST_EPW][WBC_NFEET];                         // s_f = 1 + kappa (1 - c_f)
  const int lane = threadIdx.x, half = lane / EST_LPE, l = lane - half * EST_LPE;
  const int eu = blockIdx.x * EST_EPW + half;
  const bool live = eu < a.n;
  const size_t e = live ? eu : a.n - 1;
  const int m = a.foot_height ? EST_MAXM : EST_MAXM - WBC_NFEET;
  const bool reset = a.reset_all || (a.reset_mask && a.reset_mask[e] != 0);
  float (*P)[EST_PP] = sP[half];
  float (*W)[EST_PW] = sW[half];
  float (*S)[EST_PS] = sS[half];
  float *D = sD[half], *X = sX[half];
  const float dt = cfg.dt;

  // the trunk's rotation from the quaternion, normalised, and the gyro in trunk axes
  const float* qr = a.quat + e * a.quat_stride;
  const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
  const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
  float R[9];
  quat_to_mat(qu, R);
  const f3 wb = a.gyro ? ld3(a.gyro + e * 3) : matT_mul(R, ld3(a.root + e * 26 + 10));

  if (l < WBC_NFEET) {
    const int b = K.foot_body[l];
    const float* dq = a.dofs + e * (2 * WBC_NDOF);
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f), w = p, vo = p;                      // in trunk axes, relative to the trunk: origin, angular velocity, the origin's velocity
#pragma nounroll
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int j = K.path[b][k];
      if (j < 0) break;
      const int d = K.dof[j];
      vo = vo + cross(w, mat_mul(E, mk3(K.joint_xyz[j][0], K.joint_xyz[j][1], K.joint_xyz[j][2])));
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[j], dq[2 * d], Q);
      const f3 Sw = tree_frame_step(E, p, Q, K.joint_xyz[j], u);
      w = w + Sw * dq[2 * d + 1];
    }
    const f3 off = mat_mul(E, mk3(K.foot_off[l][0], K.foot_off[l][1], K.foot_off[l][2]));
    const f3 fk = p + off;
    st3(sK[half][l], mat_mul(R, fk));
    st3(sK[half][l] + 3, mat_mul(R, cross(wb, fk) + (vo + cross(w, off))));
    sC[half][l] = 1.f + cfg.kappa * (1.f - clampf(a.contact[e * WBC_NFEET + l], 0.f, 1.f));
  }
  if (l < EST_NX) {                                                // x-: p + v dt + a dt^2 / 2, v + a dt, the feet as they are
    float xl = a.x[e * EST_NX + l];
    if (l < 6) {
      const int j = l < 3 ? l : l - 3;
      float acc = 0.f;
      if (a.accel) acc = est_sel(mat_mul(R, ld3(a.accel + e * 3)), j) + K.gravity[j];
      xl = l < 3 ? xl + a.x[e * EST_NX + l + 3] * dt + 0.5f * acc * dt * dt : xl + acc * dt;
    }
    X[l] = xl;
  }
  __syncthreads();

  {                                                                // P- = A P A^T + Q
    const float* Pg = a.P + e * (EST_NX * EST_NX);
    auto G = [&](int r, int c) { return r >= c ? Pg[r * EST_NX + c] : Pg[c * EST_NX + r]; };
#pragma nounroll
    for (int t = l; t < EST_NX * (EST_NX + 1) / 2; t += EST_LPE) {
      int i, j;
      delassus_tri(t, i, j);
      float v = Pg[i * EST_NX + j];
      if (j < 3) v = i < 3 ? v + dt * (G(i + 3, j) + G(j + 3, i)) + dt * dt * G(i + 3, j + 3) : v + dt * G(i, j + 3);
      if (i == j) v += dt * (i < 3 ? cfg.sigma_p * cfg.sigma_p : (i < 6 ? cfg.sigma_v * cfg.sigma_v : cfg.sigma_f * cfg.sigma_f * sC[half][(i - 6) / 3]));
      P[i][j] = v; P[j][i] = v;
    }
  }
  __syncthreads();

#pragma nounroll
  for (int t = l; t < m * EST_NX; t += EST_LPE) {                  // C P-
    const int k = t / EST_NX, j = t - k * EST_NX;
    int c1, c2, f, g;
    est_row(k, c1, c2, f, g);
    W[k][j] = c2 >= 0 ? P[c1][j] - P[c2][j] : P[c1][j];
  }
#pragma nounroll
  for (int k = l; k < m; k += EST_LPE) {                           // the residual
    int c1, c2, f, g;
    est_row(k, c1, c2, f, g);
    const int ax = g == 2 ? 2 : (g == 0 ? c1 : c1 - 3);
    W[k][EST_NX] = g == 0 ? -sK[half][f][ax] - (X[c1] - X[c2]) : (g == 1 ? -sK[half][f][3 + ax] - X[c1] : a.foot_height[e * WBC_NFEET + f] - X[c1]);
  }
  __syncthreads();
#pragma nounroll
  for (int t = l; t < m * (m + 1) / 2; t += EST_LPE) {             // S = C P- C^T + R_m, the lower triangle
    int i, j, c1, c2, f, g;
    delassus_tri(t, i, j);
    est_row(j, c1, c2, f, g);
    float s = c2 >= 0 ? W[i][c1] - W[i][c2] : W[i][c1];
    if (i == j) {
      const float sg = g == 0 ? cfg.sigma_r : (g == 1 ? cfg.sigma_rdot : cfg.sigma_z);
      s += sg * sg * sC[half][f];
    }
    S[i][j] = s;
  }
  delassus_cholesky(S, D, m, l);
  __syncthreads();
  const bool bad = l < m && !(D[l] > 0.f && D[l] <= 3.4e38f);
  const unsigned long long group_mask = EST_LPE == 64 ? ~0ull : ((1ull << (EST_LPE & 63)) - 1ull) << (half * EST_LPE & 63);
  const bool failed = (__ballot(bad) & group_mask) != 0ull;

  if (l <= EST_NX) delassus_column_forward(S, D, &W[0][l], EST_PW, m);   // W = L^-1 C P-, y = L^-1 e
  __syncthreads();

  float out = 0.f;                                                 // lane l < 18: x_l as it leaves; lane 18: NIS
  if (l < EST_NX) {
    float s = 0.f;
#pragma unroll 4
    for (int k = 0; k < m; ++k) s += W[k][l] * W[k][EST_NX];
    out = failed ? X[l] : X[l] + s;
    if (reset) {
      const int j = l % 3;
      const float p0 = a.p_init ? a.p_init[e * 3 + j] : 0.f;
      out = l < 3 ? p0 : (l < 6 ? 0.f : p0 + sK[half][(l - 6) / 3][j]);
    }
  } else if (l == EST_NX) {
#pragma unroll 4
    for (int k = 0; k < m; ++k) out += W[k][EST_NX] * W[k][EST_NX];
    if (failed || reset) out = 0.f;
  }
#pragma nounroll
  for (int t = l; t < EST_NX * (EST_NX + 1) / 2; t += EST_LPE) {   // P+ = P- - W^T W
    int i, j;
    delassus_tri(t, i, j);
    float s = P[i][j];
    if (!failed) {
#pragma unroll 4
      for (int k = 0; k < m; ++k) s -= W[k][i] * W[k][j];
    }
    if (reset) s = i != j ? 0.f : (i < 3 ? cfg.p0_p : (i < 6 ? cfg.p0_v : cfg.p0_f));
    P[i][j] = s; P[j][i] = s;
  }
  __syncthreads();                                                 // x- has been read by every lane that needs it
  if (l < EST_NX) X[l] = out;
  __syncthreads();
  if (!live) return;
  if (l < EST_NX) a.x[e * EST_NX + l] = out;
  else if (l == EST_NX) {
    if (a.nis) a.nis[e] = out;
  } else if (l == EST_NX + 1) {
    if (a.status) a.status[e] = reset ? WBC_ESTIMATOR_STATUS_RESET : (failed ? WBC_ESTIMATOR_STATUS_FAILED : WBC_ESTIMATOR_STATUS_OK);
  } else if (l < EST_NX + 5) {
    if (a.vel_body) a.vel_body[e * 3 + (l - EST_NX - 2)] = est_sel(matT_mul(R, ld3(X + 3)), l - EST_NX - 2);
  }
  float* Po = a.P + e * (EST_NX * EST_NX);
#pragma nounroll
  for (int t = l; t < EST_NX * EST_NX; t += EST_LPE) {
    const int i = t / EST_NX;
    Po[t] = P[i][t - i * EST_NX];
  }
}

void wbc_estimator_launch(const EstConst& K, const wbc_estimator_cfg& cfg, const EstArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_leg_odometry_kernel, dim3((a.n + EST_EPW - 1) / EST_EPW), dim3(64), 0, (hipStream_t)stream, K, cfg, a);
}
