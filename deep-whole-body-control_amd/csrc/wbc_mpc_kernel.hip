// wbc_mpc_kernel.hip -- the kernel of wbc_sim_centroidal_mpc (include/wbc_sim.h, which states the problem and the algorithm); its entry point
// and argument checks are with the other whole-body calls in wbc_arm_kernel.hip. A translation unit of its own: tests/test_identification.py
// pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_mpc.h"
#include "wbc_delassus.h"

// ---- convex centroidal MPC: ADMM around a Riccati solve, the whole problem in LDS ---------------------------------------------------------
// MPC_EPW envs per 64-lane workgroup, a single wavefront: env `half` on lanes MPC_LPE half .. MPC_LPE half + MPC_LPE - 1, `l` the lane in
// its group (a launch with an odd env count repeats the last env on the idle group and stores nothing from it).
//  setup    lane 0 leaves x0 (given, or from the root state and the centroidal kernel's rows); lanes l < 4 walk their leg where foot_pos is
//           NULL; one (stage, foot) per lane and round: W = I_G^-1 [r]x (zero for a swing foot); -Q x_ref, z and y (shifted, masked);
//  factor   k = H-1 .. 0, one entry of a 12 x 12 product per lane and round: B_k from the W blocks, P B, G (delassus_cholesky, lane = row),
//           [K | G^-1] by delassus_column_solve on [B^T P A | 1] in place (lane = column, 24 lanes), A - B K, P (A - B K), P_k;
//  iterate  backward: s, v, (kappa, p) -- lane = row, 12-term products against [K | G^-1] and the W blocks; forward: u, x; projection of
//           the H x 20 rows, one per lane and round. No triangular solve in the loop.
//  finish   residuals (lane-wise maxima through LDS), the clipped stage-0 forces, base_acc, every store.
// Control flow around the barriers is uniform: a failed env runs the same instructions and its stores are replaced by zeros.

// What grows with the horizon lies in dynamic LDS, one MpcStage per env and stage (445 dwords: an odd pitch between stages), so that the
// footprint that decides how many envs fit on a CU follows H; the work matrices are static.
struct MpcStage {
  float KG[MPC_NU][MPC_PK];                     // [K_k | G_k^-1]
  float W[WBC_NFEET][9];                        // I_G^-1 [r_ki]x, zero for a swing foot
  float Pd[MPC_NX];                             // P_{k+1} d
  float Z[MPC_NZ], Y[MPC_NZ], DZ[MPC_NZ];
  float U[MPC_NU];                              // kappa_k, then u_k
  float XP[MPC_NX];                             // x_{k+1}
  float QX[MPC_NX];                             // -Q x_ref_{k+1}
  int32_t cm;                                   // bit f: foot f in stance at stage k
};
static_assert(sizeof(MpcStage) == MPC_STAGE_BYTES && (MPC_STAGE_BYTES / 4) % 2 == 1, "the launcher sizes the dynamic LDS with MPC_STAGE_BYTES");
struct MpcLds {
  float P[MPC_NX][MPC_PM], T1[MPC_NX][MPC_PM], T2[MPC_NX][MPC_PM], B[MPC_NX][MPC_PM], G[MPC_NU][MPC_PM];
  float D[16], X0[MPC_NX], sv[MPC_NX], vv[MPC_NU], F[MPC_NU];
  float R0[WBC_NFEET][3], FP[WBC_NFEET][3];     // r_0i; the feet's world positions where foot_pos is NULL
  float red[2][64 / MPC_EPW];
};

__device__ __forceinline__ bool mpc_finite(float v) { return fabsf(v) <= 3.4028235e38f; }
__device__ __forceinline__ float mpc_sel(f3 v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : v.z); }

// (C^T w)_j for control j = 3 f + c from the five rows w of foot f.
__device__ __forceinline__ float mpc_ct(const float* w, int c, float mu) {
  return c == 0 ? w[1] - w[0] : (c == 1 ? w[3] - w[2] : mu * (w[0] + w[1] + w[2] + w[3]) + w[4]);
}

extern "C" __global__ void __launch_bounds__(64) wbc_centroidal_mpc_kernel(MpcConst K, wbc_mpc_cfg cfg, MpcArgs a) {
  __shared__ MpcLds lds[MPC_EPW];
  extern __shared__ float mpc_stages[];         // MpcStage [MPC_EPW][H]
  const int lane = threadIdx.x, half = lane / MPC_LPE, l = lane - half * MPC_LPE;
  const int eu = blockIdx.x * MPC_EPW + half;
  const bool live = eu < a.n;
  const size_t e = live ? eu : a.n - 1;
  MpcLds& S = lds[half];
  const int H = cfg.horizon;
  MpcStage* St = reinterpret_cast<MpcStage*>(mpc_stages) + half * H;
  const float dt = cfg.dt, hdt2 = 0.5f * cfg.dt * cfg.dt, rho = cfg.rho, mu = cfg.mu;
  bool bad = false;

  // ---- setup: mass, I_G^-1 (every lane), x0 (lane 0), the feet (lanes < 4) ----
  float m, I[9];
  if (a.mass) m = a.mass[e]; else m = a.inr[e * MPC_CM_INR];
  if (a.inertia) {
#pragma unroll
    for (int j = 0; j < 9; ++j) I[j] = a.inertia[e * 9 + j];
  } else {
    const float* q = a.inr + e * MPC_CM_INR + 1;                    // xx yy zz xy xz yz
    I[0] = q[0]; I[4] = q[1]; I[8] = q[2]; I[1] = I[3] = q[3]; I[2] = I[6] = q[4]; I[5] = I[7] = q[5];
  }
  bad = bad || !mpc_finite(m) || !(m > 0.f);
#pragma unroll
  for (int j = 0; j < 9; ++j) bad = bad || !mpc_finite(I[j]);
  float Ii[9];
  {
    const float A0 = I[4] * I[8] - I[5] * I[7], A1 = I[2] * I[7] - I[1] * I[8], A2 = I[1] * I[5] - I[2] * I[4];
    const float det = I[0] * A0 + I[3] * A1 + I[6] * A2;
    bad = bad || !(det > 0.f) || !mpc_finite(det);
    Ii[0] = A0 / det; Ii[1] = A1 / det; Ii[2] = A2 / det;
    Ii[3] = (I[5] * I[6] - I[3] * I[8]) / det; Ii[4] = (I[0] * I[8] - I[2] * I[6]) / det; Ii[5] = (I[2] * I[3] - I[0] * I[5]) / det;
    Ii[6] = (I[3] * I[7] - I[4] * I[6]) / det; Ii[7] = (I[1] * I[6] - I[0] * I[7]) / det; Ii[8] = (I[0] * I[4] - I[1] * I[3]) / det;
  }
  const float im = 1.f / m;
  const float* rs = a.root + e * 26;
  float R[9];
  {
    const float qn = 1.f / sqrtf(rs[3] * rs[3] + rs[4] * rs[4] + rs[5] * rs[5] + rs[6] * rs[6]);
    const float qu[4] = {rs[3] * qn, rs[4] * qn, rs[5] * qn, rs[6] * qn};
    quat_to_mat(qu, R);
  }
  if (l == 0) {
    if (a.x0) {
#pragma unroll
      for (int j = 0; j < MPC_NX; ++j) S.X0[j] = a.x0[e * MPC_NX + j];
    } else {
      const float psi = atan2f(R[3], R[0]);
      float sp, cp;
      sincosf(psi, &sp, &cp);
      float M[9];                                                  // R Rz(psi)^T
#pragma unroll
      for (int i = 0; i < 3; ++i) { M[3 * i] = R[3 * i] * cp - R[3 * i + 1] * sp; M[3 * i + 1] = R[3 * i] * sp + R[3 * i + 1] * cp; M[3 * i + 2] = R[3 * i + 2]; }
      const float ang = acosf(clampf((M[0] + M[4] + M[8] - 1.f) * 0.5f, -1.f, 1.f));
      const float kf = ang > 1e-3f ? ang / (2.f * sinf(ang)) : 0.5f * (1.f + ang * ang / 6.f);
      S.X0[0] = kf * (M[7] - M[5]); S.X0[1] = kf * (M[2] - M[6]); S.X0[2] = kf * (M[3] - M[1]);
      const float* cw = a.com + e * MPC_CM_COM;
#pragma unroll
      for (int j = 0; j < 3; ++j) { S.X0[3 + j] = rs[j] + cw[j]; S.X0[6 + j] = rs[10 + j]; S.X0[9 + j] = cw[3 + j]; }
    }
  }
  if (!a.foot_pos && l < WBC_NFEET) {                              // the leg walk of wbc_leg_odometry_kernel: trunk -> foot in trunk axes
    const int b = K.foot_body[l];
    const float* dq = a.dofs + e * (2 * WBC_NDOF);
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f);
#pragma nounroll
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int j = K.path[b][k];
      if (j < 0) break;
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[j], dq[2 * K.dof[j]], Q);
      tree_frame_step(E, p, Q, K.joint_xyz[j], u);
    }
    const f3 fk = p + mat_mul(E, mk3(K.foot_off[l][0], K.foot_off[l][1], K.foot_off[l][2]));
    st3(S.FP[l], ld3(rs) + mat_mul(R, fk));
  }
  if (l < H) {
    const uint8_t* c = a.contact + (e * H + l) * WBC_NFEET;
    St[l].cm = (c[0] ? 1 : 0) | (c[1] ? 2 : 0) | (c[2] ? 4 : 0) | (c[3] ? 8 : 0);
  }
  __syncthreads();
  if (l < MPC_NX) bad = bad || !mpc_finite(S.X0[l]);

#pragma nounroll
  for (int t = l; t < H * WBC_NFEET; t += MPC_LPE) {               // the W blocks
    const int k = t / WBC_NFEET, f = t - k * WBC_NFEET;
    const f3 pbar = k == 0 ? ld3(S.X0 + 3) : ld3(a.x_ref + (e * H + (k - 1)) * MPC_NX + 3);
    const f3 fp = a.foot_pos ? ld3(a.foot_pos + ((e * a.foot_pos_stages + (a.foot_pos_stages == 1 ? 0 : k)) * WBC_NFEET + f) * 3) : ld3(S.FP[f]);
    const f3 r = fp - pbar;
    bad = bad || !mpc_finite(r.x) || !mpc_finite(r.y) || !mpc_finite(r.z);
    if (k == 0) st3(S.R0[f], r);
    const bool on = (St[k].cm >> f) & 1;
    float* w = St[k].W[f];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w[3 * i] = on ? Ii[3 * i + 1] * r.z - Ii[3 * i + 2] * r.y : 0.f;
      w[3 * i + 1] = on ? Ii[3 * i + 2] * r.x - Ii[3 * i] * r.z : 0.f;
      w[3 * i + 2] = on ? Ii[3 * i] * r.y - Ii[3 * i + 1] * r.x : 0.f;
    }
  }
#pragma nounroll
  for (int t = l; t < H * MPC_NX; t += MPC_LPE) {                  // -Q x_ref
    const int k = t / MPC_NX, i = t - k * MPC_NX;
    const float xr = a.x_ref[(e * H + k) * MPC_NX + i];
    bad = bad || !mpc_finite(xr);
    St[k].QX[i] = -cfg.q[i] * xr;
  }
  const bool cold = !a.warm || (a.flags & WBC_MPC_COLD);
#pragma nounroll
  for (int t = l; t < H * MPC_NZ; t += MPC_LPE) {                  // z and y
    const int k = t / MPC_NZ, row = t - k * MPC_NZ;
    float z = 0.f, y = 0.f;
    if (!cold) {
      const int ks = (a.flags & WBC_MPC_SHIFT) ? (k + 1 < H ? k + 1 : H - 1) : k;
      z = a.warm[((e * 2 + 0) * H + ks) * MPC_NZ + row];
      y = a.warm[((e * 2 + 1) * H + ks) * MPC_NZ + row];
      bad = bad || !mpc_finite(z) || !mpc_finite(y);
    }
    const bool on = (St[k].cm >> (row / 5)) & 1;
    St[k].Z[row] = on ? z : 0.f;
    St[k].Y[row] = on ? y : 0.f;
  }
#pragma nounroll
  for (int t = l; t < MPC_NX * MPC_NX; t += MPC_LPE) {             // P_H = Q
    const int i = t / MPC_NX, j = t - i * MPC_NX;
    S.P[i][j] = i == j ? cfg.q[i] : 0.f;
  }
  const int dj = l < MPC_NX ? l % 3 : 0;
  const float dl = (l >= 3 && l < 6) ? hdt2 * K.gravity[dj] : ((l >= 9 && l < 12) ? dt * K.gravity[dj] : 0.f);   // lane l < 12: d_l
  __syncthreads();

  // ---- factor ----
#pragma nounroll
  for (int k = H - 1; k >= 0; --k) {
    const int cmk = St[k].cm;
#pragma nounroll
    for (int t = l; t < MPC_NX * MPC_NU; t += MPC_LPE) {           // B_k
      const int i = t / MPC_NU, j = t - i * MPC_NU, f = j / 3, c = j - 3 * f, blk = i / 3, r = i - 3 * blk;
      const bool on = (cmk >> f) & 1;
      const float w = St[k].W[f][3 * r + c], d = r == c ? im : 0.f;
      const float v = blk == 0 ? hdt2 * w : (blk == 1 ? hdt2 * d : (blk == 2 ? dt * w : dt * d));
      S.B[i][j] = on ? v : 0.f;
    }
    if (l < MPC_NX) {                                              // P_{k+1} d: d is zero outside rows 3..5 and 9..11
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) s += S.P[l][3 + j] * (hdt2 * K.gravity[j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) s += S.P[l][9 + j] * (dt * K.gravity[j]);
      St[k].Pd[l] = s;
    }
    __syncthreads();
#pragma nounroll
    for (int t = l; t < MPC_NX * MPC_NU; t += MPC_LPE) {           // T1 = P B
      const int i = t / MPC_NU, j = t - i * MPC_NU;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < MPC_NX; ++c) s += S.P[i][c] * S.B[c][j];
      S.T1[i][j] = s;
    }
    __syncthreads();
#pragma nounroll
    for (int t = l; t < MPC_NU * MPC_NU; t += MPC_LPE) {           // G = Rt + B^T P B; [B^T P A | 1]
      const int i = t / MPC_NU, j = t - i * MPC_NU;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < MPC_NX; ++c) s += S.B[c][i] * S.T1[c][j];
      if (i == j) {
        const int c3 = i % 3;
        s += cfg.r[c3] + rho * (c3 == 2 ? 4.f * mu * mu + 1.f : 2.f);
      }
      S.G[i][j] = s;
      St[k].KG[i][j] = j >= 6 ? S.T1[j][i] + dt * S.T1[j - 6][i] : S.T1[j][i];
      St[k].KG[i][MPC_NX + j] = i == j ? 1.f : 0.f;
    }
    delassus_cholesky(S.G, S.D, MPC_NU, l);
    __syncthreads();
    if (l < MPC_NU) bad = bad || !(S.D[l] > 0.f && S.D[l] <= 3.4e38f);
    if (l < MPC_NX + MPC_NU) delassus_column_solve(S.G, S.D, &St[k].KG[0][l], MPC_PK, MPC_NU);
    __syncthreads();
#pragma nounroll
    for (int t = l; t < MPC_NX * MPC_NX; t += MPC_LPE) {           // T2 = A - B K
      const int i = t / MPC_NX, j = t - i * MPC_NX;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < MPC_NU; ++c) s += S.B[i][c] * St[k].KG[c][j];
      S.T2[i][j] = (i == j ? 1.f : (j == i + 6 ? dt : 0.f)) - s;
    }
    __syncthreads();
#pragma nounroll
    for (int t = l; t < MPC_NX * MPC_NX; t += MPC_LPE) {           // T1 = P (A - B K)
      const int i = t / MPC_NX, j = t - i * MPC_NX;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < MPC_NX; ++c) s += S.P[i][c] * S.T2[c][j];
      S.T1[i][j] = s;
    }
    __syncthreads();
#pragma nounroll
    for (int t = l; t < MPC_NX * MPC_NX; t += MPC_LPE) {           // P_k = Q_k + A^T T1, symmetrised
      const int i = t / MPC_NX, j = t - i * MPC_NX;
      float pij = i >= 6 ? S.T1[i][j] + dt * S.T1[i - 6][j] : S.T1[i][j];
      float pji = j >= 6 ? S.T1[j][i] + dt * S.T1[j - 6][i] : S.T1[j][i];
      if (i == j && k > 0) { pij += cfg.q[i]; pji += cfg.q[i]; }
      S.P[i][j] = 0.5f * (pij + pji);
    }
    __syncthreads();
  }

  // ---- iterate ----
  float rp = 0.f;
#pragma nounroll
  for (int it = 0; it < cfg.iters; ++it) {
    const bool last = it == cfg.iters - 1;
    float pl = l < MPC_NX ? St[H - 1].QX[l] : 0.f;                  // lane l < 12: p_{k+1}, entry l
#pragma nounroll
    for (int k = H - 1; k >= 0; --k) {
      if (l < MPC_NX) S.sv[l] = pl + St[k].Pd[l];
      __syncthreads();
      if (l < MPC_NU) {
        const int f = l / 3, c = l - 3 * f;
        const float* w = St[k].W[f];
        float bts = 0.f;
        if ((St[k].cm >> f) & 1) {
#pragma unroll
          for (int i = 0; i < 3; ++i) bts += (hdt2 * w[3 * i + c]) * S.sv[i];
          bts += (hdt2 * im) * S.sv[3 + c];
#pragma unroll
          for (int i = 0; i < 3; ++i) bts += (dt * w[3 * i + c]) * S.sv[6 + i];
          bts += (dt * im) * S.sv[9 + c];
        }
        float zy[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) zy[i] = St[k].Z[5 * f + i] - St[k].Y[5 * f + i];
        S.vv[l] = bts + -rho * mpc_ct(zy, c, mu);
      }
      __syncthreads();
      if (l < MPC_NX) {
        float kap = 0.f, ktv = 0.f;
#pragma unroll
        for (int j = 0; j < MPC_NU; ++j) kap += St[k].KG[l][MPC_NX + j] * S.vv[j];
#pragma unroll
        for (int j = 0; j < MPC_NU; ++j) ktv += St[k].KG[j][l] * S.vv[j];
        St[k].U[l] = kap;
        const float ats = l >= 6 ? S.sv[l] + dt * S.sv[l - 6] : S.sv[l];
        pl = ats - ktv;
        if (k > 0) pl += St[k - 1].QX[l];
      }
      __syncthreads();
    }
#pragma nounroll
    for (int k = 0; k < H; ++k) {
      const float* x = k == 0 ? S.X0 : St[k - 1].XP;
      if (l < MPC_NU) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MPC_NX; ++i) s += St[k].KG[l][i] * x[i];
        St[k].U[l] = -s - St[k].U[l];
      }
      __syncthreads();
      if (l < MPC_NX) {
        const int blk = l / 3, r = l - 3 * blk;
        const int cmk = St[k].cm;
        const float* uk = St[k].U;
        float s = 0.f;
        if ((blk & 1) == 0) {                                      // theta / omega rows: the W blocks
          const float sc = blk == 0 ? hdt2 : dt;
#pragma unroll
          for (int f = 0; f < WBC_NFEET; ++f)
#pragma unroll
            for (int c = 0; c < 3; ++c) s += (sc * St[k].W[f][3 * r + c]) * uk[3 * f + c];
        } else {                                                   // p / v rows
          const float sc = (blk == 1 ? hdt2 : dt) * im;
#pragma unroll
          for (int f = 0; f < WBC_NFEET; ++f) s += ((cmk >> f) & 1) ? sc * uk[3 * f + r] : 0.f;
        }
        const float ax = l < 6 ? x[l] + dt * x[l + 6] : x[l];
        St[k].XP[l] = (ax + s) + dl;
      }
      __syncthreads();
    }
#pragma nounroll
    for (int t = l; t < H * MPC_NZ; t += MPC_LPE) {                // projection and dual update
      const int k = t / MPC_NZ, row = t - k * MPC_NZ, f = row / 5, r = row - 5 * f;
      const bool on = (St[k].cm >> f) & 1;
      const float* uf = St[k].U + 3 * f;
      const float cu = r == 4 ? uf[2] : ((r & 1) ? uf[r >> 1] : -uf[r >> 1]) + mu * uf[2];
      const float y = St[k].Y[row], w = cu + y;
      float zn = r == 4 ? fminf(fmaxf(w, cfg.fz_min), cfg.fz_max) : fmaxf(w, 0.f);
      float yn = w - zn;
      if (!on) { zn = 0.f; yn = 0.f; }
      if (last) {
        St[k].DZ[row] = zn - St[k].Z[row];
        if (on) rp = fmaxf(rp, fabsf(cu - zn));
      }
      St[k].Z[row] = zn;
      St[k].Y[row] = yn;
    }
    __syncthreads();
  }

  // ---- residuals, forces, base_acc ----
  float rd = 0.f;
#pragma nounroll
  for (int t = l; t < H * MPC_NU; t += MPC_LPE) {
    const int k = t / MPC_NU, j = t - k * MPC_NU, f = j / 3;
    rd = fmaxf(rd, fabsf(mpc_ct(St[k].DZ + 5 * f, j - 3 * f, mu)));
  }
  S.red[0][l] = rp;
  S.red[1][l] = rd;
  if (l < MPC_NU) {
    const int f = l / 3, c = l - 3 * f;
    const float fz = fminf(fmaxf(St[0].U[3 * f + 2], cfg.fz_min), cfg.fz_max), lim = mu * fz;
    const float v = c == 2 ? fz : fminf(fmaxf(St[0].U[l], -lim), lim);
    S.F[l] = ((St[0].cm >> f) & 1) ? v : 0.f;
  }
  __syncthreads();
  rp = 0.f; rd = 0.f;
#pragma nounroll
  for (int j = 0; j < MPC_LPE; ++j) { rp = fmaxf(rp, S.red[0][j]); rd = fmaxf(rd, S.red[1][j]); }
  rd *= rho;
  float acc = 0.f;                                                 // lane l < 6: base_acc_l
  if (l < 3) {
    acc = (((S.F[l] + S.F[3 + l]) + S.F[6 + l]) + S.F[9 + l]) / m + K.gravity[l];
  } else if (l < 6) {
    f3 tq = mk3(0.f, 0.f, 0.f);
#pragma unroll
    for (int f = 0; f < WBC_NFEET; ++f) tq = tq + cross(ld3(S.R0[f]), ld3(S.F + 3 * f));
    const int i = l - 3;
    acc = Ii[3 * i] * tq.x + Ii[3 * i + 1] * tq.y + Ii[3 * i + 2] * tq.z;
  }
  bad = bad || !mpc_finite(rp) || !mpc_finite(rd) || !mpc_finite(acc);
#pragma nounroll
  for (int t = l; t < H * MPC_NU; t += MPC_LPE) {
    const int k = t / MPC_NU, j = t - k * MPC_NU;
    bad = bad || !mpc_finite(St[k].U[j]) || !mpc_finite(St[k].XP[j]);
  }
#pragma nounroll
  for (int t = l; t < H * MPC_NZ; t += MPC_LPE) {
    const int k = t / MPC_NZ, row = t - k * MPC_NZ;
    bad = bad || !mpc_finite(St[k].Z[row]) || !mpc_finite(St[k].Y[row]);
  }
  const unsigned long long group_mask = MPC_LPE == 64 ? ~0ull : ((1ull << (MPC_LPE & 63)) - 1ull) << (half * MPC_LPE & 63);
  const bool failed = (__ballot(bad) & group_mask) != 0ull;
  if (!live) return;

  // ---- stores ----
  if (l < MPC_NU) {
    if (a.forces) a.forces[e * MPC_NU + l] = failed ? 0.f : S.F[l];
  }
  if (l < 6) {
    if (a.base_acc) a.base_acc[e * 6 + l] = failed ? 0.f : acc;
  } else if (l < 8) {
    if (a.res) a.res[e * 2 + (l - 6)] = failed ? 0.f : (l == 6 ? rp : rd);
  } else if (l == 8) {
    if (a.status) a.status[e] = failed ? WBC_MPC_STATUS_FAILED : ((rp <= cfg.tol && rd <= cfg.tol) ? WBC_MPC_STATUS_OK : WBC_MPC_STATUS_ITERATIONS);
  }
#pragma nounroll
  for (int t = l; t < H * MPC_NU; t += MPC_LPE) {
    const int k = t / MPC_NU, j = t - k * MPC_NU;
    if (a.u) a.u[e * H * MPC_NU + t] = failed ? 0.f : St[k].U[j];
    if (a.x_pred) a.x_pred[e * H * MPC_NX + t] = failed ? 0.f : St[k].XP[j];
  }
  if (a.warm) {
#pragma nounroll
    for (int t = l; t < H * MPC_NZ; t += MPC_LPE) {
      const int k = t / MPC_NZ, row = t - k * MPC_NZ;
      a.warm[((e * 2 + 0) * H + k) * MPC_NZ + row] = failed ? 0.f : St[k].Z[row];
      a.warm[((e * 2 + 1) * H + k) * MPC_NZ + row] = failed ? 0.f : St[k].Y[row];
    }
  }
}

void wbc_mpc_launch(const MpcConst& K, const wbc_mpc_cfg& cfg, const MpcArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_centroidal_mpc_kernel, dim3((a.n + MPC_EPW - 1) / MPC_EPW), dim3(64),
                     (size_t)MPC_EPW * cfg.horizon * MPC_STAGE_BYTES, (hipStream_t)stream, K, cfg, a);
}
