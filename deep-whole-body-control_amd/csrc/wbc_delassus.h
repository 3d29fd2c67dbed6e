// wbc_delassus.h -- the contact algebra that wbc_constraint_solve_kernel, wbc_taskid_solve_kernel and wbc_taskqp_solve_kernel of
// wbc_arm_kernel.hip share: the Delassus matrix A = J Y^T + damping I of m <= 32 contact rows in LDS, its Cholesky factor and the two
// ways the kernels solve with it. One lane group (`stride` lanes, `lane` the index in it) works on one env; every kernel that calls these
// is a single-wavefront workgroup, so the __syncthreads() order the LDS traffic and cost no barrier instruction. LD and LA are the LDS
// pitches of the 26-column blocks and of A. Every kernel's bits depend on the order of these sums: do not re-associate. The unrolling of
// every loop is stated, to what the compiler chose while these statements stood in the kernels.
#pragma once
#include "wbc_device.h"

// Entry t of a lower triangle stored row by row: t = i (i + 1) / 2 + j, j <= i.
__device__ __forceinline__ void delassus_tri(int t, int& i, int& j) {
  i = (int)((__fsqrt_rn(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  i = i * (i + 1) / 2 > t ? i - 1 : ((i + 1) * (i + 2) / 2 <= t ? i + 1 : i);
  j = t - i * (i + 1) / 2;
}

// The lower triangle of A, one entry per lane and round: row i of J against row j of Y, the damping on the diagonal; where row i or j
// belongs to an inactive body (bit of `act` clear) the identity's entry instead.
template <int LD, int LA>
__device__ __forceinline__ void delassus_fill(const float (*J)[LD], const float (*Y)[LD], float (*A)[LA], int m, uint32_t act, float damping,
                                              int lane, int stride) {
#pragma nounroll
  for (int t = lane; t < m * (m + 1) / 2; t += stride) {
    int i, j;
    delassus_tri(t, i, j);
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < WBC_NCOL; ++c) a += J[i][c] * Y[j][c];
    const bool on = ((act >> i) & 1u) && ((act >> j) & 1u);
    A[i][j] = on ? (i == j ? a + damping : a) : (i == j ? 1.f : 0.f);
  }
}

// A = L L^T in place, lane i = row i, one column per round (left-looking: row i meets row j only); D[j] = 1 / L_jj. The first barrier
// orders the caller's writes of A before the first read.
template <int LA>
__device__ __forceinline__ void delassus_cholesky(float (*A)[LA], float* D, int m, int i) {
  const bool row = i < m;
#pragma nounroll
  for (int j = 0; j < m; ++j) {
    __syncthreads();
    float d = A[j][j];
#pragma unroll 8
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    const float id = 1.f / __fsqrt_rn(d);
    if (row && i > j) {
      float s = A[i][j];
#pragma unroll 8
      for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
      A[i][j] = s * id;
    }
    if (i == j) D[j] = id;
  }
}

// L L^T x = c with lane i holding entry i (ci) and the pivot's value handed round through V; on return V[0..m) = x, behind a barrier.
template <int LA>
__device__ __forceinline__ void delassus_lane_solve(const float (*A)[LA], const float* D, float* V, int m, int i, float ci) {
  const bool row = i < m;
#pragma nounroll
  for (int j = 0; j < m; ++j) {                    // L y = c
    if (i == j) V[j] = ci * D[j];
    __syncthreads();
    const float yj = V[j];
    if (i == j) ci = yj;
    else if (row && i > j) ci -= A[i][j] * yj;
  }
#pragma nounroll
  for (int j = m - 1; j >= 0; --j) {               // L^T x = y
    __syncthreads();
    if (i == j) V[j] = ci * D[j];
    __syncthreads();
    const float lj = V[j];
    if (row && i < j) ci -= A[j][i] * lj;
  }
  __syncthreads();
}

// L L^T x = x in place by one lane: x[0], x[pitch], ... is a column of a row-major block in LDS.
template <int LA>
__device__ __forceinline__ void delassus_column_solve(const float (*A)[LA], const float* D, float* x, int pitch, int m) {
#pragma nounroll
  for (int i = 0; i < m; ++i) {
    float s = x[i * pitch];
#pragma unroll 8
    for (int k = 0; k < i; ++k) s -= A[i][k] * x[k * pitch];
    x[i * pitch] = s * D[i];
  }
#pragma nounroll
  for (int i = m - 1; i >= 0; --i) {
    float s = x[i * pitch];
#pragma unroll 8
    for (int k = i + 1; k < m; ++k) s -= A[k][i] * x[k * pitch];
    x[i * pitch] = s * D[i];
  }
}

// L y = x in place by one lane, the forward half of delassus_column_solve alone (what a Kalman gain in square-root form needs: L^-1 B, never
// L^-T): x[0], x[pitch], ... is a column of a row-major block in LDS.
template <int LA>
__device__ __forceinline__ void delassus_column_forward(const float (*A)[LA], const float* D, float* x, int pitch, int m) {
#pragma nounroll
  for (int i = 0; i < m; ++i) {
    float s = x[i * pitch];
#pragma unroll 8
    for (int k = 0; k < i; ++k) s -= A[i][k] * x[k * pitch];
    x[i * pitch] = s * D[i];
  }
}
