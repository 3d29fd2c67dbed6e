// wbc_tree.h -- what the whole-body kernels of wbc_arm_kernel.hip share: the parts of their argument structs and the steps of their tree
// walks. The walks differ on purpose (what they carry, about which point, in which axes: see each kernel) and stay in the kernels. Every
// kernel's bits depend on the operand order and association of these expressions (and on their FMA contraction): do not re-associate.
#pragma once
#include "wbc_device.h"

// ---- parts of the kernel-argument structs (a kernel's struct inherits the parts its kernel reads, and no others) ------------------------
struct TreeJoints {                            // the joint between moving body b and its parent
  int32_t axis[WBC_NB], dof[WBC_NB];           // -1 for the root: no joint
  float joint_xyz[WBC_NB][3];
};
struct TreeWalk : TreeJoints {                 // what a walk from the root DOWN to b reads
  int32_t path[WBC_NB][WBC_MAX_DEPTH];         // moving bodies on the way root -> b (root excluded, b last), padded with -1
};
struct TreeCols {                              // generalised coordinates against bodies
  uint32_t anc[WBC_NB];                        // bit a: moving body a is on the path root..b (b included)
  int32_t col_body[WBC_NDOF];                  // moving body DoF d drives; -1: none (the locked fingers)
};
struct TreeRigid {                             // rigid bodies riding on the moving bodies
  int32_t rb_body[WBC_NRB];
  float rb_offset[WBC_NRB][3];
};
struct TreeInertia {                           // the model's inertias; the root's and the gripper body's are per env (tree_body_inertia)
  int32_t gripper_body;
  float mass[WBC_NB], com[WBC_NB][3], inertia[WBC_NB][6];
};
struct TreeConst : TreeWalk, TreeCols, TreeInertia {};   // a root-to-leaf walk, the column maps and the inertias

// ---- steps of the walks -----------------------------------------------------------------------------------------------------------------
// The Rodrigues matrix of a rotation about the unit vector u from (sin, cos, 1 - cos); with their derivatives instead, its derivative.
__device__ __forceinline__ void tree_rodrigues(f3 u, float s, float c, float t, float* Q) {
  const float ux = u.x, uy = u.y, uz = u.z;
  Q[0] = c + t * ux * ux; Q[1] = t * ux * uy - s * uz; Q[2] = t * ux * uz + s * uy;
  Q[3] = t * uy * ux + s * uz; Q[4] = c + t * uy * uy; Q[5] = t * uy * uz - s * ux;
  Q[6] = t * uz * ux - s * uy; Q[7] = t * uz * uy + s * ux; Q[8] = c + t * uz * uz;
}

// The joint's unit axis in its body's axes, from wbc_model's axis index (0 / 1 / 2; anything else, the root's -1: no axis, zero).
__device__ __forceinline__ f3 tree_axis(int ax) { return mk3(ax == 0 ? 1.f : 0.f, ax == 1 ? 1.f : 0.f, ax == 2 ? 1.f : 0.f); }

// Joint rotation Q of angle q about axis index ax; returns the unit axis and leaves (sin q, cos q) for the caller that differentiates.
__device__ __forceinline__ f3 tree_joint_rot(int ax, float q, float* Q, float& s, float& c) {
  const f3 u = tree_axis(ax);
  sincosf(q, &s, &c);
  tree_rodrigues(u, s, c, 1.f - c, Q);
  return u;
}
__device__ __forceinline__ f3 tree_joint_rot(int ax, float q, float* Q) {
  float s, c;
  return tree_joint_rot(ax, q, Q, s, c);
}

// En = E Q: the child's frame from the parent's, root-to-leaf. (The leaf-to-root walk of wbc_body_dynamics_kernel composes Q E.)
__device__ __forceinline__ void tree_frame_mul(const float* E, const float* Q, float* En) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) En[r * 3 + j] = E[r * 3] * Q[j] + E[r * 3 + 1] * Q[3 + j] + E[r * 3 + 2] * Q[6 + j];
}

// E <- E Q in place.
__device__ __forceinline__ void tree_frame_rot(float* E, const float* Q) {
  float En[9];
  tree_frame_mul(E, Q, En);
#pragma unroll
  for (int j = 0; j < 9; ++j) E[j] = En[j];
}

// One joint of a root-to-leaf walk: (E, p) <- (E Q, p + E xyz). Returns the joint's axis E u in the walk's axes (the new E).
__device__ __forceinline__ f3 tree_frame_step(float* E, f3& p, const float* Q, const float* xyz, f3 u) {
  p = p + mat_mul(E, mk3(xyz[0], xyz[1], xyz[2]));
  tree_frame_rot(E, Q);
  return mat_mul(E, u);
}

// One joint of the walks that carry, in the axes of E, the angular velocity w and acceleration aw and the CLASSICAL acceleration ao of the
// body's own origin (and its velocity vo, if given): the frame step, the parent's w and aw carrying its origin's motion over the lever r,
// then aw += S qdd + w x (S qd) and w += S qd. Returns the joint's axis S in the walk's axes.
__device__ __forceinline__ f3 tree_accel_step(const TreeWalk& K, int a, size_t e, const float* __restrict__ dofs, const float* __restrict__ nudot,
                                              float* E, f3& p, f3& w, f3& aw, f3& ao, f3* vo) {
  const int d = K.dof[a];
  float Q[9];
  const f3 u = tree_joint_rot(K.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * d], Q);
  const f3 r = mat_mul(E, mk3(K.joint_xyz[a][0], K.joint_xyz[a][1], K.joint_xyz[a][2]));
  p = p + r;
  if (vo) *vo = *vo + cross(w, r);
  ao = ao + cross(aw, r) + cross(w, cross(w, r));
  tree_frame_rot(E, Q);
  const f3 Sw = mat_mul(E, u);
  const float qd = dofs[e * (2 * WBC_NDOF) + 2 * d + 1], qdd = nudot ? nudot[e * WBC_NCOL + 6 + d] : 0.f;
  const f3 jw = Sw * qd;
  aw = aw + Sw * qdd + cross(w, jw);
  w = w + jw;
  return Sw;
}

// ---- inertias ---------------------------------------------------------------------------------------------------------------------------
// body_params [N, 20]: (m, com xyz, inertia xx yy zz xy xz yz) of the root's composite at slot 0 and of the gripper body at slot 10; every
// other body has the model's values. The kernels write this lookup out: as a shared inline function (results by pointer, reference or
// value) it changes which products around it the compiler contracts into FMAs, or makes a flat load, and results move by an ulp.
#define TREE_BP_STRIDE 20
#define TREE_BP_ROOT 0
#define TREE_BP_GRIPPER 10

// E I_b E^T as (xx yy zz xy xz yz): a body's rotational inertia in the axes of E.
__device__ __forceinline__ void tree_rotate_inertia(const float* E, const float* I6, float* Iw) {
  const float Ib[9] = {I6[0], I6[3], I6[4], I6[3], I6[1], I6[5], I6[4], I6[5], I6[2]};
  float EI[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) EI[r * 3 + k] = E[r * 3] * Ib[k] + E[r * 3 + 1] * Ib[3 + k] + E[r * 3 + 2] * Ib[6 + k];
  auto ibar = [&](int r, int k) { return EI[r * 3] * E[k * 3] + EI[r * 3 + 1] * E[k * 3 + 1] + EI[r * 3 + 2] * E[k * 3 + 2]; };
  Iw[0] = ibar(0, 0); Iw[1] = ibar(1, 1); Iw[2] = ibar(2, 2); Iw[3] = ibar(0, 1); Iw[4] = ibar(0, 2); Iw[5] = ibar(1, 2);
}
