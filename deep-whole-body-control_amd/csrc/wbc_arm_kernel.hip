// wbc_arm_kernel.hip -- the quantities Isaac Gym hands to the torque-supervision path:
// reference widowGo1.py:550-558 wraps gym.acquire_mass_matrix_tensor / acquire_jacobian_tensor and uses
//   mm        = mass_matrix[:, -8:-2, -8:-2]          the arm's 6x6 joint-space inertia block          (WG:558)
//   ee_j_eef  = jacobian[:, gripper_idx, :6, -8:-2]    world-frame [linear; angular] Jacobian of the EE (WG:557)
//   g_torque  = sum over the last 9 rigid bodies of J_body^T (0, 0, 9.81 m_body, 0, 0, 0), arm columns  (WG:1201-1207)
// in get_arm_ee_control_torques (WG:1217-1242). Here they come from the same state tensors the step kernel keeps:
// one thread per env walks the 6-joint arm chain (forward kinematics in the base frame F, composite spatial inertias
// from the tip inwards, M_ij = S_i^T Ic_j S_j) -- an optional, once-per-step pre-pass (torque_supervision=False as shipped).
#include <cstdio>

#include "wbc_device.h"
#include "wbc_delassus.h"
#include "wbc_stream_guard.h"
#include "wbc_tree.h"
#include "wbc_proximity.h"
#include "wbc_estimator.h"
#include "wbc_footstep.h"
#include "wbc_contact.h"
#include "wbc_legctl.h"
#include "wbc_attitude.h"
#include "wbc_ground.h"
#include "wbc_slip.h"
#include "wbc_mpc.h"

#define ARM_N 6
#define ARM_NLINK 9          // rigid bodies whose weight the reference compensates: the last 9 of the actor

struct ArmConst {
  int body[ARM_N], ax[ARM_N], dof[ARM_N];      // arm chain, root outwards
  int gripper_body_depth;                      // depth of the (randomised) gripper body in the chain, -1 if none
  float joint_xyz[ARM_N][3], mass[ARM_N], com[ARM_N][3], inertia[ARM_N][6];
  int ee_depth; float ee_off[3];               // EE rigid body: chain depth of its moving body (-1: not on the arm), offset in it
  int link_depth[ARM_NLINK]; float link_off[ARM_NLINK][3], link_mass[ARM_NLINK];
  int gripper_link;                            // index in the 9 links of the randomised rigid body (-1 none)
};

extern "C" __global__ void __launch_bounds__(64) wbc_arm_dynamics_kernel(ArmConst A, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                        const float* __restrict__ body_params, const float* __restrict__ mass_params,
                                                                        int n, float* __restrict__ mm, float* __restrict__ jac,
                                                                        float* __restrict__ gtorque) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  float R[9];
  quat_to_mat(root + (size_t)env * 26 + 3, R);
  const f3 rp = ld3(root + (size_t)env * 26);
  // forward kinematics of the chain in F (base frame): E_d (columns = body axes), origin pos_d
  float E[ARM_N][9];
  f3 pos[ARM_N];
  {
    float Ep[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 pp = mk3(0.f, 0.f, 0.f);
#pragma unroll
    for (int d = 0; d < ARM_N; ++d) {
      const float q = dofs[(size_t)env * 40 + 2 * A.dof[d]];
      float sq, cq;
      sincosf(q, &sq, &cq);
      const int ax = A.ax[d], a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
      pos[d] = pp + mat_mul(Ep, mk3(A.joint_xyz[d][0], A.joint_xyz[d][1], A.joint_xyz[d][2]));
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float e0 = Ep[r * 3 + ax], e1 = Ep[r * 3 + a1], e2 = Ep[r * 3 + a2];
        E[d][r * 3 + ax] = e0;
        E[d][r * 3 + a1] = cq * e1 + sq * e2;
        E[d][r * 3 + a2] = -sq * e1 + cq * e2;
      }
#pragma unroll
      for (int e = 0; e < 9; ++e) Ep[e] = E[d][e];
      pp = pos[d];
    }
  }
  // joint axes in F; levers are formed in F (base-relative, metres) and rotated to the world afterwards, so that no
  // world-scale coordinate (envs sit at |y| up to 115 m) enters a difference
  f3 axF[ARM_N];
#pragma unroll
  for (int d = 0; d < ARM_N; ++d) {
    const int ax = A.ax[d];
    axF[d] = mk3(E[d][ax], E[d][3 + ax], E[d][6 + ax]);
  }
  (void)rp;
  // EE Jacobian, world frame, rows [linear; angular], columns = arm joints
  {
    f3 pe = mk3(0.f, 0.f, 0.f);
    if (A.ee_depth >= 0) pe = pos[A.ee_depth] + mat_mul(E[A.ee_depth], mk3(A.ee_off[0], A.ee_off[1], A.ee_off[2]));
    float* J = jac + (size_t)env * 36;
#pragma unroll
    for (int d = 0; d < ARM_N; ++d) {
      const bool moves = A.ee_depth >= d;
      const f3 lin = moves ? mat_mul(R, cross(axF[d], pe - pos[d])) : mk3(0.f, 0.f, 0.f);
      const f3 ang = moves ? mat_mul(R, axF[d]) : mk3(0.f, 0.f, 0.f);
      J[0 * 6 + d] = lin.x; J[1 * 6 + d] = lin.y; J[2 * 6 + d] = lin.z;
      J[3 * 6 + d] = ang.x; J[4 * 6 + d] = ang.y; J[5 * 6 + d] = ang.z;
    }
  }
  // gravity compensation as the reference computes it: link ORIGINS (not centres of mass), the last 9 rigid bodies;
  // the link masses are those of env 0 after its randomisation (WG:664-670 reads env 0's properties: quirk kept)
  {
    float g[ARM_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < ARM_NLINK; ++k) {
      const int dk = A.link_depth[k];
      if (dk < 0) continue;
      float mk = A.link_mass[k];
      if (k == A.gripper_link) mk += mass_params[4];
      const f3 pk = pos[dk] + mat_mul(E[dk], mk3(A.link_off[k][0], A.link_off[k][1], A.link_off[k][2]));
#pragma unroll
      for (int d = 0; d < ARM_N; ++d)
        if (d <= dk) g[d] += mk * 9.81f * mat_mul(R, cross(axF[d], pk - pos[d])).z;
    }
#pragma unroll
    for (int d = 0; d < ARM_N; ++d) gtorque[(size_t)env * ARM_N + d] = g[d];
  }
  // joint-space inertia block: composite spatial inertias in F about F's origin, from the tip inwards
  {
    float Ic[36];
#pragma unroll
    for (int e = 0; e < 36; ++e) Ic[e] = 0.f;
    float S[ARM_N][6];
#pragma unroll
    for (int d = 0; d < ARM_N; ++d) {
      const f3 l = cross(pos[d], axF[d]);
      S[d][0] = axF[d].x; S[d][1] = axF[d].y; S[d][2] = axF[d].z; S[d][3] = l.x; S[d][4] = l.y; S[d][5] = l.z;
    }
    float* M = mm + (size_t)env * 36;
#pragma unroll
    for (int d = ARM_N - 1; d >= 0; --d) {
      float m = A.mass[d], com[3], I6[6];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = A.com[d][j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = A.inertia[d][j];
      if (d == A.gripper_body_depth) {             // per-env randomised gripper body (body_params[10:20])
        const float* bp = body_params + (size_t)env * 20 + 10;
        m = bp[0];
#pragma unroll
        for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
        for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
      }
      const float* Ed = E[d];
      const f3 Cc = pos[d] + mat_mul(Ed, mk3(com[0], com[1], com[2]));
      const float Ib[9] = {I6[0], I6[3], I6[4], I6[3], I6[1], I6[5], I6[4], I6[5], I6[2]};
      float EI[9], Ibar[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) EI[r * 3 + c] = Ed[r * 3] * Ib[c] + Ed[r * 3 + 1] * Ib[3 + c] + Ed[r * 3 + 2] * Ib[6 + c];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Ibar[r * 3 + c] = EI[r * 3] * Ed[c * 3] + EI[r * 3 + 1] * Ed[c * 3 + 1] + EI[r * 3 + 2] * Ed[c * 3 + 2];
      const float CC = dot(Cc, Cc);
      const float Cv[3] = {Cc.x, Cc.y, Cc.z};
      const float Cx[9] = {0.f, -Cc.z, Cc.y, Cc.z, 0.f, -Cc.x, -Cc.y, Cc.x, 0.f};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          Ic[r * 6 + c] += Ibar[r * 3 + c] + m * ((r == c ? CC : 0.f) - Cv[r] * Cv[c]);
          Ic[r * 6 + 3 + c] += m * Cx[r * 3 + c];
          Ic[(3 + r) * 6 + c] += m * Cx[c * 3 + r];
          Ic[(3 + r) * 6 + 3 + c] += (r == c) ? m : 0.f;
        }
      float IS[6];                                 // Ic_d S_d
#pragma unroll
      for (int r = 0; r < 6; ++r) IS[r] = dot6(&Ic[r * 6], S[d]);
#pragma unroll
      for (int i = 0; i <= d; ++i) {
        const float v = dot6(S[i], IS);
        M[i * 6 + d] = v; M[d * 6 + i] = v;
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------
struct wbc_sim;
extern "C" int wbc_sim_internal_arm_inputs(wbc_sim* s, const DevConst** hc, const float** root, const float** dofs, const float** body_params,
                                           const float** mass_params, int* n);

// link_mass9: masses of the actor's last 9 rigid bodies (host pointer). Outputs (device): mm f32 [N,6,6], jac f32 [N,6,6]
// (rows linear xyz then angular xyz, world frame), gtorque f32 [N,6].
extern "C" int wbc_sim_arm_dynamics(wbc_sim* s, const int* link_rb9, const float* link_mass9, float* mm, float* jac, float* gtorque, void* stream) {
  StreamDeviceGuard sdg(stream);
  const DevConst* hc; const float *root, *dofs, *bp, *mp; int n;
  if (!s || !link_rb9 || !link_mass9 || !mm || !jac || !gtorque) return -1;
  if (wbc_sim_internal_arm_inputs(s, &hc, &root, &dofs, &bp, &mp, &n) != 0) return -1;
  const wbc_model& m = hc->model;
  ArmConst A;
  int arm = -1;
  for (int c = 0; c < WBC_NCHAIN; ++c) if (hc->chain_len[c] == ARM_N) arm = c;
  if (arm < 0) return -3;
  A.gripper_body_depth = -1;
  for (int d = 0; d < ARM_N; ++d) {
    const int b = hc->chain_body[arm][d];
    A.body[d] = b; A.ax[d] = m.axis[b]; A.dof[d] = m.dof[b]; A.mass[d] = m.mass[b];
    for (int j = 0; j < 3; ++j) { A.joint_xyz[d][j] = m.joint_xyz[b][j]; A.com[d][j] = m.com[b][j]; }
    for (int j = 0; j < 6; ++j) A.inertia[d][j] = m.inertia[b][j];
    if (b == m.gripper_body) A.gripper_body_depth = d;
  }
  auto depth_of = [&](int body) { for (int d = 0; d < ARM_N; ++d) if (A.body[d] == body) return d; return -1; };
  A.ee_depth = depth_of(m.rb_body[m.gripper_rb]);
  for (int j = 0; j < 3; ++j) A.ee_off[j] = m.rb_offset[m.gripper_rb][j];
  A.gripper_link = -1;
  for (int k = 0; k < ARM_NLINK; ++k) {
    const int rb = link_rb9[k];
    if (rb < 0 || rb >= WBC_NRB) return -1;
    A.link_depth[k] = depth_of(m.rb_body[rb]);
    for (int j = 0; j < 3; ++j) A.link_off[k][j] = m.rb_offset[rb][j];
    A.link_mass[k] = link_mass9[k];
    if (rb == m.gripper_rb) A.gripper_link = k;
  }
  hipLaunchKernelGGL(wbc_arm_dynamics_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, A, root, dofs, bp, mp, n, mm, jac, gtorque);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- whole-body Jacobian and mass matrix (Isaac Gym's acquire_jacobian_tensor / acquire_mass_matrix_tensor, WG:509-510, 550-558) --
// Coordinates nu = (v_root, omega_root, qd[0..WBC_NDOF-1]) (include/wbc_sim.h). One 64-lane workgroup per env: forward kinematics,
// spatial inertias and composites into LDS, then two sweeps in which consecutive lanes store consecutive 16-byte pieces of the env's
// J [27,6,26] and M [26,26] rows (structural zeros included), so every store instruction writes 1 KB of one contiguous range.
// J is assembled in LDS a chunk of rigid bodies at a time (one lane per rigid body and column) and copied out.
#define BD_NCOL WBC_NCOL                        // 26 generalised coordinates
#define BD_JROW (6 * BD_NCOL)                  // 156 floats of J per rigid body
#define BD_JENV (WBC_NRB * BD_JROW)            // 4212 floats of J per env
#define BD_MENV (BD_NCOL * BD_NCOL)            // 676 floats of M per env
#define BD_JCHUNK 9                            // rigid bodies per LDS chunk of J (5.6 KB)
static_assert(WBC_NRB % BD_JCHUNK == 0 && (BD_JCHUNK * BD_JROW) % 4 == 0, "J chunks");

struct BodyConst : TreeJoints, TreeCols, TreeRigid, TreeInertia {
  int32_t parent[WBC_NB];                      // this kernel walks from b UP to the root
};

extern "C" __global__ void __launch_bounds__(64) wbc_body_dynamics_kernel(BodyConst B, const float* __restrict__ root,
                                                                         const float* __restrict__ dofs,
                                                                         const float* __restrict__ body_params, int n,
                                                                         float* __restrict__ jac, float* __restrict__ mm) {
  __shared__ float sE[WBC_NB][9], sP[WBC_NB][3];   // body rotation (columns = body axes) and origin in F
  __shared__ float sI[WBC_NB][10];                 // spatial inertia about F's origin, in F: m, m c (3), rotational xx yy zz xy xz yz
  __shared__ float sIc[WBC_NB][10];                // the same, composite of the subtree
  __shared__ float sAw[WBC_NB][3], sOw[WBC_NB][3]; // joint axis and body origin, world axes, relative to the root origin
  __shared__ float sDw[WBC_NRB][3];                // rigid-body origin, world axes, relative to the root origin
  __shared__ uint32_t sAnc[WBC_NB], sRbAnc[WBC_NRB];
  __shared__ int32_t sColBody[BD_NCOL];            // 0 for the six root columns, the driven body, or -1
  __shared__ float sS[BD_NCOL][6], sF[BD_NCOL][6]; // per column: motion subspace (omega; v at F's origin) in F, and Ic S
  extern __shared__ float4 sJ4[];                  // dynamic, only when jac is written: BD_JCHUNK rigid bodies' rows of J, as stored
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= n) return;
  float R[9];
  quat_to_mat(root + (size_t)env * 26 + 3, R);

  // 1) forward kinematics in F, lane b = moving body b: compose the joint transforms from b up to the root
  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f);
    int a = b;
    for (int it = 0; it < WBC_MAX_DEPTH && a > 0; ++it) {      // (E, p) <- (Rot_a E, xyz_a + Rot_a p)
      float Q[9], En[9];
      tree_joint_rot(B.axis[a], dofs[(size_t)env * (2 * WBC_NDOF) + 2 * B.dof[a]], Q);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) En[r * 3 + k] = Q[r * 3] * E[k] + Q[r * 3 + 1] * E[3 + k] + Q[r * 3 + 2] * E[6 + k];
#pragma unroll
      for (int e = 0; e < 9; ++e) E[e] = En[e];
      p = mk3(B.joint_xyz[a][0], B.joint_xyz[a][1], B.joint_xyz[a][2]) + mat_mul(Q, p);
      a = B.parent[a];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) sE[b][e] = E[e];
    st3(sP[b], p);
    // spatial inertia about F's origin: the per-env root composite and gripper body (body_params), the model's otherwise
    float m = B.mass[b], com[3] = {B.com[b][0], B.com[b][1], B.com[b][2]}, I6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) I6[j] = B.inertia[b][j];
    const int slot = b == 0 ? TREE_BP_ROOT : (b == B.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + (size_t)env * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
    }
    float Ibar[6];
    const f3 C = p + mat_mul(E, mk3(com[0], com[1], com[2]));
    tree_rotate_inertia(E, I6, Ibar);
    const float CC = dot(C, C);
    sI[b][0] = m; sI[b][1] = m * C.x; sI[b][2] = m * C.y; sI[b][3] = m * C.z;
    sI[b][4] = Ibar[0] + m * (CC - C.x * C.x);
    sI[b][5] = Ibar[1] + m * (CC - C.y * C.y);
    sI[b][6] = Ibar[2] + m * (CC - C.z * C.z);
    sI[b][7] = Ibar[3] - m * C.x * C.y;
    sI[b][8] = Ibar[4] - m * C.x * C.z;
    sI[b][9] = Ibar[5] - m * C.y * C.z;
    const int ax = B.axis[b];                                  // -1 for the root: no joint axis
    const f3 axF = mk3(ax == 0 ? E[0] : ax == 1 ? E[1] : ax == 2 ? E[2] : 0.f,
                       ax == 0 ? E[3] : ax == 1 ? E[4] : ax == 2 ? E[5] : 0.f,
                       ax == 0 ? E[6] : ax == 1 ? E[7] : ax == 2 ? E[8] : 0.f);
    st3(sAw[b], mat_mul(R, axF));
    st3(sOw[b], mat_mul(R, p));
    sAnc[b] = B.anc[b];
  }
  __syncthreads();

  // 2) composite inertias (a plain sum: every body's inertia is already about F's origin) and the rigid-body levers
  if (lane < WBC_NB) {
    float acc[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) acc[j] = 0.f;
    for (int d = 0; d < WBC_NB; ++d)
      if ((sAnc[d] >> lane) & 1u) {
#pragma unroll
        for (int j = 0; j < 10; ++j) acc[j] += sI[d][j];
      }
#pragma unroll
    for (int j = 0; j < 10; ++j) sIc[lane][j] = acc[j];
  } else if (lane >= 32 && lane < 32 + WBC_NRB) {
    const int r = lane - 32, b = B.rb_body[r];
    const f3 pF = ld3(sP[b]) + mat_mul(sE[b], mk3(B.rb_offset[r][0], B.rb_offset[r][1], B.rb_offset[r][2]));
    st3(sDw[r], mat_mul(R, pF));
    sRbAnc[r] = sAnc[b];
  }
  __syncthreads();

  // 3) per generalised coordinate c: its motion subspace S_c in F and F_c = Ic S_c of the subtree it moves. The root columns are
  //    those of the world-frame coordinates (v_F = R^T v_root, omega_F = R^T omega_root), i.e. M = T^T M_F T with T = diag(R^T, R^T, 1).
  if (lane < BD_NCOL) {
    const int c = lane;
    int b = 0;
    float S[6];
    if (c < 6) {
      const int j = c < 3 ? c : c - 3;
      const f3 row = matT_mul(R, mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f));
      const bool lin = c < 3;
      S[0] = lin ? 0.f : row.x; S[1] = lin ? 0.f : row.y; S[2] = lin ? 0.f : row.z;
      S[3] = lin ? row.x : 0.f; S[4] = lin ? row.y : 0.f; S[5] = lin ? row.z : 0.f;
    } else {
      b = B.col_body[c - 6];
      if (b >= 0) {
        const int ax = B.axis[b];
        const f3 a = mk3(sE[b][ax], sE[b][3 + ax], sE[b][6 + ax]), l = cross(ld3(sP[b]), a);
        S[0] = a.x; S[1] = a.y; S[2] = a.z; S[3] = l.x; S[4] = l.y; S[5] = l.z;
      } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) S[j] = 0.f;
      }
    }
    float Fv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (b >= 0) {
      const float* I = sIc[b];
      const f3 w = mk3(S[0], S[1], S[2]), v = mk3(S[3], S[4], S[5]), h = mk3(I[1], I[2], I[3]);
      const f3 top = mk3(I[4] * w.x + I[7] * w.y + I[8] * w.z, I[7] * w.x + I[5] * w.y + I[9] * w.z,
                         I[8] * w.x + I[9] * w.y + I[6] * w.z) + cross(h, v);
      const f3 bot = cross(w, h) + I[0] * v;
      Fv[0] = top.x; Fv[1] = top.y; Fv[2] = top.z; Fv[3] = bot.x; Fv[4] = bot.y; Fv[5] = bot.z;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) { sS[c][j] = S[j]; sF[c][j] = Fv[j]; }
    sColBody[c] = b;
  }
  __syncthreads();

  // 4) M: M_ij = S_i . (Ic S_j) with j's body in the subtree of i's (and symmetrically), 0 where neither moves the other
  if (mm) {
    float4* out = reinterpret_cast<float4*>(mm + (size_t)env * BD_MENV);
    for (int t = lane; t < BD_MENV / 4; t += 64) {
      float v[4];
      int i = (4 * t) / BD_NCOL, j = 4 * t - i * BD_NCOL;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int bi = sColBody[i], bj = sColBody[j];
        float x = 0.f;
        if (bi >= 0 && bj >= 0) {
          if ((sAnc[bj] >> bi) & 1u) x = dot6(sS[i], sF[j]);
          else if ((sAnc[bi] >> bj) & 1u) x = dot6(sS[j], sF[i]);
        }
        v[u] = x;
        if (++j == BD_NCOL) { j = 0; ++i; }
      }
      out[t] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }

  // 5) J, BD_JCHUNK rigid bodies at a time: one lane per (rigid body, column) writes that column's six rows into an LDS copy of the
  //    output rows, which the wave then stores 16 bytes per lane. Levers from world-axis vectors relative to the root origin.
  if (jac) {
    float* sJ = reinterpret_cast<float*>(sJ4);
    float4* out = reinterpret_cast<float4*>(jac + (size_t)env * BD_JENV);
    for (int r0 = 0; r0 < WBC_NRB; r0 += BD_JCHUNK) {
      for (int it = lane; it < BD_JCHUNK * BD_NCOL; it += 64) {
        const int rr = it / BD_NCOL, c = it - rr * BD_NCOL, r = r0 + rr;
        const f3 d = ld3(sDw[r]);
        f3 lin = mk3(0.f, 0.f, 0.f), ang = mk3(0.f, 0.f, 0.f);
        if (c < 6) {
          const int j = c < 3 ? c : c - 3;
          const f3 e = mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
          if (c < 3) lin = e;                                  // v_root: identity on the linear rows
          else { lin = cross(e, d); ang = e; }                 // omega_root: e_j x d_r, identity on the angular rows
        } else {
          const int b = sColBody[c];
          if (b >= 0 && ((sRbAnc[r] >> b) & 1u)) {
            ang = ld3(sAw[b]);
            lin = cross(ang, d - ld3(sOw[b]));
          }
        }
        float* o = sJ + rr * BD_JROW + c;
        o[0] = lin.x; o[BD_NCOL] = lin.y; o[2 * BD_NCOL] = lin.z;
        o[3 * BD_NCOL] = ang.x; o[4 * BD_NCOL] = ang.y; o[5 * BD_NCOL] = ang.z;
      }
      __syncthreads();
      for (int t = lane; t < BD_JCHUNK * BD_JROW / 4; t += 64) out[r0 * (BD_JROW / 4) + t] = sJ4[t];
      __syncthreads();
    }
  }
}

// ---- host side of the whole-body calls ------------------------------------------------------------------------------------------------
extern "C" int wbc_sim_internal_fail(int code, const char* msg);

// What every whole-body entry point starts from: the stream's device current for the call's duration, the sim's state tensors (`have`:
// there is a sim) and the refusals "<entry point>: <what>" for wbc_last_error(). Its own argument checks stay in the entry point, in order.
struct WbCall {
  StreamDeviceGuard sdg;
  const char* who;
  const DevConst* hc = nullptr;
  const float *root = nullptr, *dofs = nullptr, *bp = nullptr, *mp = nullptr;
  int n = 0;
  bool have;
  WbCall(const char* who_, wbc_sim* s, void* stream) : sdg(stream), who(who_) {
    have = s && wbc_sim_internal_arm_inputs(s, &hc, &root, &dofs, &bp, &mp, &n) == 0;
  }
  int fail(int code, const char* what) const {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return wbc_sim_internal_fail(code, msg);
  }
  int no_sim() const { return fail(-1, "sim is NULL"); }
  int no_state() const { return fail(-1, "no sim state"); }
  int no_tree() const { return fail(-3, "the model's tree is not one the kernel walks"); }
  int launched() const { return hipGetLastError() == hipSuccess ? 0 : fail(-2, "launch failed"); }   // after a launch
};

// The parts of the argument structs (wbc_tree.h) from the model, one function each. 0, or 1: a tree the kernels cannot walk.
static int tree_joints_fill(const wbc_model& m, TreeJoints& J) {
  for (int b = 0; b < WBC_NB; ++b) {
    J.axis[b] = m.axis[b]; J.dof[b] = m.dof[b];
    for (int j = 0; j < 3; ++j) J.joint_xyz[b][j] = m.joint_xyz[b][j];
    // the kernels walk at most WBC_MAX_DEPTH joints between a body and the root and index 32-bit ancestor masks
    int depth = 0;
    for (int a = b; a > 0; a = m.parent[a])
      if (m.parent[a] < 0 || m.parent[a] >= a || ++depth > WBC_MAX_DEPTH || m.axis[a] < 0 || m.axis[a] > 2 || m.dof[a] < 0 || m.dof[a] >= WBC_NDOF)
        return 1;
  }
  return 0;
}
static int tree_walk_fill(const wbc_model& m, TreeWalk& W) {
  if (tree_joints_fill(m, W) != 0) return 1;
  for (int b = 0; b < WBC_NB; ++b) {
    int up[WBC_MAX_DEPTH], depth = 0;                          // tree_joints_fill bounded the depth
    for (int a = b; a > 0; a = m.parent[a]) up[depth++] = a;
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) W.path[b][k] = k < depth ? up[depth - 1 - k] : -1;
  }
  return 0;
}
static void tree_cols_fill(const wbc_model& m, TreeCols& C) {
  for (int d = 0; d < WBC_NDOF; ++d) C.col_body[d] = -1;
  for (int b = 0; b < WBC_NB; ++b) {
    C.anc[b] = 1u << b;
    for (int a = b; a > 0; a = m.parent[a]) C.anc[b] |= 1u << m.parent[a];
    if (b > 0) C.col_body[m.dof[b]] = b;
  }
}
static bool tree_rigid_ok(const wbc_model& m) {
  for (int r = 0; r < WBC_NRB; ++r)
    if (m.rb_body[r] < 0 || m.rb_body[r] >= WBC_NB) return false;
  return true;
}
// 0, or 2: a rigid body that rides on no moving body.
static int tree_rigid_fill(const wbc_model& m, TreeRigid& B) {
  if (!tree_rigid_ok(m)) return 2;
  for (int r = 0; r < WBC_NRB; ++r) {
    B.rb_body[r] = m.rb_body[r];
    for (int j = 0; j < 3; ++j) B.rb_offset[r][j] = m.rb_offset[r][j];
  }
  return 0;
}
static void tree_inertia_fill(const wbc_model& m, TreeInertia& I) {
  I.gripper_body = m.gripper_body;
  for (int b = 0; b < WBC_NB; ++b) {
    I.mass[b] = m.mass[b];
    for (int j = 0; j < 3; ++j) I.com[b][j] = m.com[b][j];
    for (int j = 0; j < 6; ++j) I.inertia[b][j] = m.inertia[b][j];
  }
}
// 0, or 1: a model the whole-body calls refuse (a bad rb_body too, whether or not the kernel reads the rigid bodies).
static int tree_const_fill(const wbc_model& m, TreeConst& K) {
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return 1;
  tree_cols_fill(m, K); tree_inertia_fill(m, K);
  return 0;
}

// Outputs (device, caller-owned, 16-byte aligned, either may be NULL): jac f32 [N,27,6,26], mm f32 [N,26,26] (include/wbc_sim.h).
extern "C" int wbc_sim_body_dynamics(wbc_sim* s, float* jac, float* mm, void* stream) {
  WbCall c("wbc_sim_body_dynamics", s, stream);
  if (!s) return c.no_sim();
  if (!jac && !mm) return c.fail(-1, "jac and mm are both NULL");
  if (((uintptr_t)jac | (uintptr_t)mm) & 15u) return c.fail(-1, "jac / mm must be 16-byte aligned");
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  BodyConst B;
  if (tree_joints_fill(m, B) != 0) return c.no_tree();
  if (tree_rigid_fill(m, B) != 0) return c.fail(-3, "bad rb_body");
  tree_cols_fill(m, B); tree_inertia_fill(m, B);
  for (int b = 0; b < WBC_NB; ++b) B.parent[b] = m.parent[b];
  // the J chunk is dynamic LDS: a mass-matrix-only refresh keeps the small footprint (twice the resident envs per CU)
  const size_t jbytes = jac ? BD_JCHUNK * BD_JROW * sizeof(float) : 0;
  hipLaunchKernelGGL(wbc_body_dynamics_kernel, dim3(c.n), dim3(64), jbytes, (hipStream_t)stream, B, c.root, c.dofs, c.bp, c.n, jac, mm);
  return c.launched();
}

// ---- whole-body inverse dynamics: tau = M nudot + C nu + g in the coordinates of wbc_sim_body_dynamics (include/wbc_sim.h) ---------
// Recursive Newton-Euler with every spatial vector about F's origin in F's axes, so neither pass needs a parent-child transform.
// Two envs per 64-lane workgroup, one per 32-lane half (19 bodies / 26 columns fit in 32 lanes); two phases, ONE LDS hand-over:
//  1) lane b = moving body b walks its ancestor path from the root DOWN (TreeWalk::path), one tree_frame_step per joint, and carries in registers the frame (E, p),
//     the spatial velocity and the spatial acceleration. The depth-sequential velocity-product term v x S qd is thereby a
//     loop-carried register dependence of at most WBC_MAX_DEPTH steps (each lane redoes its ancestors' joints) instead of an LDS
//     round trip per tree level. Then the body's force m a_com and its moment about F's origin (from I_b alpha + omega x I_b omega
//     about the centre of mass, in body axes) go to LDS with (m, m c), and with the torque of the body's own force and weight
//     about its OWN joint, formed in body axes.
//  2) lane c = generalised coordinate c sums the forces of the subtree it moves (ancestor masks; a joint's own body through its
//     own-joint torque) and projects on S_c; the root columns carry T = diag(R^T, R^T, 1) as in the mass matrix. g(q) comes from
//     the subtree's (m, m c) and is added at the end (equivalent to a_0 -= g, more accurate: see phase 2).
// The root position is never read.
#ifndef ID_EPW
#define ID_EPW 2                                // envs per workgroup: 2, or 1 (-DID_EPW=1, the variant DESIGN.md compares with)
#endif
static_assert(ID_EPW == 1 || ID_EPW == 2, "one env per 64 lanes or one per 32-lane half");
struct IdConst : TreeConst { float gravity[3]; };

extern "C" __global__ void __launch_bounds__(64) wbc_inverse_dynamics_kernel(IdConst K, const float* __restrict__ root,
                                                                            const float* __restrict__ dofs,
                                                                            const float* __restrict__ body_params,
                                                                            const float* __restrict__ nudot, int n,
                                                                            float* __restrict__ tau, float* __restrict__ grav) {
  __shared__ __align__(16) float sF[ID_EPW][WBC_NB][12];   // per body: force (moment about F's origin; force) in F at 0..5, own-joint torques at 6, 7, (m, m c) at 8..11
  __shared__ float sS[ID_EPW][WBC_NB][6];          // the body's joint in F: axis, origin
  const int half = ID_EPW == 2 ? threadIdx.x >> 5 : 0, lane = ID_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * ID_EPW + half;
  const bool live = env < n, dyn = tau != nullptr;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  const f3 gF = matT_mul(R, mk3(K.gravity[0], K.gravity[1], K.gravity[2]));

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f), Sw = p, Sv = p;
    // spatial velocity (vw; vv) and acceleration (aw; av) of the root in F. nudot[0:3] is the CLASSICAL acceleration of the
    // root origin: a spatial acceleration's linear part is R^T a - omega x v.
    f3 vw = p, vv = p, aw = p, av = p;
    if (dyn) {
      vv = matT_mul(R, ld3(root + e * 26 + 7));
      vw = matT_mul(R, ld3(root + e * 26 + 10));
      if (nudot) { av = matT_mul(R, ld3(nudot + e * BD_NCOL)); aw = matT_mul(R, ld3(nudot + e * BD_NCOL + 3)); }
      av = av - cross(vw, vv);
    }
#pragma nounroll                                  // kept a loop, as the compiler chose to while the step was written out here
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int a = K.path[b][k];
      if (a < 0) break;
      const int d = K.dof[a];
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * d], Q);
      Sw = tree_frame_step(E, p, Q, K.joint_xyz[a], u);
      Sv = cross(p, Sw);
      if (dyn) {
        const float qd = dofs[e * (2 * WBC_NDOF) + 2 * d + 1], qdd = nudot ? nudot[e * BD_NCOL + 6 + d] : 0.f;
        const f3 jw = Sw * qd, jv = Sv * qd;                   // a += S qdd + v x (S qd), then v += S qd
        aw = aw + Sw * qdd + cross(vw, jw);
        av = av + Sv * qdd + cross(vw, jv) + cross(vv, jw);
        vw = vw + jw; vv = vv + jv;
      }
    }
    // spatial inertia about F's origin: the per-env root composite and gripper body (body_params), the model's otherwise
    float m = K.mass[b], com[3] = {K.com[b][0], K.com[b][1], K.com[b][2]}, I6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) I6[j] = K.inertia[b][j];
    const int slot = b == 0 ? TREE_BP_ROOT : (b == K.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + e * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
    }
    // The body's own joint sees the body's own force through the lever (com x axis) in BODY axes, where the axis is a unit vector
    // and the lever is the model's: a force that (nearly) passes through the axis then yields its small torque to fp32 accuracy,
    // which the difference of two moments about the far base origin would not. Descendants reach the joint through F (phase 2).
    const int axb = K.axis[b];                                 // -1 for the root: no joint axis
    const f3 cm = mk3(com[0], com[1], com[2]), ub = tree_axis(axb);
    const f3 C = p + mat_mul(E, cm), h = m * C, lev = cross(cm, ub);
    float* o = sF[half][b];
    if (dyn) {
      // classical acceleration of the centre of mass from the spatial one, force m a_com in F, moment about the centre of mass in
      // body axes (I_b alpha + omega x I_b omega with the model's inertia as it stands)
      const f3 acom = av + cross(aw, C) + cross(vw, vv + cross(vw, C)), fl = m * acom;
      const f3 wl = matT_mul(E, vw), al = matT_mul(E, aw);
      const float Ib[9] = {I6[0], I6[3], I6[4], I6[3], I6[1], I6[5], I6[4], I6[5], I6[2]};
      const f3 ncl = mat_mul(Ib, al) + cross(wl, mat_mul(Ib, wl));
      st3(o, mat_mul(E, ncl) + cross(C, fl)); st3(o + 3, fl);  // about F's origin, in F: what the ancestors' joints see
      o[6] = dot(ub, ncl) - dot(lev, matT_mul(E, fl));         // u . (n_c + com x f) = u . n_c - (com x u) . f, body axes
    }
    o[7] = m * dot(matT_mul(E, gF), lev);                      // the same for the body's weight -m g: m g . (com x u)
    o[8] = m; st3(o + 9, h);
    st3(sS[half][b], Sw); st3(sS[half][b] + 3, p);
  }
  __syncthreads();

  if (lane < BD_NCOL) {
    const int c = lane, b = c < 6 ? 0 : K.col_body[c - 6], bb = b < 0 ? 0 : b;
    const int j = c < 3 ? c : c - 3;
    float S[6];                                                // motion subspace (omega; v at F's origin) in F
    f3 po = mk3(0.f, 0.f, 0.f);                                // joint origin in F
    if (c < 6) {                                               // world-frame root coordinates: rows of R
      const f3 row = matT_mul(R, mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f));
      const bool lin = c < 3;
      S[0] = lin ? 0.f : row.x; S[1] = lin ? 0.f : row.y; S[2] = lin ? 0.f : row.z;
      S[3] = lin ? row.x : 0.f; S[4] = lin ? row.y : 0.f; S[5] = lin ? row.z : 0.f;
    } else {
      const f3 a = ld3(sS[half][bb]);
      po = ld3(sS[half][bb] + 3);
      const f3 l = cross(po, a);
      S[0] = a.x; S[1] = a.y; S[2] = a.z; S[3] = l.x; S[4] = l.y; S[5] = l.z;
    }
    float acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.f;
    for (int d = 0; d < WBC_NB; ++d) {                         // subtree sums: every force is already about F's origin
      const bool in = ((K.anc[d] >> bb) & 1u) && (c < 6 || d != bb);   // a joint's own body comes in through slots 6, 7
      const float4* f4 = reinterpret_cast<const float4*>(sF[half][d]);
      if (dyn) {
        const float4 u = f4[0];
        const float2 w = *reinterpret_cast<const float2*>(sF[half][d] + 4);
        acc[0] += in ? u.x : 0.f; acc[1] += in ? u.y : 0.f; acc[2] += in ? u.z : 0.f; acc[3] += in ? u.w : 0.f;
        acc[4] += in ? w.x : 0.f; acc[5] += in ? w.y : 0.f;
      }
      const float4 u = f4[2];
      acc[8] += in ? u.x : 0.f; acc[9] += in ? u.y : 0.f; acc[10] += in ? u.z : 0.f; acc[11] += in ? u.w : 0.f;
    }
    // g(q) from the subtree's (m, m c): the net force is -m g in WORLD axes as it stands, the root moment is formed in world axes
    // and a joint's torque takes the lever about the joint's own origin, so that the weight (the largest term of most rows) meets
    // no rotation there and back and no moment about the far base origin. tau = (Newton-Euler without gravity) + g(q).
    float gv = 0.f;
    if (b >= 0) {
      const f3 gw = mk3(K.gravity[0], K.gravity[1], K.gravity[2]), hs = mk3(acc[9], acc[10], acc[11]);
      if (c < 3) gv = -acc[8] * (j == 0 ? gw.x : j == 1 ? gw.y : gw.z);
      else if (c < 6) { const f3 nw = cross(gw, mat_mul(R, hs)); gv = j == 0 ? nw.x : j == 1 ? nw.y : nw.z; }
      else gv = sF[half][bb][7] + dot(mk3(S[0], S[1], S[2]), cross(gF, hs - acc[8] * po));
    }
    if (live) {
      if (tau) tau[e * BD_NCOL + c] = b >= 0 ? ((c < 6 ? 0.f : sF[half][bb][6]) + dot6(S, acc)) + gv : 0.f;
      if (grav) grav[e * BD_NCOL + c] = gv;
    }
  }
}

// Fills K from the model. 0, or 1: a model the kernels refuse.
static int id_const_fill(const DevConst* hc, IdConst& K) {
  if (tree_const_fill(hc->model, K) != 0) return 1;
  for (int j = 0; j < 3; ++j) K.gravity[j] = hc->cfg.gravity[j];
  return 0;
}

// nudot (device f32 [N,26] or NULL = zeros), tau / grav (device f32 [N,26], caller-owned, either may be NULL): include/wbc_sim.h.
extern "C" int wbc_sim_inverse_dynamics(wbc_sim* s, const float* nudot, float* tau, float* grav, void* stream) {
  WbCall c("wbc_sim_inverse_dynamics", s, stream);
  if (!s) return c.no_sim();
  if (!tau && !grav) return c.fail(-1, "tau and grav are both NULL");
  if (((uintptr_t)nudot | (uintptr_t)tau | (uintptr_t)grav) & 3u) return c.fail(-1, "nudot / tau / grav must be 4-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  IdConst K;
  if (id_const_fill(c.hc, K) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_inverse_dynamics_kernel, dim3((c.n + ID_EPW - 1) / ID_EPW), dim3(64), 0, (hipStream_t)stream, K, c.root, c.dofs, c.bp, nudot,
                     c.n, tau, grav);
  return c.launched();
}

// ---- mass-matrix solves: out = M^-1 rhs in the coordinates of wbc_sim_body_dynamics (include/wbc_sim.h) ------------------------------
// M never leaves the launch. Live coordinates s (the 24 that are not locked fingers) are ordered root 0..5, then chain by chain from
// the root outwards, so every coordinate's ancestors precede it: the six root coordinates (a "chain" of six) and the joints between the
// root and its own. Row s of M is kept in LDS as [the root columns | its chain's columns up to itself]: position u of a row is the same
// coordinate in the rows of all its ancestors, and nothing outside these rows is ever non-zero -- Featherstone's L^T D L factorisation
// (leaves first) has no fill-in. MS_EPW envs per 64-lane workgroup, one per lane group:
//  1) lane b = moving body b: forward kinematics root -> b in registers (tree_frame_step per joint), centre of mass and
//     rotational inertia about it in F to LDS;
//  2) lane s = coordinate s: composite of the subtree it moves ABOUT ITS OWN JOINT ORIGIN (the root: F's origin), so that the light
//     wrist joints' entries are not the difference of two moments about the far base origin, and F_s = Ic_s S_s;
//  3) M[s][i] = S_i . F_s for every ancestor-or-self i of s, the force moved to i's origin (a chain-local lever), one entry per lane;
//  4) elimination k = last .. first: the ancestors' rows lose row_k^T row_k / D_k, one entry pair per lane, one LDS round per k;
//  5) lane r = right-hand side r: x = L^-1 D^-1 L^-T b with the root's six values and one chain's values in registers.
// A single-wavefront workgroup: the __syncthreads() below order the LDS traffic and cost no barrier instruction.
// The root position is never read.
#ifndef MS_EPW
#define MS_EPW 2                                // envs per workgroup: 2, or 1 (-DMS_EPW=1, the variant DESIGN.md compares with)
#endif
static_assert(MS_EPW == 1 || MS_EPW == 2, "one env per 64 lanes or one per 32-lane half");
#define MS_NS (6 + WBC_NB - 1)                  // live coordinates at most: the root's six and one per joint
#define MS_W (6 + WBC_MAX_DEPTH)                // a row: the root columns, the chain's, the diagonal at position (number of ancestors)
#define MS_LPE (64 / MS_EPW)                    // lanes per env
#define MS_BT 16                                // floats per body / per coordinate in the tables of phases 1-3
#define MS_TN ((WBC_NB + MS_NS) * MS_BT)        // those tables; the solve's hand-over between its two passes reuses them
static_assert(WBC_SOLVE_MAX_RHS <= MS_LPE && (MS_NS - 6) * WBC_SOLVE_MAX_RHS <= MS_TN && WBC_NB <= MS_LPE && MS_NS <= MS_LPE, "lanes / LDS reuse");
struct MsConst {
  TreeConst K;
  int32_t ns;                                  // live coordinates
  int32_t co_body[MS_NS], co_col[MS_NS];       // moving body and column (of 26) of coordinate s
  int32_t co_na[MS_NS], co_anc0[MS_NS];        // number of ancestors; the coordinate at row position 6 (its chain's first joint)
  int32_t nchain, ch_base[WBC_NCHAIN], ch_len[WBC_NCHAIN];
  float arm[MS_NS];                            // wbc_task_cfg.joint_armature of coordinate s (0 for the root's)
};

extern "C" __global__ void __launch_bounds__(64) wbc_mass_solve_kernel(MsConst C, const float* __restrict__ root,
                                                                      const float* __restrict__ dofs,
                                                                      const float* __restrict__ body_params,
                                                                      const float* __restrict__ rhs, int64_t rhs_stride, int nrhs,
                                                                      const float* __restrict__ sub, int n, float* __restrict__ out,
                                                                      int64_t out_stride, int armature) {
  __shared__ float sH[MS_EPW][MS_NS][MS_W];        // rows of M, then of L (unit lower, M = L^T D L)
  __shared__ float sID[MS_EPW][MS_NS];             // 1 / D
  __shared__ float sT[MS_EPW][MS_TN];
  const TreeConst& K = C.K;
  const int half = MS_EPW == 2 ? threadIdx.x >> 5 : 0, lane = MS_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * MS_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  float* sB = sT[half];                            // per body: origin 0..2, joint axis 3..5, m 6, centre of mass 7..9, inertia about it 10..15, all in F
  float* sC = sT[half] + WBC_NB * MS_BT;           // per coordinate: S = (w 0..2; v 3..5) about P 6..8, F = Ic S = (n 9..11; f 12..14) about P
  float (*H)[MS_W] = sH[half];
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f), Sw = p;
#pragma nounroll                                  // kept a loop, as the compiler chose to while the step was written out here
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int a = K.path[b][k];
      if (a < 0) break;
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * K.dof[a]], Q);
      Sw = tree_frame_step(E, p, Q, K.joint_xyz[a], u);
    }
    float m = K.mass[b], com[3] = {K.com[b][0], K.com[b][1], K.com[b][2]}, I6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) I6[j] = K.inertia[b][j];
    const int slot = b == 0 ? TREE_BP_ROOT : (b == K.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + e * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
    }
    float Iw[6];
    tree_rotate_inertia(E, I6, Iw);
    float* o = sB + b * MS_BT;
    st3(o, p); st3(o + 3, Sw); o[6] = m; st3(o + 7, p + mat_mul(E, mk3(com[0], com[1], com[2])));
    o[10] = Iw[0]; o[11] = Iw[1]; o[12] = Iw[2]; o[13] = Iw[3]; o[14] = Iw[4]; o[15] = Iw[5];
  }
  __syncthreads();

  if (lane < C.ns) {
    const int s = lane, b = C.co_body[s];
    const f3 P = ld3(sB + b * MS_BT);              // the root's origin is F's: (0, 0, 0)
    float m = 0.f, xx = 0.f, yy = 0.f, zz = 0.f, xy = 0.f, xz = 0.f, yz = 0.f;
    f3 h = mk3(0.f, 0.f, 0.f);
    for (int d = 0; d < WBC_NB; ++d)
      if ((K.anc[d] >> b) & 1u) {
        const float* q = sB + d * MS_BT;
        const float md = q[6];
        const f3 r = ld3(q + 7) - P;
        const float rr = dot(r, r);
        m += md; h = h + md * r;
        xx += q[10] + md * (rr - r.x * r.x); yy += q[11] + md * (rr - r.y * r.y); zz += q[12] + md * (rr - r.z * r.z);
        xy += q[13] - md * r.x * r.y; xz += q[14] - md * r.x * r.z; yz += q[15] - md * r.y * r.z;
      }
    f3 w = mk3(0.f, 0.f, 0.f), v = w;
    if (s < 6) {                                   // world-frame root coordinates: rows of R
      const int j = s < 3 ? s : s - 3;
      const f3 row = matT_mul(R, mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f));
      if (s < 3) v = row; else w = row;
    } else {
      w = ld3(sB + b * MS_BT + 3);
    }
    const f3 nn = mk3(xx * w.x + xy * w.y + xz * w.z, xy * w.x + yy * w.y + yz * w.z, xz * w.x + yz * w.y + zz * w.z) + cross(h, v);
    const f3 ff = cross(w, h) + m * v;
    float* o = sC + s * MS_BT;
    st3(o, w); st3(o + 3, v); st3(o + 6, P); st3(o + 9, nn); st3(o + 12, ff);
  }
  __syncthreads();

  for (int t = lane; t < C.ns * MS_W; t += MS_LPE) {
    const int s = t / MS_W, u = t - s * MS_W, na = C.co_na[s];
    if (u > na) continue;
    const int i = u == na ? s : (u < 6 ? u : C.co_anc0[s] + u - 6);
    const float *ci = sC + i * MS_BT, *cs = sC + s * MS_BT;
    const f3 f = ld3(cs + 12);
    float x = dot(ld3(ci), ld3(cs + 9) + cross(ld3(cs + 6) - ld3(ci + 6), f)) + dot(ld3(ci + 3), f);
    if (i == s && armature) x += C.arm[s];
    H[s][u] = x;
  }
  __syncthreads();

  for (int k = C.ns - 1; k > 0; --k) {
    const int na = C.co_na[k], a0 = C.co_anc0[k];
    const float id = 1.f / H[k][na];
    for (int t = lane; t < na * (na + 1) / 2; t += MS_LPE) {
      int u = (int)((__fsqrt_rn(8.f * (float)t + 1.f) - 1.f) * 0.5f);          // t = u (u + 1) / 2 + v, v <= u
      u = u * (u + 1) / 2 > t ? u - 1 : ((u + 1) * (u + 2) / 2 <= t ? u + 1 : u);
      const int v = t - u * (u + 1) / 2;
      H[u < 6 ? u : a0 + u - 6][v] -= H[k][u] * id * H[k][v];
    }
    __syncthreads();
  }
  for (int t = lane; t < C.ns * MS_W; t += MS_LPE) {
    const int s = t / MS_W, u = t - s * MS_W, na = C.co_na[s];
    const float id = 1.f / H[s][na];
    if (u < na) H[s][u] *= id;
    if (u == MS_W - 1) sID[half][s] = id;
  }
  __syncthreads();                                 // (also: the tables of phases 1-3 are dead from here on)

  if (lane >= nrhs || !live) return;
  const float* bp = rhs ? rhs + e * rhs_stride + (size_t)lane * BD_NCOL : nullptr;
  const float* hp = sub ? sub + e * BD_NCOL : nullptr;
  float* op = out + e * out_stride + (size_t)lane * BD_NCOL;
  float* stash = sT[half] + lane;                  // [coordinate - 6][right-hand side]
  auto ld = [&](int s) { const int c = C.co_col[s]; return (bp ? bp[c] : 0.f) - (hp ? hp[c] : 0.f); };
  float xr[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) xr[j] = ld(j);
  for (int c = 0; c < C.nchain; ++c) {             // x <- L^-T b, leaves first; D^-1 on the way out
    const int base = C.ch_base[c], len = C.ch_len[c];
    float xc[WBC_MAX_DEPTH];
#pragma unroll
    for (int d = 0; d < WBC_MAX_DEPTH; ++d) xc[d] = d < len ? ld(base + d) : 0.f;
#pragma unroll
    for (int d = WBC_MAX_DEPTH - 1; d >= 0; --d)
      if (d < len) {
        const float* row = H[base + d];
        const float xk = xc[d];
#pragma unroll
        for (int j = 0; j < 6; ++j) xr[j] -= row[j] * xk;
#pragma unroll
        for (int q = 0; q < d; ++q) xc[q] -= row[6 + q] * xk;
        stash[(base + d - 6) * WBC_SOLVE_MAX_RHS] = xk * sID[half][base + d];
      }
  }
#pragma unroll
  for (int k = 5; k > 0; --k)
#pragma unroll
    for (int j = 0; j < k; ++j) xr[j] -= H[k][j] * xr[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) {                    // x <- L^-1 x, the root first
    float a = xr[k] * sID[half][k];
#pragma unroll
    for (int j = 0; j < k; ++j) a -= H[k][j] * xr[j];
    xr[k] = a;
    op[C.co_col[k]] = a;
  }
  for (int c = 0; c < C.nchain; ++c) {
    const int base = C.ch_base[c], len = C.ch_len[c];
    float xc[WBC_MAX_DEPTH];
#pragma unroll
    for (int d = 0; d < WBC_MAX_DEPTH; ++d)
      if (d < len) {
        const float* row = H[base + d];
        float a = stash[(base + d - 6) * WBC_SOLVE_MAX_RHS];
#pragma unroll
        for (int j = 0; j < 6; ++j) a -= row[j] * xr[j];
#pragma unroll
        for (int q = 0; q < d; ++q) a -= row[6 + q] * xc[q];
        xc[d] = a;
        op[C.co_col[base + d]] = a;
      }
  }
  for (int d = 0; d < WBC_NDOF; ++d)               // the locked fingers: exactly 0
    if (K.col_body[d] < 0) op[6 + d] = 0.f;
}

extern "C" int wbc_sim_internal_fd_scratch(wbc_sim* s, float** h);

// Fills C from the model and the chains. 0, or 1: a tree the kernel cannot walk.
static int ms_const_fill(const DevConst* hc, MsConst& C) {
  const wbc_model& m = hc->model;
  if (tree_const_fill(m, C.K) != 0) return 1;
  for (int s = 0; s < MS_NS; ++s) { C.co_body[s] = 0; C.co_col[s] = s < 6 ? s : 0; C.co_na[s] = s < 6 ? s : 0; C.co_anc0[s] = 6; C.arm[s] = 0.f; }
  int s = 6;
  C.nchain = 0;
  for (int c = 0; c < WBC_NCHAIN; ++c) {
    const int len = hc->chain_len[c];
    if (len <= 0) continue;
    if (len > WBC_MAX_DEPTH || s + len > MS_NS) return 1;
    C.ch_base[C.nchain] = s; C.ch_len[C.nchain] = len; ++C.nchain;
    for (int d = 0; d < len; ++d, ++s) {
      const int b = hc->chain_body[c][d];
      // every chain hangs off the root and is serial: the rows' layout and the solve's register passes rely on it
      if (b <= 0 || b >= WBC_NB || m.parent[b] != (d == 0 ? 0 : hc->chain_body[c][d - 1])) return 1;
      C.co_body[s] = b; C.co_col[s] = 6 + m.dof[b]; C.co_na[s] = 6 + d; C.co_anc0[s] = s - d;
      C.arm[s] = m.dof[b] < WBC_NACT ? hc->cfg.joint_armature[m.dof[b]] : 0.f;
    }
  }
  for (int c = C.nchain; c < WBC_NCHAIN; ++c) { C.ch_base[c] = 6; C.ch_len[c] = 0; }
  if (s != 6 + WBC_NB - 1) return 1;                // a moving body on no chain
  C.ns = s;
  return 0;
}

// out_env_stride (floats): 26 nrhs for the contiguous [N, nrhs, 26]; a caller that solves a wider block in chunks passes the block's own.
static int mass_solve_launch(const WbCall& c, const float* rhs, int64_t rhs_env_stride, int nrhs, const float* sub, float* out,
                             int64_t out_env_stride, int flags, void* stream) {
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  MsConst C;
  if (ms_const_fill(c.hc, C) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_mass_solve_kernel, dim3((c.n + MS_EPW - 1) / MS_EPW), dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, c.bp, rhs,
                     rhs_env_stride, nrhs, sub, c.n, out, out_env_stride, (flags & WBC_SOLVE_ARMATURE) ? 1 : 0);
  return c.launched();
}

// rhs (device f32, right-hand side k of env e at rhs + e * rhs_env_stride + 26 k), out (device f32 [N, nrhs, 26]): include/wbc_sim.h.
extern "C" int wbc_sim_mass_solve(wbc_sim* s, const float* rhs, int64_t rhs_env_stride, int nrhs, float* out, int flags, void* stream) {
  WbCall c("wbc_sim_mass_solve", s, stream);
  if (!s) return c.no_sim();
  if (!rhs || !out) return c.fail(-1, "rhs / out is NULL");
  if (nrhs < 1 || nrhs > WBC_SOLVE_MAX_RHS) return c.fail(-1, "nrhs must be 1..WBC_SOLVE_MAX_RHS");
  if (rhs_env_stride < (int64_t)BD_NCOL * nrhs) return c.fail(-1, "rhs_env_stride is below 26 * nrhs");
  if (flags & ~WBC_SOLVE_ARMATURE) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)rhs | (uintptr_t)out) & 3u) return c.fail(-1, "rhs / out must be 4-byte aligned");
  return mass_solve_launch(c, rhs, rhs_env_stride, nrhs, nullptr, out, (int64_t)nrhs * BD_NCOL, flags, stream);
}

// nudot = M^-1 (tau - h): wbc_inverse_dynamics_kernel writes h into the sim's [N, 26] scratch, the solve subtracts it as it loads.
// The two launches, arguments checked by the entry point c speaks for (wbc_sim_forward_dynamics, wbc_sim_forward_dynamics_sensitivity).
static int forward_dynamics_run(const WbCall& c, wbc_sim* s, const float* tau, float* nudot, int flags, void* stream) {
  float* h = nullptr;
  if (wbc_sim_internal_fd_scratch(s, &h) != 0) return -1;
  const int rc = wbc_sim_inverse_dynamics(s, nullptr, h, nullptr, stream);
  if (rc != 0) return rc;
  return mass_solve_launch(c, tau, BD_NCOL, 1, h, nudot, BD_NCOL, flags, stream);
}

extern "C" int wbc_sim_forward_dynamics(wbc_sim* s, const float* tau, float* nudot, int flags, void* stream) {
  WbCall c("wbc_sim_forward_dynamics", s, stream);
  if (!s) return c.no_sim();
  if (!nudot) return c.fail(-1, "nudot is NULL");
  if (flags & ~WBC_SOLVE_ARMATURE) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)tau | (uintptr_t)nudot) & 3u) return c.fail(-1, "tau / nudot must be 4-byte aligned");
  return forward_dynamics_run(c, s, tau, nudot, flags, stream);
}

// ---- rigid-body accelerations and contact-constrained forward dynamics (include/wbc_sim.h) ---------------------------------------------
// acc = J nudot + Jdot nu for every rigid-body origin, and the solve of
//     M nudot + h = tau + sum_r J_r^T lambda_r,    J_r nudot + (Jdot nu)_r = a_des_r - damping lambda_r
// for up to WBC_CONSTR_MAX_BODIES bodies whose origins' linear accelerations are prescribed. Both start from ba_walk: a lane follows
// TreeWalk::path from the root DOWN, one tree_accel_step (wbc_tree.h) per joint, and carries the frame (E, p), the angular velocity w,
// the angular acceleration a_w and the classical acceleration a_o of the body's origin in F's axes in registers. With x a point of the
// body relative to that origin, its classical acceleration is R (a_o + a_w x x + w x (w x x)) and the angular one R a_w. The root
// position is never read.
#ifndef BA_EPW
#define BA_EPW 2                                // envs per workgroup of the three kernels below: 2, or 1 (-DBA_EPW=1, the variant DESIGN.md compares with)
#endif
static_assert(BA_EPW == 1 || BA_EPW == 2, "one env per 64 lanes or one per 32-lane half");
#define BA_LPE (64 / BA_EPW)                    // lanes per env
#define CD_MAXROWS (3 * WBC_CONSTR_MAX_BODIES)  // 15 constraint rows at most
#define CD_GSTRIDE 16                           // floats of gamma per env in the workspace
#define CD_LD 27                                // LDS row pitch of the 26-column blocks (odd: rows land in different banks)
static_assert(WBC_NRB <= BA_LPE && WBC_NB + WBC_CONSTR_MAX_BODIES <= BA_LPE && CD_MAXROWS + 1 <= WBC_SOLVE_MAX_RHS && CD_MAXROWS <= CD_GSTRIDE, "lanes");
struct BaConst : TreeWalk, TreeRigid {};

// The walk root -> b. On return (E, p) is body b's frame in F, w and aw its angular velocity and acceleration and ao the CLASSICAL
// acceleration of its own origin p, all in F's axes. Every body's acceleration is carried at that body's origin, not about F's: the
// terms added per joint are aw x r + w x (w x r) with r the step from the parent's origin to the child's, so the rounding error is
// proportional to the terms the tests' magnitude sums. (Spatial vectors about F's origin, as wbc_inverse_dynamics_kernel carries them,
// add w x v_O and w x (w x x) of size |w|^2 |x| that cancel down to |w|^2 |x - p| at a far body: 78 x 2^-24 of the magnitude at the
// arm's links in rollout states.) The root's linear velocity enters no acceleration and is never read; nudot[0:3] is the classical
// acceleration of the root origin, so a body fixed to a root that does not accelerate gets exactly w x (w x x).
__device__ __forceinline__ void ba_walk(const TreeWalk& K, int b, size_t e, const float* R, const float* __restrict__ root,
                                        const float* __restrict__ dofs, const float* __restrict__ nudot, float* E, f3& p, f3& w, f3& aw,
                                        f3& ao) {
  p = mk3(0.f, 0.f, 0.f);
  aw = p; ao = p;
  w = matT_mul(R, ld3(root + e * 26 + 10));
  if (nudot) { ao = matT_mul(R, ld3(nudot + e * BD_NCOL)); aw = matT_mul(R, ld3(nudot + e * BD_NCOL + 3)); }
#pragma nounroll                                  // kept a loop, as the compiler chose to while the step was written out here
  for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
    const int a = K.path[b][k];
    if (a < 0) break;
    tree_accel_step(K, a, e, dofs, nudot, E, p, w, aw, ao, nullptr);
  }
}

// Lane r = rigid body r (27 of the 32 lanes of an env's half). No LDS: a lane stores its own six floats (the output needs 4-byte
// alignment only, so the stores are single dwords; a wavefront's two rows are one contiguous 1296-byte range).
extern "C" __global__ void __launch_bounds__(64) wbc_body_accel_kernel(BaConst K, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                      const float* __restrict__ nudot, int n, float* __restrict__ acc) {
  const int half = BA_EPW == 2 ? threadIdx.x >> 5 : 0, lane = BA_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * BA_EPW + half;
  if (env >= n || lane >= WBC_NRB) return;
  const size_t e = env;
  const int r = lane;
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  f3 p, w, aw, ao;
  ba_walk(K, K.rb_body[r], e, R, root, dofs, nudot, E, p, w, aw, ao);
  const f3 xo = mat_mul(E, mk3(K.rb_offset[r][0], K.rb_offset[r][1], K.rb_offset[r][2]));   // the rigid body's origin from the moving body's
  const f3 lin = mat_mul(R, ao + cross(aw, xo) + cross(w, cross(w, xo))), ang = mat_mul(R, aw);
  float* o = acc + (e * WBC_NRB + r) * 6;
  st3(o, lin); st3(o + 3, ang);
}

struct CdConst : TreeWalk, TreeRigid, TreeCols {
  int32_t nb, rb[WBC_CONSTR_MAX_BODIES];       // the listed rigid bodies
};

// The walk phase of the two right-hand-side kernels, one lane (W and B: the bases of the kernel's argument struct): lane b < 19 = moving
// body b leaves its joint axis and origin (F) in sJ[b]; a lane past them walks to listed body k (rigid body r), leaves its origin in
// sX[k] and returns true with the body's Jdot nu in world axes: lin of its origin, ang.
__device__ __forceinline__ bool rhs_walk_lane(const TreeWalk& W, const TreeRigid& B, int lane, int k, int r, size_t e, const float* R,
                                              const float* __restrict__ root, const float* __restrict__ dofs, float (*sJ)[6], float (*sX)[3],
                                              f3& lin, f3& ang) {
  const bool body = lane < WBC_NB;
  const int b = body ? lane : B.rb_body[r];
  float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  f3 p, w, aw, ao;
  ba_walk(W, b, e, R, root, dofs, nullptr, E, p, w, aw, ao);
  if (body) {
    st3(sJ[b], mat_mul(E, tree_axis(W.axis[b])));    // -1 for the root: no joint axis
    st3(sJ[b] + 3, p);
    return false;
  }
  const f3 xo = mat_mul(E, mk3(B.rb_offset[r][0], B.rb_offset[r][1], B.rb_offset[r][2]));
  st3(sX[k], p + xo);
  lin = mat_mul(R, ao + cross(aw, xo) + cross(w, cross(w, xo)));
  ang = mat_mul(R, aw);
  return true;
}

// Column c's entry of the three linear Jacobian rows of a rigid body that rides on moving body lb with its origin at x (F): b the moving
// body column c drives (-1: none), ej the unit vector of a root column.
__device__ __forceinline__ f3 rhs_jac_lin(const TreeCols& C, int c, int b, int lb, f3 ej, const float* R, f3 x, const float (*sJ)[6]) {
  f3 lin = mk3(0.f, 0.f, 0.f);
  if (c < 3) lin = ej;                                   // v_root: identity
  else if (c < 6) lin = cross(ej, mat_mul(R, x));        // omega_root: e_j x (origin relative to the root, world axes)
  else if (b >= 0 && ((C.anc[lb] >> b) & 1u)) lin = mat_mul(R, cross(ld3(sJ[b]), x - ld3(sJ[b] + 3)));
  return lin;
}

// The right-hand-side block of the solve, [N, 3 nb + 1, 26]: rows 3k..3k+2 the linear Jacobian rows of listed body k (zeros where it
// is inactive), the last row tau - h; and gamma [N, CD_GSTRIDE] = (Jdot nu) of those rows. Lane b < 19 = moving body b leaves its joint
// axis and origin (F) in LDS, lane 19 + k walks to listed body k and leaves its origin; then lane c = column c writes its entry of
// every row, so a row is one 104-byte store of consecutive lanes.
extern "C" __global__ void __launch_bounds__(64) wbc_constraint_rhs_kernel(CdConst C, const float* __restrict__ root,
                                                                          const float* __restrict__ dofs,
                                                                          const uint8_t* __restrict__ active, const float* __restrict__ tau,
                                                                          const float* __restrict__ h, int n, float* __restrict__ rhs,
                                                                          float* __restrict__ gamma) {
  __shared__ float sJ[BA_EPW][WBC_NB][6];          // joint axis, joint origin, in F
  __shared__ float sX[BA_EPW][WBC_CONSTR_MAX_BODIES][3];   // listed body's origin in F
  const int half = BA_EPW == 2 ? threadIdx.x >> 5 : 0, lane = BA_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * BA_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  const int nb = C.nb, nrow = 3 * nb + 1;
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  if (lane < WBC_NB + nb) {
    const int k = lane < WBC_NB ? 0 : lane - WBC_NB;
    f3 lin, ang;
    if (rhs_walk_lane(C, C, lane, k, C.rb[k], e, R, root, dofs, sJ[half], sX[half], lin, ang) && live) st3(gamma + e * CD_GSTRIDE + 3 * k, lin);
  }
  __syncthreads();
  if (lane < BD_NCOL && live) {
    const int c = lane, b = c < 6 ? 0 : C.col_body[c - 6], j = c < 3 ? c : c - 3;
    const f3 ej = mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
    float* o = rhs + e * (size_t)(nrow * BD_NCOL) + c;
    for (int k = 0; k < nb; ++k) {
      const bool act = active ? active[e * nb + k] != 0 : true;
      f3 lin = mk3(0.f, 0.f, 0.f);
      if (act) lin = rhs_jac_lin(C, c, b, C.rb_body[C.rb[k]], ej, R, ld3(sX[half][k]), sJ[half]);
      o[(3 * k) * BD_NCOL] = lin.x; o[(3 * k + 1) * BD_NCOL] = lin.y; o[(3 * k + 2) * BD_NCOL] = lin.z;
    }
    o[3 * nb * BD_NCOL] = b >= 0 ? (tau ? tau[e * BD_NCOL + c] : 0.f) - h[e * BD_NCOL + c] : 0.f;
  }
}

// Per env, with m = 3 nb rows, J the rows of the right-hand-side block and Y = (M^-1 [J^T | tau - h])^T the mass solve's output:
// A = J Y^T + damping I from its lower triangle (one entry per lane and round), identity rows and columns where a body is inactive;
// c = a_des - gamma - J a_free; Cholesky A = L L^T in LDS, lane i = row i, one column per round (left-looking: row i meets row j only);
// the two triangular solves with lane i holding entry i and the pivot's value handed round through LDS; nudot = a_free + Y^T lambda,
// lane c = column c. The fill, the factor and the solves are wbc_delassus.h's, on this half's views of the LDS arrays. A single-wavefront
// workgroup: the __syncthreads() order the LDS traffic and cost no barrier instruction.
extern "C" __global__ void __launch_bounds__(64) wbc_constraint_solve_kernel(const float* __restrict__ rhs, const float* __restrict__ Y,
                                                                            const float* __restrict__ gamma,
                                                                            const uint8_t* __restrict__ active,
                                                                            const float* __restrict__ acc_des, float damping, int nb,
                                                                            uint32_t live_cols, int n, float* __restrict__ nudot,
                                                                            float* __restrict__ lambda) {
  __shared__ float sJ[BA_EPW][CD_MAXROWS][CD_LD], sY[BA_EPW][CD_MAXROWS + 1][CD_LD];
  __shared__ float sA[BA_EPW][CD_MAXROWS][CD_MAXROWS + 1];   // lower triangle: A, then L
  __shared__ float sD[BA_EPW][CD_MAXROWS + 1], sV[BA_EPW][CD_MAXROWS + 1];   // 1 / L_jj; the value handed round
  const int half = BA_EPW == 2 ? threadIdx.x >> 5 : 0, lane = BA_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * BA_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  const int m = 3 * nb;
  float (*J)[CD_LD] = sJ[half], (*Yt)[CD_LD] = sY[half];
  float (*A)[CD_MAXROWS + 1] = sA[half];
  float *D = sD[half], *V = sV[half];
  const float *rp = rhs + e * (size_t)((m + 1) * BD_NCOL), *yp = Y + e * (size_t)((m + 1) * BD_NCOL);
  for (int t = lane; t < (m + 1) * BD_NCOL; t += BA_LPE) {
    const int r = t / BD_NCOL, c = t - r * BD_NCOL;
    Yt[r][c] = yp[t];
    if (r < m) J[r][c] = rp[t];
  }
  uint32_t act = 0;                                // bit i: row i belongs to an active body
  for (int k = 0; k < nb; ++k)
    if (!active || active[e * nb + k]) act |= 7u << (3 * k);
  __syncthreads();

  delassus_fill(J, Yt, A, m, act, damping, lane, BA_LPE);
  const int i = lane;
  const bool row = i < m, on = row && ((act >> i) & 1u);
  float ci = 0.f;
  if (on) {
    float a = 0.f;
    for (int c = 0; c < BD_NCOL; ++c) a += J[i][c] * Yt[m][c];
    ci = ((acc_des ? acc_des[e * m + i] : 0.f) - gamma[e * CD_GSTRIDE + i]) - a;
  }
  delassus_cholesky(A, D, m, i);
  delassus_lane_solve(A, D, V, m, i, ci);
  if (!live) return;
  if (lambda && row) lambda[e * m + i] = on ? V[i] : 0.f;
  if (lane < BD_NCOL) {
    float a = Yt[m][lane];
    for (int k = 0; k < m; ++k) a += Yt[k][lane] * V[k];
    nudot[e * BD_NCOL + lane] = ((live_cols >> lane) & 1u) ? a : 0.f;
  }
}

// W and B are the two bases of one argument struct (BaConst, CdConst, TiConst). 0, or 1: a model the kernels refuse.
static int ba_const_fill(const wbc_model& m, TreeWalk& W, TreeRigid& B) { return tree_walk_fill(m, W) != 0 || tree_rigid_fill(m, B) != 0; }

// nudot (device f32 [N,26] or NULL = zeros), acc (device f32 [N,27,6]): include/wbc_sim.h.
extern "C" int wbc_sim_body_accelerations(wbc_sim* s, const float* nudot, float* acc, void* stream) {
  WbCall c("wbc_sim_body_accelerations", s, stream);
  if (!s) return c.no_sim();
  if (!acc) return c.fail(-1, "acc is NULL");
  if (((uintptr_t)nudot | (uintptr_t)acc) & 3u) return c.fail(-1, "nudot / acc must be 4-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  BaConst A;
  if (ba_const_fill(c.hc->model, A, A) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_body_accel_kernel, dim3((c.n + BA_EPW - 1) / BA_EPW), dim3(64), 0, (hipStream_t)stream, A, c.root, c.dofs, nudot, c.n, acc);
  return c.launched();
}

// Workspace layout (floats): the right-hand-side block [N, 3 nb + 1, 26], the mass solve's output of the same shape, gamma [N, 16].
extern "C" size_t wbc_sim_constrained_dynamics_workspace_floats(int num_envs, int nbodies) {
  if (num_envs <= 0 || nbodies < 1 || nbodies > WBC_CONSTR_MAX_BODIES) return 0;
  return (size_t)num_envs * (2 * (size_t)(3 * nbodies + 1) * BD_NCOL + CD_GSTRIDE);
}

// Four launches on `stream`: h (the existing inverse-dynamics kernel, into the sim's scratch), the right-hand-side block, the existing
// mass solve with 3 nb + 1 right-hand sides, the constraint solve. Arguments and conventions: include/wbc_sim.h. The body of
// wbc_sim_constrained_dynamics and the first stage of wbc_sim_constrained_dynamics_derivatives (c.who names the entry point in a refusal);
// C comes back filled for the caller that goes on.
static int constrained_dynamics_run(const WbCall& c, wbc_sim* s, const int32_t* rigid_bodies, int nbodies, const uint8_t* active, const float* tau,
                                    const float* acc_des, float damping, int flags, float* nudot, float* lambda, float* workspace, void* stream,
                                    CdConst& C) {
  if (!s) return c.no_sim();
  if (!rigid_bodies || !nudot || !workspace) return c.fail(-1, "rigid_bodies / nudot / workspace is NULL");
  if (nbodies < 1 || nbodies > WBC_CONSTR_MAX_BODIES) return c.fail(-1, "nbodies must be 1..WBC_CONSTR_MAX_BODIES");
  if (!(damping >= 0.f) || !(damping <= 3.4e38f)) return c.fail(-1, "damping must be finite and >= 0");
  if (flags & ~WBC_SOLVE_ARMATURE) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)tau | (uintptr_t)acc_des | (uintptr_t)nudot | (uintptr_t)lambda | (uintptr_t)workspace) & 3u)
    return c.fail(-1, "tau / acc_des / nudot / lambda / workspace must be 4-byte aligned");
  if (!c.have) return c.no_state();
  for (int k = 0; k < nbodies; ++k)
    if (rigid_bodies[k] < 0 || rigid_bodies[k] >= WBC_NRB) return c.fail(-1, "rigid-body index outside 0..WBC_NRB-1");
  if (ba_const_fill(c.hc->model, C, C) != 0) return c.no_tree();
  for (int k = 0; k < nbodies; ++k)
    for (int l = 0; l < k; ++l)
      if (C.rb_body[rigid_bodies[k]] == C.rb_body[rigid_bodies[l]])
        return c.fail(-1, "two listed rigid bodies ride on the same moving body (dependent rows)");
  const int n = c.n;
  if (n <= 0) return 0;
  tree_cols_fill(c.hc->model, C);
  uint32_t live_cols = 63u;
  for (int d = 0; d < WBC_NDOF; ++d) if (C.col_body[d] >= 0) live_cols |= 1u << (6 + d);
  C.nb = nbodies;
  for (int k = 0; k < WBC_CONSTR_MAX_BODIES; ++k) C.rb[k] = rigid_bodies[k < nbodies ? k : 0];
  float* h = nullptr;
  if (wbc_sim_internal_fd_scratch(s, &h) != 0) return -1;
  const int nrow = 3 * nbodies + 1;
  float *blk = workspace, *Y = blk + (size_t)n * nrow * BD_NCOL, *gamma = Y + (size_t)n * nrow * BD_NCOL;
  int rc = wbc_sim_inverse_dynamics(s, nullptr, h, nullptr, stream);
  if (rc != 0) return rc;
  const dim3 grid((n + BA_EPW - 1) / BA_EPW);
  hipLaunchKernelGGL(wbc_constraint_rhs_kernel, grid, dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, active, tau, (const float*)h, n, blk, gamma);
  if ((rc = c.launched()) != 0) return rc;
  rc = mass_solve_launch(c, blk, (int64_t)nrow * BD_NCOL, nrow, nullptr, Y, (int64_t)nrow * BD_NCOL, flags, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(wbc_constraint_solve_kernel, grid, dim3(64), 0, (hipStream_t)stream, (const float*)blk, (const float*)Y, (const float*)gamma, active,
                     acc_des, damping, nbodies, live_cols, n, nudot, lambda);
  return c.launched();
}

extern "C" int wbc_sim_constrained_dynamics(wbc_sim* s, const int32_t* rigid_bodies, int nbodies, const uint8_t* active, const float* tau,
                                            const float* acc_des, float damping, int flags, float* nudot, float* lambda, float* workspace,
                                            void* stream) {
  WbCall c("wbc_sim_constrained_dynamics", s, stream);
  CdConst C;
  return constrained_dynamics_run(c, s, rigid_bodies, nbodies, active, tau, acc_des, damping, flags, nudot, lambda, workspace, stream, C);
}

// ---- contact impulses and post-impact velocities (include/wbc_sim.h: wbc_sim_impulse_dynamics) ------------------------------------------
// The impulse-level counterpart of the call above: with u_r = J_r nu the pre-impact velocity of listed body r's origin,
//     M (nu+ - nu) = iota + sum_r J_r^T Lambda_r ,    J_r nu+ + damping Lambda_r = vdes_r - e_r (u_r - vdes_r) .
// No h enters, so there are three launches: the right-hand-side block [J_c^T | iota], the mass solve, the impulse solve.

// The right-hand-side block [N, 3 nb + 1, 26] as wbc_constraint_rhs_kernel writes it, with iota (zeros where NULL or on a finger column)
// in the last row. Positions and joint axes only: lane b < 19 = moving body b walks root -> b with frame steps alone (no velocity or
// acceleration is carried: the pre-impact contact velocity is the product J nu, formed in the solve kernel) and leaves its joint axis
// and origin (F) in LDS; lane 19 + k walks to listed body k and leaves its origin. Then lane c = column c writes its entry of every
// row: a row is one 104-byte store of consecutive lanes.
extern "C" __global__ void __launch_bounds__(64) wbc_impulse_rhs_kernel(CdConst C, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                       const uint8_t* __restrict__ active,
                                                                       const float* __restrict__ impulse_ext, int n, float* __restrict__ rhs) {
  __shared__ float sJ[BA_EPW][WBC_NB][6];          // joint axis, joint origin, in F
  __shared__ float sX[BA_EPW][WBC_CONSTR_MAX_BODIES][3];   // listed body's origin in F
  const int half = BA_EPW == 2 ? threadIdx.x >> 5 : 0, lane = BA_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * BA_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  const int nb = C.nb, nrow = 3 * nb + 1;
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  if (lane < WBC_NB + nb) {
    const bool body = lane < WBC_NB;
    const int k = body ? 0 : lane - WBC_NB, r = C.rb[k];
    const int b = body ? lane : C.rb_body[r];
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f);
#pragma nounroll
    for (int s = 0; s < WBC_MAX_DEPTH; ++s) {
      const int a = C.path[b][s];
      if (a < 0) break;
      float Q[9];
      const f3 ax = tree_joint_rot(C.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * C.dof[a]], Q);
      tree_frame_step(E, p, Q, C.joint_xyz[a], ax);
    }
    if (body) {
      st3(sJ[half][b], mat_mul(E, tree_axis(C.axis[b])));    // -1 for the root: no joint axis
      st3(sJ[half][b] + 3, p);
    } else {
      st3(sX[half][k], p + mat_mul(E, mk3(C.rb_offset[r][0], C.rb_offset[r][1], C.rb_offset[r][2])));
    }
  }
  __syncthreads();
  if (lane < BD_NCOL && live) {
    const int c = lane, b = c < 6 ? 0 : C.col_body[c - 6], j = c < 3 ? c : c - 3;
    const f3 ej = mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
    float* o = rhs + e * (size_t)(nrow * BD_NCOL) + c;
    for (int k = 0; k < nb; ++k) {
      const bool act = active ? active[e * nb + k] != 0 : true;
      f3 lin = mk3(0.f, 0.f, 0.f);
      if (act) lin = rhs_jac_lin(C, c, b, C.rb_body[C.rb[k]], ej, R, ld3(sX[half][k]), sJ[half]);
      o[(3 * k) * BD_NCOL] = lin.x; o[(3 * k + 1) * BD_NCOL] = lin.y; o[(3 * k + 2) * BD_NCOL] = lin.z;
    }
    o[3 * nb * BD_NCOL] = (b >= 0 && impulse_ext) ? impulse_ext[e * BD_NCOL + c] : 0.f;
  }
}

// Per env, with m = 3 nb rows, J the rows of the right-hand-side block, iota its last row and Y = (M^-1 [J^T | iota])^T: the Delassus
// matrix, its Cholesky factor and the lane solve are wbc_constraint_solve_kernel's (wbc_delassus.h), with the right-hand side
// c_i = (vdes_i - e (u_i - vdes_i)) - u_i - (J dnu_free)_i; an inactive body's e and vdes are never loaded. u_i = sum_c J_ic nu_c is
// the 26-term product in column order, lane c's nu_c (0 on a finger) handed to the row lanes by a shuffle. Then lane c = column c:
// dnu_c = Y_iota,c + sum_k Y_kc Lambda_k, nu+_c = nu_c + dnu_c (nu_c itself where dnu_c is 0, so that -0 stays), and the generalised
// impulse g_c = iota_c + sum_k J_kc Lambda_k, whose product with nu + dnu / 2 summed over the lanes of the half is T(nu+) - T(nu)
// = g^T nu + g^T M^-1 g / 2: the quadratic form, not the difference of two energies.
// MAP: X = (A + damping)^-1 diag(1 + e) J in place of J, one column per lane (delassus_column_solve), then P = 1 - Y^T X staged in LDS
// as the env's contiguous [26, 26] block, which leaves in 16-byte stores (676 floats = 169 of them). Without MAP the kernel holds no
// LDS beyond the sibling's. A single-wavefront workgroup: the __syncthreads() order the LDS traffic and cost no barrier instruction.
#define IM_MAP_FLOATS (BD_NCOL * BD_NCOL)
static_assert(IM_MAP_FLOATS % 4 == 0, "the map leaves in 16-byte stores");
struct ImArgs {
  const float *rhs, *Y, *root, *dofs;
  const uint8_t* active;
  const float *restitution, *vel_des;
  float damping;
  int nb;
  uint32_t live_cols;
  int n;
  float *nu_plus, *impulse, *denergy, *dnu_dnu;
};

template <bool MAP>
__device__ __forceinline__ void impulse_solve_body(const ImArgs& a, float* sP) {
  __shared__ float sJ[BA_EPW][CD_MAXROWS][CD_LD], sY[BA_EPW][CD_MAXROWS + 1][CD_LD];
  __shared__ float sA[BA_EPW][CD_MAXROWS][CD_MAXROWS + 1];   // lower triangle: A, then L
  __shared__ float sD[BA_EPW][CD_MAXROWS + 1], sV[BA_EPW][CD_MAXROWS + 1];   // 1 / L_jj; the value handed round
  const int half = BA_EPW == 2 ? threadIdx.x >> 5 : 0, lane = BA_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * BA_EPW + half;
  const bool live = env < a.n;
  const size_t e = live ? env : a.n - 1;           // the idle half of the last workgroup recomputes the last env and stores nothing
  const int nb = a.nb, m = 3 * nb;
  float (*J)[CD_LD] = sJ[half], (*Yt)[CD_LD] = sY[half];
  float (*A)[CD_MAXROWS + 1] = sA[half];
  float *D = sD[half], *V = sV[half];
  const float *rp = a.rhs + e * (size_t)((m + 1) * BD_NCOL), *yp = a.Y + e * (size_t)((m + 1) * BD_NCOL);
  for (int t = lane; t < (m + 1) * BD_NCOL; t += BA_LPE) {
    const int r = t / BD_NCOL, c = t - r * BD_NCOL;
    Yt[r][c] = yp[t];
    if (r < m) J[r][c] = rp[t];
  }
  uint32_t act = 0;                                // bit i: row i belongs to an active body
  for (int k = 0; k < nb; ++k)
    if (!a.active || a.active[e * nb + k]) act |= 7u << (3 * k);
  __syncthreads();

  delassus_fill(J, Yt, A, m, act, a.damping, lane, BA_LPE);
  const int i = lane;
  const bool row = i < m, on = row && ((act >> i) & 1u);
  const bool lc = lane < BD_NCOL && ((a.live_cols >> lane) & 1u);
  float v = 0.f;                                   // lane c: nu_c of the state, 0 on a finger and past the columns
  if (lc) v = lane < 6 ? a.root[e * 26 + 7 + lane] : a.dofs[e * (2 * WBC_NDOF) + 2 * (lane - 6) + 1];
  float ui = 0.f;                                  // lane i: the pre-impact velocity along row i
  for (int c = 0; c < BD_NCOL; ++c) {
    const float vc = __shfl(v, c, BA_LPE);
    if (row) ui += J[i][c] * vc;
  }
  float ci = 0.f, e1 = 0.f;                        // e1 = 1 + e of the row's body (MAP)
  if (on) {
    float s = 0.f;
    for (int c = 0; c < BD_NCOL; ++c) s += J[i][c] * Yt[m][c];
    const float vd = a.vel_des ? a.vel_des[e * m + i] : 0.f;
    const float er = a.restitution ? a.restitution[e * nb + i / 3] : 0.f;
    ci = ((vd - er * (ui - vd)) - ui) - s;
    e1 = 1.f + er;
  }
  delassus_cholesky(A, D, m, i);
  delassus_lane_solve(A, D, V, m, i, ci);
  if (live && a.impulse && row) a.impulse[e * m + i] = on ? V[i] : 0.f;
  float gn = 0.f;                                  // this column's share of the energy change
  if (lane < BD_NCOL) {
    const int c = lane;
    float dv = Yt[m][c], g = rp[m * BD_NCOL + c];
    for (int k = 0; k < m; ++k) {
      const float lk = ((act >> k) & 1u) ? V[k] : 0.f;
      dv += Yt[k][c] * lk;
      g += J[k][c] * lk;
    }
    if (lc) gn = g * (v + 0.5f * dv);
    if (live) a.nu_plus[e * BD_NCOL + c] = lc ? (dv != 0.f ? v + dv : v) : 0.f;
  }
  if (a.denergy) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) gn += __shfl_xor(gn, off);
    if (live && lane == 0) a.denergy[e] = gn;
  }
  if constexpr (MAP) {
    float* P = sP + half * IM_MAP_FLOATS;
    __syncthreads();                               // every lane has read J
    if (row)
      for (int c = 0; c < BD_NCOL; ++c) J[i][c] *= e1;   // 0 for an inactive row, whose J is 0 already
    __syncthreads();
    if (lane < BD_NCOL) delassus_column_solve(A, D, &J[0][lane], CD_LD, m);
    __syncthreads();
    for (int t = lane; t < IM_MAP_FLOATS; t += BA_LPE) {
      const int r = t / BD_NCOL, c = t - r * BD_NCOL;
      float s = 0.f;
      for (int k = 0; k < m; ++k) s += Yt[k][r] * J[k][c];
      const bool lrc = ((a.live_cols >> r) & 1u) && ((a.live_cols >> c) & 1u);
      P[t] = lrc ? (r == c ? 1.f : 0.f) - s : 0.f;
    }
    __syncthreads();
    if (live) {
      float4* o = reinterpret_cast<float4*>(a.dnu_dnu + e * (size_t)IM_MAP_FLOATS);
      const float4* P4 = reinterpret_cast<const float4*>(P);
      for (int t = lane; t < IM_MAP_FLOATS / 4; t += BA_LPE) o[t] = P4[t];
    }
  }
}

extern "C" __global__ void __launch_bounds__(64) wbc_impulse_solve_kernel(ImArgs a) { impulse_solve_body<false>(a, nullptr); }

extern "C" __global__ void __launch_bounds__(64) wbc_impulse_solve_map_kernel(ImArgs a) {
  __shared__ __attribute__((aligned(16))) float sP[BA_EPW * IM_MAP_FLOATS];
  impulse_solve_body<true>(a, sP);
}

// Workspace layout (floats): the right-hand-side block [N, 3 nb + 1, 26], the mass solve's output of the same shape.
extern "C" size_t wbc_sim_impulse_dynamics_workspace_floats(int num_envs, int nbodies) {
  if (num_envs <= 0 || nbodies < 1 || nbodies > WBC_CONSTR_MAX_BODIES) return 0;
  return (size_t)num_envs * 2 * (size_t)(3 * nbodies + 1) * BD_NCOL;
}

// Three launches on `stream`: the right-hand-side block, the existing mass solve with 3 nb + 1 right-hand sides, the impulse solve
// (its map variant where dnu_dnu is asked for). Arguments and conventions: include/wbc_sim.h. The checks that need no sim come first.
extern "C" int wbc_sim_impulse_dynamics(wbc_sim* s, const int32_t* rigid_bodies, int nbodies, const uint8_t* active, const float* restitution,
                                        const float* vel_des, const float* impulse_ext, float damping, int flags, float* nu_plus,
                                        float* impulse, float* denergy, float* dnu_dnu, float* workspace, void* stream) {
  WbCall c("wbc_sim_impulse_dynamics", s, stream);
  if (!rigid_bodies || !nu_plus || !workspace) return c.fail(-1, "rigid_bodies / nu_plus / workspace is NULL");
  if (nbodies < 1 || nbodies > WBC_CONSTR_MAX_BODIES) return c.fail(-1, "nbodies must be 1..WBC_CONSTR_MAX_BODIES");
  if (!(damping >= 0.f) || !(damping <= 3.4e38f)) return c.fail(-1, "damping must be finite and >= 0");
  if (flags & ~WBC_SOLVE_ARMATURE) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)restitution | (uintptr_t)vel_des | (uintptr_t)impulse_ext | (uintptr_t)nu_plus | (uintptr_t)impulse | (uintptr_t)denergy |
       (uintptr_t)dnu_dnu | (uintptr_t)workspace) & 3u)
    return c.fail(-1, "restitution / vel_des / impulse_ext / nu_plus / impulse / denergy / dnu_dnu / workspace must be 4-byte aligned");
  if ((uintptr_t)dnu_dnu & 15u) return c.fail(-1, "dnu_dnu must be 16-byte aligned");
  for (int k = 0; k < nbodies; ++k)
    if (rigid_bodies[k] < 0 || rigid_bodies[k] >= WBC_NRB) return c.fail(-1, "rigid-body index outside 0..WBC_NRB-1");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  CdConst C;
  if (ba_const_fill(c.hc->model, C, C) != 0) return c.no_tree();
  for (int k = 0; k < nbodies; ++k)
    for (int l = 0; l < k; ++l)
      if (C.rb_body[rigid_bodies[k]] == C.rb_body[rigid_bodies[l]])
        return c.fail(-1, "two listed rigid bodies ride on the same moving body (dependent rows)");
  const int n = c.n;
  if (n <= 0) return 0;
  tree_cols_fill(c.hc->model, C);
  uint32_t live_cols = 63u;
  for (int d = 0; d < WBC_NDOF; ++d) if (C.col_body[d] >= 0) live_cols |= 1u << (6 + d);
  C.nb = nbodies;
  for (int k = 0; k < WBC_CONSTR_MAX_BODIES; ++k) C.rb[k] = rigid_bodies[k < nbodies ? k : 0];
  const int nrow = 3 * nbodies + 1;
  float *blk = workspace, *Y = blk + (size_t)n * nrow * BD_NCOL;
  const dim3 grid((n + BA_EPW - 1) / BA_EPW);
  hipLaunchKernelGGL(wbc_impulse_rhs_kernel, grid, dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, active, impulse_ext, n, blk);
  int rc = c.launched();
  if (rc != 0) return rc;
  rc = mass_solve_launch(c, blk, (int64_t)nrow * BD_NCOL, nrow, nullptr, Y, (int64_t)nrow * BD_NCOL, flags, stream);
  if (rc != 0) return rc;
  const ImArgs a = {blk, Y, c.root, c.dofs, active, restitution, vel_des, damping, nbodies, live_cols, n, nu_plus, impulse, denergy, dnu_dnu};
  if (dnu_dnu) hipLaunchKernelGGL(wbc_impulse_solve_map_kernel, grid, dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(wbc_impulse_solve_kernel, grid, dim3(64), 0, (hipStream_t)stream, a);
  return c.launched();
}

// ---- centre of mass, centroidal momentum and its matrix (include/wbc_sim.h: wbc_sim_centroidal) ----------------------------------------
// With c the centre of mass, d_b = c_b - c and every vector in WORLD axes relative to the root origin (the walk starts from E = R):
//     h_G = (m v_com ; sum I_b w_b + m_b d_b x v_cb),   hdot_G = (m a_com ; sum I_b al_b + w_b x I_b w_b + m_b d_b x a_cb),
//     I_G = sum I_b + m_b (|d_b|^2 1 - d_b d_b^T).
// sum m_b d_b x X vanishes for any X common to all bodies, so the walk carries each body's velocity and classical acceleration RELATIVE
// to the root origin's linear motion (v_root and nudot[0:3] never enter it) at the body's own origin: ba_walk's step (tree_accel_step)
// with the origin's velocity carried too. No angular row then holds a term that grows with |v_root| or |nudot[0:3]|, and the linear rows
// add m v_root and m nudot[0:3] at the end.
// CM_EPW envs per 64-lane workgroup, one per lane group, three LDS hand-overs:
//  1) lane b = moving body b walks root -> b in registers and leaves (m, c_b - its origin, its origin, its joint axis, I_b about c_b)
//     in LDS;
//  2) every lane sums (m, m c) over the bodies; lane b leaves its body's share of the 18 sums (m_b v_cb, m_b a_cb, the two angular
//     shares, I_G's) in LDS; lane t sums share t, writes the entries of com / mom / inertia it completes and leaves the sum in LDS;
//  3) lane c = column c of A_G: (m 1 ; 0) for v_root, (-m [c]x ; I_G) for omega_root, and for a joint the composite (m, m c, I) of the
//     subtree it moves ABOUT THE JOINT'S OWN ORIGIN o, as wbc_mass_solve_kernel forms it: f = a x (m c)_s, n_o = I_s a, moved to the
//     centre of mass as n_o + (o - c) x f. A wrist column is then not the difference of two moments about a far point; the levers
//     are (o_d - o) + (c_d - o_d), so that the joint's own body enters with its model lever and not with a difference of two
//     root-relative points (fp32 emulation of A_G: 31 x 2^-24 of the magnitude this way, 90 with c_d - o).
// A single-wavefront workgroup: the __syncthreads() order the LDS traffic and cost no barrier instruction. The root position is never read.
#ifndef CM_EPW
#define CM_EPW 2                                // envs per workgroup: 2, or 1 (-DCM_EPW=1, the variant DESIGN.md compares with)
#endif
static_assert(CM_EPW == 1 || CM_EPW == 2, "one env per 64 lanes or one per 32-lane half");
#define CM_BT 16                                // floats per body: m 0, c_b - origin 1..3, origin 4..6, joint axis 7..9, I_b about c_b 10..15
#define CM_NS 18                                // sums over the bodies: m v 0..2, m a 3..5, k_G 6..8, kdot_G 9..11, I_G 12..17
#define CM_COM 9
#define CM_MOM 12
#define CM_INR 7
static_assert(WBC_NB <= 64 / CM_EPW && BD_NCOL <= 64 / CM_EPW && CM_NS + 4 <= 64 / CM_EPW, "lanes");

extern "C" __global__ void __launch_bounds__(64) wbc_centroidal_kernel(TreeConst K, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                      const float* __restrict__ body_params,
                                                                      const float* __restrict__ nudot, int n, float* __restrict__ com,
                                                                      float* __restrict__ mom, float* __restrict__ cmm,
                                                                      float* __restrict__ inertia) {
  __shared__ float sB[CM_EPW][WBC_NB][CM_BT];
  __shared__ float sD[CM_EPW][WBC_NB][CM_NS];
  __shared__ float sSum[CM_EPW][CM_NS];
  const int half = CM_EPW == 2 ? threadIdx.x >> 5 : 0, lane = CM_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * CM_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  float (*B)[CM_BT] = sB[half];
  f3 vc = mk3(0.f, 0.f, 0.f), ac = vc, Lw = vc, Nw = vc;   // lane b: relative velocity / acceleration of c_b, I_b w_b, I_b al_b + w_b x I_b w_b

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9];
    quat_to_mat(root + e * 26 + 3, E);
    f3 p = mk3(0.f, 0.f, 0.f), Sw = p, vo = p, ao = p, aw = p;
    f3 w = ld3(root + e * 26 + 10);
    if (nudot) aw = ld3(nudot + e * BD_NCOL + 3);
#pragma unroll                                     // fully unrolled, as the compiler chose to while the step was written out here
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int a = K.path[b][k];
      if (a < 0) break;
      Sw = tree_accel_step(K, a, e, dofs, nudot, E, p, w, aw, ao, &vo);
    }
    float m = K.mass[b], cm[3] = {K.com[b][0], K.com[b][1], K.com[b][2]}, I6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) I6[j] = K.inertia[b][j];
    const int slot = b == 0 ? TREE_BP_ROOT : (b == K.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + e * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) cm[j] = bp[1 + j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
    }
    float Iw6[6];
    tree_rotate_inertia(E, I6, Iw6);
    const float Iw[9] = {Iw6[0], Iw6[3], Iw6[4], Iw6[3], Iw6[1], Iw6[5], Iw6[4], Iw6[5], Iw6[2]};
    const f3 rc = mat_mul(E, mk3(cm[0], cm[1], cm[2]));
    vc = vo + cross(w, rc);
    ac = ao + cross(aw, rc) + cross(w, cross(w, rc));
    Lw = mat_mul(Iw, w);
    Nw = mat_mul(Iw, aw) + cross(w, Lw);
    float* o = B[b];
    o[0] = m; st3(o + 1, rc); st3(o + 4, p); st3(o + 7, Sw);
    o[10] = Iw6[0]; o[11] = Iw6[1]; o[12] = Iw6[2]; o[13] = Iw6[3]; o[14] = Iw6[4]; o[15] = Iw6[5];
  }
  __syncthreads();

  float mt = 0.f;
  f3 mc = mk3(0.f, 0.f, 0.f);
  for (int d = 0; d < WBC_NB; ++d) { mt += B[d][0]; mc = mc + B[d][0] * (ld3(B[d] + 4) + ld3(B[d] + 1)); }
  const float im = 1.f / mt;
  const f3 cg = mc * im;
  if (lane < WBC_NB) {
    const float* q = B[lane];
    const float m = q[0];
    const f3 d = (ld3(q + 4) + ld3(q + 1)) - cg, P = m * vc, F = m * ac;
    const float dd = dot(d, d);
    float* o = sD[half][lane];
    st3(o, P); st3(o + 3, F); st3(o + 6, Lw + cross(d, P)); st3(o + 9, Nw + cross(d, F));
    o[12] = q[10] + m * (dd - d.x * d.x); o[13] = q[11] + m * (dd - d.y * d.y); o[14] = q[12] + m * (dd - d.z * d.z);
    o[15] = q[13] - m * d.x * d.y; o[16] = q[14] - m * d.x * d.z; o[17] = q[15] - m * d.y * d.z;
  }
  __syncthreads();

  if (lane < CM_NS) {
    const int t = lane, j = t % 3;
    float s = 0.f;
    for (int d = 0; d < WBC_NB; ++d) s += sD[half][d][t];
    sSum[half][t] = s;
    if (live) {
      if (t < 6) {                                             // linear rows: the root origin's own motion comes in here
        const bool vel = t < 3;
        const float x0 = vel ? root[e * 26 + 7 + j] : (nudot ? nudot[e * BD_NCOL + j] : 0.f);
        if (com) com[e * CM_COM + 3 + t] = x0 + s * im;
        if (mom) mom[e * CM_MOM + (vel ? 0 : 6) + j] = mt * x0 + s;
      } else if (t < 12) {
        if (mom) mom[e * CM_MOM + (t < 9 ? 3 : 9) + j] = s;
      } else if (inertia) {
        inertia[e * CM_INR + 1 + (t - 12)] = s;
      }
    }
  } else if (lane < CM_NS + 3) {
    const int j = lane - CM_NS;
    if (live && com) com[e * CM_COM + j] = j == 0 ? cg.x : j == 1 ? cg.y : cg.z;
  } else if (lane == CM_NS + 3) {
    if (live && inertia) inertia[e * CM_INR] = mt;
  }
  if (!cmm) return;
  __syncthreads();

  if (lane < BD_NCOL && live) {
    const int c = lane, j = c < 3 ? c : c - 3;
    const f3 ej = mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
    f3 lin = mk3(0.f, 0.f, 0.f), ang = lin;
    if (c < 3) {
      lin = mt * ej;                                           // exactly m on the diagonal, exactly 0 elsewhere
    } else if (c < 6) {
      const float* I = sSum[half] + 12;                        // xx yy zz xy xz yz
      lin = cross(ej, mc);
      ang = j == 0 ? mk3(I[0], I[3], I[4]) : j == 1 ? mk3(I[3], I[1], I[5]) : mk3(I[4], I[5], I[2]);
    } else {
      const int b = K.col_body[c - 6];
      if (b >= 0) {
        const f3 P = ld3(B[b] + 4), a = ld3(B[b] + 7);
        float xx = 0.f, yy = 0.f, zz = 0.f, xy = 0.f, xz = 0.f, yz = 0.f;
        f3 h = mk3(0.f, 0.f, 0.f);
        for (int d = 0; d < WBC_NB; ++d)
          if ((K.anc[d] >> b) & 1u) {
            const float* q = B[d];
            const float md = q[0];
            const f3 r = (ld3(q + 4) - P) + ld3(q + 1);      // the joint's own body: exactly its model lever
            const float rr = dot(r, r);
            h = h + md * r;
            xx += q[10] + md * (rr - r.x * r.x); yy += q[11] + md * (rr - r.y * r.y); zz += q[12] + md * (rr - r.z * r.z);
            xy += q[13] - md * r.x * r.y; xz += q[14] - md * r.x * r.z; yz += q[15] - md * r.y * r.z;
          }
        lin = cross(a, h);
        ang = mk3(xx * a.x + xy * a.y + xz * a.z, xy * a.x + yy * a.y + yz * a.z, xz * a.x + yz * a.y + zz * a.z) + cross(P - cg, lin);
      }
    }
    float* o = cmm + e * (6 * BD_NCOL) + c;
    o[0] = lin.x; o[BD_NCOL] = lin.y; o[2 * BD_NCOL] = lin.z;
    o[3 * BD_NCOL] = ang.x; o[4 * BD_NCOL] = ang.y; o[5 * BD_NCOL] = ang.z;
  }
}

// nudot (device f32 [N,26] or NULL = zeros); com [N,9], mom [N,12], cmm [N,6,26], inertia [N,7] (device f32, caller-owned, any may be NULL,
// not all): include/wbc_sim.h.
extern "C" int wbc_sim_centroidal(wbc_sim* s, const float* nudot, float* com, float* mom, float* cmm, float* inertia, void* stream) {
  WbCall c("wbc_sim_centroidal", s, stream);
  if (!s) return c.no_sim();
  if (!com && !mom && !cmm && !inertia) return c.fail(-1, "com, mom, cmm and inertia are all NULL");
  if (((uintptr_t)nudot | (uintptr_t)com | (uintptr_t)mom | (uintptr_t)cmm | (uintptr_t)inertia) & 3u)
    return c.fail(-1, "nudot / com / mom / cmm / inertia must be 4-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  TreeConst K;
  if (tree_const_fill(c.hc->model, K) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_centroidal_kernel, dim3((c.n + CM_EPW - 1) / CM_EPW), dim3(64), 0, (hipStream_t)stream, K, c.root, c.dofs, c.bp, nudot, c.n,
                     com, mom, cmm, inertia);
  return c.launched();
}

// ---- analytic derivatives of inverse and forward dynamics (include/wbc_sim.h: wbc_sim_inverse_dynamics_derivatives) ----------------------
// The tangent of wbc_inverse_dynamics_kernel's recursion (its walk in classical form), carried in forward mode: a lane owns one (moving body d, direction x) pair,
// redoes d's path walk root -> d with every quantity paired with its derivative along x, and leaves d(force about F's origin), d(own-joint
// torques) and d(m c) in LDS; lanes over the entries (row c, direction x) then sum the subtrees with the ancestor masks and add dS_c . F_c,
// which is closed form (a joint above c turns c's axis and origin about its own). A body depends only on the root directions and on the
// joints of its own path, so for this robot 102 pairs are live per output (19 x 3 root directions + 45 path joints): two rounds of 64 lanes.
// The root's LINEAR velocity is not read at all: the walk carries angular velocities and classical accelerations, which hold no linear
// velocity (Galilean invariance), and those columns are written as literal zeros, as are
// the translation columns (the root position is not read either), the fingers and every pair of joints on different chains.
// Root rotation (world rotation vector, world components of nu / nudot held fixed): in F every root vector w, wdot, vdot, g turns by
// -phi x (.), phi = R^T e_j, the joints' S do not change, and the world rows 0:6 of the result turn by e_j x (.).
// One env per 64-lane workgroup; 17.4 KB of LDS (8 workgroups per CU).
#define DD_NT 18                                // tangent slots per body: root rotation 0..2, root omega 3..5, q of path[b][i] 6 + i, qd of path[b][i] 12 + i
#define DD_PT 12                                // floats per (body, slot): d(moment about F's origin) 0..2, d(force) 3..5, d(own-joint torques) 6, 7, d(m c) 8..10
#define DD_MAXPAIR (WBC_NB * (3 + WBC_MAX_DEPTH))
#define DD_MENV (BD_NCOL * BD_NCOL)
struct DdConst {
  IdConst K;
  int32_t depth[WBC_NB];                        // joints between the root and b
  int32_t npair;                                // live (body, direction) pairs of one output
  uint8_t pair_body[DD_MAXPAIR], pair_u[DD_MAXPAIR];   // u: 0..2 a root direction, 3 + i the joint path[b][i]
};
struct d3 { f3 v, d; };                         // a vector and its derivative along the lane's direction
struct du { float v, d; };
__device__ __forceinline__ d3 mkd3(f3 v, f3 d) { d3 r; r.v = v; r.d = d; return r; }
__device__ __forceinline__ d3 operator+(d3 a, d3 b) { return mkd3(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ d3 operator*(d3 a, du s) { return mkd3(a.v * s.v, a.d * s.v + a.v * s.d); }
__device__ __forceinline__ d3 operator*(d3 a, float s) { return mkd3(a.v * s, a.d * s); }
__device__ __forceinline__ d3 cross(d3 a, d3 b) { return mkd3(cross(a.v, b.v), cross(a.d, b.v) + cross(a.v, b.d)); }
__device__ __forceinline__ du dot(d3 a, d3 b) { du r; r.v = dot(a.v, b.v); r.d = dot(a.d, b.v) + dot(a.v, b.d); return r; }
__device__ __forceinline__ d3 mat_mul(const float* M, const float* dM, d3 x) { return mkd3(mat_mul(M, x.v), mat_mul(dM, x.v) + mat_mul(M, x.d)); }
__device__ __forceinline__ d3 matT_mul(const float* M, const float* dM, d3 x) { return mkd3(matT_mul(M, x.v), matT_mul(dM, x.v) + matT_mul(M, x.d)); }

extern "C" __global__ void __launch_bounds__(64) wbc_dynamics_derivatives_kernel(DdConst C, const float* __restrict__ root,
                                                                                const float* __restrict__ dofs,
                                                                                const float* __restrict__ body_params,
                                                                                const float* __restrict__ nudot, int n,
                                                                                float* __restrict__ out_dq, float* __restrict__ out_dnu,
                                                                                float* __restrict__ eye, int transposed, int negate) {
  __shared__ __align__(16) float sT[WBC_NB][DD_NT][DD_PT];
  __shared__ __align__(16) float sF[WBC_NB][12];  // per body: moment about F's origin 0..2, force 3..5 (gravity excluded), m 8, m c 9..11
  __shared__ float sS[WBC_NB][6];                  // the body's joint in F: axis, origin
  const IdConst& K = C.K;
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;
  if (eye && blockIdx.x == 0)
    for (int idx = lane; idx < DD_MENV; idx += 64) eye[idx] = idx / BD_NCOL == idx % BD_NCOL ? 1.f : 0.f;
  if (!out_dq && !out_dnu) return;
  const f3 zero = mk3(0.f, 0.f, 0.f);
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  const f3 gF = matT_mul(R, mk3(K.gravity[0], K.gravity[1], K.gravity[2]));
  const f3 w0 = matT_mul(R, ld3(root + e * 26 + 10));
  const f3 al0 = nudot ? matT_mul(R, ld3(nudot + e * BD_NCOL + 3)) : zero, a0 = nudot ? matT_mul(R, ld3(nudot + e * BD_NCOL)) : zero;

  for (int which = 0; which < 2; ++which) {
    if (!(which ? out_dnu : out_dq)) continue;
    for (int pi = lane; pi < C.npair; pi += 64) {
      const int b = C.pair_body[pi], u = C.pair_u[pi];
      const int t = u < 3 ? u + 3 * which : 3 + u + 6 * which;
      // seeds of the root directions: rotation turns every root vector by -phi x (.), omega_j moves the angular velocity alone
      const f3 phi = matT_mul(R, mk3(u == 0 ? 1.f : 0.f, u == 1 ? 1.f : 0.f, u == 2 ? 1.f : 0.f));
      const float rot = t < 3 ? 1.f : 0.f, omg = t >= 3 && t < 6 ? 1.f : 0.f;
      const d3 g = mkd3(gF, cross(gF, phi) * rot);
      // angular velocity, angular acceleration and the CLASSICAL acceleration of the body's own origin, in F's axes (tree_accel_step, paired with its tangent):
      // every later lever is then a link offset or a centre-of-mass offset, never the distance to the base origin
      d3 vw = mkd3(w0, cross(w0, phi) * rot + phi * omg);
      d3 aw = mkd3(al0, cross(al0, phi) * rot), ao = mkd3(a0, cross(a0, phi) * rot);
      float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, dE[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      d3 p = mkd3(zero, zero), Sw = p;
#pragma nounroll                                  // kept a loop, as the compiler chose to while the step was written out here
      for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
        const int a = K.path[b][k];
        if (a < 0) break;
        const int d = K.dof[a];
        const float dq = t == 6 + k ? 1.f : 0.f;
        float s, c, Q[9], dQ[9];
        const f3 uu = tree_joint_rot(K.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * d], Q, s, c);
        tree_rodrigues(uu, c * dq, -s * dq, s * dq, dQ);          // d(sin, cos, 1 - cos) along the lane's direction
        const f3 xyz = mk3(K.joint_xyz[a][0], K.joint_xyz[a][1], K.joint_xyz[a][2]);
        const d3 r = mkd3(mat_mul(E, xyz), mat_mul(dE, xyz));   // a_o <- a_o + alpha x r + w x (w x r) with the parent's alpha, w; (E, p) <- (E Rot_a, p + E xyz_a)
        ao = ao + cross(aw, r) + cross(vw, cross(vw, r));
        p = p + r;
        float En[9], dEQ[9], EdQ[9];                           // (E, dE) <- (E Q, dE Q + E dQ)
        tree_frame_mul(E, Q, En);
        tree_frame_mul(dE, Q, dEQ);
        tree_frame_mul(E, dQ, EdQ);
#pragma unroll
        for (int j = 0; j < 9; ++j) { E[j] = En[j]; dE[j] = dEQ[j] + EdQ[j]; }
        Sw = mkd3(mat_mul(E, uu), mat_mul(dE, uu));
        du qd;
        qd.v = dofs[e * (2 * WBC_NDOF) + 2 * d + 1];
        qd.d = t == 12 + k ? 1.f : 0.f;
        const float qdd = nudot ? nudot[e * BD_NCOL + 6 + d] : 0.f;
        const d3 jw = Sw * qd;                                 // alpha += axis qdd + w x (axis qd), then w += axis qd
        aw = aw + Sw * qdd + cross(vw, jw);
        vw = vw + jw;
      }
      float m = K.mass[b], com[3] = {K.com[b][0], K.com[b][1], K.com[b][2]}, I6[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = K.inertia[b][j];
      const int slot = b == 0 ? TREE_BP_ROOT : (b == K.gripper_body ? TREE_BP_GRIPPER : -1);
      if (slot >= 0) {
        const float* bp = body_params + e * TREE_BP_STRIDE + slot;
        m = bp[0];
#pragma unroll
        for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
        for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
      }
      // as wbc_inverse_dynamics_kernel: the body's own joint sees the body's own force and weight through the lever in BODY axes
      const int axb = K.axis[b];
      const f3 cm = mk3(com[0], com[1], com[2]), ub = tree_axis(axb);
      const f3 lev = cross(cm, ub);
      const d3 cmd = mkd3(cm, zero), ubd = mkd3(ub, zero), levd = mkd3(lev, zero);
      const d3 rc = mat_mul(E, dE, cmd), Cc = p + rc;
      const d3 fl = (ao + cross(aw, rc) + cross(vw, cross(vw, rc))) * m;
      const d3 wl = matT_mul(E, dE, vw), al = matT_mul(E, dE, aw);
      const float Ib[9] = {I6[0], I6[3], I6[4], I6[3], I6[1], I6[5], I6[4], I6[5], I6[2]};
      const d3 Iw = mkd3(mat_mul(Ib, wl.v), mat_mul(Ib, wl.d));
      const d3 ncl = mkd3(mat_mul(Ib, al.v), mat_mul(Ib, al.d)) + cross(wl, Iw);
      const d3 nF = mat_mul(E, dE, ncl) + cross(Cc, fl);
      const float o6d = dot(ubd, ncl).d - dot(levd, matT_mul(E, dE, fl)).d;
      const float o7d = m * dot(matT_mul(E, dE, g), levd).d;
      float* o = sT[b][t];
      st3(o, nF.d); st3(o + 3, fl.d); o[6] = o6d; o[7] = o7d; st3(o + 8, Cc.d * m); o[11] = 0.f;
      if (u == 0) {                                            // every body has this pair: it leaves the primal quantities too
        float* f = sF[b];
        st3(f, nF.v); st3(f + 3, fl.v); f[6] = 0.f; f[7] = 0.f; f[8] = m; st3(f + 9, Cc.v * m);
        st3(sS[b], Sw.v); st3(sS[b] + 3, p.v);
      }
    }
  }
  __syncthreads();

  for (int which = 0; which < 2; ++which) {
    float* __restrict__ out = which ? out_dnu : out_dq;
    if (!out) continue;
    for (int idx = lane; idx < DD_MENV; idx += 64) {
      const int i = idx / BD_NCOL, j = idx - i * BD_NCOL;
      const int c = transposed ? j : i, x = transposed ? i : j;   // row of tau, direction
      const int rb = c < 6 ? 0 : K.col_body[c - 6], cb = x < 6 ? 0 : K.col_body[x - 6];
      float val = 0.f;
      // live: neither a finger nor a root translation / linear-velocity direction, and the two on one chain
      if (rb >= 0 && cb >= 0 && x >= 3 && (((K.anc[rb] >> cb) & 1u) || ((K.anc[cb] >> rb) & 1u))) {
        const int tr = x < 6 ? x - 3 + 3 * which : 6 + 6 * which + C.depth[cb] - 1;
        const int jr = c < 3 ? c : c - 3;
        const bool theta = which == 0 && x < 6;
        f3 Np = zero, Fp = zero, hs = zero, dN = zero, dF = zero, dH = zero;
        float ms = 0.f;
        for (int d = 0; d < WBC_NB; ++d) {
          const bool inC = ((K.anc[d] >> rb) & 1u) && (c < 6 || d != rb);   // a joint's own body comes in through slots 6, 7
          if (!inC) continue;
          const float4* f4 = reinterpret_cast<const float4*>(sF[d]);
          const float4 u0 = f4[0], u1 = f4[1], u2 = f4[2];
          Np = Np + mk3(u0.x, u0.y, u0.z); Fp = Fp + mk3(u0.w, u1.x, u1.y);
          ms += u2.x; hs = hs + mk3(u2.y, u2.z, u2.w);
          if ((K.anc[d] >> cb) & 1u) {                         // d is moved by the direction: the pair (d, tr) was written
            const float4* t4 = reinterpret_cast<const float4*>(sT[d][tr]);
            const float4 v0 = t4[0], v1 = t4[1], v2 = t4[2];
            dN = dN + mk3(v0.x, v0.y, v0.z); dF = dF + mk3(v0.w, v1.x, v1.y);
            dH = dH + mk3(v2.x, v2.y, v2.z);
          }
        }
        const f3 phi = matT_mul(R, mk3(x == 3 ? 1.f : 0.f, x == 4 ? 1.f : 0.f, x == 5 ? 1.f : 0.f));   // R^T e_(x-3): root directions only
        const f3 gw = mk3(K.gravity[0], K.gravity[1], K.gravity[2]);
        if (c < 6) {
          const f3 row = matT_mul(R, mk3(jr == 0 ? 1.f : 0.f, jr == 1 ? 1.f : 0.f, jr == 2 ? 1.f : 0.f));
          if (c < 3) {
            val = dot(row, dF);
            if (theta) val += dot(row, cross(phi, Fp));
          } else {
            val = dot(row, dN);
            if (theta) val += dot(row, cross(phi, Np));
            if (which == 0) {                                  // the weight's moment, formed in world axes as the primal kernel forms it
              const f3 Rh = mat_mul(R, hs);
              const f3 ej = mk3(x == 3 ? 1.f : 0.f, x == 4 ? 1.f : 0.f, x == 5 ? 1.f : 0.f);
              const f3 nw = cross(gw, theta ? cross(ej, Rh) : mat_mul(R, dH));
              val += jr == 0 ? nw.x : jr == 1 ? nw.y : nw.z;
            }
          }
        } else {
          const f3 a = ld3(sS[rb]), po = ld3(sS[rb] + 3), l = cross(po, a);
          f3 da = zero, dpo = zero;
          if (which == 0 && x >= 6 && cb != rb && ((K.anc[rb] >> cb) & 1u)) {   // a joint above c turns c's axis and origin about its own
            const f3 ak = ld3(sS[cb]), pk = ld3(sS[cb] + 3);
            da = cross(ak, a); dpo = cross(ak, po - pk);
          }
          const f3 dl = cross(dpo, a) + cross(po, da);
          const bool own = (K.anc[rb] >> cb) & 1u;              // the pair (rb, tr) exists
          val = (own ? sT[rb][tr][6] : 0.f) + (dot(a, dN) + dot(l, dF)) + (dot(da, Np) + dot(dl, Fp));
          if (which == 0) {
            const f3 w = hs - ms * po, dw = dH - ms * dpo;
            const f3 dg = theta ? cross(gF, phi) : zero;
            val += (own ? sT[rb][tr][7] : 0.f) + dot(da, cross(gF, w)) + dot(a, cross(dg, w)) + dot(a, cross(gF, dw));
          }
        }
        if (negate) val = -val;
      }
      out[e * DD_MENV + idx] = val;
    }
  }
}

// dst[e, i, j] = src[e, j, i] for up to three [N, 26, 26] tensors (NULL pairs are skipped): the conventional layout of the forward-dynamics
// derivatives, whose solves produce one direction's 26 values contiguously.
extern "C" __global__ void __launch_bounds__(64) wbc_derivatives_transpose_kernel(const float* __restrict__ s0, float* __restrict__ d0,
                                                                                 const float* __restrict__ s1, float* __restrict__ d1,
                                                                                 const float* __restrict__ s2, float* __restrict__ d2) {
  const size_t base = (size_t)blockIdx.x * DD_MENV;
  for (int idx = threadIdx.x; idx < DD_MENV; idx += 64) {
    const int i = idx / BD_NCOL, j = idx - i * BD_NCOL, src = j * BD_NCOL + i;
    if (d0) d0[base + idx] = s0[base + src];
    if (d1) d1[base + idx] = s1[base + src];
    if (d2) d2[base + idx] = s2[base + src];
  }
}

// Fills C from the model. 0, or 1: a tree the kernel cannot walk.
static int dd_const_fill(const DevConst* hc, DdConst& C) {
  if (id_const_fill(hc, C.K) != 0) return 1;
  C.npair = 0;
  for (int b = 0; b < WBC_NB; ++b) {
    int depth = 0;
    while (depth < WBC_MAX_DEPTH && C.K.path[b][depth] >= 0) ++depth;
    C.depth[b] = depth;
    for (int u = 0; u < 3 + depth; ++u) { C.pair_body[C.npair] = (uint8_t)b; C.pair_u[C.npair] = (uint8_t)u; ++C.npair; }
  }
  for (int i = C.npair; i < DD_MAXPAIR; ++i) { C.pair_body[i] = 0; C.pair_u[i] = 0; }
  return 0;
}

static int derivatives_launch(const WbCall& c, const float* nudot, float* dq, float* dnu, float* eye, int transposed, int negate, void* stream) {
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  DdConst C;
  if (dd_const_fill(c.hc, C) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_dynamics_derivatives_kernel, dim3(dq || dnu ? c.n : 1), dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, c.bp, nudot, c.n,
                     dq, dnu, eye, transposed, negate);
  return c.launched();
}

// nudot (device f32 [N,26] or NULL = zeros); dtau_dq / dtau_dnu (device f32 [N,26,26], caller-owned, either may be NULL): include/wbc_sim.h.
extern "C" int wbc_sim_inverse_dynamics_derivatives(wbc_sim* s, const float* nudot, float* dtau_dq, float* dtau_dnu, int flags, void* stream) {
  WbCall c("wbc_sim_inverse_dynamics_derivatives", s, stream);
  if (!s) return c.no_sim();
  if (!dtau_dq && !dtau_dnu) return c.fail(-1, "dtau_dq and dtau_dnu are both NULL");
  if (flags & ~WBC_DERIV_TRANSPOSED) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)nudot | (uintptr_t)dtau_dq | (uintptr_t)dtau_dnu) & 3u) return c.fail(-1, "nudot / dtau_dq / dtau_dnu must be 4-byte aligned");
  return derivatives_launch(c, nudot, dtau_dq, dtau_dnu, nullptr, (flags & WBC_DERIV_TRANSPOSED) ? 1 : 0, 0, stream);
}

// Workspace: -dtau/dq^T and -dtau/dnu^T (the solves' right-hand sides), three solve results awaiting their transpose, one 26 x 26 identity.
extern "C" size_t wbc_sim_forward_dynamics_derivatives_workspace_floats(int num_envs) {
  return num_envs > 0 ? (size_t)num_envs * DD_MENV * 5 + DD_MENV : 0;
}

// tau (device f32 [N,26] or NULL), nudot [N,26], dnudot_dq / dnudot_dnu / minv [N,26,26] (any may be NULL, not all): include/wbc_sim.h.
extern "C" int wbc_sim_forward_dynamics_derivatives(wbc_sim* s, const float* tau, float* nudot, float* dnudot_dq, float* dnudot_dnu, float* minv,
                                                    int flags, float* workspace, void* stream) {
  WbCall c("wbc_sim_forward_dynamics_derivatives", s, stream);
  if (!s) return c.no_sim();
  if (!nudot || !workspace) return c.fail(-1, "nudot / workspace is NULL");
  if (!dnudot_dq && !dnudot_dnu && !minv) return c.fail(-1, "dnudot_dq, dnudot_dnu and minv are all NULL");
  if (flags & ~(WBC_SOLVE_ARMATURE | WBC_DERIV_TRANSPOSED)) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)tau | (uintptr_t)nudot | (uintptr_t)dnudot_dq | (uintptr_t)dnudot_dnu | (uintptr_t)minv | (uintptr_t)workspace) & 3u)
    return c.fail(-1, "tau / nudot / dnudot_dq / dnudot_dnu / minv / workspace must be 4-byte aligned");
  if (!c.have) return c.no_state();
  const int n = c.n;
  if (n <= 0) return 0;
  const int solve_flags = flags & WBC_SOLVE_ARMATURE;
  const bool tr = flags & WBC_DERIV_TRANSPOSED;
  int rc = wbc_sim_forward_dynamics(s, tau, nudot, solve_flags, stream);
  if (rc != 0) return rc;
  const size_t blk = (size_t)n * DD_MENV;
  float* rq = dnudot_dq ? workspace : nullptr;
  float* rn = dnudot_dnu ? workspace + blk : nullptr;
  float* eye = minv ? workspace + 5 * blk : nullptr;
  rc = derivatives_launch(c, nudot, rq, rn, eye, 1, 1, stream);
  if (rc != 0) return rc;
  // one direction's 26 values are one right-hand side: the solves write the transposed layout, straight into the caller's tensors if asked
  float* xq = tr ? dnudot_dq : workspace + 2 * blk;
  float* xn = tr ? dnudot_dnu : workspace + 3 * blk;
  float* xm = tr ? minv : workspace + 4 * blk;
  if (dnudot_dq && (rc = mass_solve_launch(c, rq, DD_MENV, BD_NCOL, nullptr, xq, DD_MENV, solve_flags, stream)) != 0) return rc;
  if (dnudot_dnu && (rc = mass_solve_launch(c, rn, DD_MENV, BD_NCOL, nullptr, xn, DD_MENV, solve_flags, stream)) != 0) return rc;
  if (minv && (rc = mass_solve_launch(c, eye, 0, BD_NCOL, nullptr, xm, DD_MENV, solve_flags, stream)) != 0) return rc;
  if (!tr) {
    hipLaunchKernelGGL(wbc_derivatives_transpose_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, xq, dnudot_dq, xn, dnudot_dnu, xm, minv);
    return c.launched();
  }
  return 0;
}

// ---- body-parameter regressor of inverse dynamics (include/wbc_sim.h: wbc_sim_inverse_dynamics_regressor) --------------------------------
// tau = Y(q, nu, nudot) pi: inverse dynamics is linear in every body's (m, m c, Ibar about the body's own origin, body axes). One env per
// 64-lane workgroup, two phases, one LDS hand-over:
//  1) lane b = moving body b: ba_walk root -> b (angular velocity, angular acceleration and the CLASSICAL acceleration of the body's own
//     origin, every lever a link offset), then E, p, the joint axis in F and, in BODY axes, w, alpha and d = E^T (a_o - g) go to LDS with
//     the body's current (m, c). In body axes about the body origin the wrench of body b is closed form in these three vectors:
//         force = m d + alpha x h + w x (w x h),   moment = h x d + Ibar alpha + w x Ibar w,   h = m c.
//  2) work item = (coordinate c, listed body b in the subtree c moves): with u^ = E_b^T u_c and w^ = u^ x E_b^T (p_b - o_c), the lever
//     between two origins of one chain, entry (c, b) is u^ . moment + w^ . force, column by column:
//         m: w^ . d;   h: w^ x alpha + (w^ x w) x w + d x u^;   Ibar: sym(u^, alpha) + sym(u^ x w, w),
//     sym(a, b) = (ax bx, ay by, az bz, ax by + ay bx, ax bz + az bx, ay bz + az by). The root rows take u_c = R^T e_j about F's origin
//     (rows 0:3: the force alone, w^ = E_b^T R^T e_j, whose Ibar columns are literal zeros). With `native` the ten values are chained to
//     d/d(m, c, I_c) at the body's own (m, c): Ibar = I_c + m (|c|^2 1 - c c^T).
// The output of one env is assembled in LDS a chunk at a time (RG_STAGE floats: whole rows, or whole bodies when transposed), zero-filled
// first -- the structural zeros and the fingers' rows are never computed -- and stored 16 bytes per lane. The root position is never read.
#define RG_NP 10                                // parameters per body
#define RG_BT 28                                // floats per body in LDS: E 0..8, p 9..11, joint axis in F 12..14, then body axes: w 15..17, alpha 18..20, d 21..23; m 24, c 25..27
#define RG_STAGE (12 * WBC_NB * RG_NP)          // 12 rows of all bodies, or 8 bodies' 260 floats and a rest
#define RG_TBODIES (RG_STAGE / (BD_NCOL * RG_NP))   // bodies per chunk, transposed
#define RG_MAXCHUNK 3
#define RG_MAXITEM (WBC_NB * (6 + WBC_MAX_DEPTH))   // every body under the six root rows and under the joints of its own path
static_assert((BD_NCOL + 11) / 12 <= RG_MAXCHUNK && (WBC_NB + RG_TBODIES - 1) / RG_TBODIES <= RG_MAXCHUNK && RG_STAGE % 4 == 0, "chunks");
static_assert((RG_STAGE + WBC_NB * RG_BT) * sizeof(float) <= 20 * 1024, "8 workgroups per CU");
struct RgConst : IdConst {
  int32_t nitem, nchunk;
  int32_t stride_c, stride_s, stride_k;         // floats between rows, listed bodies and parameters of one env's output
  int32_t env_floats;                           // 26 * 10 * listed bodies
  int32_t chunk_item[RG_MAXCHUNK + 1];          // the items of chunk k: chunk_item[k] .. chunk_item[k + 1]
  int32_t chunk_off[RG_MAXCHUNK], chunk_len[RG_MAXCHUNK];   // its floats of the env's output: first, count (both multiples of 4)
  uint8_t item_c[RG_MAXITEM], item_b[RG_MAXITEM], item_s[RG_MAXITEM];   // row, moving body, the body's place in the caller's list
};

extern "C" __global__ void __launch_bounds__(64) wbc_inverse_dynamics_regressor_kernel(RgConst C, const float* __restrict__ root,
                                                                                      const float* __restrict__ dofs,
                                                                                      const float* __restrict__ body_params,
                                                                                      const float* __restrict__ nudot, float* __restrict__ Y,
                                                                                      int native, int negate) {
  __shared__ __align__(16) float sStage[RG_STAGE];
  __shared__ float sB[WBC_NB][RG_BT];
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p, w, aw, ao;
    ba_walk(C, b, e, R, root, dofs, nudot, E, p, w, aw, ao);
    const f3 gF = matT_mul(R, mk3(C.gravity[0], C.gravity[1], C.gravity[2]));
    float m = C.mass[b], com[3] = {C.com[b][0], C.com[b][1], C.com[b][2]};
    const int slot = b == 0 ? TREE_BP_ROOT : (b == C.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + e * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
    }
    float* o = sB[b];
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = E[j];
    st3(o + 9, p); st3(o + 12, mat_mul(E, tree_axis(C.axis[b])));   // -1 for the root: no joint axis
    st3(o + 15, matT_mul(E, w)); st3(o + 18, matT_mul(E, aw)); st3(o + 21, matT_mul(E, ao - gF));
    o[24] = m; o[25] = com[0]; o[26] = com[1]; o[27] = com[2];
  }
  __syncthreads();

  float4* stage4 = reinterpret_cast<float4*>(sStage);
  float4* out4 = reinterpret_cast<float4*>(Y + e * (size_t)C.env_floats);
  for (int ch = 0; ch < C.nchunk; ++ch) {
    const int off = C.chunk_off[ch], len4 = C.chunk_len[ch] >> 2;
    for (int t = lane; t < len4; t += 64) stage4[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int it = C.chunk_item[ch] + lane; it < C.chunk_item[ch + 1]; it += 64) {
      const int c = C.item_c[it], b = C.item_b[it], s = C.item_s[it];
      const float* B = sB[b];
      f3 u, lever = ld3(B + 9);
      if (c < 6) {
        const int j = c < 3 ? c : c - 3;
        u = matT_mul(R, mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f));
      } else {
        const float* J = sB[C.col_body[c - 6]];
        u = ld3(J + 12);
        lever = lever - ld3(J + 9);
      }
      const f3 uh = matT_mul(B, u), w = ld3(B + 15), al = ld3(B + 18), d = ld3(B + 21);
      const bool lin = c < 3;
      const f3 wh = lin ? uh : cross(uh, matT_mul(B, lever));
      float y[RG_NP];
      y[0] = dot(wh, d);
      f3 yh = cross(wh, al) + cross(cross(wh, w), w);
      if (lin) {
#pragma unroll
        for (int k = 4; k < RG_NP; ++k) y[k] = 0.f;
      } else {
        yh = yh + cross(d, uh);
        const f3 t = cross(uh, w);
        y[4] = uh.x * al.x + t.x * w.x; y[5] = uh.y * al.y + t.y * w.y; y[6] = uh.z * al.z + t.z * w.z;
        y[7] = (uh.x * al.y + uh.y * al.x) + (t.x * w.y + t.y * w.x);
        y[8] = (uh.x * al.z + uh.z * al.x) + (t.x * w.z + t.z * w.x);
        y[9] = (uh.y * al.z + uh.z * al.y) + (t.y * w.z + t.z * w.y);
      }
      y[1] = yh.x; y[2] = yh.y; y[3] = yh.z;
      if (native) {                                          // d/d(m, c, I_c) from d/d(m, h, Ibar): h = m c, Ibar = I_c + m (|c|^2 1 - c c^T)
        const float m = B[24], cx = B[25], cy = B[26], cz = B[27];
        const float n0 = y[0] + (y[1] * cx + y[2] * cy + y[3] * cz) +
                         ((y[4] * (cy * cy + cz * cz) + y[5] * (cx * cx + cz * cz) + y[6] * (cx * cx + cy * cy)) -
                          (y[7] * (cx * cy) + y[8] * (cx * cz) + y[9] * (cy * cz)));
        const float n1 = m * (y[1] + ((2.f * cx) * (y[5] + y[6]) - (y[7] * cy + y[8] * cz)));
        const float n2 = m * (y[2] + ((2.f * cy) * (y[4] + y[6]) - (y[7] * cx + y[9] * cz)));
        const float n3 = m * (y[3] + ((2.f * cz) * (y[4] + y[5]) - (y[8] * cx + y[9] * cy)));
        y[0] = n0; y[1] = n1; y[2] = n2; y[3] = n3;
      }
      float* o = sStage + (c * C.stride_c + s * C.stride_s - off);
#pragma unroll
      for (int k = 0; k < RG_NP; ++k) o[k * C.stride_k] = negate ? -y[k] : y[k];
    }
    __syncthreads();
    for (int t = lane; t < len4; t += 64) out4[(off >> 2) + t] = stage4[t];
    __syncthreads();
  }
}

// The caller's list of bodies (NULL with 0: all, in order) into sel / nsel. False: not 1..WBC_NB distinct indices in 0..WBC_NB-1.
static bool rg_bodies(const int32_t* bodies, int nbodies, int32_t* sel, int& nsel) {
  if (!bodies) {
    if (nbodies != 0) return false;
    for (int b = 0; b < WBC_NB; ++b) sel[b] = b;
    nsel = WBC_NB;
    return true;
  }
  if (nbodies < 1 || nbodies > WBC_NB) return false;
  uint32_t seen = 0;
  for (int i = 0; i < nbodies; ++i) {
    if (bodies[i] < 0 || bodies[i] >= WBC_NB || ((seen >> bodies[i]) & 1u)) return false;
    seen |= 1u << bodies[i];
    sel[i] = bodies[i];
  }
  nsel = nbodies;
  return true;
}

// Fills C from the model and the list: the chunks of the layout and, chunk by chunk, the (row, body) items that are not structural zeros.
// 0, or 1: a tree the kernel cannot walk.
static int rg_const_fill(const DevConst* hc, const int32_t* sel, int nsel, int transposed, RgConst& C) {
  if (id_const_fill(hc, C) != 0) return 1;
  const int np = nsel * RG_NP;
  C.env_floats = BD_NCOL * np;
  int per;                                                   // rows (an even number: every chunk starts on 16 bytes) or bodies per chunk
  if (transposed) {
    C.stride_c = 1; C.stride_s = BD_NCOL * RG_NP; C.stride_k = BD_NCOL;
    per = RG_TBODIES;
    C.nchunk = (nsel + per - 1) / per;
  } else {
    C.stride_c = np; C.stride_s = RG_NP; C.stride_k = 1;
    per = RG_STAGE / np >= BD_NCOL ? BD_NCOL : (RG_STAGE / np) & ~1;
    C.nchunk = (BD_NCOL + per - 1) / per;
  }
  const int total = transposed ? nsel : BD_NCOL, unit = transposed ? BD_NCOL * RG_NP : np;
  C.nitem = 0;
  for (int ch = 0; ch < RG_MAXCHUNK; ++ch) {
    C.chunk_item[ch] = C.nitem;
    const int lo = ch * per, hi = ch < C.nchunk ? (lo + per < total ? lo + per : total) : lo;
    C.chunk_off[ch] = ch < C.nchunk ? lo * unit : 0;
    C.chunk_len[ch] = ch < C.nchunk ? (hi - lo) * unit : 0;
    if (ch >= C.nchunk) continue;
    for (int c = 0; c < BD_NCOL; ++c) {
      const int cb = c < 6 ? 0 : C.col_body[c - 6];
      if (cb < 0) continue;                                  // a locked finger: its rows stay zero
      for (int s = 0; s < nsel; ++s) {
        const int key = transposed ? s : c;
        if (key < lo || key >= hi || !((C.anc[sel[s]] >> cb) & 1u)) continue;
        if (C.nitem >= RG_MAXITEM) return 1;
        C.item_c[C.nitem] = (uint8_t)c; C.item_b[C.nitem] = (uint8_t)sel[s]; C.item_s[C.nitem] = (uint8_t)s;
        ++C.nitem;
      }
    }
  }
  C.chunk_item[RG_MAXCHUNK] = C.nitem;
  for (int i = C.nitem; i < RG_MAXITEM; ++i) { C.item_c[i] = 0; C.item_b[i] = 0; C.item_s[i] = 0; }
  return 0;
}

static int regressor_launch(const WbCall& c, const int32_t* sel, int nsel, const float* nudot, float* Y, int native, int transposed, int negate,
                            void* stream) {
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  RgConst C;
  if (rg_const_fill(c.hc, sel, nsel, transposed, C) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_inverse_dynamics_regressor_kernel, dim3(c.n), dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, c.bp, nudot, Y, native,
                     negate);
  return c.launched();
}

// bodies (host, or NULL with 0 = all), nudot (device f32 [N,26] or NULL = zeros), Y (device f32 [N,26,nbodies,10], 16-byte aligned): include/wbc_sim.h.
extern "C" int wbc_sim_inverse_dynamics_regressor(wbc_sim* s, const int32_t* bodies, int nbodies, const float* nudot, float* Y, int flags,
                                                  void* stream) {
  WbCall c("wbc_sim_inverse_dynamics_regressor", s, stream);
  if (!s) return c.no_sim();
  if (!Y) return c.fail(-1, "Y is NULL");
  int32_t sel[WBC_NB];
  int nsel = 0;
  if (!rg_bodies(bodies, nbodies, sel, nsel)) return c.fail(-1, "bodies must be 1..WBC_NB distinct moving-body indices, or NULL with nbodies 0");
  if (flags & ~(WBC_DERIV_TRANSPOSED | WBC_REGRESSOR_NATIVE)) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)nudot & 3u) || ((uintptr_t)Y & 15u)) return c.fail(-1, "nudot must be 4-byte aligned, Y 16-byte aligned");
  return regressor_launch(c, sel, nsel, nudot, Y, (flags & WBC_REGRESSOR_NATIVE) ? 1 : 0, (flags & WBC_DERIV_TRANSPOSED) ? 1 : 0, 0, stream);
}

// nudot = M^-1 (tau - h), then d nudot / d(parameters) = -M^-1 Y(q, nu, nudot): the regressor leaves -Y^T, one parameter's 26 values per
// right-hand side, in the workspace, and the solves go over it WBC_SOLVE_MAX_RHS columns at a time (include/wbc_sim.h).
extern "C" int wbc_sim_forward_dynamics_sensitivity(wbc_sim* s, const int32_t* bodies, int nbodies, const float* tau, float* nudot,
                                                    float* dnudot_dpi, float* workspace, int flags, void* stream) {
  WbCall c("wbc_sim_forward_dynamics_sensitivity", s, stream);
  if (!s) return c.no_sim();
  if (!nudot || !dnudot_dpi || !workspace) return c.fail(-1, "nudot / dnudot_dpi / workspace is NULL");
  int32_t sel[WBC_NB];
  int nsel = 0;
  if (!rg_bodies(bodies, nbodies, sel, nsel)) return c.fail(-1, "bodies must be 1..WBC_NB distinct moving-body indices, or NULL with nbodies 0");
  if (flags & ~(WBC_SOLVE_ARMATURE | WBC_REGRESSOR_NATIVE)) return c.fail(-1, "unknown flag bits");
  if ((((uintptr_t)tau | (uintptr_t)nudot | (uintptr_t)dnudot_dpi) & 3u) || ((uintptr_t)workspace & 15u))
    return c.fail(-1, "tau / nudot / dnudot_dpi must be 4-byte aligned, workspace 16-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  const int ncol = nsel * RG_NP;
  const int64_t env_stride = (int64_t)ncol * BD_NCOL;
  // nudot is written by the first two launches and read by the regressor while the workspace is written: none of the three may share bytes
  const uintptr_t bytes = (uintptr_t)c.n * env_stride * sizeof(float), x0 = (uintptr_t)dnudot_dpi, w0 = (uintptr_t)workspace;
  const uintptr_t n0 = (uintptr_t)nudot, nbytes = (uintptr_t)c.n * BD_NCOL * sizeof(float);
  if (x0 < w0 + bytes && w0 < x0 + bytes) return c.fail(-1, "dnudot_dpi overlaps workspace");
  if ((n0 < w0 + bytes && w0 < n0 + nbytes) || (n0 < x0 + bytes && x0 < n0 + nbytes)) return c.fail(-1, "nudot overlaps dnudot_dpi / workspace");
  const int solve_flags = flags & WBC_SOLVE_ARMATURE;
  int rc = forward_dynamics_run(c, s, tau, nudot, solve_flags, stream);
  if (rc != 0) return rc;
  rc = regressor_launch(c, sel, nsel, nudot, workspace, (flags & WBC_REGRESSOR_NATIVE) ? 1 : 0, 1, 1, stream);
  if (rc != 0) return rc;
  for (int k0 = 0; k0 < ncol; k0 += WBC_SOLVE_MAX_RHS) {
    const int k = ncol - k0 < WBC_SOLVE_MAX_RHS ? ncol - k0 : WBC_SOLVE_MAX_RHS;
    rc = mass_solve_launch(c, workspace + (size_t)k0 * BD_NCOL, env_stride, k, nullptr, dnudot_dpi + (size_t)k0 * BD_NCOL, env_stride,
                           solve_flags, stream);
    if (rc != 0) return rc;
  }
  return 0;
}

// ---- recursive identification of inertial parameters (include/wbc_sim.h: wbc_sim_identification_accumulate / _solve) ---------------------
// The consumer of the regressor: per env the normal equations A = sum Phi^T W Phi, b = sum Phi^T W z of the listed bodies' P = 10 nbodies
// linear parameters, with exponential forgetting, one launch per control step. Phi is the regressor's columns of the listed bodies and
// z = tau_gen - sum over the OTHER bodies of Y_b pi_b, both from the regressor's closed-form entries; Y never reaches HBM. One env per
// 64-lane workgroup, four phases:
//  1) lane b = moving body b: the regressor's phase 1 (ba_walk; E, p, the joint axis, w, alpha, d to LDS) and the body's current linear
//     parameters pi_b = (m, m c, I_c + m (|c|^2 1 - c c^T)) to LDS; the other lanes clear Phi and fetch the env's A, 16 bytes per lane;
//  2) work item = (row c, body b in the subtree c moves), ALL bodies: the ten closed-form values y. A listed body's go to Phi[c][s * 10 + k];
//     another body's are folded with its pi_b into one float per item (nothing is formed as tau - Phi pi: nothing cancels);
//  3) lane c = row c: z_c = tau_gen_c - (its items' floats, in item order), the row's weight (0 for the fingers' rows), z to `target`;
//  4) lane t = entries t, t + 64, ... of A's lower triangle: forget * A_ij + sum_c (w_c Phi_ci) Phi_cj over the 26 rows in order, written
//     to (i, j) and (j, i) of the LDS copy, which goes back 16 bytes per lane; lane i = entry i of b; lane 0 the two floats of stat.
// Every sum has a fixed order and no atomics: the bits repeat from run to run. An env without a row of positive weight stores nothing but
// its target (with WBC_IDENT_RESET: zeros). The root position is never read.
#define IA_MAXP (WBC_IDENT_MAX_BODIES * RG_NP)  // 30 parameters at most: the m <= 32 Cholesky core of wbc_delassus.h
#define IA_LP (IA_MAXP + 1)                     // LDS pitch of Phi's rows
#define IA_OTHER 0xff                           // item_s of a body that is not listed
static_assert(RG_MAXITEM < 256 && IA_MAXP <= 32 && (RG_NP * RG_NP) % 4 == 0, "items index in a byte, P fits the core, A is whole float4s");
struct IaConst : IdConst {
  int32_t nitem, np;                            // np = 10 * listed bodies
  uint32_t live;                                // bit c: row c is not a locked finger's
  uint8_t row_item[BD_NCOL + 1];                // the items of row c: row_item[c] .. row_item[c + 1]
  uint8_t item_c[RG_MAXITEM], item_b[RG_MAXITEM], item_s[RG_MAXITEM];   // row, moving body, its place in the caller's list or IA_OTHER
};

// The ten values of regressor entry (row c, body b) in the linear parameters: wbc_inverse_dynamics_regressor_kernel's phase 2, its
// statements as they stand there. Written out a second time, not shared: that kernel's bits depend on how its own statements contract
// into FMAs (wbc_tree.h), and it is left untouched.
__device__ __forceinline__ void ia_entry(const IaConst& C, const float* R, const float (*sB)[RG_BT], int c, int b, float* y) {
  const float* B = sB[b];
  f3 u, lever = ld3(B + 9);
  if (c < 6) {
    const int j = c < 3 ? c : c - 3;
    u = matT_mul(R, mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f));
  } else {
    const float* J = sB[C.col_body[c - 6]];
    u = ld3(J + 12);
    lever = lever - ld3(J + 9);
  }
  const f3 uh = matT_mul(B, u), w = ld3(B + 15), al = ld3(B + 18), d = ld3(B + 21);
  const bool lin = c < 3;
  const f3 wh = lin ? uh : cross(uh, matT_mul(B, lever));
  y[0] = dot(wh, d);
  f3 yh = cross(wh, al) + cross(cross(wh, w), w);
  if (lin) {
#pragma unroll
    for (int k = 4; k < RG_NP; ++k) y[k] = 0.f;
  } else {
    yh = yh + cross(d, uh);
    const f3 t = cross(uh, w);
    y[4] = uh.x * al.x + t.x * w.x; y[5] = uh.y * al.y + t.y * w.y; y[6] = uh.z * al.z + t.z * w.z;
    y[7] = (uh.x * al.y + uh.y * al.x) + (t.x * w.y + t.y * w.x);
    y[8] = (uh.x * al.z + uh.z * al.x) + (t.x * w.z + t.z * w.x);
    y[9] = (uh.y * al.z + uh.z * al.y) + (t.y * w.z + t.z * w.y);
  }
  y[1] = yh.x; y[2] = yh.y; y[3] = yh.z;
}

extern "C" __global__ void __launch_bounds__(64) wbc_identification_accumulate_kernel(
    IaConst C, const float* __restrict__ root, const float* __restrict__ dofs, const float* __restrict__ body_params,
    const float* __restrict__ nudot, const float* __restrict__ tau_gen, const float* __restrict__ row_weight, float forget, int reset,
    float* __restrict__ info_mat, float* __restrict__ info_vec, float* __restrict__ stat, float* __restrict__ target) {
  __shared__ __align__(16) float sA[IA_MAXP * IA_MAXP];   // the env's A, [P][P] as in HBM
  __shared__ float sPhi[BD_NCOL][IA_LP];
  __shared__ float sB[WBC_NB][RG_BT];
  __shared__ float sPi[WBC_NB][RG_NP];
  __shared__ float sT[RG_MAXITEM];                        // an unlisted body's y . pi_b, per item
  __shared__ float sZ[BD_NCOL], sW[BD_NCOL];
  const int lane = threadIdx.x, P = C.np;
  const size_t e = blockIdx.x;
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p, w, aw, ao;
    ba_walk(C, b, e, R, root, dofs, nudot, E, p, w, aw, ao);
    const f3 gF = matT_mul(R, mk3(C.gravity[0], C.gravity[1], C.gravity[2]));
    float m = C.mass[b], com[3] = {C.com[b][0], C.com[b][1], C.com[b][2]}, I6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) I6[j] = C.inertia[b][j];
    const int slot = b == 0 ? TREE_BP_ROOT : (b == C.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + e * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
    }
    float* o = sB[b];
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = E[j];
    st3(o + 9, p); st3(o + 12, mat_mul(E, tree_axis(C.axis[b])));   // -1 for the root: no joint axis
    st3(o + 15, matT_mul(E, w)); st3(o + 18, matT_mul(E, aw)); st3(o + 21, matT_mul(E, ao - gF));
    o[24] = m; o[25] = com[0]; o[26] = com[1]; o[27] = com[2];
    const float cx = com[0], cy = com[1], cz = com[2];
    float* q = sPi[b];
    q[0] = m; q[1] = m * cx; q[2] = m * cy; q[3] = m * cz;
    q[4] = I6[0] + m * (cy * cy + cz * cz); q[5] = I6[1] + m * (cx * cx + cz * cz); q[6] = I6[2] + m * (cx * cx + cy * cy);
    q[7] = I6[3] - m * (cx * cy); q[8] = I6[4] - m * (cx * cz); q[9] = I6[5] - m * (cy * cz);
  }
  for (int t = lane; t < BD_NCOL * IA_LP; t += 64) (&sPhi[0][0])[t] = 0.f;
  if (!reset) {
    const float4* in4 = reinterpret_cast<const float4*>(info_mat + e * (size_t)(P * P));
    for (int t = lane; t < (P * P) >> 2; t += 64) reinterpret_cast<float4*>(sA)[t] = in4[t];
  }
  __syncthreads();

  for (int it = lane; it < C.nitem; it += 64) {
    const int c = C.item_c[it], b = C.item_b[it], s = C.item_s[it];
    float y[RG_NP];
    ia_entry(C, R, sB, c, b, y);
    if (s != IA_OTHER) {
#pragma unroll
      for (int k = 0; k < RG_NP; ++k) sPhi[c][s * RG_NP + k] = y[k];
    } else {
      const float* q = sPi[b];
      sT[it] = (y[0] * q[0] + (y[1] * q[1] + y[2] * q[2] + y[3] * q[3])) +
               ((y[4] * q[4] + y[5] * q[5] + y[6] * q[6]) + (y[7] * q[7] + y[8] * q[8] + y[9] * q[9]));
    }
  }
  __syncthreads();

  if (lane < BD_NCOL) {
    const int c = lane;
    float others = 0.f;
    for (int it = C.row_item[c]; it < C.row_item[c + 1]; ++it)
      if (C.item_s[it] == IA_OTHER) others += sT[it];
    const float z = tau_gen[e * BD_NCOL + c] - others;
    if (target) target[e * BD_NCOL + c] = z;
    sZ[c] = z;
    sW[c] = ((C.live >> c) & 1u) ? (row_weight ? row_weight[e * BD_NCOL + c] : 1.f) : 0.f;
  }
  __syncthreads();

  float wzz = 0.f;                                          // every lane the same sums in the same order: no hand-over
  int rows = 0;
#pragma unroll
  for (int c = 0; c < BD_NCOL; ++c) {
    const float w = sW[c], z = sZ[c];
    wzz += (w * z) * z;
    rows += w > 0.f ? 1 : 0;
  }
  if (rows == 0 && !reset) return;                          // nothing observed: A, b and stat keep their bits, without decay

  for (int t = lane; t < P * (P + 1) / 2; t += 64) {
    int i, j;
    delassus_tri(t, i, j);
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < BD_NCOL; ++c) a += (sW[c] * sPhi[c][i]) * sPhi[c][j];
    const float v = reset ? a : forget * sA[i * P + j] + a;
    sA[i * P + j] = v; sA[j * P + i] = v;                   // only the lower triangle is ever read: the result is bit-symmetric
  }
  if (lane < P) {
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < BD_NCOL; ++c) a += (sW[c] * sPhi[c][lane]) * sZ[c];
    float* o = info_vec + e * (size_t)P + lane;
    *o = reset ? a : forget * *o + a;
  }
  if (lane == 0) {
    float* o = stat + e * 2;
    o[0] = reset ? wzz : forget * o[0] + wzz;
    o[1] = reset ? (float)rows : forget * o[1] + (float)rows;
  }
  __syncthreads();
  float4* out4 = reinterpret_cast<float4*>(info_mat + e * (size_t)(P * P));
  for (int t = lane; t < (P * P) >> 2; t += 64) out4[t] = reinterpret_cast<const float4*>(sA)[t];
}

// Fills C from the model and the list: every (row, body) entry that is not a structural zero, row by row, bodies in order.
static int ia_const_fill(const DevConst* hc, const int32_t* sel, int nsel, IaConst& C) {
  if (id_const_fill(hc, C) != 0) return 1;
  int slot[WBC_NB];
  for (int b = 0; b < WBC_NB; ++b) slot[b] = IA_OTHER;
  for (int s = 0; s < nsel; ++s) slot[sel[s]] = s;
  C.np = nsel * RG_NP; C.nitem = 0; C.live = 0;
  for (int c = 0; c < BD_NCOL; ++c) {
    C.row_item[c] = (uint8_t)C.nitem;
    const int cb = c < 6 ? 0 : C.col_body[c - 6];
    if (cb < 0) continue;                                    // a locked finger: the row never counts
    C.live |= 1u << c;
    for (int b = 0; b < WBC_NB; ++b) {
      if (!((C.anc[b] >> cb) & 1u)) continue;
      if (C.nitem >= RG_MAXITEM) return 1;
      C.item_c[C.nitem] = (uint8_t)c; C.item_b[C.nitem] = (uint8_t)b; C.item_s[C.nitem] = (uint8_t)slot[b];
      ++C.nitem;
    }
  }
  C.row_item[BD_NCOL] = (uint8_t)C.nitem;
  for (int i = C.nitem; i < RG_MAXITEM; ++i) { C.item_c[i] = 0; C.item_b[i] = 0; C.item_s[i] = IA_OTHER; }
  return 0;
}

// True if the byte ranges [a, a + na) and [b, b + nb) of two buffers that are both there share a byte.
static bool ia_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + nb && b0 < a0 + na;
}
// True if an output (the first `nout` of the list) shares a byte with any other buffer of the list.
static bool ia_any_overlap(const void* const* ptr, const size_t* bytes, int count, int nout) {
  for (int i = 0; i < nout; ++i)
    for (int j = 0; j < count; ++j)
      if (j != i && (j > i || j >= nout) && ia_overlap(ptr[i], bytes[i], ptr[j], bytes[j])) return true;
  return false;
}

// bodies (host, 1..3 distinct), nudot / row_weight / target (device f32 [N,26] or NULL), tau_gen (device f32 [N,26]), info_mat [N,P,P],
// info_vec [N,P], stat [N,2] (device f32, read and written), all 16-byte aligned: include/wbc_sim.h.
extern "C" int wbc_sim_identification_accumulate(wbc_sim* s, const int32_t* bodies, int nbodies, const float* nudot, const float* tau_gen,
                                                 const float* row_weight, float forget, float* info_mat, float* info_vec, float* stat,
                                                 float* target, int flags, void* stream) {
  WbCall c("wbc_sim_identification_accumulate", s, stream);
  if (!s) return c.no_sim();
  if (!tau_gen || !info_mat || !info_vec || !stat) return c.fail(-1, "tau_gen / info_mat / info_vec / stat is NULL");
  int32_t sel[WBC_NB];
  int nsel = 0;
  if (!bodies || nbodies > WBC_IDENT_MAX_BODIES || !rg_bodies(bodies, nbodies, sel, nsel))
    return c.fail(-1, "bodies must be 1..WBC_IDENT_MAX_BODIES distinct moving-body indices");
  if (!(forget > 0.f && forget <= 1.f)) return c.fail(-1, "forget must be in (0, 1]");
  if (flags & ~WBC_IDENT_RESET) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)nudot | (uintptr_t)tau_gen | (uintptr_t)row_weight | (uintptr_t)info_mat | (uintptr_t)info_vec | (uintptr_t)stat |
       (uintptr_t)target) & 15u)
    return c.fail(-1, "every buffer must be 16-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  const size_t np = (size_t)nsel * RG_NP, row = (size_t)c.n * BD_NCOL * sizeof(float);
  const void* ptr[7] = {info_mat, info_vec, stat, target, nudot, tau_gen, row_weight};
  const size_t bytes[7] = {(size_t)c.n * np * np * sizeof(float), (size_t)c.n * np * sizeof(float), (size_t)c.n * 2 * sizeof(float), row, row, row, row};
  if (ia_any_overlap(ptr, bytes, 7, 4)) return c.fail(-1, "info_mat / info_vec / stat / target overlap another buffer");
  IaConst C;
  if (ia_const_fill(c.hc, sel, nsel, C) != 0) return c.no_tree();
  hipLaunchKernelGGL(wbc_identification_accumulate_kernel, dim3(c.n), dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, c.bp, nudot, tau_gen,
                     row_weight, forget, (flags & WBC_IDENT_RESET) ? 1 : 0, info_mat, info_vec, stat, target);
  return c.launched();
}

// (A + Lambda) pi = b + Lambda pi_0 per env, one env per 64-lane workgroup, lane i = parameter i. The matrix is equilibrated to a unit
// diagonal, D = diag(A + Lambda)^-1/2, factorised by delassus_cholesky and solved by delassus_lane_solve (wbc_delassus.h, as they stand);
// the strict upper triangle of the LDS block keeps A as it came, for the residual sum. An env with a diagonal entry that is not positive
// and finite, or with a squared pivot of the equilibrated factor <= pivot_tol, falls back to the prior.
#define IS_LA 33                                // LDS pitch of the 32 x 32 blocks
extern "C" __global__ void __launch_bounds__(64) wbc_identification_solve_kernel(
    int P, const float* __restrict__ info_mat, const float* __restrict__ info_vec, const float* __restrict__ stat,
    const float* __restrict__ prior, const float* __restrict__ prior_weight, float pivot_tol, float* __restrict__ pi_hat,
    float* __restrict__ theta_hat, float* __restrict__ cov_diag, float* __restrict__ sse, int32_t* __restrict__ status) {
  __shared__ float sL[32][IS_LA];                          // lower triangle: the equilibrated matrix, then its factor; above the diagonal: A
  __shared__ float sX[32][IS_LA];                          // the identity, then the columns of the equilibrated inverse (cov_diag only)
  __shared__ float sD[32], sV[32], sDiag[32], sPi[32], sQ[32], sLin[32];
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;
  const bool row = lane < P;
  for (int t = lane; t < P * P; t += 64) sL[t / P][t % P] = info_mat[e * (size_t)(P * P) + t];
  __syncthreads();
  float lam = 0.f, p0 = 0.f, bi = 0.f, dm = 1.f;
  if (row) {
    lam = prior_weight ? prior_weight[e * P + lane] : 0.f;
    p0 = prior ? prior[e * P + lane] : 0.f;
    bi = info_vec[e * P + lane];
    sDiag[lane] = sL[lane][lane];
    dm = sL[lane][lane] + lam;
  }
  const bool okd = dm > 0.f && dm < INFINITY;
  const float sc = okd ? 1.f / __fsqrt_rn(dm) : 0.f;
  if (lane < 32) sV[lane] = sc;
  __syncthreads();
  if (row) {
    for (int j = 0; j < lane; ++j) sL[lane][j] = (sc * sL[lane][j]) * sV[j];
    sL[lane][lane] = (sc * dm) * sc;
  }
  delassus_cholesky<IS_LA>(sL, sD, P, lane);
  __syncthreads();
  const float idv = row ? sD[lane] : 0.f;
  const bool bad = __any((row && !okd) || !(idv * idv * pivot_tol < 1.f)) != 0;
  delassus_lane_solve<IS_LA>(sL, sD, sV, P, lane, row ? sc * (bi + lam * p0) : 0.f);
  const float pi = row ? (bad ? p0 : sc * sV[lane]) : 0.f;
  if (row) {
    sPi[lane] = pi;
    pi_hat[e * P + lane] = pi;
  }
  if (cov_diag) {                                          // diag((A + Lambda)^-1) = D diag((D (A + Lambda) D)^-1) D
    for (int t = lane; t < P * P; t += 64) sX[t / P][t % P] = t / P == t % P ? 1.f : 0.f;
    __syncthreads();
    if (row) {
      delassus_column_solve<IS_LA>(sL, sD, &sX[0][lane], IS_LA, P);
      cov_diag[e * P + lane] = bad ? INFINITY : (sc * sX[lane][lane]) * sc;
    }
  }
  __syncthreads();
  if (sse) {                                               // stat_0 - 2 pi^T b + pi^T A pi with A as it came
    if (row) {
      float r = 0.f;
      for (int j = 0; j < P; ++j) r += (j == lane ? sDiag[j] : (lane < j ? sL[lane][j] : sL[j][lane])) * sPi[j];
      sQ[lane] = pi * r;
      sLin[lane] = pi * bi;
    }
    __syncthreads();
    if (lane == 0) {
      float q = 0.f, l = 0.f;
      for (int j = 0; j < P; ++j) { q += sQ[j]; l += sLin[j]; }
      sse[e] = fmaxf((stat[e * 2] - 2.f * l) + q, 0.f);
    }
  }
  if (lane < P / RG_NP && (theta_hat || status)) {         // lane s = listed body s: (m, c, I_c) and the flags
    const float* q = sPi + lane * RG_NP;
    const float m = q[0], cx = q[1] / m, cy = q[2] / m, cz = q[3] / m;
    float th[RG_NP] = {m, cx, cy, cz, q[4] - m * (cy * cy + cz * cz), q[5] - m * (cx * cx + cz * cz), q[6] - m * (cx * cx + cy * cy),
                       q[7] + m * (cx * cy), q[8] + m * (cx * cz), q[9] + m * (cy * cz)};
    int st = 1;
    if (bad && !prior) {
#pragma unroll
      for (int k = 0; k < RG_NP; ++k) th[k] = 0.f;
    }
    if (!bad) {
      const float xx = th[4], yy = th[5], zz = th[6], xy = th[7], xz = th[8], yz = th[9];
      const float det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
      const bool pd = xx > 0.f && xx * yy - xy * xy > 0.f && det > 0.f;
      // lambda_1 + lambda_2 >= lambda_3  <=>  T = (trace / 2) 1 - I_c is positive semi-definite: all seven principal minors >= 0
      const float h = 0.5f * (xx + yy + zz), a = h - xx, b = h - yy, c = h - zz;
      const float dT = a * (b * c - yz * yz) - xy * (xy * c + yz * xz) - xz * (xy * yz + b * xz);   // T's off-diagonal entries are -xy, -xz, -yz
      const bool tri = a >= 0.f && b >= 0.f && c >= 0.f && a * b - xy * xy >= 0.f && a * c - xz * xz >= 0.f && b * c - yz * yz >= 0.f && dT >= 0.f;
      st = (m > 0.f ? 0 : 2) | (pd ? 0 : 4) | (tri ? 0 : 8);
    }
    if (theta_hat) {
#pragma unroll
      for (int k = 0; k < RG_NP; ++k) theta_hat[(e * (P / RG_NP) + lane) * RG_NP + k] = th[k];
    }
    if (status) status[e * (P / RG_NP) + lane] = st;
  }
}

// info_mat [N,P,P], info_vec [N,P], stat [N,2] (device f32, read), prior / prior_weight (device f32 [N,nbodies,10] or NULL), pi_hat and
// the optional theta_hat / cov_diag [N,nbodies,10], sse [N], status int32 [N,nbodies]: include/wbc_sim.h.
extern "C" int wbc_sim_identification_solve(wbc_sim* s, int nbodies, const float* info_mat, const float* info_vec, const float* stat,
                                            const float* prior, const float* prior_weight, float pivot_tol, float* pi_hat, float* theta_hat,
                                            float* cov_diag, float* sse, int32_t* status, void* stream) {
  WbCall c("wbc_sim_identification_solve", s, stream);
  if (!s) return c.no_sim();
  if (!info_mat || !info_vec || !pi_hat) return c.fail(-1, "info_mat / info_vec / pi_hat is NULL");
  if (sse && !stat) return c.fail(-1, "stat is NULL with sse given");
  if (prior_weight && !prior) return c.fail(-1, "prior is NULL with prior_weight given");
  if (nbodies < 1 || nbodies > WBC_IDENT_MAX_BODIES) return c.fail(-1, "nbodies must be 1..WBC_IDENT_MAX_BODIES");
  if (!(pivot_tol > 0.f && pivot_tol < INFINITY)) return c.fail(-1, "pivot_tol must be positive and finite");
  if (((uintptr_t)info_mat | (uintptr_t)info_vec | (uintptr_t)stat | (uintptr_t)prior | (uintptr_t)prior_weight | (uintptr_t)pi_hat |
       (uintptr_t)theta_hat | (uintptr_t)cov_diag | (uintptr_t)sse | (uintptr_t)status) & 15u)
    return c.fail(-1, "every buffer must be 16-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  const size_t np = (size_t)nbodies * RG_NP, vec = (size_t)c.n * np * sizeof(float);
  const void* ptr[10] = {pi_hat, theta_hat, cov_diag, sse, status, info_mat, info_vec, stat, prior, prior_weight};
  const size_t bytes[10] = {vec, vec, vec, (size_t)c.n * sizeof(float), (size_t)c.n * nbodies * sizeof(int32_t), vec * np, vec,
                            (size_t)c.n * 2 * sizeof(float), vec, vec};
  if (ia_any_overlap(ptr, bytes, 10, 5)) return c.fail(-1, "an output overlaps another buffer");
  hipLaunchKernelGGL(wbc_identification_solve_kernel, dim3(c.n), dim3(64), 0, (hipStream_t)stream, (int)np, info_mat, info_vec, stat, prior,
                     prior_weight, pivot_tol, pi_hat, theta_hat, cov_diag, sse, status);
  return c.launched();
}

// ---- analytic derivatives of stance-constrained forward dynamics (include/wbc_sim.h: wbc_sim_constrained_dynamics_derivatives) ----------
// The solution (nudot, lambda) of wbc_sim_constrained_dynamics satisfies r1 = ID(q, nu, nudot) [+ armature nudot] - Jc^T lambda - tau = 0
// and r2 = Jc nudot + (Jdot nu)_c - a_des + damping lambda = 0. With x a direction of q or of nu, X = -M^-1 dr1/dx, Y = M^-1 Jc^T:
//     dlambda/dx = -(A + damping I)^-1 (Jc X + dr2/dx),   dnudot/dx = X + Y dlambda/dx;   for tau, X = M^-1 and Jc X = Y^T.
// dr1/dx is wbc_dynamics_derivatives_kernel's output at the solution's nudot, less d(Jc^T lambda)/dq; the two kernels below supply that
// term and dr2/dx, and the algebra per env. The tangent convention is wbc_sim_inverse_dynamics_derivatives'.
#define CT_MAXPAIR (WBC_CONSTR_MAX_BODIES * (3 + WBC_MAX_DEPTH))   // (listed body, direction) pairs of one output: 45
#define CT_R2ENV (2 * CD_MAXROWS * BD_NCOL)     // floats of dr2/dq, dr2/dnu per env in the workspace: [2][15][26]
static_assert(CT_MAXPAIR <= 64 && WBC_NB + WBC_CONSTR_MAX_BODIES <= 64, "one round of lanes");
struct CtConst : TreeWalk, TreeRigid, TreeCols {
  int32_t nb, rb[WBC_CONSTR_MAX_BODIES];       // the listed rigid bodies
  int32_t npair;                               // live (listed body, direction) pairs of one output
  uint8_t pair_k[CT_MAXPAIR], pair_u[CT_MAXPAIR];   // u: 0..2 a root direction, 3 + i the joint path[body][i]
};

// One env per 64-lane workgroup.
//  1) lane b < 19 = moving body b walks root -> b (frames only) and leaves its joint axis and origin (F) in LDS; lane 19 + k leaves listed
//     body k's origin and lambda_k turned to F's axes.
//  2) dr2/dq and dr2/dnu [3 nb, 26], the partials of the listed origins' classical acceleration Jc nudot + Jdot nu at fixed nudot: lane =
//     (listed body, direction) pair redoes the body's path walk with omega, alpha and the classical acceleration of the body's own origin
//     paired with their tangents (the vw, aw, ao lines of wbc_dynamics_derivatives_kernel's walk; the root rotation is seeded in the
//     root body's frame, see below), carries them to rb_offset and turns the result to world axes. Every lever is a link or body offset. Every other entry of a row is exactly 0, as are the rows of an inactive body.
//  3) + d(Jc^T lambda)/dq into the block of -dtau/dq [direction][row]: the tangent of a world-fixed force lambda_k applied at the origin
//     x_k, in closed form from the joints' axes a and origins o (the root rotation counts as a joint above all with axis e_j, the root's
//     angular rows as one with axis e_j that nothing turns): with l_c = x_k - o_c, a direction x strictly above row c turns c's axis and
//     lever, d(a_c x l_c) = a_x x (a_c x l_c); otherwise it moves x_k alone, d(a_c x l_c) = a_c x (a_x x l_x). Triple products with lambda
//     are formed in F's axes.
// A single-wavefront workgroup: the __syncthreads() order the LDS traffic and cost no barrier instruction. The root position and linear
// velocity are never read.
extern "C" __global__ void __launch_bounds__(64) wbc_constraint_tangent_kernel(CtConst C, const float* __restrict__ root,
                                                                              const float* __restrict__ dofs,
                                                                              const uint8_t* __restrict__ active,
                                                                              const float* __restrict__ nudot, const float* __restrict__ lambda,
                                                                              int n, int want_q, int want_nu, float* __restrict__ rq,
                                                                              float* __restrict__ r2) {
  __shared__ float sJ[WBC_NB][6];                  // joint axis, joint origin, in F
  __shared__ float sX[WBC_CONSTR_MAX_BODIES][6];   // listed body's origin, lambda, in F
  __shared__ float sR[2][CD_MAXROWS][CD_LD];       // dr2/dq, dr2/dnu
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;
  if ((int)blockIdx.x >= n) return;
  const int nb = C.nb, m = 3 * nb;
  const f3 zero = mk3(0.f, 0.f, 0.f);
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  uint32_t act = 0;                                // bit k: listed body k is active
#pragma unroll
  for (int k = 0; k < WBC_CONSTR_MAX_BODIES; ++k)
    if (k < nb && (!active || active[e * nb + k])) act |= 1u << k;

  if (lane < WBC_NB + nb) {
    const bool body = lane < WBC_NB;
    const int k = body ? 0 : lane - WBC_NB, r = C.rb[k], b = body ? lane : C.rb_body[r];
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = zero, Sw = zero;
#pragma nounroll
    for (int i = 0; i < WBC_MAX_DEPTH; ++i) {
      const int a = C.path[b][i];
      if (a < 0) break;
      float Q[9];
      const f3 u = tree_joint_rot(C.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * C.dof[a]], Q);
      Sw = tree_frame_step(E, p, Q, C.joint_xyz[a], u);
    }
    if (body) {
      st3(sJ[b], Sw); st3(sJ[b] + 3, p);
    } else {
      st3(sX[k], p + mat_mul(E, mk3(C.rb_offset[r][0], C.rb_offset[r][1], C.rb_offset[r][2])));
      st3(sX[k] + 3, ((act >> k) & 1u) ? matT_mul(R, ld3(lambda + e * m + 3 * k)) : zero);
    }
  }
  for (int t = lane; t < 2 * CD_MAXROWS * CD_LD; t += 64) (&sR[0][0][0])[t] = 0.f;
  __syncthreads();

  const f3 w0 = matT_mul(R, ld3(root + e * 26 + 10));
  const f3 al0 = matT_mul(R, ld3(nudot + e * BD_NCOL + 3)), a0 = matT_mul(R, ld3(nudot + e * BD_NCOL));
#pragma nounroll
  for (int which = 0; which < 2; ++which) {
    if (!(which ? want_nu : want_q) || lane >= C.npair) continue;
    const int k = C.pair_k[lane], u = C.pair_u[lane], r = C.rb[k], b = C.rb_body[r];
    if (k >= nb || !((act >> k) & 1u)) continue;
    const int t = u < 3 ? u + 3 * which : 3 + u + 6 * which;   // the derivative kernel's slots: rotation 0..2, omega 3..5, q 6 + i, qd 12 + i
    const f3 phi = matT_mul(R, mk3(u == 0 ? 1.f : 0.f, u == 1 ? 1.f : 0.f, u == 2 ? 1.f : 0.f));
    // Root rotation: the walk's axes stay where F stood, so the root vectors (world components held) keep their components and have no
    // tangent; the root BODY's frame turns in them, dE = [phi]x. (wbc_dynamics_derivatives_kernel turns the root vectors by -phi x (.)
    // instead and the world rows back by e_j x (.): the same derivative, but a_root x phi and e_j x a_root then cancel only to rounding,
    // an error the size of |nudot[0:3]| that no term of these rows accounts for.)
    const float rot = t < 3 ? 1.f : 0.f, omg = t >= 3 && t < 6 ? 1.f : 0.f;
    d3 vw = mkd3(w0, phi * omg);
    d3 aw = mkd3(al0, zero), ao = mkd3(a0, zero);
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    float dE[9] = {0.f, -phi.z * rot, phi.y * rot, phi.z * rot, 0.f, -phi.x * rot, -phi.y * rot, phi.x * rot, 0.f};
    int col = 3 + u;                               // the output column: a root direction, or the joint's
#pragma nounroll
    for (int i = 0; i < WBC_MAX_DEPTH; ++i) {
      const int a = C.path[b][i];
      if (a < 0) break;
      const int d = C.dof[a];
      if (u == 3 + i) col = 6 + d;
      const float dq = t == 6 + i ? 1.f : 0.f;
      float s, c, Q[9], dQ[9];
      const f3 uu = tree_joint_rot(C.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * d], Q, s, c);
      tree_rodrigues(uu, c * dq, -s * dq, s * dq, dQ);
      const f3 xyz = mk3(C.joint_xyz[a][0], C.joint_xyz[a][1], C.joint_xyz[a][2]);
      const d3 rr = mkd3(mat_mul(E, xyz), mat_mul(dE, xyz));
      ao = ao + cross(aw, rr) + cross(vw, cross(vw, rr));
      float En[9], dEQ[9], EdQ[9];
      tree_frame_mul(E, Q, En);
      tree_frame_mul(dE, Q, dEQ);
      tree_frame_mul(E, dQ, EdQ);
#pragma unroll
      for (int j = 0; j < 9; ++j) { E[j] = En[j]; dE[j] = dEQ[j] + EdQ[j]; }
      const d3 Sw = mkd3(mat_mul(E, uu), mat_mul(dE, uu));
      du qd;
      qd.v = dofs[e * (2 * WBC_NDOF) + 2 * d + 1];
      qd.d = t == 12 + i ? 1.f : 0.f;
      const float qdd = nudot[e * BD_NCOL + 6 + d];
      const d3 jw = Sw * qd;
      aw = aw + Sw * qdd + cross(vw, jw);
      vw = vw + jw;
    }
    const f3 off = mk3(C.rb_offset[r][0], C.rb_offset[r][1], C.rb_offset[r][2]);
    const d3 xo = mkd3(mat_mul(E, off), mat_mul(dE, off));
    const d3 lin = ao + cross(aw, xo) + cross(vw, cross(vw, xo));
    const f3 val = mat_mul(R, lin.d);
    sR[which][3 * k][col] = val.x; sR[which][3 * k + 1][col] = val.y; sR[which][3 * k + 2][col] = val.z;
  }
  __syncthreads();
  for (int t = lane; t < 2 * m * BD_NCOL; t += 64) {
    const int g = t / (m * BD_NCOL), rem = t - g * (m * BD_NCOL), i = rem / BD_NCOL, x = rem - i * BD_NCOL;
    if (g ? want_nu : want_q) r2[e * CT_R2ENV + g * (CD_MAXROWS * BD_NCOL) + rem] = sR[g][i][x];
  }

  if (!want_q) return;
  for (int idx = lane; idx < DD_MENV; idx += 64) {
    const int x = idx / BD_NCOL, c = idx - x * BD_NCOL;          // direction, row of tau: the block is [direction][row]
    const int xb = x < 6 ? 0 : C.col_body[x - 6], cb = c < 6 ? 0 : C.col_body[c - 6];
    if (x < 3 || c < 3 || xb < 0 || cb < 0) continue;
    const f3 ax = x < 6 ? matT_mul(R, mk3(x == 3 ? 1.f : 0.f, x == 4 ? 1.f : 0.f, x == 5 ? 1.f : 0.f)) : ld3(sJ[xb]);
    const f3 ac = c < 6 ? matT_mul(R, mk3(c == 3 ? 1.f : 0.f, c == 4 ? 1.f : 0.f, c == 5 ? 1.f : 0.f)) : ld3(sJ[cb]);
    const f3 ox = x < 6 ? zero : ld3(sJ[xb] + 3), oc = c < 6 ? zero : ld3(sJ[cb] + 3);
    // x strictly above c: the root rotation above every joint, a joint above the joints further out on its chain
    const bool above = c >= 6 && (x < 6 || (xb != cb && ((C.anc[cb] >> xb) & 1u)));
    float val = 0.f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < WBC_CONSTR_MAX_BODIES; ++k) {
      if (k >= nb || !((act >> k) & 1u)) continue;
      const uint32_t anc = C.anc[C.rb_body[C.rb[k]]];
      if (!((anc >> xb) & 1u) || !((anc >> cb) & 1u)) continue;
      const f3 xk = ld3(sX[k]), lam = ld3(sX[k] + 3);
      const f3 v = above ? cross(ax, cross(ac, xk - oc)) : cross(ac, cross(ax, xk - ox));
      val += dot(v, lam);
      any = true;
    }
    if (any) rq[e * DD_MENV + idx] += val;
  }
}

// Per env, one 64-lane workgroup: A + damping I rebuilt from the workspace's J and Y (delassus_fill, identity rows where a body is
// inactive) and factorised (delassus_cholesky); then per requested group g (q, nu, tau), one after the other in the same LDS blocks:
// X [direction][row] = the mass solve's output; Z[i][x] = Jc_i . X_x + dr2_i/dx (for tau: Y_i[x]); lane x solves its column
// (delassus_column_solve) and negates it: dlambda/dx; dnudot/dx = X_x + sum_i Y_i Z[i][x]. The blocks sit in LDS, so either layout is
// stored directly with consecutive lanes on consecutive addresses. Literal zeros: columns 0:3 of the q / nu groups, the fingers' rows and
// columns, the rows of an inactive body. A single-wavefront workgroup: the __syncthreads() order the LDS traffic.
struct CsOut { float *dnd[3], *dlam[3]; const float* X[3]; };
extern "C" __global__ void __launch_bounds__(64) wbc_constraint_derivatives_solve_kernel(const float* __restrict__ rhs, const float* __restrict__ Y,
                                                                                        const float* __restrict__ r2,
                                                                                        const uint8_t* __restrict__ active, float damping,
                                                                                        int nb, uint32_t live_cols, int n, int transposed,
                                                                                        CsOut O) {
  __shared__ float sJ[CD_MAXROWS][CD_LD], sY[CD_MAXROWS][CD_LD], sZ[CD_MAXROWS][CD_LD];
  __shared__ float sX[BD_NCOL][CD_LD];
  __shared__ float sA[CD_MAXROWS][CD_MAXROWS + 1];   // lower triangle: A, then L
  __shared__ float sD[CD_MAXROWS + 1];
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;
  if ((int)blockIdx.x >= n) return;
  const int m = 3 * nb;
  const float *rp = rhs + e * (size_t)((m + 1) * BD_NCOL), *yp = Y + e * (size_t)((m + 1) * BD_NCOL);
  for (int t = lane; t < m * BD_NCOL; t += 64) {
    const int r = t / BD_NCOL, c = t - r * BD_NCOL;
    sJ[r][c] = rp[t]; sY[r][c] = yp[t];
  }
  uint32_t act = 0;                                // bit i: row i belongs to an active body
#pragma unroll
  for (int k = 0; k < WBC_CONSTR_MAX_BODIES; ++k)
    if (k < nb && (!active || active[e * nb + k])) act |= 7u << (3 * k);
  __syncthreads();
  delassus_fill(sJ, sY, sA, m, act, damping, lane, 64);
  delassus_cholesky(sA, sD, m, lane);
  __syncthreads();

#pragma nounroll
  for (int g = 0; g < 3; ++g) {
    float *dnd = O.dnd[g], *dlam = O.dlam[g];
    if (!dnd && !dlam) continue;
    const float* X = O.X[g];                       // NULL: the tau group with dlambda alone, where Z needs no X
    if (X)
      for (int t = lane; t < DD_MENV; t += 64) {
        const int x = t / BD_NCOL, c = t - x * BD_NCOL;
        sX[x][c] = X[e * DD_MENV + t];
      }
    __syncthreads();
    for (int t = lane; t < m * BD_NCOL; t += 64) {
      const int i = t / BD_NCOL, x = t - i * BD_NCOL;
      float z;
      if (g == 2) z = sY[i][x];
      else {
        z = r2[e * CT_R2ENV + g * (CD_MAXROWS * BD_NCOL) + t];
#pragma unroll
        for (int c = 0; c < BD_NCOL; ++c) z += sJ[i][c] * sX[x][c];
      }
      sZ[i][x] = ((act >> i) & 1u) ? z : 0.f;
    }
    __syncthreads();
    if (lane < BD_NCOL) {
      delassus_column_solve(sA, sD, &sZ[0][lane], CD_LD, m);
#pragma nounroll
      for (int i = 0; i < m; ++i) sZ[i][lane] = -sZ[i][lane];
    }
    __syncthreads();
    const uint32_t cols = g == 2 ? live_cols : live_cols & ~7u;   // directions that are not literal zeros
    if (dnd)
      for (int idx = lane; idx < DD_MENV; idx += 64) {
        const int hi = idx / BD_NCOL, lo = idx - hi * BD_NCOL;
        const int c = transposed ? lo : hi, x = transposed ? hi : lo;   // row of nudot, direction
        float v = sX[x][c];
#pragma unroll
        for (int i = 0; i < CD_MAXROWS; ++i)
          if (i < m) v += sY[i][c] * sZ[i][x];
        dnd[e * DD_MENV + idx] = (((live_cols >> c) & 1u) && ((cols >> x) & 1u)) ? v : 0.f;
      }
    if (dlam)
      for (int idx = lane; idx < m * BD_NCOL; idx += 64) {
        const int i = transposed ? idx % m : idx / BD_NCOL, x = transposed ? idx / m : idx - i * BD_NCOL;
        dlam[e * (size_t)(m * BD_NCOL) + idx] = (((act >> i) & 1u) && ((cols >> x) & 1u)) ? sZ[i][x] : 0.f;
      }
    __syncthreads();
  }
}

// Workspace layout (floats): wbc_sim_constrained_dynamics' own; lambda [N, 16] for the call without a lambda output; -dr1/dq and -dr1/dnu
// [N, 26, 26] ([direction][row]); the three solve results of the same shape; dr2/dq, dr2/dnu [N, 2, 15, 26]; one 26 x 26 identity.
extern "C" size_t wbc_sim_constrained_dynamics_derivatives_workspace_floats(int num_envs, int nbodies) {
  const size_t base = wbc_sim_constrained_dynamics_workspace_floats(num_envs, nbodies);
  return base ? base + (size_t)num_envs * (CD_GSTRIDE + 5 * DD_MENV + CT_R2ENV) + DD_MENV : 0;
}

// Launches on `stream`: the four of wbc_sim_constrained_dynamics, wbc_dynamics_derivatives_kernel at that nudot, the tangent kernel (if a
// q or nu output is asked for), one mass solve of 26 right-hand sides per requested group, the solve kernel. Arguments: include/wbc_sim.h.
extern "C" int wbc_sim_constrained_dynamics_derivatives(wbc_sim* s, const int32_t* rigid_bodies, int nbodies, const uint8_t* active,
                                                        const float* tau, const float* acc_des, float damping, int flags, float* nudot,
                                                        float* lambda, float* dnudot_dq, float* dnudot_dnu, float* dnudot_dtau,
                                                        float* dlambda_dq, float* dlambda_dnu, float* dlambda_dtau, float* workspace,
                                                        void* stream) {
  WbCall c("wbc_sim_constrained_dynamics_derivatives", s, stream);
  if (!s) return c.no_sim();
  if (!rigid_bodies || !nudot || !workspace) return c.fail(-1, "rigid_bodies / nudot / workspace is NULL");
  if (!dnudot_dq && !dnudot_dnu && !dnudot_dtau && !dlambda_dq && !dlambda_dnu && !dlambda_dtau)
    return c.fail(-1, "all six derivative outputs are NULL");
  if (flags & ~(WBC_SOLVE_ARMATURE | WBC_DERIV_TRANSPOSED)) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)dnudot_dq | (uintptr_t)dnudot_dnu | (uintptr_t)dnudot_dtau | (uintptr_t)dlambda_dq | (uintptr_t)dlambda_dnu |
       (uintptr_t)dlambda_dtau) & 3u)
    return c.fail(-1, "the derivative outputs must be 4-byte aligned");
  const size_t base = wbc_sim_constrained_dynamics_workspace_floats(c.n, nbodies);   // 0: refused below
  const int n = c.n;
  const size_t blk = (size_t)(n > 0 ? n : 0) * DD_MENV;
  float* lam = lambda ? lambda : workspace + base;
  const int solve_flags = flags & WBC_SOLVE_ARMATURE;
  CtConst T;
  {
    CdConst C;
    const int rc = constrained_dynamics_run(c, s, rigid_bodies, nbodies, active, tau, acc_des, damping, solve_flags, nudot, lam, workspace,
                                            stream, C);
    if (rc != 0 || n <= 0) return rc;
    static_cast<TreeWalk&>(T) = C; static_cast<TreeRigid&>(T) = C; static_cast<TreeCols&>(T) = C;
    T.nb = C.nb;
    for (int k = 0; k < WBC_CONSTR_MAX_BODIES; ++k) T.rb[k] = C.rb[k];
  }
  T.npair = 0;
  for (int k = 0; k < nbodies; ++k) {
    const int b = T.rb_body[T.rb[k]];
    int depth = 0;
    while (depth < WBC_MAX_DEPTH && T.path[b][depth] >= 0) ++depth;
    for (int u = 0; u < 3 + depth; ++u) { T.pair_k[T.npair] = (uint8_t)k; T.pair_u[T.npair] = (uint8_t)u; ++T.npair; }
  }
  for (int i = T.npair; i < CT_MAXPAIR; ++i) { T.pair_k[i] = 0; T.pair_u[i] = 0; }
  uint32_t live_cols = 63u;
  for (int d = 0; d < WBC_NDOF; ++d) if (T.col_body[d] >= 0) live_cols |= 1u << (6 + d);
  const bool gq = dnudot_dq || dlambda_dq, gn = dnudot_dnu || dlambda_dnu;
  const int nrow = 3 * nbodies + 1;
  const float *jblk = workspace, *Y = workspace + (size_t)n * nrow * BD_NCOL;
  float* w = workspace + base + (size_t)n * CD_GSTRIDE;
  float *rq = gq ? w : nullptr, *rn = gn ? w + blk : nullptr;
  float *xq = w + 2 * blk, *xn = w + 3 * blk, *xm = w + 4 * blk, *r2 = w + 5 * blk, *eye = dnudot_dtau ? r2 + (size_t)n * CT_R2ENV : nullptr;
  int rc;
  if ((gq || gn || eye) && (rc = derivatives_launch(c, nudot, rq, rn, eye, 1, 1, stream)) != 0) return rc;
  if (gq || gn) {
    hipLaunchKernelGGL(wbc_constraint_tangent_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, T, c.root, c.dofs, active, (const float*)nudot,
                       (const float*)lam, n, gq ? 1 : 0, gn ? 1 : 0, rq, r2);
    if ((rc = c.launched()) != 0) return rc;
  }
  if (gq && (rc = mass_solve_launch(c, rq, DD_MENV, BD_NCOL, nullptr, xq, DD_MENV, solve_flags, stream)) != 0) return rc;
  if (gn && (rc = mass_solve_launch(c, rn, DD_MENV, BD_NCOL, nullptr, xn, DD_MENV, solve_flags, stream)) != 0) return rc;
  if (eye && (rc = mass_solve_launch(c, eye, 0, BD_NCOL, nullptr, xm, DD_MENV, solve_flags, stream)) != 0) return rc;
  CsOut O;
  O.dnd[0] = dnudot_dq; O.dnd[1] = dnudot_dnu; O.dnd[2] = dnudot_dtau;
  O.dlam[0] = dlambda_dq; O.dlam[1] = dlambda_dnu; O.dlam[2] = dlambda_dtau;
  O.X[0] = xq; O.X[1] = xn; O.X[2] = eye ? xm : nullptr;
  hipLaunchKernelGGL(wbc_constraint_derivatives_solve_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, jblk, Y, (const float*)r2, active, damping,
                     nbodies, live_cols, n, (flags & WBC_DERIV_TRANSPOSED) ? 1 : 0, O);
  return c.launched();
}

// ---- whole-body inverse dynamics for task-space accelerations (include/wbc_sim.h: wbc_sim_task_inverse_dynamics) ---------------------
// Per env: the joint torques tau_j (18) that minimise the weighted task, posture, contact-force and torque terms subject to the
// equations of motion and the active stance rows. The feasible set is the image of tau_j under stance-constrained forward dynamics,
//     (nudot, lambda) = (a_0, lambda_0) + (G_a, G_lambda) tau_j ,
// so the problem is an unconstrained least-squares one in 18 unknowns. It is solved in its SQUARE-ROOT form: the sqrt(weight)-scaled
// rows [posture 24 | force 3 ns | task 6 nt | torque 18] x [18 columns | constant] are stacked (at most 90 x 19) and reduced by
// Householder reflections; the normal equations G^T H G are never formed (their condition number is the square of the stack's: the
// internal-force directions of a multi-foot stance are seen by w_force and w_torque alone). The outputs (nudot, lambda) are then
// RECOMPUTED from tau_j by the constrained-dynamics chain itself (a_free = M^-1 (S^T tau_j - h), Cholesky of the Delassus matrix), so
// the equations of motion and the stance rows hold to that chain's rounding whatever the least-squares solve did.
// Launches: h (wbc_inverse_dynamics_kernel), wbc_taskid_rhs_kernel, the mass solve with 3 ns + 1 + 18 right-hand sides
// [J_c^T | -h | S^T], wbc_taskid_solve_kernel. The root position is never read.
#define TI_NJ WBC_NJ                             // joint torques: the unknowns
#define TI_NL (6 + TI_NJ)                        // live coordinates
#define TI_MAXS (3 * WBC_TASKID_MAX_STANCE)      // 12 stance rows at most
#define TI_MAXT (6 * WBC_TASKID_MAX_TASKS)       // 36 task rows at most
#define TI_MAXRHS (TI_MAXS + 1 + TI_NJ)          // 31 right-hand sides of the mass solve at most
#define TI_NC (TI_NJ + 1)                        // columns of the stack: the unknowns and the constant
#define TI_MAXROWS (TI_NL + TI_MAXS + TI_MAXT + TI_NJ)   // 90 rows of the stack at most
#define TI_QG 3                                  // row groups of the reflections: lane = group * TI_NC + column
static_assert(TI_MAXRHS <= WBC_SOLVE_MAX_RHS && WBC_NB + WBC_TASKID_MAX_STANCE + WBC_TASKID_MAX_TASKS <= BA_LPE && TI_MAXS <= CD_GSTRIDE &&
              TI_QG * TI_NC <= 64 && WBC_TASKID_MAX_STANCE <= WBC_CONSTR_MAX_BODIES, "lanes");
struct TiConst : TreeWalk, TreeRigid, TreeCols {
  int32_t ns, nt, srb[WBC_TASKID_MAX_STANCE], trb[WBC_TASKID_MAX_TASKS];   // the listed stance and task rigid bodies
  int32_t jcol[TI_NJ];                         // column (of 26) of joint torque j
};

// The mass solve's right-hand sides [N, 3 ns + 1 + 18, 26]: the stance bodies' linear Jacobian rows (zeros where inactive), -h, the 18
// unit rows S^T; gamma [N, CD_GSTRIDE] = (Jdot nu) of the stance rows; the task bodies' Jacobian rows jt [N, 6 nt, 26] (linear, angular)
// and gt [N, TI_MAXT] = their Jdot nu. Lanes as wbc_constraint_rhs_kernel: b < 19 = moving body b, then one lane per listed body.
extern "C" __global__ void __launch_bounds__(64) wbc_taskid_rhs_kernel(TiConst C, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                      const uint8_t* __restrict__ active, const float* __restrict__ h, int n,
                                                                      float* __restrict__ rhs, float* __restrict__ gamma,
                                                                      float* __restrict__ jt, float* __restrict__ gt) {
  __shared__ float sJ[BA_EPW][WBC_NB][6];          // joint axis, joint origin, in F
  __shared__ float sX[BA_EPW][WBC_TASKID_MAX_STANCE + WBC_TASKID_MAX_TASKS][3];   // listed body's origin in F
  const int half = BA_EPW == 2 ? threadIdx.x >> 5 : 0, lane = BA_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * BA_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  const int ns = C.ns, nt = C.nt, m = 3 * ns, nr = m + 1 + TI_NJ;
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  if (lane < WBC_NB + ns + nt) {
    const bool body = lane < WBC_NB;
    const int k = body ? 0 : lane - WBC_NB, r = body ? 0 : (k < ns ? C.srb[k] : C.trb[k - ns]);
    f3 lin, ang;
    if (rhs_walk_lane(C, C, lane, k, r, e, R, root, dofs, sJ[half], sX[half], lin, ang) && live) {
      if (k < ns) st3(gamma + e * CD_GSTRIDE + 3 * k, lin);
      else { st3(gt + e * TI_MAXT + 6 * (k - ns), lin); st3(gt + e * TI_MAXT + 6 * (k - ns) + 3, ang); }
    }
  }
  __syncthreads();
  if (lane < BD_NCOL && live) {
    const int c = lane, b = c < 6 ? 0 : C.col_body[c - 6], j = c < 3 ? c : c - 3;
    const f3 ej = mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
    float* o = rhs + e * (size_t)(nr * BD_NCOL) + c;
    for (int k = 0; k < ns; ++k) {
      const bool act = active ? active[e * ns + k] != 0 : true;
      f3 lin = mk3(0.f, 0.f, 0.f);
      if (act) lin = rhs_jac_lin(C, c, b, C.rb_body[C.srb[k]], ej, R, ld3(sX[half][k]), sJ[half]);
      o[(3 * k) * BD_NCOL] = lin.x; o[(3 * k + 1) * BD_NCOL] = lin.y; o[(3 * k + 2) * BD_NCOL] = lin.z;
    }
    o[m * BD_NCOL] = b >= 0 ? 0.f - h[e * BD_NCOL + c] : 0.f;
    for (int q = 0; q < TI_NJ; ++q) o[(m + 1 + q) * BD_NCOL] = C.jcol[q] == c ? 1.f : 0.f;
    float* t = jt + e * (size_t)(6 * nt * BD_NCOL) + c;
    for (int k = 0; k < nt; ++k) {
      const f3 x = ld3(sX[half][ns + k]);
      f3 lin = mk3(0.f, 0.f, 0.f), ang = lin;
      if (c < 3) lin = ej;
      else if (c < 6) { lin = cross(ej, mat_mul(R, x)); ang = ej; }
      else if (b >= 0 && ((C.anc[C.rb_body[C.trb[k]]] >> b) & 1u)) {
        const f3 a = ld3(sJ[half][b]);
        lin = mat_mul(R, cross(a, x - ld3(sJ[half][b] + 3)));
        ang = mat_mul(R, a);
      }
      t[(6 * k) * BD_NCOL] = lin.x; t[(6 * k + 1) * BD_NCOL] = lin.y; t[(6 * k + 2) * BD_NCOL] = lin.z;
      t[(6 * k + 3) * BD_NCOL] = ang.x; t[(6 * k + 4) * BD_NCOL] = ang.y; t[(6 * k + 5) * BD_NCOL] = ang.z;
    }
  }
}

struct TsConst {
  int32_t jcol[TI_NJ];                         // column (of 26) of joint torque j
  int32_t lcol[TI_NL];                         // column of live coordinate s: the root's six, then the joints'
  float sp, sf, st, damping;                   // sqrt of the posture, force and torque weights; the Delassus damping
};

// ---- the same problem with torque limits and friction pyramids (include/wbc_sim.h: wbc_sim_task_inverse_dynamics_qp) ------------------
// Launches 1-3 are the sibling's, and wbc_taskqp_solve_kernel is the sibling's body (ts_solve below) with tq_active_set between its
// steps 4 and the recomputation of (nudot, lambda). It reads [G_lambda | lambda_0] as kept from before the force rows are scaled, and
// with R, c of the reflected stack solves
//     min 1/2 |R x + c|^2   s.t.  |x_j| <= lim_j,  a_i . (lambda_0 + G_lambda x) >= b_i  (five rows per active stance body)
// by the dual active-set method of Goldfarb and Idnani in the variable y = R x + c, where the objective is 1/2 |y|^2, the unconstrained
// optimum is y = 0 and row i reads d_i . y >= beta_i with d_i = R^-T n_i, beta_i = b_i + d_i . c. One lane per row (36 + 5 ns <= 56).
// The working set W (at most 18 independent rows) is carried as D_W = Q T, Q orthonormal [18, q] and T upper triangular, built column
// by column by twice-applied Gram-Schmidt from the ORIGINAL d_i: a column depends on the columns before it alone, so adding a row
// appends one column, dropping row l rebuilds the columns after l, and the factor never drifts (it is what a rebuild from scratch gives).
// After every accepted row the iterate and the multipliers are REBUILT from W, never accumulated:
//     v = T^-T beta_W,  y = Q v,  u = T^-1 v,  x = R^-1 (y - c).
// A candidate p that depends on W (|z|^2 <= TQ_DEP2 |d_p|^2, z = d_p - Q Q^T d_p; always so at q = 18) takes the method's dual step: no
// primal move, u -= t r, u_p += t with r = T^-1 Q^T d_p, and the blocking row leaves W; with no blocking row the rows admit no point.
// A dependent candidate whose slack as W implies it, sum_j r_j b_j - b_p, is no violation is set aside until W changes: the rounding
// of x alone made it look violated (the fourth and fifth row of a pyramid whose apex is the optimum), and swapping it in would cycle.
// Between accepted rows only the candidate's slack s_p (+= t |z|^2) and the multipliers move. Slacks are evaluated in x: lambda(x) and
// the sum of its absolute terms per stance row, then each row's value and scale; a contact row counts as violated below -TQ_TOL scale, a box row below 0.
#define TQ_NROW (2 * TI_NJ + 5 * WBC_TASKID_MAX_STANCE)    // 56 rows at most: bit = lane = row
#define TQ_C0 (2 * TI_NJ)                        // first contact row
#define TQ_PITCH (TI_NJ + 1)                     // LDS pitch of the 18-vectors (odd)
#define TQ_TOL 1.52587891e-5f                    // 256 x 2^-24 of a row's scale: an fp32 evaluation of a row at the rebuilt x is off by 100-300 x
                                                 // 2^-24 of it, and a tolerance below that level makes the five rows of a pyramid's apex cycle
#define TQ_DEP2 1e-8f                            // |z|^2 / |d_p|^2 at or below which p depends on W
#define TQ_DEFAULT_ITER 100
static_assert(TQ_NROW <= 64 && TQ_NROW * TQ_PITCH <= (TI_MAXROWS - TI_NJ) * TI_NC && WBC_TASKQP_MAX_ITER >= TQ_DEFAULT_ITER, "rows");
struct TqConst {
  TsConst s;
  float lim[TI_NJ];                              // wbc_task_cfg.torque_limits of joint torque j
  float mu, fn_min;
  int32_t max_iter;
};
struct TqArgs {                                  // the QP kernel's own arguments, handed through the shared body
  const TqConst& K;
  const float *tau_limit, *normal, *mu;
  int32_t *status_out, *iter_out;
  int64_t* set_out;
};

// Steps 5 and 6 of wbc_taskqp_solve_kernel, for env e with act its active-row mask: in, sTau the unconstrained optimum, sS the reflected
// stack (R above the diagonal, c in the last column), sDiag R's diagonal and sG [G_lambda | lambda_0]; out, sTau the constrained optimum
// (behind a barrier) and the env's status, active set and iteration count. Rows 18.. of sS are overwritten with the d_i.
__device__ __forceinline__ void tq_active_set(const TqArgs& io, size_t e, int lane, int ns, uint32_t act, float* sS, const float (*sG)[TI_NC],
                                              const float* sDiag, float* sTau) {
  __shared__ float sQ[TI_NJ][TQ_PITCH], sT[TI_NJ][TQ_PITCH];   // sQ[j]: column j of Q; sT[a][b], a <= b
  __shared__ float sBeta[64], sB[64], sKey[64], sSl[64], sSc[64];   // beta_i, b_i; the key of a search over the lanes; the rows' slacks, scales
  __shared__ float sLam[TI_MAXS], sMag[TI_MAXS];   // lambda(x) and the sum of its absolute terms
  __shared__ float sX0[TI_NJ], sU[TI_NJ + 1], sR[TI_NJ], sW[TI_NJ], sW1[TI_NJ], sZ[TI_NJ], sH[TI_NJ + 1];
  __shared__ int32_t sRow[TI_NJ + 1];              // the rows of W, in the order of Q's columns
  const TqConst& Cq = io.K;
  const float *tau_limit = io.tau_limit, *normal = io.normal, *mu = io.mu;
  const int m = 3 * ns;
  // 5) the rows: lane j < 18: x_j <= lim_j; lane 18 + j: x_j >= -lim_j; lane 36 + 5 k + t: row t of active stance body k
  float* sDm = sS + TI_NJ * TI_NC;                 // d_i = R^-T n_i at sDm[i * TQ_PITCH + 0..17]
  const int jl = lane < TI_NJ ? lane : lane - TI_NJ, rc = lane - TQ_C0, kf = rc >= 0 ? rc / 5 : 0, tf = rc - 5 * kf;
  const bool box = lane < TQ_C0, valid = box || (rc < 5 * ns && ((act >> (3 * kf)) & 1u));
  float lim = 0.f, bq = 0.f, mu0 = Cq.mu;
  asm volatile("" : "+s"(mu0));                 // the host scalar as a value: a select between its address and `mu` would be a flat load
  f3 ar = mk3(0.f, 0.f, 0.f);                      // a contact row in force space: a . lambda_k >= bq
  if (box) {
    for (int q = 0; q < TI_NJ; ++q) lim = q == jl ? Cq.lim[q] : lim;
    if (tau_limit) lim = tau_limit[e * TI_NJ + jl];
  } else if (valid) {
    f3 nn = mk3(0.f, 0.f, 1.f), t1 = mk3(1.f, 0.f, 0.f), t2 = mk3(0.f, 1.f, 0.f);
    if (normal) {
      nn = ld3(normal + (e * ns + kf) * 3);
      nn = nn * (1.f / __fsqrt_rn(dot(nn, nn)));
      t1 = cross(nn, fabsf(nn.x) > 0.9f ? mk3(0.f, 1.f, 0.f) : mk3(1.f, 0.f, 0.f));
      t1 = t1 * (1.f / __fsqrt_rn(dot(t1, t1)));
      t2 = cross(nn, t1);
    }
    float mk = mu0;
    if (mu) mk = mu[e * ns + kf];
    const f3 tg = tf < 3 ? t1 : t2;
    ar = tf == 0 ? nn : ((tf & 1) ? mk * nn - tg : mk * nn + tg);
    bq = tf == 0 ? Cq.fn_min : 0.f;
  }
  for (int j = lane; j < TI_NJ; j += 64) sX0[j] = sTau[j];
  // lambda(x) = lambda_0 + G_lambda x with the sum of its absolute terms, then every row's slack and its key: the violation in units
  // of |d_i| (the distance in y) where it exceeds TQ_TOL of the row's scale and the row is not in W, else 0
  uint64_t inW = 0, skip = 0;                      // rows in W; rows that W implies (set aside until W changes)
  float inv_d = 1.f;                               // 1 / |d_i| once the d_i exist
  auto slacks = [&]() {
    __syncthreads();
    if (lane < m) {
      float l = sG[lane][TI_NJ], g = fabsf(l);
      for (int j = 0; j < TI_NJ; ++j) { const float t = sG[lane][j] * sTau[j]; l += t; g += fabsf(t); }
      sLam[lane] = l; sMag[lane] = g;
    }
    __syncthreads();
    float s = 0.f, sc = 0.f;
    if (box) { const float x = sTau[jl]; s = lane < TI_NJ ? lim - x : lim + x; sc = lim + fabsf(x); }
    else if (valid) {
      s = ((ar.x * sLam[3 * kf] + ar.y * sLam[3 * kf + 1]) + ar.z * sLam[3 * kf + 2]) - bq;
      sc = ((fabsf(ar.x) * sMag[3 * kf] + fabsf(ar.y) * sMag[3 * kf + 1]) + fabsf(ar.z) * sMag[3 * kf + 2]) + fabsf(bq);
    }
    // a box row has no tolerance (lim -+ x is exact in sign): with no row violated every torque is inside its limit exactly
    const bool viol = valid && !(((inW | skip) >> lane) & 1ull) && s < (box ? 0.f : 0.f - TQ_TOL * sc);
    sSl[lane] = s; sSc[lane] = sc;
    sKey[lane] = viol ? (0.f - s) * inv_d : 0.f;
    __syncthreads();
  };
  slacks();
  const bool any = __any(sKey[lane] > 0.f) != 0;   // no row violated at the unconstrained optimum: the solve ends here with the sibling's result
  int status = 0, iters = 0;
  if (any) {
    // d_i = R^-T n_i (R^T is lower triangular: forward substitution, one lane per row) and beta_i = b_i + d_i . c
    if (valid) {
      float* d = sDm + lane * TQ_PITCH;
      float dc = 0.f, dd = 0.f;
      for (int k = 0; k < TI_NJ; ++k) {
        float s;
        if (box) s = k == jl ? (lane < TI_NJ ? -1.f : 1.f) : 0.f;
        else s = (ar.x * sG[3 * kf][k] + ar.y * sG[3 * kf + 1][k]) + ar.z * sG[3 * kf + 2][k];
        for (int j = 0; j < k; ++j) s -= sS[j * TI_NC + k] * d[j];
        s = s / sDiag[k];
        d[k] = s;
        dc += s * sS[k * TI_NC + TI_NJ];
        dd += s * s;
      }
      const float b = box ? 0.f - lim : bq - ((ar.x * sG[3 * kf][TI_NJ] + ar.y * sG[3 * kf + 1][TI_NJ]) + ar.z * sG[3 * kf + 2][TI_NJ]);
      sBeta[lane] = b + dc; sB[lane] = b;
      inv_d = 1.f / __fsqrt_rn(dd);
    }
    int q = 0, p = -1;                             // |W|; the candidate row
    float sp = 0.f;                                // the candidate's slack; its multiplier is rebuilt with W's when it joins
    const int max_iter = Cq.max_iter;
    // Gram-Schmidt, twice, of d_row against the first nq columns of Q: sW = Q^T d, sZ = the rest; returns |z|^2 and |d|^2
    auto orth = [&](int row, int nq, float& dd) -> float {
      const float* d = sDm + row * TQ_PITCH;
      __syncthreads();
      if (lane < nq) { float a = 0.f; for (int i = 0; i < TI_NJ; ++i) a += sQ[lane][i] * d[i]; sW1[lane] = a; }
      __syncthreads();
      if (lane < TI_NJ) {
        float z = d[lane];
        for (int j = 0; j < TI_NJ; ++j) { if (j >= nq) break; z -= sW1[j] * sQ[j][lane]; }
        sZ[lane] = z;
      }
      __syncthreads();
      if (lane < nq) { float a = 0.f; for (int i = 0; i < TI_NJ; ++i) a += sQ[lane][i] * sZ[i]; sW[lane] = a; }
      __syncthreads();
      float z = 0.f;
      if (lane < TI_NJ) {
        z = sZ[lane];
        for (int j = 0; j < TI_NJ; ++j) { if (j >= nq) break; z -= sW[j] * sQ[j][lane]; }
      }
      __syncthreads();
      if (lane < TI_NJ) sZ[lane] = z;
      if (lane < nq) sW[lane] += sW1[lane];
      __syncthreads();
      float zz = 0.f;
      dd = 0.f;
      for (int i = 0; i < TI_NJ; ++i) { zz += sZ[i] * sZ[i]; dd += d[i] * d[i]; }
      return zz;
    };
    // column nq of Q and T from orth's result
    auto append = [&](int row, int nq, float zz) {
      const float rho = __fsqrt_rn(zz);
      if (lane < TI_NJ) sQ[nq][lane] = sZ[lane] / rho;
      if (lane < nq) sT[lane][nq] = sW[lane];
      if (lane == 0) { sT[nq][nq] = rho; sRow[nq] = row; }
    };
    for (int it = 0; it <= WBC_TASKQP_MAX_ITER; ++it) {
      if (p < 0) {
        slacks();
        float best = 0.f;
        for (int i = 0; i < TQ_NROW; ++i) { const float k = sKey[i]; if (k > best) { best = k; p = i; } }
        if (p < 0) break;                          // optimal
        sp = sSl[p];
      }
      if (it >= max_iter) { status = 1; break; }
      iters = it + 1;
      float dd;
      const float zz = orth(p, q, dd);
      const bool dep = q >= TI_NJ || !(zz > TQ_DEP2 * dd);
      // r = T^-1 Q^T d_p, then the blocking row: the smallest u_j / r_j over r_j > 0
      {
        float s = lane < q ? sW[lane] : 0.f;
        for (int b = TI_NJ - 1; b >= 0; --b) {
          if (b >= q) continue;
          if (lane == b) sH[b] = s / sT[b][b];
          __syncthreads();
          if (lane < b) s -= sT[lane][b] * sH[b];
        }
        if (lane < q) sR[lane] = sH[lane];
        __syncthreads();
      }
      float t1 = 3.402823466e38f;
      int l = -1;
      for (int j = 0; j < TI_NJ; ++j) {
        if (j >= q) break;
        const float r = sR[j];
        if (r > 0.f) { const float t = fmaxf(sU[j], 0.f) / r; if (t < t1) { t1 = t; l = j; } }
      }
      if (dep && q > 0) {
        // n_p = sum_j r_j n_j, so with W's rows tight the slack of p is sum_j r_j b_j - b_p whatever x is: the rounding of x says
        // nothing about it. Where that is no violation (the fourth and fifth row at a pyramid's apex) p is set aside, not swapped in
        float si = 0.f, sa = 0.f;
        for (int j = 0; j < TI_NJ; ++j) { if (j >= q) break; const float t = sR[j] * sB[sRow[j]]; si += t; sa += fabsf(t); }
        if (si - sB[p] >= 0.f - TQ_TOL * ((sa + fabsf(sB[p])) + sSc[p])) { skip |= 1ull << p; p = -1; continue; }
      }
      if (!dep && !(l >= 0 && t1 * zz < 0.f - sp)) {
        // the full step: p joins W; x, y and u are rebuilt from W
        append(p, q, zz);
        inW |= 1ull << p; skip = 0;
        ++q; p = -1;
        __syncthreads();
        float s = lane < q ? sBeta[sRow[lane]] : 0.f;                     // v = T^-T beta_W
        for (int a = 0; a < TI_NJ; ++a) {
          if (a >= q) break;
          if (lane == a) sH[a] = s / sT[a][a];
          __syncthreads();
          if (lane > a && lane < q) s -= sT[a][lane] * sH[a];
        }
        float yv = 0.f;
        if (lane < TI_NJ) {                                               // y = Q v, then s = y - c
          for (int j = 0; j < TI_NJ; ++j) { if (j >= q) break; yv += sQ[j][lane] * sH[j]; }
          yv -= sS[lane * TI_NC + TI_NJ];
        }
        s = lane < q ? sH[lane] : 0.f;                                    // u = T^-1 v
        __syncthreads();
        for (int b = TI_NJ - 1; b >= 0; --b) {
          if (b >= q) continue;
          if (lane == b) sU[b] = s / sT[b][b];
          __syncthreads();
          if (lane < b) s -= sT[lane][b] * sU[b];
        }
        for (int j = TI_NJ - 1; j >= 0; --j) {                            // x = R^-1 (y - c)
          if (lane == j) sTau[j] = yv / sDiag[j];
          __syncthreads();
          if (lane < j) yv -= sS[lane * TI_NC + j] * sTau[j];
        }
        continue;
      }
      if (l < 0) { status = 2; break; }            // p depends on W and nothing blocks: the rows admit no point
      // the partial step: the multipliers move by t1, row l leaves W, the columns after l are rebuilt
      if (!dep) sp += t1 * zz;
      __syncthreads();
      float un = 0.f;
      int rn = 0;
      if (lane < q) { un = sU[lane] - t1 * sR[lane]; if (lane >= l && lane + 1 < q) { un = sU[lane + 1] - t1 * sR[lane + 1]; rn = sRow[lane + 1]; } }
      inW &= ~(1ull << sRow[l]); skip = 0;
      __syncthreads();
      if (lane < q - 1) { sU[lane] = un; if (lane >= l) sRow[lane] = rn; }
      --q;
      __syncthreads();
      for (int j = 0; j < TI_NJ; ++j) {
        if (j < l) continue;
        if (j >= q) break;
        float d2;
        const int row = sRow[j];
        const float z2 = orth(row, j, d2);
        append(row, j, fmaxf(z2, 1e-30f * d2));
      }
      __syncthreads();
    }
  }

  // 6) tau_j: a joint whose limit row is in W sits on the limit exactly; every joint inside the box. Status 1, 2: the unconstrained
  //    optimum clamped to the box
  __syncthreads();
  if (lane < TI_NJ) {
    const float lj = lim;                          // lane j < 18 is joint j's upper row
    float x = status == 0 ? sTau[lane] : sX0[lane];
    if (status == 0 && ((inW >> lane) & 1ull)) x = lj;
    if (status == 0 && ((inW >> (lane + TI_NJ)) & 1ull)) x = 0.f - lj;
    if (any) x = fminf(fmaxf(x, 0.f - lj), lj);    // !any: no box row is violated, by any amount, at the unconstrained optimum
    sTau[lane] = x;
  }
  if (lane == 0) {
    if (io.status_out) io.status_out[e] = status;
    if (io.set_out) io.set_out[e] = status == 0 ? (int64_t)inW : 0;
    if (io.iter_out) io.iter_out[e] = iters;
  }
  __syncthreads();
}

// One env per 64-lane workgroup. With m = 3 ns, Y = (M^-1 [J_c^T | -h | S^T])^T the mass solve's output and S the stack in LDS:
//  1) A = J_c Y_c^T + damping I (lower triangle, identity where inactive) and, in the stack's force rows, [-J_c Y_s^T | a_stance - gamma
//     - J_c y_h]; Cholesky of A; lane j = column j solves its column in place: [G_lambda | lambda_0] (the pieces of wbc_delassus.h);
//  2) posture rows [G_a | a_0] = [Y_s^T | y_h] + Y_c^T [G_lambda | lambda_0] on the live coordinates; task rows sqrt(w) (J_t [G_a | a_0] +
//     (0 | Jdot nu - acc)), zero where w = 0 (acc is not read there); then the posture rows lose nudot_ref and take sqrt(w_posture),
//     the force rows sqrt(w_force), and the torque rows are sqrt(w_torque) I: w_torque > 0 gives the stack full column rank;
//  3) 18 Householder reflections, lane = group * 19 + column: three groups share the rows of a column's dot product with the pivot
//     column (rows k + group, step 3: 57 consecutive LDS words per read), partial sums meet in LDS. The pivot column is left as it
//     is (its reflected value alpha goes to sDiag), so no lane writes what another reads;
//  4) R tau_j = -(Q^T b) by back-substitution;
//  5, 6) with QP, tq_active_set between the two: it moves tau_j inside the limits and the friction pyramids;
//  then a_free = y_h + Y_s^T tau_j, c = a_stance - gamma - J_c a_free, L L^T lambda = c and nudot = a_free + Y_c^T lambda.
// The body of both solve kernels: one text, so where no inequality binds the QP kernel's outputs are its sibling's bit for bit. A
// single-wavefront workgroup: the __syncthreads() order the LDS traffic and cost no barrier instruction.
template <bool QP>
__device__ __forceinline__ void ts_solve(const TsConst& C, const float* __restrict__ rhs, const float* __restrict__ Y,
                                         const float* __restrict__ gamma, const float* __restrict__ jt, const float* __restrict__ gt,
                                         const uint8_t* __restrict__ active, const float* __restrict__ stance_acc,
                                         const float* __restrict__ task_acc, const float* __restrict__ task_weight,
                                         const float* __restrict__ nudot_ref, int ns, int nt, int n, float* __restrict__ tau,
                                         float* __restrict__ nudot, float* __restrict__ lambda, const TqArgs* io) {
  __shared__ float sY[TI_MAXRHS][CD_LD], sJc[TI_MAXS][CD_LD], sJt[TI_MAXT][CD_LD];
  __shared__ float sS[TI_MAXROWS * TI_NC];         // the stack, row-major, pitch 19
  __shared__ float sA[TI_MAXS][TI_MAXS + 1];       // lower triangle: A, then L
  __shared__ float sD[TI_MAXS + 1], sV[TI_MAXS + 1];   // 1 / L_jj; the value handed round
  __shared__ float sP[TI_QG][TI_NC], sDiag[TI_NJ], sTau[TI_NJ], sAf[BD_NCOL];
  __shared__ float sG[QP ? TI_MAXS : 1][TI_NC];    // QP: [G_lambda | lambda_0], unscaled
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= n) return;
  const size_t e = blockIdx.x;
  const int m = 3 * ns, mt = 6 * nt, nr = m + 1 + TI_NJ;
  const int F0 = TI_NL, T0 = F0 + m, Q0 = T0 + mt, nrow = Q0 + TI_NJ;
  const float *rp = rhs + e * (size_t)(nr * BD_NCOL), *yp = Y + e * (size_t)(nr * BD_NCOL), *jp = jt + e * (size_t)(mt * BD_NCOL);
  for (int t = lane; t < nr * BD_NCOL; t += 64) {
    const int r = t / BD_NCOL, c = t - r * BD_NCOL;
    sY[r][c] = yp[t];
    if (r < m) sJc[r][c] = rp[t];
  }
  for (int t = lane; t < mt * BD_NCOL; t += 64) {
    const int r = t / BD_NCOL, c = t - r * BD_NCOL;
    sJt[r][c] = jp[t];
  }
  uint32_t act = 0;                                // bit i: row i belongs to an active stance body
  for (int k = 0; k < ns; ++k)
    if (!active || active[e * ns + k]) act |= 7u << (3 * k);
  __syncthreads();

  // 1) the Delassus matrix and the 19 right-hand sides of its factor
  delassus_fill(sJc, sY, sA, m, act, C.damping, lane, 64);
  for (int t = lane; t < m * TI_NC; t += 64) {
    const int i = t / TI_NC, j = t - i * TI_NC;
    float v = 0.f;
    if ((act >> i) & 1u) {
      const float* y = sY[j < TI_NJ ? m + 1 + j : m];
      float a = 0.f;
      for (int c = 0; c < BD_NCOL; ++c) a += sJc[i][c] * y[c];
      v = j < TI_NJ ? 0.f - a : ((stance_acc ? stance_acc[e * m + i] : 0.f) - gamma[e * CD_GSTRIDE + i]) - a;
    }
    sS[(F0 + i) * TI_NC + j] = v;
  }
  delassus_cholesky(sA, sD, m, lane);
  __syncthreads();
  if (lane < TI_NC) delassus_column_solve(sA, sD, sS + F0 * TI_NC + lane, TI_NC, m);   // column `lane`, in place
  __syncthreads();
  if constexpr (QP)                                // [G_lambda | lambda_0] from before the force rows are scaled
    for (int t = lane; t < m * TI_NC; t += 64) sG[t / TI_NC][t % TI_NC] = sS[F0 * TI_NC + t];

  // 2) the stack
  for (int t = lane; t < TI_NL * TI_NC; t += 64) {
    const int s = t / TI_NC, j = t - s * TI_NC, c = C.lcol[s];
    float a = sY[j < TI_NJ ? m + 1 + j : m][c];
    for (int k = 0; k < m; ++k) a += sY[k][c] * sS[(F0 + k) * TI_NC + j];
    sS[t] = a;
  }
  __syncthreads();
  for (int t = lane; t < mt * TI_NC; t += 64) {
    const int r = t / TI_NC, j = t - r * TI_NC;
    const float w = task_weight ? task_weight[e * mt + r] : 1.f;
    float v = 0.f;
    if (w > 0.f) {
      float a = 0.f;
      for (int s = 0; s < TI_NL; ++s) a += sJt[r][C.lcol[s]] * sS[s * TI_NC + j];
      if (j == TI_NJ) a += gt[e * TI_MAXT + r] - task_acc[e * mt + r];
      v = __fsqrt_rn(w) * a;
    }
    sS[(T0 + r) * TI_NC + j] = v;
  }
  __syncthreads();
  for (int t = lane; t < TI_NL * TI_NC; t += 64) {
    const int s = t / TI_NC, j = t - s * TI_NC;
    const float ref = (j == TI_NJ && nudot_ref) ? nudot_ref[e * BD_NCOL + C.lcol[s]] : 0.f;
    sS[t] = C.sp * (sS[t] - ref);
  }
  for (int t = lane; t < m * TI_NC; t += 64) sS[F0 * TI_NC + t] *= C.sf;
  for (int t = lane; t < TI_NJ * TI_NC; t += 64) {
    const int i = t / TI_NC, j = t - i * TI_NC;
    sS[Q0 * TI_NC + t] = i == j ? C.st : 0.f;
  }
  __syncthreads();

  // 3) Householder reflections
  {
    const int g = lane / TI_NC, j = lane - g * TI_NC;
    const bool mine = g < TI_QG;
    // The two row loops of a reflection are 60 and 96 bytes of code with a taken branch per round, in a workgroup of one wavefront:
    // their time depends on where they start in the 32-byte instruction-fetch windows (PERF_LOG.md: 204 to 216 us for the same
    // instructions of wbc_taskid_solve_kernel, 444 to 464 for the QP call). Pinned from here, so that the steps above can change
    // without moving them: the first loop starts 16 bytes into a window, where it stood when the reflections were written.
    asm volatile(".p2align 5\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0");
    for (int k = 0; k < TI_NJ; ++k) {
      if (mine) {
        float part = 0.f;
        if (j >= k)
          for (int r = k + g; r < nrow; r += TI_QG) part += sS[r * TI_NC + k] * sS[r * TI_NC + j];
        sP[g][j] = part;
      }
      __syncthreads();
      const float skk = (sP[0][k] + sP[1][k]) + sP[2][k], akk = sS[k * TI_NC + k];
      const float nrm = __fsqrt_rn(skk), alpha = akk >= 0.f ? 0.f - nrm : nrm, vk = akk - alpha;
      float tj = 0.f;                              // 2 (v . a_j) / (v . v), v = a_k - alpha e_k: v . v = -2 alpha v_k
      if (mine && j > k) tj = (((sP[0][j] + sP[1][j]) + sP[2][j]) - alpha * sS[k * TI_NC + j]) * (-1.f / (alpha * vk));
      __syncthreads();
      if (mine && j > k)
        for (int r = k + g; r < nrow; r += TI_QG) sS[r * TI_NC + j] -= tj * (r == k ? vk : sS[r * TI_NC + k]);
      if (lane == k) sDiag[k] = alpha;
      __syncthreads();
    }
  }

  // 4) the unconstrained optimum tau_j: R x = -(Q^T b)
#pragma unroll                                     // all 18 steps written out, as the compiler chose while this stood in the kernels
  for (int k = TI_NJ - 1; k >= 0; --k) {
    float x = 0.f - sS[k * TI_NC + TI_NJ];
#pragma unroll
    for (int j = k + 1; j < TI_NJ; ++j) x -= sS[k * TI_NC + j] * sTau[j];
    if (lane == 0) sTau[k] = x / sDiag[k];
    __syncthreads();
  }
  if constexpr (QP) tq_active_set(*io, e, lane, ns, act, sS, sG, sDiag, sTau);

  // (nudot, lambda) of constrained forward dynamics with tau_j
  int jq = -1;                                     // lane c < 26: the joint torque that drives column c
  for (int q = 0; q < TI_NJ; ++q) jq = C.jcol[q] == lane ? q : jq;
  if (lane < BD_NCOL) {
    float a = sY[m][lane];
    for (int q = 0; q < TI_NJ; ++q) a += sY[m + 1 + q][lane] * sTau[q];
    sAf[lane] = a;
  }
  __syncthreads();
  const int i = lane;
  const bool row = i < m, on = row && ((act >> i) & 1u);
  float ci = 0.f;
  if (on) {
    float a = 0.f;
    for (int c = 0; c < BD_NCOL; ++c) a += sJc[i][c] * sAf[c];
    ci = ((stance_acc ? stance_acc[e * m + i] : 0.f) - gamma[e * CD_GSTRIDE + i]) - a;
  }
  delassus_lane_solve(sA, sD, sV, m, i, ci);
  if (lambda && row) lambda[e * m + i] = on ? sV[i] : 0.f;
  if (lane < BD_NCOL) {
    tau[e * BD_NCOL + lane] = jq >= 0 ? sTau[jq] : 0.f;
    if (nudot) {
      float a = sAf[lane];
      for (int k = 0; k < m; ++k) a += sY[k][lane] * sV[k];
      nudot[e * BD_NCOL + lane] = (lane < 6 || jq >= 0) ? a : 0.f;
    }
  }
}


extern "C" __global__ void __launch_bounds__(64) wbc_taskid_solve_kernel(TsConst C, const float* __restrict__ rhs, const float* __restrict__ Y,
                                                                        const float* __restrict__ gamma, const float* __restrict__ jt,
                                                                        const float* __restrict__ gt, const uint8_t* __restrict__ active,
                                                                        const float* __restrict__ stance_acc, const float* __restrict__ task_acc,
                                                                        const float* __restrict__ task_weight, const float* __restrict__ nudot_ref,
                                                                        int ns, int nt, int n, float* __restrict__ tau, float* __restrict__ nudot,
                                                                        float* __restrict__ lambda) {
  ts_solve<false>(C, rhs, Y, gamma, jt, gt, active, stance_acc, task_acc, task_weight, nudot_ref, ns, nt, n, tau, nudot, lambda, nullptr);
}

extern "C" __global__ void __launch_bounds__(64) wbc_taskqp_solve_kernel(TqConst Cq, const float* __restrict__ rhs, const float* __restrict__ Y,
                                                                        const float* __restrict__ gamma, const float* __restrict__ jt,
                                                                        const float* __restrict__ gt, const uint8_t* __restrict__ active,
                                                                        const float* __restrict__ stance_acc, const float* __restrict__ task_acc,
                                                                        const float* __restrict__ task_weight, const float* __restrict__ nudot_ref,
                                                                        const float* __restrict__ tau_limit, const float* __restrict__ normal,
                                                                        const float* __restrict__ mu, int ns, int nt, int n,
                                                                        float* __restrict__ tau, float* __restrict__ nudot, float* __restrict__ lambda,
                                                                        int32_t* __restrict__ status_out, int64_t* __restrict__ set_out,
                                                                        int32_t* __restrict__ iter_out) {
  const TqArgs io = {Cq, tau_limit, normal, mu, status_out, iter_out, set_out};
  ts_solve<true>(Cq.s, rhs, Y, gamma, jt, gt, active, stance_acc, task_acc, task_weight, nudot_ref, ns, nt, n, tau, nudot, lambda, &io);
}

// Workspace layout (floats): the right-hand-side block [N, 3 ns + 19, 26], the mass solve's output of the same shape, gamma [N, 16],
// the task rows' Jacobian [N, 6 nt, 26] and their Jdot nu [N, 36].
extern "C" size_t wbc_sim_task_inverse_dynamics_workspace_floats(int num_envs, int nstance, int ntasks) {
  if (num_envs <= 0 || nstance < 0 || nstance > WBC_TASKID_MAX_STANCE || ntasks < 0 || ntasks > WBC_TASKID_MAX_TASKS) return 0;
  return (size_t)num_envs * (2 * (size_t)(3 * nstance + 1 + TI_NJ) * BD_NCOL + CD_GSTRIDE + (size_t)6 * ntasks * BD_NCOL + TI_MAXT);
}

// What wbc_sim_task_inverse_dynamics_qp takes beyond its sibling.
struct TaskQpArgs {
  const wbc_taskqp_limits* limits;
  const float *tau_limit, *normal, *mu;
  int32_t* status;
  int64_t* active_set;
  int32_t* iterations;
};

// The four launches of both entry points on `stream`; qp NULL: the sibling without inequalities.
static int taskid_launch(const char* who, wbc_sim* s, const int32_t* stance_bodies, int nstance, const uint8_t* active, const float* stance_acc,
                         const int32_t* task_bodies, int ntasks, const float* task_acc, const float* task_weight, const float* nudot_ref,
                         const wbc_taskid_weights* weights, int flags, float* tau, float* nudot, float* lambda, float* workspace, void* stream,
                         const TaskQpArgs* qp) {
  WbCall c(who, s, stream);
  auto fin_ge0 = [](float x) { return x >= 0.f && x <= 3.402823466e38f; };   // finite: up to FLT_MAX
  // the new entry point's own arguments first: they need no sim, so a binding can be checked without a device
  if (qp) {
    const wbc_taskqp_limits* limits = qp->limits;
    if (!limits) return c.fail(-1, "limits is NULL");
    if (!(limits->mu > 0.f) || !fin_ge0(limits->mu)) return c.fail(-1, "limits.mu must be finite and > 0");
    if (!fin_ge0(fabsf(limits->fn_min))) return c.fail(-1, "limits.fn_min must be finite");
    if (limits->max_iter < 0 || limits->max_iter > WBC_TASKQP_MAX_ITER) return c.fail(-1, "limits.max_iter must be 0 (the default) or 1..WBC_TASKQP_MAX_ITER");
    if ((((uintptr_t)qp->tau_limit | (uintptr_t)qp->normal | (uintptr_t)qp->mu | (uintptr_t)qp->status | (uintptr_t)qp->iterations) & 3u) ||
        ((uintptr_t)qp->active_set & 7u))
      return c.fail(-1, "tau_limit / normal / mu / status / iterations must be 4-byte aligned and active_set 8-byte aligned");
  }
  if (!s) return c.no_sim();
  if (!tau || !workspace || !weights) return c.fail(-1, "tau / workspace / weights is NULL");
  if (nstance < 0 || nstance > WBC_TASKID_MAX_STANCE) return c.fail(-1, "nstance must be 0..WBC_TASKID_MAX_STANCE");
  if (ntasks < 0 || ntasks > WBC_TASKID_MAX_TASKS) return c.fail(-1, "ntasks must be 0..WBC_TASKID_MAX_TASKS");
  if ((nstance > 0 && !stance_bodies) || (ntasks > 0 && (!task_bodies || !task_acc)))
    return c.fail(-1, "stance_bodies / task_bodies / task_acc is NULL with a count above 0");
  if (!(weights->torque > 0.f) || !fin_ge0(weights->torque)) return c.fail(-1, "weights.torque must be finite and > 0");
  if (!fin_ge0(weights->posture) || !fin_ge0(weights->force) || !fin_ge0(weights->damping))
    return c.fail(-1, "weights.posture / force / damping must be finite and >= 0");
  if (flags & ~WBC_SOLVE_ARMATURE) return c.fail(-1, "unknown flag bits");
  if (((uintptr_t)stance_acc | (uintptr_t)task_acc | (uintptr_t)task_weight | (uintptr_t)nudot_ref | (uintptr_t)tau | (uintptr_t)nudot | (uintptr_t)lambda |
       (uintptr_t)workspace) & 3u)
    return c.fail(-1, "stance_acc / task_acc / task_weight / nudot_ref / tau / nudot / lambda / workspace must be 4-byte aligned");
  if (!c.have) return c.no_state();
  for (int k = 0; k < nstance; ++k)
    if (stance_bodies[k] < 0 || stance_bodies[k] >= WBC_NRB) return c.fail(-1, "rigid-body index outside 0..WBC_NRB-1");
  for (int k = 0; k < ntasks; ++k)
    if (task_bodies[k] < 0 || task_bodies[k] >= WBC_NRB) return c.fail(-1, "rigid-body index outside 0..WBC_NRB-1");
  TiConst C;
  if (ba_const_fill(c.hc->model, C, C) != 0) return c.no_tree();
  for (int k = 0; k < nstance; ++k)
    for (int l = 0; l < k; ++l)
      if (C.rb_body[stance_bodies[k]] == C.rb_body[stance_bodies[l]])
        return c.fail(-1, "two stance bodies ride on the same moving body (dependent rows)");
  for (int k = 0; k < ntasks; ++k)
    for (int l = 0; l < k; ++l)
      if (C.rb_body[task_bodies[k]] == C.rb_body[task_bodies[l]])
        return c.fail(-1, "two task bodies ride on the same moving body (dependent rows)");
  tree_cols_fill(c.hc->model, C);
  TqConst Q;
  TsConst& T = Q.s;
  int nj = 0;
  for (int d = 0; d < WBC_NDOF; ++d)
    if (C.col_body[d] >= 0) { if (nj < TI_NJ) C.jcol[nj] = 6 + d; ++nj; }
  if (nj != TI_NJ) return c.no_tree();
  const int n = c.n;
  if (n <= 0) return 0;
  C.ns = nstance; C.nt = ntasks;
  for (int k = 0; k < WBC_TASKID_MAX_STANCE; ++k) C.srb[k] = nstance > 0 ? stance_bodies[k < nstance ? k : 0] : 0;
  for (int k = 0; k < WBC_TASKID_MAX_TASKS; ++k) C.trb[k] = ntasks > 0 ? task_bodies[k < ntasks ? k : 0] : 0;
  for (int q = 0; q < TI_NJ; ++q) { T.jcol[q] = C.jcol[q]; T.lcol[6 + q] = C.jcol[q]; }
  for (int q = 0; q < 6; ++q) T.lcol[q] = q;
  T.sp = sqrtf(weights->posture); T.sf = sqrtf(weights->force); T.st = sqrtf(weights->torque); T.damping = weights->damping;
  float* h = nullptr;
  if (wbc_sim_internal_fd_scratch(s, &h) != 0) return -1;
  const int nr = 3 * nstance + 1 + TI_NJ;
  float *blk = workspace, *Y = blk + (size_t)n * nr * BD_NCOL, *gamma = Y + (size_t)n * nr * BD_NCOL, *jt = gamma + (size_t)n * CD_GSTRIDE,
        *gt = jt + (size_t)n * 6 * ntasks * BD_NCOL;
  int rc = wbc_sim_inverse_dynamics(s, nullptr, h, nullptr, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(wbc_taskid_rhs_kernel, dim3((n + BA_EPW - 1) / BA_EPW), dim3(64), 0, (hipStream_t)stream, C, c.root, c.dofs, active, (const float*)h,
                     n, blk, gamma, jt, gt);
  if ((rc = c.launched()) != 0) return rc;
  rc = mass_solve_launch(c, blk, (int64_t)nr * BD_NCOL, nr, nullptr, Y, (int64_t)nr * BD_NCOL, flags, stream);
  if (rc != 0) return rc;
  if (!qp) {
    hipLaunchKernelGGL(wbc_taskid_solve_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, T, (const float*)blk, (const float*)Y, (const float*)gamma,
                       (const float*)jt, (const float*)gt, active, stance_acc, task_acc, task_weight, nudot_ref, nstance, ntasks, n, tau, nudot, lambda);
    return c.launched();
  }
  for (int q = 0; q < TI_NJ; ++q) Q.lim[q] = c.hc->cfg.torque_limits[C.jcol[q] - 6];
  Q.mu = qp->limits->mu; Q.fn_min = qp->limits->fn_min; Q.max_iter = qp->limits->max_iter > 0 ? qp->limits->max_iter : TQ_DEFAULT_ITER;
  hipLaunchKernelGGL(wbc_taskqp_solve_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, Q, (const float*)blk, (const float*)Y, (const float*)gamma,
                     (const float*)jt, (const float*)gt, active, stance_acc, task_acc, task_weight, nudot_ref, qp->tau_limit, qp->normal, qp->mu, nstance,
                     ntasks, n, tau, nudot, lambda, qp->status, qp->active_set, qp->iterations);
  return c.launched();
}

// Four launches on `stream`. Arguments and conventions: include/wbc_sim.h.
extern "C" int wbc_sim_task_inverse_dynamics(wbc_sim* s, const int32_t* stance_bodies, int nstance, const uint8_t* active, const float* stance_acc,
                                             const int32_t* task_bodies, int ntasks, const float* task_acc, const float* task_weight,
                                             const float* nudot_ref, const wbc_taskid_weights* weights, int flags, float* tau, float* nudot,
                                             float* lambda, float* workspace, void* stream) {
  return taskid_launch("wbc_sim_task_inverse_dynamics", s, stance_bodies, nstance, active, stance_acc, task_bodies, ntasks, task_acc, task_weight,
                       nudot_ref, weights, flags, tau, nudot, lambda, workspace, stream, nullptr);
}

// The sibling's workspace: the solve kernel keeps everything else in LDS.
extern "C" size_t wbc_sim_task_inverse_dynamics_qp_workspace_floats(int num_envs, int nstance, int ntasks) {
  return wbc_sim_task_inverse_dynamics_workspace_floats(num_envs, nstance, ntasks);
}

// Four launches on `stream`, the last one wbc_taskqp_solve_kernel. Arguments and conventions: include/wbc_sim.h.
extern "C" int wbc_sim_task_inverse_dynamics_qp(wbc_sim* s, const int32_t* stance_bodies, int nstance, const uint8_t* active, const float* stance_acc,
                                                const int32_t* task_bodies, int ntasks, const float* task_acc, const float* task_weight,
                                                const float* nudot_ref, const wbc_taskid_weights* weights, const wbc_taskqp_limits* limits,
                                                const float* tau_limit, const float* normal, const float* mu, int flags, float* tau, float* nudot,
                                                float* lambda, int32_t* status, int64_t* active_set, int32_t* iterations, float* workspace,
                                                void* stream) {
  const TaskQpArgs qp = {limits, tau_limit, normal, mu, status, active_set, iterations};
  return taskid_launch("wbc_sim_task_inverse_dynamics_qp", s, stance_bodies, nstance, active, stance_acc, task_bodies, ntasks, task_acc,
                       task_weight, nudot_ref, weights, flags, tau, nudot, lambda, workspace, stream, &qp);
}

// ---- whole-body inverse kinematics with joint limits (include/wbc_sim.h: wbc_sim_inverse_kinematics) -----------------------------------
// Projected Levenberg-Marquardt over the 24 live coordinates, one launch, everything between the loads and the stores in LDS and registers.
// IK_EPW envs per 64-lane workgroup, one per lane group; the state is (root position RELATIVE to the start's, root quaternion, q[20]):
//  evaluate   lane b < 19 = moving body b walks root -> b in WORLD axes (tree_frame_step) and leaves its joint axis and origin in LDS;
//             lane 19 + k walks to target k's body with the body's quaternion carried along, leaves the target's origin, its six residuals
//             (target - x; phi = log(R_target R^T) from the error quaternion) and its share of the cost; lane j < 18 adds the posture
//             share; a butterfly sum gives every lane of the group the same bits.
//  accept     trip 0 takes the start; later trips take the candidate if the cost did not rise (lambda /= 8), else lambda *= 8.
//  linearise  lane c = coordinate c fills column c of the listed bodies' Jacobian rows (pitch 25) and forms g_c; the lower triangle of
//             H = J^T W J + posture S^T S, one entry per lane and round. Kept only when the point was accepted.
//  solve      A = H + lambda diag H + floor, the identity's row and column for a joint that sits at a limit with the gradient pushing
//             outward; delassus_cholesky / delassus_lane_solve (m = 24). Where a free joint's step would leave its limits, a second
//             solve with that joint's step held at the distance to the limit; lane c retracts and clamps coordinate c into the candidate.
// Every loop has a compile-time bound and every barrier is reached by all 64 lanes: what ends the loop is one value per lane group in
// LDS, read back behind a barrier, and a group that is done keeps taking the trips (its stores predicated off) until both are.
#ifndef IK_EPW
#define IK_EPW 2                                // envs per workgroup: 2, or 1 (-DIK_EPW=1, the variant DESIGN.md compares with)
#endif
static_assert(IK_EPW == 1 || IK_EPW == 2, "one env per 64 lanes or one per 32-lane half");
#define IK_LPE (64 / IK_EPW)                    // lanes per env
#define IK_M (6 + WBC_NJ)                       // 24 live coordinates
#define IK_ROWS (6 * WBC_IK_MAX_TARGETS)        // 36 residual rows at most
#define IK_LD (IK_M + 1)                        // LDS pitch of J, H and A (odd)
#define IK_NS (7 + WBC_NDOF)                    // a state: position 0..2, quaternion 3..6, q 7..26
#define IK_TRI (IK_M * (IK_M + 1) / 2)
#define IK_LAMBDA_MIN 1e-9f
#define IK_LAMBDA_MAX 1e8f                      // the damping's ceiling: status 2 beyond it
#define IK_FLOOR 1e-9f
static_assert(WBC_NB + WBC_IK_MAX_TARGETS <= IK_LPE && IK_M <= 32 && IK_NS <= IK_LPE && WBC_NJ <= WBC_NB, "lanes");
struct IkConst : TreeWalk, TreeRigid, TreeCols {
  int32_t nt, rb[WBC_IK_MAX_TARGETS];          // the listed rigid bodies
  int32_t jdof[WBC_NJ];                         // DoF of coordinate 6 + j
  float lo[WBC_NDOF], hi[WBC_NDOF];
  uint32_t limited;                             // bit d: DoF d has limits
  float posture, lambda0, step_tol;
  int32_t max_iter;
};
struct IkArgs {
  const float *root, *dofs;                     // the start: rows root_stride / dof_env_stride floats apart, DoF d at d * dof_stride
  int root_stride, dof_env_stride, dof_stride;
  const float *target_pos, *target_quat, *w_pos, *w_ori, *q_ref;
  int n;
  float *root_out, *dof_out, *residual, *cost;
  int32_t *status, *iterations;
};

__device__ __forceinline__ float ik_sum(float v) {   // the same bits in every lane of the group
#pragma unroll
  for (int off = IK_LPE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

extern "C" __global__ void __launch_bounds__(64) wbc_ik_kernel(IkConst C, IkArgs a) {
  __shared__ float sJ[IK_EPW][IK_ROWS][IK_LD];
  __shared__ float sH[IK_EPW][IK_M][IK_LD], sA[IK_EPW][IK_M][IK_LD];   // lower triangles: H; A, then L
  __shared__ float sD[IK_EPW][IK_M + 1], sV[IK_EPW][IK_M + 1];
  __shared__ float sFr[IK_EPW][WBC_NB][6];                             // joint axis, joint origin (world axes, relative position)
  __shared__ float sX[IK_EPW][WBC_IK_MAX_TARGETS][3], sRes[IK_EPW][IK_ROWS], sWr[IK_EPW][IK_ROWS];
  __shared__ float sT[IK_EPW][WBC_IK_MAX_TARGETS][8];                  // target: position relative to the start root's 0..2, unit quaternion 3..6
  __shared__ float sCur[IK_EPW][IK_NS + 1], sCand[IK_EPW][IK_NS + 1];
  __shared__ float sB[IK_EPW][IK_M + 1];                               // the second pass's held steps
  __shared__ int sDone[2], sHit[2], sAcc[2];
  const int half = IK_EPW == 2 ? threadIdx.x >> 5 : 0, lane = IK_EPW == 2 ? threadIdx.x & 31 : threadIdx.x;
  const int env = blockIdx.x * IK_EPW + half;
  const bool live = env < a.n;
  const size_t e = live ? env : a.n - 1;           // the idle half of the last workgroup recomputes the last env and stores nothing
  const int nt = C.nt < WBC_IK_MAX_TARGETS ? C.nt : WBC_IK_MAX_TARGETS, nrow = 6 * nt;
  float (*J)[IK_LD] = sJ[half], (*H)[IK_LD] = sH[half], (*A)[IK_LD] = sA[half];
  float *D = sD[half], *V = sV[half], *cur = sCur[half], *cand = sCand[half], *res = sRes[half], *wr = sWr[half];
  const float *rs = a.root + e * (size_t)a.root_stride, *ds = a.dofs + e * (size_t)a.dof_env_stride;
  const bool tl = lane >= WBC_NB && lane < WBC_NB + nt;   // a target's lane
  const int tk = tl ? lane - WBC_NB : 0;
  const int cdof = lane >= 6 && lane < IK_M ? C.jdof[lane - 6] : 0;   // lane c >= 6: the DoF of coordinate c
  const bool clim = lane >= 6 && lane < IK_M && ((C.limited >> cdof) & 1u);
  const float clo = C.lo[cdof], chi = C.hi[cdof];

  // the start: positions relative to its root, unit quaternion, limited joints clamped
  if (lane < IK_NS) {
    float v = 0.f;
    if (lane >= 3 && lane < 7) v = rs[lane] * (1.f / __fsqrt_rn(rs[3] * rs[3] + rs[4] * rs[4] + rs[5] * rs[5] + rs[6] * rs[6]));
    if (lane >= 7) {
      const int d = lane - 7;
      v = ds[d * a.dof_stride];
      if (C.col_body[d] >= 0 && ((C.limited >> d) & 1u)) v = fminf(fmaxf(v, C.lo[d]), C.hi[d]);
    }
    cand[lane] = v;
  }
  if (tl) {
    const size_t ek = e * nt + tk;
    const float wo = a.target_quat ? (a.w_ori ? a.w_ori[ek] : 1.f) : 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float w = a.w_pos ? a.w_pos[ek * 3 + i] : 1.f;
      wr[6 * tk + i] = w; wr[6 * tk + 3 + i] = wo;
      sT[half][tk][i] = w != 0.f ? a.target_pos[ek * 3 + i] - rs[i] : 0.f;   // a skipped row's target is never loaded
    }
    float q4[4] = {0.f, 0.f, 0.f, 1.f};
    if (wo != 0.f) {
      const float* tq = a.target_quat + ek * 4;
      const float inv = 1.f / __fsqrt_rn(tq[0] * tq[0] + tq[1] * tq[1] + tq[2] * tq[2] + tq[3] * tq[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) q4[i] = tq[i] * inv;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sT[half][tk][3 + i] = q4[i];
  }
  __syncthreads();
  const float qref = lane >= 6 && lane < IK_M ? (a.q_ref ? a.q_ref[e * WBC_NDOF + cdof] : cand[7 + cdof]) : 0.f;

  float lambda = C.lambda0, cost = 0.f, cost0 = 0.f, gc = 0.f;
  float rcand[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rcur[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // a target lane's residuals
  uint32_t fix = 0;                                // bit c: coordinate c sits at a limit with the gradient pushing outward
  int status = 1, iters = 0;
  bool done = false, moved = false;

#pragma nounroll
  for (int trip = 0; trip <= WBC_IK_MAX_ITER; ++trip) {
    // ---- evaluate the candidate (trip 0: the start)
    float share = 0.f;
    if (lane < WBC_NB + nt) {
      const int r = C.rb[tk], b = tl ? C.rb_body[r] : lane;
      float qa[4] = {cand[3], cand[4], cand[5], cand[6]}, E[9];
      quat_to_mat(qa, E);
      f3 p = mk3(cand[0], cand[1], cand[2]), ax = mk3(0.f, 0.f, 0.f);
#pragma nounroll
      for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
        const int jb = C.path[b][k];
        if (jb < 0) break;
        float sh, ch, Q[9];
        sincosf(0.5f * cand[7 + C.dof[jb]], &sh, &ch);
        const f3 u = tree_axis(C.axis[jb]);
        tree_rodrigues(u, 2.f * sh * ch, 1.f - 2.f * sh * sh, 2.f * sh * sh, Q);
        ax = tree_frame_step(E, p, Q, C.joint_xyz[jb], u);
        const float qj[4] = {u.x * sh, u.y * sh, u.z * sh, ch};
        quat_mul(qa, qj, qa);
      }
      if (!tl) {
        st3(sFr[half][b], ax); st3(sFr[half][b] + 3, p);
      } else {
        const f3 x = p + mat_mul(E, mk3(C.rb_offset[r][0], C.rb_offset[r][1], C.rb_offset[r][2]));
        st3(sX[half][tk], x);
        const float xs[3] = {x.x, x.y, x.z};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float w = wr[6 * tk + i];
          rcand[i] = w != 0.f ? sT[half][tk][i] - xs[i] : 0.f;
          share += w != 0.f ? 0.5f * w * rcand[i] * rcand[i] : 0.f;
        }
        const float wo = wr[6 * tk + 3];
        f3 phi = mk3(0.f, 0.f, 0.f);
        if (wo != 0.f) {                           // phi = log(R_target R^T) from the error quaternion q_target conj(q)
          const float qc[4] = {-qa[0], -qa[1], -qa[2], qa[3]};
          float qe[4];
          quat_mul(&sT[half][tk][3], qc, qe);
          const float sg = qe[3] < 0.f ? -1.f : 1.f;
          const f3 v = mk3(qe[0] * sg, qe[1] * sg, qe[2] * sg);
          const float w = qe[3] * sg, nv = __fsqrt_rn(dot(v, v));
          phi = v * (nv > 1e-6f ? 2.f * atan2f(nv, w) / nv : 2.f / w);
          share += 0.5f * wo * dot(phi, phi);
        }
        rcand[3] = phi.x; rcand[4] = phi.y; rcand[5] = phi.z;
#pragma unroll
        for (int i = 0; i < 6; ++i) res[6 * tk + i] = rcand[i];
      }
    }
    if (lane >= 6 && lane < IK_M) {
      const float dq = cand[7 + cdof] - qref;
      share += 0.5f * C.posture * dq * dq;
    }
    const float cc = ik_sum(share);

    // ---- accept or reject
    bool acc;
    if (trip == 0) {
      cost0 = cost = cc;
      if (!(fabsf(cc) <= 3.4e38f)) { status = 3; done = true; }
      acc = !done;
    } else {
      acc = !done && cc <= cost;
      if (!done) {
        ++iters;
        if (acc) { lambda = fmaxf(lambda * 0.125f, IK_LAMBDA_MIN); moved = true; cost = cc; }
        else {
          lambda *= 8.f;
          if (lambda > IK_LAMBDA_MAX) { status = 2; done = true; }
        }
      }
    }
    if (acc) {
      if (lane < IK_NS) cur[lane] = cand[lane];
#pragma unroll
      for (int i = 0; i < 6; ++i) rcur[i] = rcand[i];
    }
    if (lane == 0) sAcc[half] = acc;
    __syncthreads();

    // ---- linearise at the evaluated point: kept only where it was accepted, and skipped by the whole workgroup where neither env's was
    if (sAcc[0] != 0 || (IK_EPW == 2 && sAcc[1] != 0)) {
      if (lane < IK_M) {
        const int c = lane, jb = c >= 6 ? C.col_body[cdof] : 0, j = c < 3 ? c : c - 3;
        const f3 ej = mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f);
        const f3 pr = mk3(cand[0], cand[1], cand[2]);
        float g = 0.f;
        for (int k = 0; k < WBC_IK_MAX_TARGETS; ++k) {
          if (k >= nt) break;
          const f3 x = ld3(sX[half][k]);
          f3 lin = mk3(0.f, 0.f, 0.f), ang = lin;
          if (c < 3) lin = ej;
          else if (c < 6) { lin = cross(ej, x - pr); ang = ej; }
          else if ((C.anc[C.rb_body[C.rb[k]]] >> jb) & 1u) { ang = ld3(sFr[half][jb]); lin = cross(ang, x - ld3(sFr[half][jb] + 3)); }
          const float col[6] = {lin.x, lin.y, lin.z, ang.x, ang.y, ang.z};
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            J[6 * k + i][c] = col[i];
            g -= wr[6 * k + i] * col[i] * res[6 * k + i];
          }
        }
        if (c >= 6) g += C.posture * (cand[7 + cdof] - qref);
        if (acc) gc = g;
      }
      {
        const float qv = cand[7 + cdof];
        const bool f = clim && ((qv <= clo && gc > 0.f) || (qv >= chi && gc < 0.f));
        const uint32_t m = (uint32_t)(__ballot(f) >> (32 * half));
        if (acc) fix = m;
      }
      __syncthreads();
#pragma nounroll
      for (int t = lane; t < IK_TRI; t += IK_LPE) {
        int i, j;
        delassus_tri(t, i, j);
        float h = 0.f;
        for (int r = 0; r < IK_ROWS; ++r) {
          if (r >= nrow) break;
          h += wr[r] * J[r][i] * J[r][j];
        }
        if (i == j && i >= 6) h += C.posture;
        if (acc) H[i][j] = h;
      }
    }
    __syncthreads();

    // ---- the damped step from the current point
    auto damped_solve = [&](uint32_t held, float ci) {   // the identity's rows and columns on `held`; lane c: entry c of the right-hand side
#pragma nounroll
      for (int t = lane; t < IK_TRI; t += IK_LPE) {
        int i, j;
        delassus_tri(t, i, j);
        const bool on = !((held >> i) & 1u) && !((held >> j) & 1u);
        const float h = H[i][j];
        A[i][j] = on ? (i == j ? h + lambda * h + IK_FLOOR : h) : (i == j ? 1.f : 0.f);   // delassus_fill's device for rows that are held
      }
      delassus_cholesky(A, D, IK_M, lane);
      delassus_lane_solve(A, D, V, IK_M, lane, ci);
    };
    const bool mine = lane < IK_M && !((fix >> lane) & 1u);
    damped_solve(fix, mine ? -gc : 0.f);
    // second pass: a free joint whose step would leave its limits goes ONTO the limit, and the others solve again with those steps held
    // (the clamped step of the first pass is not a descent step of the model). Taken by the whole workgroup if either env needs it.
    bool hit = false;
    float snap = 0.f;
    if (mine && clim) {
      const float v = cur[7 + cdof] + V[lane];
      hit = v < clo || v > chi;
      snap = v < clo ? clo : chi;
    }
    const uint32_t hits = (uint32_t)(__ballot(hit) >> (32 * half));
    if (lane < IK_M) sB[half][lane] = hit ? snap - cur[7 + cdof] : 0.f;
    if (lane == 0) sHit[half] = hits != 0u;
    __syncthreads();
    if (sHit[0] != 0 || (IK_EPW == 2 && sHit[1] != 0)) {
      float ci = 0.f;
      if (mine) {
        ci = sB[half][lane];
        if (!hit) {
          float sum = 0.f;
          for (int j = 0; j < IK_M; ++j)
            if ((hits >> j) & 1u) sum += (lane >= j ? H[lane][j] : H[j][lane]) * sB[half][j];
          ci = -gc - sum;
        }
      }
      damped_solve(fix | hits, ci);
    }
    bool far = false;                              // this coordinate's projected step exceeds step_tol (or is not a number)
    if (lane < IK_M) {
      const float d = V[lane];
      float s = fabsf(d);
      if (lane < 3) cand[lane] = cur[lane] + d;
      if (lane == 3) {                             // R <- exp([d theta]x) R
        const f3 th = mk3(V[3], V[4], V[5]);
        const float an = __fsqrt_rn(dot(th, th));
        float sh, ch;
        sincosf(0.5f * an, &sh, &ch);
        const float kk = an > 1e-6f ? sh / an : 0.5f;
        const float dq[4] = {th.x * kk, th.y * kk, th.z * kk, ch}, qo[4] = {cur[3], cur[4], cur[5], cur[6]};
        float qn[4];
        quat_mul(dq, qo, qn);
        const float inv = 1.f / __fsqrt_rn(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) cand[3 + i] = qn[i] * inv;
      }
      if (lane >= 6) {
        const float q0 = cur[7 + cdof];
        float qn = q0 + d;
        if (clim) qn = fminf(fmaxf(qn, clo), chi);
        if (hit) qn = snap;
        cand[7 + cdof] = qn;
        s = fabsf(qn - q0);
      }
      far = !(s <= C.step_tol) || !(d == d);
    }
    const bool anyfar = (uint32_t)(__ballot(far) >> (32 * half)) != 0u;
    if (!done) {
      if (!anyfar && lambda <= C.lambda0) { status = 0; done = true; }
      else if (trip >= C.max_iter) done = true;    // status 1
    }
    // ---- one exit decision for the workgroup
    if (lane == 0) sDone[half] = done || !live;
    __syncthreads();
    const bool all = sDone[0] != 0 && (IK_EPW == 1 || sDone[1] != 0);
    __syncthreads();
    if (all) break;
  }

  if (!live) return;
  const bool start = status == 3 || !moved;        // no step was accepted: the start's own bits
  if (lane < 7) a.root_out[e * 7 + lane] = start ? rs[lane] : (lane < 3 ? rs[lane] + cur[lane] : cur[lane]);
  if (lane < WBC_NDOF) {
    const bool joint = C.col_body[lane] >= 0;
    a.dof_out[e * WBC_NDOF + lane] = joint && status != 3 ? cur[7 + lane] : ds[lane * a.dof_stride];
  }
  if (a.residual && tl) {
#pragma unroll
    for (int i = 0; i < 6; ++i) a.residual[(e * nt + tk) * 6 + i] = status == 3 ? rcand[i] : rcur[i];
  }
  if (lane == 0) {
    if (a.cost) { a.cost[e * 2] = cost0; a.cost[e * 2 + 1] = cost; }
    if (a.status) a.status[e] = status;
    if (a.iterations) a.iterations[e] = iters;
  }
}

// One launch on `stream`, no workspace. Arguments and conventions: include/wbc_sim.h. The checks that need no sim come first.
extern "C" int wbc_sim_inverse_kinematics(wbc_sim* s, const int32_t* bodies, int ntargets, const float* target_pos, const float* target_quat,
                                          const float* w_pos, const float* w_ori, const float* root_init, const float* dof_init,
                                          const float* q_ref, const wbc_ik_opts* opts, float* root_out, float* dof_out, float* residual,
                                          float* cost, int32_t* status, int32_t* iterations, void* stream) {
  WbCall c("wbc_sim_inverse_kinematics", s, stream);
  if (!bodies || !target_pos || !opts || !root_out || !dof_out) return c.fail(-1, "bodies / target_pos / opts / root_out / dof_out is NULL");
  if (ntargets < 1 || ntargets > WBC_IK_MAX_TARGETS) return c.fail(-1, "ntargets must be 1..WBC_IK_MAX_TARGETS");
  for (int k = 0; k < ntargets; ++k)
    if (bodies[k] < 0 || bodies[k] >= WBC_NRB) return c.fail(-1, "rigid-body index outside 0..WBC_NRB-1");
  if (w_ori && !target_quat) return c.fail(-1, "w_ori given without target_quat");
  if (!(opts->posture >= 0.f) || !(opts->posture <= 3.4e38f)) return c.fail(-1, "posture must be finite and >= 0");
  if (!(opts->damping > 0.f) || !(opts->damping <= 3.4e38f)) return c.fail(-1, "damping must be finite and > 0");
  if (!(opts->step_tol > 0.f) || !(opts->step_tol <= 3.4e38f)) return c.fail(-1, "step_tol must be finite and > 0");
  if (opts->max_iter < 0 || opts->max_iter > WBC_IK_MAX_ITER) return c.fail(-1, "max_iter must be 0..WBC_IK_MAX_ITER");
  if (((uintptr_t)target_pos | (uintptr_t)target_quat | (uintptr_t)w_pos | (uintptr_t)w_ori | (uintptr_t)root_init | (uintptr_t)dof_init |
       (uintptr_t)q_ref | (uintptr_t)root_out | (uintptr_t)dof_out | (uintptr_t)residual | (uintptr_t)cost | (uintptr_t)status |
       (uintptr_t)iterations) & 3u)
    return c.fail(-1, "every device pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  IkConst C;
  if (ba_const_fill(m, C, C) != 0) return c.no_tree();
  tree_cols_fill(m, C);
  int nj = 0;
  C.limited = 0;
  for (int d = 0; d < WBC_NDOF; ++d) {
    C.lo[d] = m.q_lower[d]; C.hi[d] = m.q_upper[d];
    if (C.col_body[d] < 0) continue;
    if (!(m.q_lower[d] == 0.f && m.q_upper[d] == 0.f)) {
      if (!(m.q_lower[d] <= m.q_upper[d])) return c.fail(-3, "a joint's lower limit exceeds its upper limit");
      C.limited |= 1u << d;
    }
    if (nj < WBC_NJ) C.jdof[nj] = d;
    ++nj;
  }
  if (nj != WBC_NJ) return c.no_tree();
  const int n = c.n;
  if (n <= 0) return 0;
  C.nt = ntargets;
  for (int k = 0; k < WBC_IK_MAX_TARGETS; ++k) C.rb[k] = bodies[k < ntargets ? k : 0];
  C.posture = opts->posture; C.lambda0 = opts->damping; C.step_tol = opts->step_tol;
  C.max_iter = opts->max_iter > 0 ? opts->max_iter : WBC_IK_MAX_ITER;
  IkArgs a;
  a.root = root_init ? root_init : c.root; a.root_stride = root_init ? 7 : 26;
  a.dofs = dof_init ? dof_init : c.dofs; a.dof_env_stride = dof_init ? WBC_NDOF : 2 * WBC_NDOF; a.dof_stride = dof_init ? 1 : 2;
  a.target_pos = target_pos; a.target_quat = target_quat; a.w_pos = w_pos; a.w_ori = w_ori; a.q_ref = q_ref;
  a.n = n;
  a.root_out = root_out; a.dof_out = dof_out; a.residual = residual; a.cost = cost; a.status = status; a.iterations = iterations;
  hipLaunchKernelGGL(wbc_ik_kernel, dim3((n + IK_EPW - 1) / IK_EPW), dim3(64), 0, (hipStream_t)stream, C, a);
  return c.launched();
}

// ---- Coriolis matrix, dM/dt, generalised momentum and the momentum observer (include/wbc_sim.h: wbc_sim_coriolis) ----------------------
// C(q, nu) of M nudot + C nu + g = tau in the factorisation with C + C^T = dM/dt (Echeandia and Wensing):
//     C = sum_k J_k^T (I_k Jdot_k + B_k J_k),    B_k = 1/2 [crf(v_k) I_k + crfbar(I_k v_k) - I_k crm(v_k)],
// every spatial vector (angular; linear) about F's origin in F's axes AS AN INERTIAL FRAME that coincides with the base at this instant:
// the root's own origin has the lever 0 and the velocity v_root. With I_k = [Ib, h x; -h x, m] (h = m c), v_k = (w; u) and the momentum
// I_k v_k = (n; l), B_k has two non-zero blocks only,
//     B_k = [B11, 0; -l x, 0],    2 B11 = P + P^T - h u^T - u h^T + 2 (u . h) 1 - n x,    P = w x Ib,
// so that B_k^T v_k = 0 and the whole of C's first three columns (the root's linear coordinates) is structurally 0. Over the tree the sum
// collapses to C[r, c] = S_r . (Ic_d Sdot_c + Bc_d S_c), d the deeper of the two coordinates' bodies, Ic / Bc the subtree's sums.
// Two envs per 64-lane workgroup, one per 32-lane half:
//  1) lane b = moving body b walks root -> b as wbc_inverse_dynamics_kernel does (tree_frame_step per joint) with the frame and the
//     spatial velocity in registers; its joint's S and Sdot = v_parent x S, its momentum (n; l) and, for the matrices, I_k and B11 go to LDS;
//  2) lane c = coordinate c sums the subtree it moves through the ancestor masks, in registers: p_c = S_c . h^C, (C^T nu)_c = Sdot_c . h^C
//     leave from here (and the observer's update, if asked for); for the matrices f_c = Ic Sdot_c + Bc S_c, Ic S_c and Bc^T S_c go to LDS;
//  3) the 26 x 26 entries, one or two six-term products each, into an LDS tile; C leaves as the tile, dM/dt as tile + tile^T, both in
//     contiguous 16-byte stores.
// The vector kernel is the same text without step 3 and without anything 26 x 26. What both kernels share (the walk, the momenta, the
// sums, the two projections) is written with explicit fused multiply-adds where a product meets a sum and is compiled without
// contraction otherwise, so that `vec` has the same bits from either kernel. The root position is never read.
#define CO_EPW 2                                // envs per workgroup
#define CO_LPE (64 / CO_EPW)                    // lanes per env
#define CO_BT 28                                // floats per body, matrices: n 0..2, l 3..5, m 6, h 7..9, Ib xx yy zz xy xz yz 10..15, B11 16..24
#define CO_BV 8                                 // floats per body, vectors: n 0..2, l 3..5
#define CO_CT 28                                // floats per coordinate: S 0..5, Sdot 6..11, f 12..17, Ic S 18..23, angular part of Bc^T S 24..26
static_assert(WBC_NB <= CO_LPE && BD_NCOL <= CO_LPE && BD_MENV % 4 == 0, "lanes");
struct CoObs {                                  // the observer's update in the vector kernel's epilogue; state NULL: none
  const float *tau, *grav;
  float gain, dt;
  int reset;
  float* state;
};

__device__ __forceinline__ float co_dot3(float a, float b, float c, f3 v) { return __builtin_fmaf(c, v.z, __builtin_fmaf(b, v.y, a * v.x)); }
__device__ __forceinline__ f3 co_cross(f3 a, f3 b) {
  return mk3(__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x)));
}
__device__ __forceinline__ float co_dot6(const float* a, const float* b) {
  float s = a[0] * b[0];
#pragma unroll
  for (int j = 1; j < 6; ++j) s = __builtin_fmaf(a[j], b[j], s);
  return s;
}
// A value the compiler cannot look through: what only the matrix kernel computes starts from such copies, so that none of its
// expressions is merged with one of the shared text.
__device__ __forceinline__ float co_opaque(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ f3 co_opaque(f3 v) { return mk3(co_opaque(v.x), co_opaque(v.y), co_opaque(v.z)); }
// (Ib w + h x v; w x h + m v) of the spatial inertia I = (m, h, Ib xx yy zz xy xz yz) at I[0..9].
__device__ __forceinline__ void co_inertia_mul(const float* I, const float* s, float* o) {
  const f3 w = mk3(s[0], s[1], s[2]), v = mk3(s[3], s[4], s[5]), h = mk3(I[1], I[2], I[3]);
  const f3 hv = co_cross(h, v), wh = co_cross(w, h);
  o[0] = co_dot3(I[4], I[7], I[8], w) + hv.x; o[1] = co_dot3(I[7], I[5], I[9], w) + hv.y; o[2] = co_dot3(I[8], I[9], I[6], w) + hv.z;
  o[3] = __builtin_fmaf(I[0], v.x, wh.x); o[4] = __builtin_fmaf(I[0], v.y, wh.y); o[5] = __builtin_fmaf(I[0], v.z, wh.z);
}

template <bool MAT>
__device__ __forceinline__ void coriolis_body(const TreeConst& K, const float* __restrict__ root, const float* __restrict__ dofs,
                                              const float* __restrict__ body_params, int n, float* __restrict__ cmat,
                                              float* __restrict__ mdot, float* __restrict__ vec, const CoObs& ob) {
#pragma clang fp contract(off)
  constexpr int BT = MAT ? CO_BT : CO_BV, NT = MAT ? 25 : 6;
  // per body: the table above, then the body's joint in F: S (axis; origin x axis) and Sdot. Dead after step 2: step 3's tile (C as
  // stored) lies over them.
  constexpr int BS = WBC_NB * (BT + 12);
  static_assert(!MAT || BS >= BD_MENV, "the tile lies over the body tables");
  __shared__ __align__(16) float sBS[CO_EPW][BS];
  __shared__ __align__(16) float sC[MAT ? CO_EPW : 1][MAT ? BD_NCOL : 1][CO_CT];
  __shared__ int32_t sCb[MAT ? CO_EPW : 1][BD_NCOL];
  __shared__ uint32_t sAnc[MAT ? CO_EPW : 1][WBC_NB];
  const int half = threadIdx.x >> 5, lane = threadIdx.x & 31;
  float *sB = sBS[half], *sS = sBS[half] + WBC_NB * BT;
  const int env = blockIdx.x * CO_EPW + half;
  const bool live = env < n;
  const size_t e = live ? env : n - 1;             // the idle half of the last workgroup recomputes the last env and stores nothing
  float R[9];
  quat_to_mat(root + e * 26 + 3, R);
  const f3 v0 = matT_mul(R, ld3(root + e * 26 + 7)), w0 = matT_mul(R, ld3(root + e * 26 + 10));   // the root's velocity in F

  if (lane < WBC_NB) {
    const int b = lane;
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 p = mk3(0.f, 0.f, 0.f), Sw = p, Sv = p, Dw = p, Dv = p, vw = w0, vv = v0;
#pragma nounroll
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int a = K.path[b][k];
      if (a < 0) break;
      const int d = K.dof[a];
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[a], dofs[e * (2 * WBC_NDOF) + 2 * d], Q);
      Sw = tree_frame_step(E, p, Q, K.joint_xyz[a], u);
      Sv = co_cross(p, Sw);
      Dw = co_cross(vw, Sw);                                   // Sdot = v_parent x S
      Dv = co_cross(vw, Sv) + co_cross(vv, Sw);
      const float qd = dofs[e * (2 * WBC_NDOF) + 2 * d + 1];
      vw = mk3(__builtin_fmaf(Sw.x, qd, vw.x), __builtin_fmaf(Sw.y, qd, vw.y), __builtin_fmaf(Sw.z, qd, vw.z));
      vv = mk3(__builtin_fmaf(Sv.x, qd, vv.x), __builtin_fmaf(Sv.y, qd, vv.y), __builtin_fmaf(Sv.z, qd, vv.z));
    }
    // spatial inertia about F's origin: the per-env root composite and gripper body (body_params), the model's otherwise
    float m = K.mass[b], com[3] = {K.com[b][0], K.com[b][1], K.com[b][2]}, I6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) I6[j] = K.inertia[b][j];
    const int slot = b == 0 ? TREE_BP_ROOT : (b == K.gripper_body ? TREE_BP_GRIPPER : -1);
    if (slot >= 0) {
      const float* bp = body_params + e * TREE_BP_STRIDE + slot;
      m = bp[0];
#pragma unroll
      for (int j = 0; j < 3; ++j) com[j] = bp[1 + j];
#pragma unroll
      for (int j = 0; j < 6; ++j) I6[j] = bp[4 + j];
    }
    // every sum of products below names its fused multiply-adds: left to the compiler, which product of a sum it fuses depends on what
    // else uses that product, and that differs between the two kernels
    const f3 cm = mk3(com[0], com[1], com[2]);
    const f3 C = mk3(p.x + co_dot3(E[0], E[1], E[2], cm), p.y + co_dot3(E[3], E[4], E[5], cm), p.z + co_dot3(E[6], E[7], E[8], cm));
    const f3 h = mk3(m * C.x, m * C.y, m * C.z);
    float EI[9], Ibar[6];                                      // E I_b E^T, as tree_rotate_inertia
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float a = E[r * 3], b2 = E[r * 3 + 1], c2 = E[r * 3 + 2];
      EI[r * 3] = co_dot3(a, b2, c2, mk3(I6[0], I6[3], I6[4]));
      EI[r * 3 + 1] = co_dot3(a, b2, c2, mk3(I6[3], I6[1], I6[5]));
      EI[r * 3 + 2] = co_dot3(a, b2, c2, mk3(I6[4], I6[5], I6[2]));
    }
    Ibar[0] = co_dot3(EI[0], EI[1], EI[2], mk3(E[0], E[1], E[2])); Ibar[1] = co_dot3(EI[3], EI[4], EI[5], mk3(E[3], E[4], E[5]));
    Ibar[2] = co_dot3(EI[6], EI[7], EI[8], mk3(E[6], E[7], E[8])); Ibar[3] = co_dot3(EI[0], EI[1], EI[2], mk3(E[3], E[4], E[5]));
    Ibar[4] = co_dot3(EI[0], EI[1], EI[2], mk3(E[6], E[7], E[8])); Ibar[5] = co_dot3(EI[3], EI[4], EI[5], mk3(E[6], E[7], E[8]));
    const float CC = co_dot3(C.x, C.y, C.z, C);
    const float Ib[6] = {__builtin_fmaf(m, CC - C.x * C.x, Ibar[0]), __builtin_fmaf(m, CC - C.y * C.y, Ibar[1]),
                         __builtin_fmaf(m, CC - C.z * C.z, Ibar[2]), __builtin_fmaf(-h.x, C.y, Ibar[3]),
                         __builtin_fmaf(-h.x, C.z, Ibar[4]), __builtin_fmaf(-h.y, C.z, Ibar[5])};
    // the body's spatial momentum (n; l) = I_k v_k
    const f3 hu = co_cross(h, vv), wh = co_cross(vw, h);
    const f3 nn = mk3(co_dot3(Ib[0], Ib[3], Ib[4], vw) + hu.x, co_dot3(Ib[3], Ib[1], Ib[5], vw) + hu.y, co_dot3(Ib[4], Ib[5], Ib[2], vw) + hu.z);
    const f3 ll = mk3(__builtin_fmaf(m, vv.x, wh.x), __builtin_fmaf(m, vv.y, wh.y), __builtin_fmaf(m, vv.z, wh.z));
    float* o = sB + b * BT;
    st3(o, nn); st3(o + 3, ll);
    if (MAT) {
      const f3 w2 = co_opaque(vw), u2 = co_opaque(vv), h2 = co_opaque(h), n2 = co_opaque(nn);
      float I2[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) I2[j] = co_opaque(Ib[j]);
      o[6] = m; st3(o + 7, h2);
#pragma unroll
      for (int j = 0; j < 6; ++j) o[10 + j] = I2[j];
      // 2 B11 = P + P^T - h u^T - u h^T + 2 (u . h) 1 - n x, column j of P = w x (column j of Ib)
      const f3 P0 = co_cross(w2, mk3(I2[0], I2[3], I2[4])), P1 = co_cross(w2, mk3(I2[3], I2[1], I2[5])), P2 = co_cross(w2, mk3(I2[4], I2[5], I2[2]));
      const float P[9] = {P0.x, P1.x, P2.x, P0.y, P1.y, P2.y, P0.z, P1.z, P2.z};
      const float hv[3] = {h2.x, h2.y, h2.z}, uv[3] = {u2.x, u2.y, u2.z}, uh2 = 2.f * co_dot3(u2.x, u2.y, u2.z, h2);
      const float N[9] = {0.f, -n2.z, n2.y, n2.z, 0.f, -n2.x, -n2.y, n2.x, 0.f};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          float s = (P[i * 3 + j] + P[j * 3 + i]) - (hv[i] * uv[j] + uv[i] * hv[j]);
          if (i == j) s += uh2;
          else s -= N[i * 3 + j];
          o[16 + i * 3 + j] = 0.5f * s;
        }
      sAnc[half][b] = K.anc[b];
    }
    float* q = sS + b * 12;
    st3(q, Sw); st3(q + 3, Sv); st3(q + 6, Dw); st3(q + 9, Dv);
  }
  __syncthreads();

  if (lane < BD_NCOL) {
    const int c = lane, b = c < 6 ? 0 : K.col_body[c - 6], bb = b < 0 ? 0 : b;
    float S[6], D[6];                                          // the coordinate's motion vector in F and its rate
    if (c < 6) {                                               // world-frame root coordinates: rows of R; Sdot = (0; v_root x e_j)
      const int j = c < 3 ? c : c - 3;
      const f3 row = matT_mul(R, mk3(j == 0 ? 1.f : 0.f, j == 1 ? 1.f : 0.f, j == 2 ? 1.f : 0.f)), dr = co_cross(v0, row);
      const bool lin = c < 3;
      S[0] = lin ? 0.f : row.x; S[1] = lin ? 0.f : row.y; S[2] = lin ? 0.f : row.z;
      S[3] = lin ? row.x : 0.f; S[4] = lin ? row.y : 0.f; S[5] = lin ? row.z : 0.f;
      D[0] = D[1] = D[2] = 0.f;
      D[3] = lin ? 0.f : dr.x; D[4] = lin ? 0.f : dr.y; D[5] = lin ? 0.f : dr.z;
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) { S[j] = sS[bb * 12 + j]; D[j] = sS[bb * 12 + 6 + j]; }
    }
    float acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = 0.f;
    for (int d = 0; d < WBC_NB; ++d) {                         // the subtree's sums: everything is already about F's origin
      const bool in = (K.anc[d] >> bb) & 1u;
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] += in ? sB[d * BT + j] : 0.f;
    }
    const float pv = b >= 0 ? co_dot6(S, acc) : 0.f, ct = b >= 0 ? co_dot6(D, acc) : 0.f;
    if (live) {
      if (vec) { vec[e * (2 * BD_NCOL) + c] = pv; vec[e * (2 * BD_NCOL) + BD_NCOL + c] = ct; }
      if (!MAT && ob.state) {                                  // the observer: fingers exactly 0
        float* st = ob.state + e * (2 * BD_NCOL);
        float integral = pv, residual = 0.f;
        if (!ob.reset) {
          const float t = ob.tau ? ob.tau[e * BD_NCOL + c] : 0.f;
          integral = st[c] + ob.dt * (((t + ct) - ob.grav[e * BD_NCOL + c]) + st[BD_NCOL + c]);
          residual = ob.gain * (pv - integral);
        }
        st[c] = b >= 0 ? integral : 0.f; st[BD_NCOL + c] = b >= 0 ? residual : 0.f;
      }
    }
    if (MAT) {
      float* o = sC[half][c];
      float f[6], g[6];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = co_opaque(acc[j]);
#pragma unroll
      for (int j = 0; j < 6; ++j) { S[j] = co_opaque(S[j]); D[j] = co_opaque(D[j]); }
      co_inertia_mul(acc + 6, D, f);
      co_inertia_mul(acc + 6, S, g);
      const f3 sw = mk3(S[0], S[1], S[2]), sv = mk3(S[3], S[4], S[5]), lc = mk3(acc[3], acc[4], acc[5]);
      const f3 lw = co_cross(lc, sw), lv = co_cross(lc, sv);   // Bc S = (B11 w; -l x w), Bc^T S = (B11^T w + l x v; 0)
      f[0] += co_dot3(acc[16], acc[17], acc[18], sw); f[1] += co_dot3(acc[19], acc[20], acc[21], sw); f[2] += co_dot3(acc[22], acc[23], acc[24], sw);
      f[3] -= lw.x; f[4] -= lw.y; f[5] -= lw.z;
#pragma unroll
      for (int j = 0; j < 6; ++j) { o[j] = S[j]; o[6 + j] = D[j]; o[12 + j] = f[j]; o[18 + j] = g[j]; }
      o[24] = co_dot3(acc[16], acc[19], acc[22], sw) + lv.x;
      o[25] = co_dot3(acc[17], acc[20], acc[23], sw) + lv.y;
      o[26] = co_dot3(acc[18], acc[21], acc[24], sw) + lv.z;
      sCb[half][c] = b;
    }
  }
  if constexpr (MAT) {
    __syncthreads();

    // C[r, c]: r above c (or both on the root): S_r . f_c; r below c: (Ic_r S_r) . Sdot_c + (Bc_r^T S_r) . S_c; the root's linear columns,
    // the fingers and the pairs of which neither moves the other: 0
    for (int t = lane; t < BD_MENV; t += CO_LPE) {
      const int r = t / BD_NCOL, c = t - r * BD_NCOL;
      const int br = sCb[half][r], bc = sCb[half][c];
      float x = 0.f;
      if (br >= 0 && bc >= 0 && c >= 3) {
        const float *cr = sC[half][r], *cc = sC[half][c];
        if ((sAnc[half][bc] >> br) & 1u) x = co_dot6(cr, cc + 12);
        else if ((sAnc[half][br] >> bc) & 1u) x = co_dot6(cr + 18, cc + 6) + co_dot3(cr[24], cr[25], cr[26], mk3(cc[0], cc[1], cc[2]));
      }
      sBS[half][t] = x;
    }
    __syncthreads();
    if (!live) return;
    const float* T = sBS[half];
    if (cmat) {
      float4* out = reinterpret_cast<float4*>(cmat + e * BD_MENV);
      for (int t = lane; t < BD_MENV / 4; t += CO_LPE) out[t] = reinterpret_cast<const float4*>(T)[t];
    }
    if (mdot) {                                                  // dM/dt = C + C^T from the tile: symmetric and equal to cmat + cmat^T bit for bit
      float4* out = reinterpret_cast<float4*>(mdot + e * BD_MENV);
      for (int t = lane; t < BD_MENV / 4; t += CO_LPE) {
        float v[4];
        int i = (4 * t) / BD_NCOL, j = 4 * t - i * BD_NCOL;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v[u] = T[i * BD_NCOL + j] + T[j * BD_NCOL + i];
          if (++j == BD_NCOL) { j = 0; ++i; }
        }
        out[t] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(64) wbc_coriolis_kernel(TreeConst K, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                    const float* __restrict__ body_params, int n, float* __restrict__ cmat,
                                                                    float* __restrict__ mdot, float* __restrict__ vec) {
  const CoObs none = {nullptr, nullptr, 0.f, 0.f, 0, nullptr};
  coriolis_body<true>(K, root, dofs, body_params, n, cmat, mdot, vec, none);
}

extern "C" __global__ void __launch_bounds__(64) wbc_momentum_kernel(TreeConst K, const float* __restrict__ root, const float* __restrict__ dofs,
                                                                    const float* __restrict__ body_params, int n, float* __restrict__ vec,
                                                                    CoObs ob) {
  coriolis_body<false>(K, root, dofs, body_params, n, nullptr, nullptr, vec, ob);
}

static int coriolis_launch(const WbCall& c, float* cmat, float* mdot, float* vec, const CoObs& ob, void* stream) {
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  TreeConst K;
  if (tree_const_fill(c.hc->model, K) != 0) return c.no_tree();
  const dim3 grid((c.n + CO_EPW - 1) / CO_EPW);
  if (cmat || mdot) hipLaunchKernelGGL(wbc_coriolis_kernel, grid, dim3(64), 0, (hipStream_t)stream, K, c.root, c.dofs, c.bp, c.n, cmat, mdot, vec);
  else hipLaunchKernelGGL(wbc_momentum_kernel, grid, dim3(64), 0, (hipStream_t)stream, K, c.root, c.dofs, c.bp, c.n, vec, ob);
  return c.launched();
}

// cmat / mdot (device f32 [N,26,26], 16-byte aligned), vec (device f32 [N,2,26]: p, C^T nu), caller-owned, any may be NULL: include/wbc_sim.h.
extern "C" int wbc_sim_coriolis(wbc_sim* s, float* cmat, float* mdot, float* vec, void* stream) {
  WbCall c("wbc_sim_coriolis", s, stream);
  if (!s) return c.no_sim();
  if (!cmat && !mdot && !vec) return c.fail(-1, "cmat, mdot and vec are all NULL");
  if (((uintptr_t)cmat | (uintptr_t)mdot) & 15u) return c.fail(-1, "cmat / mdot must be 16-byte aligned");
  if ((uintptr_t)vec & 3u) return c.fail(-1, "vec must be 4-byte aligned");
  const CoObs none = {nullptr, nullptr, 0.f, 0.f, 0, nullptr};
  return coriolis_launch(c, cmat, mdot, vec, none, stream);
}

// Two launches: g(q) into the sim's [N, 26] scratch (wbc_inverse_dynamics_kernel), then the vector kernel with the update in its epilogue.
extern "C" int wbc_sim_momentum_observer(wbc_sim* s, const float* tau, float gain, float dt, int flags, float* state, void* stream) {
  WbCall c("wbc_sim_momentum_observer", s, stream);
  if (!s) return c.no_sim();
  if (!state) return c.fail(-1, "state is NULL");
  if (flags & ~WBC_OBSERVER_RESET) return c.fail(-1, "unknown flag bits");
  if (!(gain > 0.f) || !(gain <= 3.4e38f)) return c.fail(-1, "gain must be finite and > 0");
  if (!(dt > 0.f) || !(dt <= 3.4e38f)) return c.fail(-1, "dt must be finite and > 0");
  if (!(gain * dt < 1.f)) return c.fail(-1, "gain * dt must be below 1");
  if (((uintptr_t)tau | (uintptr_t)state) & 3u) return c.fail(-1, "tau / state must be 4-byte aligned");
  if (!c.have) return c.no_state();
  if (c.n <= 0) return 0;
  float* g = nullptr;
  if (wbc_sim_internal_fd_scratch(s, &g) != 0) return -1;
  const int rc = wbc_sim_inverse_dynamics(s, nullptr, nullptr, g, stream);
  if (rc != 0) return rc;
  const CoObs ob = {tau, g, gain, dt, (flags & WBC_OBSERVER_RESET) ? 1 : 0, state};
  return coriolis_launch(c, nullptr, nullptr, nullptr, ob, stream);
}

// ---- self-collision proximity: signed gaps, witness points and gap Jacobians (include/wbc_sim.h: wbc_sim_proximity) --------------------
// The host side; the kernel is in wbc_proximity_kernel.hip, its argument struct in wbc_proximity.h.
// The pair list and the primitives from the model the sim was created with (wbc_sim_create has checked the collision set's indices).
// 0; 1: a tree the kernels cannot walk; 2: more sphere-box pairs on the root than PX_MAXBOX.
static int prox_const_fill(const DevConst* hc, ProxConst& K, int32_t* pairs_out) {
  const wbc_model& m = hc->model;
  if (tree_walk_fill(m, K) != 0) return 1;
  for (int b = 0; b < WBC_NB; ++b) {
    K.anc[b] = 1u << b;
    for (int a = b; a > 0; a = m.parent[a]) K.anc[b] |= 1u << m.parent[a];
  }
  int np = 0, nbox = 0;
  for (int k = 0; k < WBC_NCP; ++k)
    if (m.pr_kind[k] == WBC_PR_LIMBS) {
      if (pairs_out) { pairs_out[4 * np] = WBC_PR_LIMBS; pairs_out[4 * np + 1] = m.pr_a[k]; pairs_out[4 * np + 2] = m.pr_b[k]; pairs_out[4 * np + 3] = 0; }
      K.pair[np++] = WBC_PR_LIMBS | m.pr_a[k] << 8 | m.pr_b[k] << 16;
    }
  for (int k = 0; k < m.ncp && k < WBC_NCP; ++k)
    if (m.cp_kind[k] == WBC_CP_BOX && m.cp_body2[k] == 0) {        // (a box on the free box actor has no generalised coordinate: not listed)
      if (nbox == PX_MAXBOX) return 2;
      if (m.cp_body[k] < 0 || m.cp_body[k] >= WBC_NB) return 1;
      K.sb_body[nbox] = m.cp_body[k]; K.sb_rad[nbox] = m.cp_radius[k];
      for (int j = 0; j < 3; ++j) { K.sb_pos[nbox][j] = m.cp_pos[k][j]; K.sb_centre[nbox][j] = m.cp_a[k][j]; K.sb_half[nbox][j] = m.cp_b[k][j]; }
      if (pairs_out) { pairs_out[4 * np] = WBC_PR_STATIC; pairs_out[4 * np + 1] = m.cp_sph[k]; pairs_out[4 * np + 2] = m.cp_rb2[k]; pairs_out[4 * np + 3] = 0; }
      K.pair[np++] = WBC_PR_STATIC | nbox << 8;
      ++nbox;
    }
  for (int k = np; k < PX_MAXP; ++k) K.pair[k] = 0;
  for (int k = nbox; k < PX_MAXBOX; ++k) {
    K.sb_body[k] = 0; K.sb_rad[k] = 0.f;
    for (int j = 0; j < 3; ++j) K.sb_pos[k][j] = K.sb_centre[k][j] = K.sb_half[k][j] = 0.f;
  }
  K.npairs = np;
  for (int l = 0; l < WBC_NLIMB; ++l) {
    const bool used = l < m.nlimb;
    K.limb_body[l] = used ? m.limb_body[l] : 0;
    const int ends[2] = {used ? hc->sph_slot[m.limb_s0[l]] : -1, used ? hc->sph_slot[m.limb_s1[l]] : -1};
    for (int i = 0; i < 2; ++i) {
      const int slot = ends[i];
      if (used && (slot < 0 || slot >= WBC_NCP || m.cp_body[slot] < 0 || m.cp_body[slot] >= WBC_NB)) return 1;
      K.end_body[l][i] = used ? m.cp_body[slot] : 0;
      const int eb = K.end_body[l][i], lb = K.limb_body[l];
      int link = eb == lb ? 0 : 3;
      for (int k = 0; k < WBC_MAX_DEPTH && link == 3; ++k) {
        if (K.path[lb][k] == eb) link = 1 | k << 4;
        else if (K.path[eb][k] == lb) link = 2 | k << 4;
      }
      K.end_link[l][i] = link;
      for (int j = 0; j < 3; ++j) K.end_pos[l][i][j] = used ? m.cp_pos[slot][j] : 0.f;
    }
    K.limb_rad[l][0] = used ? m.limb_radius[l] : 0.f; K.limb_rad[l][1] = used ? m.limb_cap0[l] : 0.f; K.limb_rad[l][2] = used ? m.limb_cap1[l] : 0.f;
  }
  return 0;
}

static int prox_pairs(const char* who, const wbc_sim* s, int32_t* out) {
  WbCall c(who, const_cast<wbc_sim*>(s), nullptr);
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  ProxConst K;
  const int rc = prox_const_fill(c.hc, K, out);
  if (rc != 0) return rc == 1 ? c.no_tree() : c.fail(-3, "more sphere-box pairs on the root body than the kernel holds");
  return K.npairs;
}

// The number of pairs P (0 for a model without self-collisions), or a negative error code.
extern "C" int wbc_sim_proximity_pair_count(const wbc_sim* s) { return prox_pairs("wbc_sim_proximity_pair_count", s, nullptr); }

// out (host int32 [P][4]): (kind, a, b, 0) per pair, include/wbc_sim.h. Returns P, or a negative error code.
extern "C" int wbc_sim_proximity_pairs(const wbc_sim* s, int32_t* out) {
  if (s && !out) { WbCall c("wbc_sim_proximity_pairs", const_cast<wbc_sim*>(s), nullptr); return c.fail(-1, "out is NULL"); }
  return prox_pairs("wbc_sim_proximity_pairs", s, out);
}

// gap [N,P], normal [N,P,3], witness [N,P,2,3], jac [N,P,26] (device f32), nearest [N,k_nearest] (device int32), caller-owned, 4-byte
// aligned, any may be NULL: include/wbc_sim.h.
extern "C" int wbc_sim_proximity(wbc_sim* s, float* gap, float* normal, float* witness, float* jac, int32_t* nearest, int k_nearest, void* stream) {
  WbCall c("wbc_sim_proximity", s, stream);
  if (!s) return c.no_sim();
  if (!gap && !normal && !witness && !jac && !nearest) return c.fail(-1, "gap, normal, witness, jac and nearest are all NULL");
  if (((uintptr_t)gap | (uintptr_t)normal | (uintptr_t)witness | (uintptr_t)jac | (uintptr_t)nearest) & 3u)
    return c.fail(-1, "gap / normal / witness / jac / nearest must be 4-byte aligned");
  if (nearest && (k_nearest < 1 || k_nearest > 8)) return c.fail(-1, "k_nearest must be 1 .. 8");
  if (!c.have) return c.no_state();
  ProxConst K;
  const int rc = prox_const_fill(c.hc, K, nullptr);
  if (rc != 0) return rc == 1 ? c.no_tree() : c.fail(-3, "more sphere-box pairs on the root body than the kernel holds");
  if (K.npairs == 0) return c.fail(-1, "the model has no self-collision pairs (self_collisions = False)");
  if (c.n <= 0) return 0;
  wbc_proximity_launch(K, c.root, c.dofs, c.n, gap, normal, witness, jac, nearest, nearest ? k_nearest : 0, stream);
  return c.launched();
}

// ---- leg-odometry Kalman filter (include/wbc_sim.h: wbc_sim_leg_odometry) -----------------------------------------------------------------
// The host side; the kernel is in wbc_estimator_kernel.hip, its argument structs in wbc_estimator.h.
extern "C" int wbc_sim_leg_odometry(wbc_sim* s, const wbc_estimator_cfg* cfg, const float* quat, const float* gyro, const float* dof,
                                    const float* accel, const float* contact, const float* foot_height, const int32_t* reset_mask,
                                    const float* p_init, int flags, float* x, float* P, float* vel_body, float* nis, int32_t* status, void* stream) {
  WbCall c("wbc_sim_leg_odometry", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!contact || !x || !P) return c.fail(-1, "contact, x or P is NULL");
  if (flags & ~WBC_ESTIMATOR_RESET) return c.fail(-1, "unknown flag bits");
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  if (!positive(cfg->dt)) return c.fail(-1, "dt must be finite and > 0");
  if (!positive(cfg->sigma_p) || !positive(cfg->sigma_v) || !positive(cfg->sigma_f) || !positive(cfg->sigma_r) || !positive(cfg->sigma_rdot) ||
      !positive(cfg->sigma_z))
    return c.fail(-1, "every sigma must be finite and > 0");
  if (!positive(cfg->p0_p) || !positive(cfg->p0_v) || !positive(cfg->p0_f)) return c.fail(-1, "every initial variance must be finite and > 0");
  if (!(cfg->kappa >= 0.f) || !(cfg->kappa <= 3.4e38f)) return c.fail(-1, "kappa must be finite and >= 0");
  if (((uintptr_t)quat | (uintptr_t)gyro | (uintptr_t)dof | (uintptr_t)accel | (uintptr_t)contact | (uintptr_t)foot_height | (uintptr_t)reset_mask |
       (uintptr_t)p_init | (uintptr_t)x | (uintptr_t)P | (uintptr_t)vel_body | (uintptr_t)nis | (uintptr_t)status) & 3u)
    return c.fail(-1, "every pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  EstConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
  }
  for (int j = 0; j < 3; ++j) K.gravity[j] = c.hc->cfg.gravity[j];
  if (c.n <= 0) return 0;
  const EstArgs a = {c.root, dof ? dof : c.dofs, quat ? quat : c.root + 3, gyro, accel, contact, foot_height, p_init, reset_mask,
                     quat ? 4 : 26, (flags & WBC_ESTIMATOR_RESET) ? 1 : 0, c.n, x, P, vel_body, nis, status};
  wbc_estimator_launch(K, *cfg, a, stream);
  return c.launched();
}

// ---- convex centroidal MPC of the foot forces (include/wbc_sim.h: wbc_sim_centroidal_mpc) ------------------------------------------------
// The host side; the kernel is in wbc_mpc_kernel.hip, its argument structs in wbc_mpc.h. Workspace: wbc_centroidal_kernel's com [N,9] and
// inertia [N,7] rows.
extern "C" size_t wbc_sim_centroidal_mpc_workspace_floats(int num_envs) {
  return num_envs > 0 ? (size_t)num_envs * (MPC_CM_COM + MPC_CM_INR) : 0;
}

extern "C" int wbc_sim_centroidal_mpc(wbc_sim* s, const wbc_mpc_cfg* cfg, const float* x0, const float* mass, const float* inertia,
                                      const float* foot_pos, int foot_pos_stages, const uint8_t* contact, const float* x_ref, float* warm,
                                      int flags, float* forces, float* u, float* x_pred, float* base_acc, float* res, int32_t* status,
                                      float* workspace, void* stream) {
  WbCall c("wbc_sim_centroidal_mpc", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!contact || !x_ref) return c.fail(-1, "contact or x_ref is NULL");
  if (flags & ~(WBC_MPC_COLD | WBC_MPC_SHIFT)) return c.fail(-1, "unknown flag bits");
  if (cfg->horizon < 1 || cfg->horizon > WBC_MPC_MAX_HORIZON) return c.fail(-1, "horizon must be in 1..16");
  if (cfg->iters < 1 || cfg->iters > 1000) return c.fail(-1, "iters must be in 1..1000");
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  auto nonneg = [](float v) { return v >= 0.f && v <= 3.4e38f; };
  if (!positive(cfg->dt) || !positive(cfg->rho) || !positive(cfg->mu) || !positive(cfg->tol))
    return c.fail(-1, "dt, rho, mu and tol must be finite and > 0");
  for (int j = 0; j < 3; ++j)
    if (!positive(cfg->r[j])) return c.fail(-1, "every r must be finite and > 0");
  for (int j = 0; j < MPC_NX; ++j)
    if (!nonneg(cfg->q[j])) return c.fail(-1, "every q must be finite and >= 0");
  if (!nonneg(cfg->fz_min)) return c.fail(-1, "fz_min must be finite and >= 0");
  if (!(cfg->fz_max >= cfg->fz_min && cfg->fz_max <= 3.4e38f)) return c.fail(-1, "fz_max must be finite and >= fz_min");
  if (foot_pos_stages != 1 && foot_pos_stages != cfg->horizon) return c.fail(-1, "foot_pos_stages must be 1 or the horizon");
  if (((uintptr_t)x0 | (uintptr_t)mass | (uintptr_t)inertia | (uintptr_t)foot_pos | (uintptr_t)x_ref | (uintptr_t)warm | (uintptr_t)forces |
       (uintptr_t)u | (uintptr_t)x_pred | (uintptr_t)base_acc | (uintptr_t)res | (uintptr_t)status | (uintptr_t)workspace) & 3u)
    return c.fail(-1, "every float or int32 pointer must be 4-byte aligned");
  const bool centroidal = !x0 || !mass || !inertia;
  if (centroidal && !workspace) return c.fail(-1, "workspace is NULL while x0, mass or inertia is NULL");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  MpcConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
  }
  for (int j = 0; j < 3; ++j) K.gravity[j] = c.hc->cfg.gravity[j];
  if (c.n <= 0) return 0;
  float *com = nullptr, *inr = nullptr;
  if (centroidal) {
    TreeConst T;
    if (tree_const_fill(m, T) != 0) return c.no_tree();
    com = workspace;
    inr = workspace + (size_t)c.n * MPC_CM_COM;
    hipLaunchKernelGGL(wbc_centroidal_kernel, dim3((c.n + CM_EPW - 1) / CM_EPW), dim3(64), 0, (hipStream_t)stream, T, c.root, c.dofs, c.bp,
                       (const float*)nullptr, c.n, com, (float*)nullptr, (float*)nullptr, inr);
  }
  const MpcArgs a = {c.root, c.dofs, com, inr, x0, mass, inertia, foot_pos, x_ref, contact, warm, forces, u, x_pred, base_acc, res, status,
                     foot_pos_stages, flags, c.n};
  wbc_mpc_launch(K, *cfg, a, stream);
  return c.launched();
}

// ---- gait clock, footholds and swing references (include/wbc_sim.h: wbc_sim_footstep_plan) -------------------------------------------------
// The host side; the kernel is in wbc_footstep_kernel.hip, its argument structs in wbc_footstep.h.
extern "C" int wbc_sim_footstep_plan(wbc_sim* s, const wbc_footstep_cfg* cfg, const float* base_pos, const float* base_vel, const float* quat,
                                     const float* dof, const float* vel_cmd, const float* yaw_rate, const int32_t* reset_mask,
                                     const float* phase_init, int flags, float* state, uint8_t* stance, float* contact, uint8_t* schedule,
                                     float* foot_pos, float* foothold, float* swing_ref, float* swing_acc, int32_t* info, void* stream) {
  WbCall c("wbc_sim_footstep_plan", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!state) return c.fail(-1, "state is NULL");
  if (flags & ~(WBC_FOOTSTEP_RESET | WBC_FOOTSTEP_HOLD)) return c.fail(-1, "unknown flag bits");
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  auto nonneg = [](float v) { return v >= 0.f && v <= 3.4e38f; };
  if (cfg->horizon < 0 || cfg->horizon > WBC_MPC_MAX_HORIZON) return c.fail(-1, "horizon must be in 0..16");
  if (cfg->search_radius < 0 || cfg->search_radius > WBC_FOOTSTEP_MAX_RADIUS) return c.fail(-1, "search_radius must be in 0..3");
  if (!positive(cfg->dt) || !positive(cfg->period) || (cfg->horizon > 0 && !positive(cfg->mpc_dt)))
    return c.fail(-1, "dt, period and mpc_dt must be finite and > 0");
  if (!positive(cfg->search_step) || !positive(cfg->probe_radius)) return c.fail(-1, "search_step and probe_radius must be finite and > 0");
  if (!positive(cfg->duty)) return c.fail(-1, "duty must be finite and > 0");
  for (int f = 0; f < WBC_NFEET; ++f) {
    if (!(cfg->offset[f] >= 0.f && cfg->offset[f] < 1.f)) return c.fail(-1, "every offset must be in [0, 1)");
    if (!(fabsf(cfg->stance_offset[f][0]) <= 3.4e38f && fabsf(cfg->stance_offset[f][1]) <= 3.4e38f))
      return c.fail(-1, "every stance_offset must be finite");
  }
  if (!nonneg(cfg->k_v) || !nonneg(cfg->kp) || !nonneg(cfg->kd)) return c.fail(-1, "the gains k_v, kp and kd must be finite and >= 0");
  if (!nonneg(cfg->com_height) || !nonneg(cfg->swing_height)) return c.fail(-1, "the heights com_height and swing_height must be finite and >= 0");
  if (!nonneg(cfg->max_reach)) return c.fail(-1, "max_reach must be finite and >= 0");
  if (!nonneg(cfg->w_dist) || !nonneg(cfg->w_rough) || !nonneg(cfg->w_slope)) return c.fail(-1, "every weight must be finite and >= 0");
  if (!nonneg(cfg->rough_max) || !nonneg(cfg->nz_min)) return c.fail(-1, "the thresholds rough_max and nz_min must be finite and >= 0");
  if (!(cfg->latch >= 0.f && cfg->latch <= 1.f)) return c.fail(-1, "latch must be in [0, 1]");
  if (((uintptr_t)base_pos | (uintptr_t)base_vel | (uintptr_t)quat | (uintptr_t)dof | (uintptr_t)vel_cmd | (uintptr_t)yaw_rate |
       (uintptr_t)reset_mask | (uintptr_t)phase_init | (uintptr_t)state | (uintptr_t)contact | (uintptr_t)foot_pos | (uintptr_t)foothold |
       (uintptr_t)swing_ref | (uintptr_t)swing_acc | (uintptr_t)info) & 3u)
    return c.fail(-1, "every float or int32 pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  FsConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
  }
  double g2 = 0.0;
  for (int j = 0; j < 3; ++j) { K.gravity[j] = c.hc->cfg.gravity[j]; g2 += (double)K.gravity[j] * K.gravity[j]; }
  K.k_c = g2 > 0.0 ? (float)(0.5 * sqrt((double)cfg->com_height / sqrt(g2))) : 0.f;
  K.hf = c.hc->hf; K.hf_rows = c.hc->hf_rows; K.hf_cols = c.hc->hf_cols; K.hf_hs = c.hc->hf_hs; K.hf_vs = c.hc->hf_vs;
  for (int j = 0; j < 3; ++j) K.hf_t[j] = c.hc->hf_t[j];
  K.ground_z = c.hc->cfg.ground_z;
  if (K.hf && (K.hf_rows < 2 || K.hf_cols < 2)) return c.fail(-3, "the heightfield has fewer than 2 x 2 samples");
  if (c.n <= 0) return 0;
  const FsArgs a = {c.root, dof ? dof : c.dofs, base_pos ? base_pos : c.root, base_vel ? base_vel : c.root + 7, quat ? quat : c.root + 3,
                    vel_cmd, yaw_rate, phase_init, reset_mask, base_pos ? 3 : 26, base_vel ? 3 : 26, quat ? 4 : 26,
                    (flags & WBC_FOOTSTEP_RESET) ? 1 : 0, (flags & WBC_FOOTSTEP_HOLD) ? 1 : 0, c.n, state, stance, schedule, contact, foot_pos,
                    foothold, swing_ref, swing_acc, info};
  wbc_footstep_launch(K, *cfg, a, stream);
  return c.launched();
}

// ---- contact detection from proprioception (include/wbc_sim.h: wbc_sim_contact_detect) -----------------------------------------------------
// The host side; the kernel is in wbc_contact_kernel.hip, its argument struct in wbc_contact.h.
extern "C" int wbc_sim_contact_detect(wbc_sim* s, const wbc_contact_cfg* cfg, const float* quat, const float* dof, const float* base_pos,
                                      const float* tau_ext, int tau_ext_stride, const float* foot_force, const float* normal, const float* ground,
                                      const float* phase, int phase_stride, const int32_t* reset_mask, const float* p_init, int flags, float* state,
                                      float* prob, uint8_t* contact, uint8_t* stance, float* force, float* terms, int32_t* info, void* stream) {
  WbCall c("wbc_sim_contact_detect", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!state) return c.fail(-1, "state is NULL");
  if (flags & ~WBC_CONTACT_RESET) return c.fail(-1, "unknown flag bits");
  auto finite = [](float v) { return fabsf(v) <= 3.4e38f; };
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  auto nonneg = [](float v) { return v >= 0.f && v <= 3.4e38f; };
  if (!positive(cfg->dt)) return c.fail(-1, "dt must be finite and > 0");
  if (!positive(cfg->duty)) return c.fail(-1, "duty must be finite and > 0");
  for (int f = 0; f < WBC_NFEET; ++f)
    if (!(cfg->offset[f] >= 0.f && cfg->offset[f] < 1.f)) return c.fail(-1, "every offset must be in [0, 1)");
  if (!positive(cfg->sigma_phase) || !positive(cfg->sigma_z) || !positive(cfg->sigma_f)) return c.fail(-1, "every sigma must be finite and > 0");
  if (!finite(cfg->mu_z) || !finite(cfg->mu_f)) return c.fail(-1, "mu_z and mu_f must be finite");
  if (!positive(cfg->var_phase) || !positive(cfg->var_z) || !positive(cfg->var_f)) return c.fail(-1, "every var must be finite and > 0");
  if (!(cfg->alpha > 0.f && cfg->alpha <= 1.f)) return c.fail(-1, "alpha must be in (0, 1]");
  if (!finite(cfg->p_on) || !finite(cfg->p_off)) return c.fail(-1, "p_on and p_off must be finite");
  if (!(cfg->p_on > cfg->p_off)) return c.fail(-1, "p_on must be above p_off");
  if (!nonneg(cfg->t_dwell)) return c.fail(-1, "t_dwell must be finite and >= 0");
  if (!(cfg->early_min >= 0.f && cfg->early_min <= 1.f) || !(cfg->late_min >= 0.f && cfg->late_min <= 1.f))
    return c.fail(-1, "early_min and late_min must be in [0, 1]");
  if (!nonneg(cfg->damping)) return c.fail(-1, "damping must be finite and >= 0");
  if (!tau_ext && !foot_force && !ground && !phase) return c.fail(-1, "no measurement source: tau_ext, foot_force, ground and phase are all NULL");
  if (tau_ext && foot_force) return c.fail(-1, "tau_ext and foot_force are both given");
  if (tau_ext && tau_ext_stride < WBC_NCOL) return c.fail(-1, "tau_ext_stride must be >= 26");
  if (phase && phase_stride < 1) return c.fail(-1, "phase_stride must be >= 1");
  if (((uintptr_t)quat | (uintptr_t)dof | (uintptr_t)base_pos | (uintptr_t)tau_ext | (uintptr_t)foot_force | (uintptr_t)normal | (uintptr_t)ground |
       (uintptr_t)phase | (uintptr_t)reset_mask | (uintptr_t)p_init | (uintptr_t)state | (uintptr_t)prob | (uintptr_t)force | (uintptr_t)terms |
       (uintptr_t)info) & 3u)
    return c.fail(-1, "every float or int32 pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  EstConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
    const int32_t* path = K.path[K.foot_body[f]];                     // the kernel unrolls exactly CT_LEG_JOINTS joints per leg
    for (int k = 0; k < WBC_MAX_DEPTH; ++k)
      if ((path[k] >= 0) != (k < CT_LEG_JOINTS)) return c.fail(-3, "a foot's leg does not have exactly three joints");
  }
  for (int j = 0; j < 3; ++j) K.gravity[j] = c.hc->cfg.gravity[j];
  if (c.n <= 0) return 0;
  const CtArgs a = {dof ? dof : c.dofs, quat ? quat : c.root + 3, base_pos ? base_pos : c.root, tau_ext, foot_force, normal, ground, phase, p_init,
                    reset_mask, quat ? 4 : 26, base_pos ? 3 : 26, tau_ext_stride, phase_stride, (flags & WBC_CONTACT_RESET) ? 1 : 0, c.n,
                    state, prob, contact, stance, force, terms, info};
  wbc_contact_launch(K, *cfg, a, stream);
  return c.launched();
}

// ---- leg controller: stance forces and swing references to joint torques (include/wbc_sim.h: wbc_sim_leg_control) --------------------------
// The host side; the kernel is in wbc_legctl_kernel.hip, its argument struct in wbc_legctl.h.
extern "C" int wbc_sim_leg_control(wbc_sim* s, const wbc_leg_control_cfg* cfg, const float* quat, const float* dof, const float* base_pos,
                                   const float* base_vel, const float* ang_vel, const float* forces, const float* swing_ref, const float* stance,
                                   const float* tau_bias, int tau_bias_stride, const float* mass_matrix, int mass_matrix_stride,
                                   const float* acc_bias, int acc_bias_stride, const float* arm_q_des, const float* tau_limit, int flags,
                                   float* tau, float* leg_force, float* foot, int32_t* info, void* stream) {
  WbCall c("wbc_sim_leg_control", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (flags & ~WBC_LEGCTL_CLIP) return c.fail(-1, "unknown flag bits");
  auto finite = [](float v) { return fabsf(v) <= 3.4e38f; };
  auto nonneg = [](float v) { return v >= 0.f && v <= 3.4e38f; };
  for (int j = 0; j < 3; ++j)
    if (!nonneg(cfg->kp[j]) || !nonneg(cfg->kd[j])) return c.fail(-1, "every kp and kd must be finite and >= 0");
  if (!nonneg(cfg->kd_stance)) return c.fail(-1, "kd_stance must be finite and >= 0");
  if (!nonneg(cfg->damping)) return c.fail(-1, "damping must be finite and >= 0");
  for (int j = 0; j < LC_ARM_DOFS; ++j) {
    if (!nonneg(cfg->kp_arm[j]) || !nonneg(cfg->kd_arm[j])) return c.fail(-1, "every kp_arm and kd_arm must be finite and >= 0");
    if (!finite(cfg->arm_q_default[j])) return c.fail(-1, "every arm_q_default must be finite");
  }
  if (!nonneg(cfg->fz_min)) return c.fail(-1, "fz_min must be finite and >= 0");
  if (!(cfg->fz_max >= cfg->fz_min && cfg->fz_max <= 3.4e38f)) return c.fail(-1, "fz_max must be finite and >= fz_min");
  if (!nonneg(cfg->mu)) return c.fail(-1, "mu must be finite and >= 0");
  if (tau_bias && tau_bias_stride < WBC_NCOL) return c.fail(-1, "tau_bias_stride must be >= 26");
  if (mass_matrix && mass_matrix_stride < WBC_NCOL * WBC_NCOL) return c.fail(-1, "mass_matrix_stride must be >= 676");
  if (acc_bias && acc_bias_stride < WBC_NRB * 6) return c.fail(-1, "acc_bias_stride must be >= 162");
  if (((uintptr_t)quat | (uintptr_t)dof | (uintptr_t)base_pos | (uintptr_t)base_vel | (uintptr_t)ang_vel | (uintptr_t)forces | (uintptr_t)swing_ref |
       (uintptr_t)stance | (uintptr_t)tau_bias | (uintptr_t)mass_matrix | (uintptr_t)acc_bias | (uintptr_t)arm_q_des | (uintptr_t)tau_limit |
       (uintptr_t)tau | (uintptr_t)leg_force | (uintptr_t)foot | (uintptr_t)info) & 3u)
    return c.fail(-1, "every pointer must be 4-byte aligned");
  if (mass_matrix && !swing_ref) return c.fail(-1, "mass_matrix is given without swing_ref");
  if (!tau && !leg_force && !foot && !info) return c.fail(-1, "every output is NULL");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  EstConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  LcArgs a = {dof ? dof : c.dofs, quat ? quat : c.root + 3, base_pos ? base_pos : c.root, base_vel ? base_vel : c.root + 7,
              ang_vel ? ang_vel : c.root + 10, forces, swing_ref, stance, tau_bias, mass_matrix, acc_bias, arm_q_des, tau_limit,
              quat ? 4 : 26, base_pos ? 3 : 26, base_vel ? 3 : 26, ang_vel ? 3 : 26, tau_bias_stride, mass_matrix_stride, acc_bias_stride,
              (flags & WBC_LEGCTL_CLIP) ? 1 : 0, c.n};
  a.tau = tau; a.leg_force = leg_force; a.foot = foot; a.info = info;
  bool in_leg[WBC_NDOF] = {};
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    a.foot_rb[f] = rb;
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
    const int32_t* path = K.path[K.foot_body[f]];                     // the kernel unrolls exactly LC_LEG_JOINTS joints per leg
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      if ((path[k] >= 0) != (k < LC_LEG_JOINTS)) return c.fail(-3, "a foot's leg does not have exactly three joints");
      if (path[k] < 0) continue;
      const int d = K.dof[path[k]];
      if (d < 0 || d >= WBC_NDOF || in_leg[d]) return c.fail(-3, "a foot's leg does not have exactly three joints of its own");
      in_leg[d] = true;
    }
  }
  for (int j = 0; j < 3; ++j) K.gravity[j] = c.hc->cfg.gravity[j];
  // the live DoFs in DoF order: their columns of tau_limit; those in no leg are the arm's; the rest (the locked fingers) get 0
  bool driven[WBC_NDOF] = {};
  for (int b = 1; b < WBC_NB; ++b)
    if (K.dof[b] >= 0 && K.dof[b] < WBC_NDOF) driven[K.dof[b]] = true;
  int nlive = 0, narm = 0, nfinger = 0;
  const int max_finger = (int)(sizeof(a.finger_dof) / sizeof(a.finger_dof[0]));
  for (int d = 0; d < WBC_NDOF; ++d) {
    a.limit_col[d] = -1;
    if (!driven[d]) {
      if (nfinger < max_finger) a.finger_dof[nfinger] = d;
      ++nfinger;
      continue;
    }
    if (nlive < LC_NLIMIT) a.limit_col[d] = nlive;
    ++nlive;
    if (!in_leg[d]) { if (narm < LC_ARM_DOFS) a.arm_dof[narm] = d; ++narm; }
  }
  if (narm != LC_ARM_DOFS || nfinger != max_finger || nlive != LC_NLIMIT) return c.fail(-3, "the model does not have exactly six arm DoFs beside the legs and the locked fingers");
  if (c.n <= 0) return 0;
  wbc_legctl_launch(K, *cfg, a, stream);
  return c.launched();
}

// ---- attitude filter (include/wbc_sim.h: wbc_sim_attitude_filter) ---------------------------------------------------------------------------
// The host side; the kernel is in wbc_attitude_kernel.hip, its argument struct in wbc_attitude.h.
extern "C" int wbc_sim_attitude_filter(wbc_sim* s, const wbc_attitude_cfg* cfg, const float* gyro, const float* accel, const float* aux_body,
                                       const float* aux_world, const float* aux_sigma, int num_aux, const int32_t* reset_mask,
                                       const float* q_init, int flags, float* q, float* b, float* P, float* gyro_out, float* gravity_body,
                                       float* nis, int32_t* status, void* stream) {
  WbCall c("wbc_sim_attitude_filter", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!q || !b || !P) return c.fail(-1, "q, b or P is NULL");
  if (num_aux < 0 || num_aux > WBC_ATTITUDE_MAX_AUX) return c.fail(-1, "num_aux must be in 0 .. 4");
  if (num_aux > 0 && (!aux_body || !aux_world || !aux_sigma)) return c.fail(-1, "num_aux > 0 needs aux_body, aux_world and aux_sigma");
  if (flags & ~WBC_ATTITUDE_RESET) return c.fail(-1, "unknown flag bits");
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  if (!positive(cfg->dt)) return c.fail(-1, "dt must be finite and > 0");
  if (!positive(cfg->sigma_g) || !positive(cfg->sigma_b) || !positive(cfg->sigma_a)) return c.fail(-1, "every sigma must be finite and > 0");
  if (!positive(cfg->p0_theta) || !positive(cfg->p0_b)) return c.fail(-1, "every initial variance must be finite and > 0");
  if (!(cfg->kappa_a >= 0.f) || !(cfg->kappa_a <= 3.4e38f)) return c.fail(-1, "kappa_a must be finite and >= 0");
  if (((uintptr_t)gyro | (uintptr_t)accel | (uintptr_t)aux_body | (uintptr_t)aux_world | (uintptr_t)aux_sigma | (uintptr_t)reset_mask |
       (uintptr_t)q_init | (uintptr_t)q | (uintptr_t)b | (uintptr_t)P | (uintptr_t)gyro_out | (uintptr_t)gravity_body | (uintptr_t)nis |
       (uintptr_t)status) & 3u)
    return c.fail(-1, "every pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  AtArgs a = {c.root, gyro, accel, aux_body, aux_world, aux_sigma, q_init, reset_mask, num_aux, (flags & WBC_ATTITUDE_RESET) ? 1 : 0, c.n};
  const float* g = c.hc->cfg.gravity;
  a.gnorm = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (!positive(a.gnorm)) return c.fail(-1, "gravity is zero");
  for (int j = 0; j < 3; ++j) a.up[j] = -g[j] / a.gnorm;
  // the half turn's axis: normalise(c x up), c the world x axis where |up_x| <= 0.9 and the world y axis otherwise
  const bool cx = fabsf(a.up[0]) <= 0.9f;
  const float h[3] = {cx ? 0.f : a.up[2], cx ? -a.up[2] : 0.f, cx ? a.up[1] : -a.up[0]};
  const float hn = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
  for (int j = 0; j < 3; ++j) a.half[j] = h[j] / hn;
  a.q = q; a.b = b; a.P = P; a.gyro_out = gyro_out; a.gravity_body = gravity_body; a.nis = nis; a.status = status;
  if (c.n <= 0) return 0;
  wbc_attitude_launch(*cfg, a, stream);
  return c.launched();
}

// ---- ground plane from the footholds (include/wbc_sim.h: wbc_sim_ground_estimate) -----------------------------------------------------------
// The host side; the kernel is in wbc_ground_kernel.hip, its argument struct in wbc_ground.h.
extern "C" int wbc_sim_ground_estimate(wbc_sim* s, const wbc_ground_cfg* cfg, const float* quat, const float* dof, const float* base_pos,
                                       const float* contact, const int32_t* reset_mask, const float* query_xy, int num_query, int flags,
                                       float* state, float* normal, float* ground, float* residual, float* trunk, float* theta_ref,
                                       float* query_z, int32_t* info, void* stream) {
  WbCall c("wbc_sim_ground_estimate", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!state || !contact) return c.fail(-1, "state or contact is NULL");
  if (flags & ~WBC_GROUND_RESET) return c.fail(-1, "unknown flag bits");
  auto finite = [](float v) { return fabsf(v) <= 3.4e38f; };
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  if (!positive(cfg->dt) || !positive(cfg->tau_age)) return c.fail(-1, "dt and tau_age must be finite and > 0");
  if (!positive(cfg->lambda) || !positive(cfg->slope_max)) return c.fail(-1, "lambda and slope_max must be finite and > 0");
  if (!finite(cfg->c_on)) return c.fail(-1, "c_on must be finite");
  if (!(cfg->tilt_gain >= 0.f && cfg->tilt_gain <= 1.f)) return c.fail(-1, "tilt_gain must be in [0, 1]");
  if (num_query < 0) return c.fail(-1, "num_query must be >= 0");
  if (query_xy && num_query == 0) return c.fail(-1, "query_xy is given with num_query 0");
  if (((uintptr_t)quat | (uintptr_t)dof | (uintptr_t)base_pos | (uintptr_t)contact | (uintptr_t)reset_mask | (uintptr_t)query_xy | (uintptr_t)state |
       (uintptr_t)normal | (uintptr_t)ground | (uintptr_t)residual | (uintptr_t)trunk | (uintptr_t)theta_ref | (uintptr_t)query_z | (uintptr_t)info) & 3u)
    return c.fail(-1, "every pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  EstConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
    const int32_t* path = K.path[K.foot_body[f]];                     // the kernel unrolls exactly GE_LEG_JOINTS joints per leg
    for (int k = 0; k < WBC_MAX_DEPTH; ++k)
      if ((path[k] >= 0) != (k < GE_LEG_JOINTS)) return c.fail(-3, "a foot's leg does not have exactly three joints");
  }
  for (int j = 0; j < 3; ++j) K.gravity[j] = c.hc->cfg.gravity[j];
  if (c.n <= 0) return 0;
  const GeArgs a = {dof ? dof : c.dofs, quat ? quat : c.root + 3, base_pos ? base_pos : c.root, contact, query_xy, reset_mask,
                    quat ? 4 : 26, base_pos ? 3 : 26, (flags & WBC_GROUND_RESET) ? 1 : 0, query_xy ? num_query : 0, c.n,
                    state, normal, ground, residual, trunk, theta_ref, query_z, info};
  wbc_ground_launch(K, *cfg, a, stream);
  return c.launched();
}

// ---- foot slip detection and friction estimate (include/wbc_sim.h: wbc_sim_slip_detect) ----------------------------------------------------
// The host side; the kernel is in wbc_slip_kernel.hip, its argument struct in wbc_slip.h.
extern "C" int wbc_sim_slip_detect(wbc_sim* s, const wbc_slip_cfg* cfg, const float* quat, const float* dof, const float* base_vel,
                                   const float* ang_vel, const float* contact, const float* foot_force, const float* normal,
                                   const int32_t* reset_mask, const float* mu_init, int flags, float* state, float* prob, uint8_t* slip,
                                   float* weight, float* foot_vel, float* speed, float* distance, float* mu, float* mu_lower, float* mu_env,
                                   int32_t* info, void* stream) {
  WbCall c("wbc_sim_slip_detect", s, stream);
  // the arguments first, so that every refusal below can be met (and tested) without a sim; then the sim
  if (!cfg) return c.fail(-1, "cfg is NULL");
  if (!state || !contact) return c.fail(-1, "state or contact is NULL");
  if (flags & ~WBC_SLIP_RESET) return c.fail(-1, "unknown flag bits");
  auto finite = [](float v) { return fabsf(v) <= 3.4e38f; };
  auto positive = [](float v) { return v > 0.f && v <= 3.4e38f; };
  auto nonneg = [](float v) { return v >= 0.f && v <= 3.4e38f; };
  if (!positive(cfg->dt) || !positive(cfg->sigma_v)) return c.fail(-1, "dt and sigma_v must be finite and > 0");
  if (!positive(cfg->fn_min) || !positive(cfg->w_min) || !positive(cfg->mu_scale)) return c.fail(-1, "fn_min, w_min and mu_scale must be finite and > 0");
  if (!finite(cfg->c_on)) return c.fail(-1, "c_on must be finite");
  if (!nonneg(cfg->v_slip) || !nonneg(cfg->t_dwell)) return c.fail(-1, "v_slip and t_dwell must be finite and >= 0");
  if (!nonneg(cfg->mu_prior) || !nonneg(cfg->mu_min)) return c.fail(-1, "mu_prior and mu_min must be finite and >= 0");
  if (!(cfg->alpha > 0.f && cfg->alpha <= 1.f) || !(cfg->gamma > 0.f && cfg->gamma <= 1.f)) return c.fail(-1, "alpha and gamma must be in (0, 1]");
  if (!finite(cfg->p_on) || !finite(cfg->p_off)) return c.fail(-1, "p_on and p_off must be finite");
  if (!(cfg->p_on > cfg->p_off)) return c.fail(-1, "p_on must be above p_off");
  if (!(cfg->common_mode >= 0.f && cfg->common_mode <= 1.f)) return c.fail(-1, "common_mode must be in [0, 1]");
  if (!(cfg->mu_max >= cfg->mu_min && cfg->mu_max <= 3.4e38f)) return c.fail(-1, "mu_max must be finite and >= mu_min");
  if (((uintptr_t)quat | (uintptr_t)dof | (uintptr_t)base_vel | (uintptr_t)ang_vel | (uintptr_t)contact | (uintptr_t)foot_force | (uintptr_t)normal |
       (uintptr_t)reset_mask | (uintptr_t)mu_init | (uintptr_t)state | (uintptr_t)prob | (uintptr_t)weight | (uintptr_t)foot_vel | (uintptr_t)speed |
       (uintptr_t)distance | (uintptr_t)mu | (uintptr_t)mu_lower | (uintptr_t)mu_env | (uintptr_t)info) & 3u)
    return c.fail(-1, "every float or int32 pointer must be 4-byte aligned");
  if (!s) return c.no_sim();
  if (!c.have) return c.no_state();
  const wbc_model& m = c.hc->model;
  EstConst K;
  if (tree_walk_fill(m, K) != 0 || !tree_rigid_ok(m)) return c.no_tree();
  for (int f = 0; f < WBC_NFEET; ++f) {
    const int rb = m.feet_rb[f];
    if (rb < 0 || rb >= WBC_NRB) return c.no_tree();
    K.foot_body[f] = m.rb_body[rb];
    for (int j = 0; j < 3; ++j) K.foot_off[f][j] = m.rb_offset[rb][j];
    const int32_t* path = K.path[K.foot_body[f]];                     // the kernel unrolls exactly SL_LEG_JOINTS joints per leg
    for (int k = 0; k < WBC_MAX_DEPTH; ++k)
      if ((path[k] >= 0) != (k < SL_LEG_JOINTS)) return c.fail(-3, "a foot's leg does not have exactly three joints");
  }
  for (int j = 0; j < 3; ++j) K.gravity[j] = c.hc->cfg.gravity[j];
  if (c.n <= 0) return 0;
  const SlArgs a = {dof ? dof : c.dofs, quat ? quat : c.root + 3, base_vel ? base_vel : c.root + 7, ang_vel ? ang_vel : c.root + 10, contact,
                    foot_force, normal, mu_init, reset_mask, quat ? 4 : 26, base_vel ? 3 : 26, ang_vel ? 3 : 26, ang_vel ? 0 : 1,
                    (flags & WBC_SLIP_RESET) ? 1 : 0, c.n, state, prob, slip, weight, foot_vel, speed, distance, mu, mu_lower, mu_env, info};
  wbc_slip_launch(K, *cfg, a, stream);
  return c.launched();
}
