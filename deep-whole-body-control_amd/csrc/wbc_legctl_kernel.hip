// wbc_legctl_kernel.hip -- the kernel of wbc_sim_leg_control (include/wbc_sim.h, whose comment is the text this kernel and
// tests/leg_control_reference.py both implement); its entry point and argument checks are with the other whole-body calls in wbc_arm_kernel.hip.
// A translation unit of its own: tests/test_identification.py pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_legctl.h"

// ---- leg controller: stance forces and swing references to joint torques -------------------------------------------------------------------
// The contact kernel's layout: lane = (env, foot), LC_EPW = 16 envs per 64-lane workgroup, a single wavefront, env `grp` on lanes
// 4 grp .. 4 grp + 3 (a launch whose env count is no multiple of LC_EPW repeats the last env on the idle groups and stores nothing from
// them). Each lane walks its own leg (tree_frame_step per joint, the three joints unrolled so that their axes and origins stay in
// registers), solves its own 3 x 3 system and writes its leg's three torques. The six arm DoFs are dealt over the env's four lanes (lane l
// takes arm joints l and l + 4); lanes 2 and 3, which have one arm joint, write the two fingers' zeros. What an env shares -- the
// non-finite vote and the OR of the info bits -- goes through two xor shuffles inside the 4-lane group. No LDS, no barrier, no scratch.
// Control flow around the shuffles is uniform; a failed env runs the same instructions and stores zeros.

__device__ __forceinline__ bool lc_finite(float v) { return fabsf(v) <= 3.4e38f; }        // false for a NaN
__device__ __forceinline__ bool lc_finite(f3 v) { return lc_finite(v.x) && lc_finite(v.y) && lc_finite(v.z); }
__device__ __forceinline__ bool lc_pivot(float v) { return v > 0.f && v <= 3.4e38f; }
__device__ __forceinline__ float lc_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// step 9 for one torque of DoF d; returns whether the clamp changed it
__device__ __forceinline__ bool lc_limit(const LcArgs& a, size_t e, int d, float& tau, bool& bad) {
  if (!a.tau_limit) return false;
  const int col = a.limit_col[d];
  if (col < 0) return false;
  const float lim = a.tau_limit[e * LC_NLIMIT + col];
  bad = bad || !(lim >= 0.f && lim <= 3.4e38f);
  const float t = lc_clamp(tau, -lim, lim);
  const bool changed = t != tau;
  tau = t;
  return changed;
}

extern "C" __global__ void __launch_bounds__(64) wbc_leg_control_kernel(EstConst K, wbc_leg_control_cfg cfg, LcArgs a) {
  const int lane = threadIdx.x, grp = lane / LC_LPE, f = lane - grp * LC_LPE;
  const int eu = blockIdx.x * LC_EPW + grp;
  const bool live = eu < a.n;
  const size_t e = live ? eu : a.n - 1;
  const size_t ef = e * WBC_NFEET + f;

  int bits = 0;
  bool bad = false;

  // 1 kinematics: the trunk's rotation from the quaternion, normalised; the leg walk with every joint's axis and origin kept
  const float* qr = a.quat + e * a.quat_stride;
  const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
  const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
  float R[9];
  quat_to_mat(qu, R);
  const f3 b = ld3(a.pos + e * a.pos_stride), v = ld3(a.vel + e * a.vel_stride), ww = ld3(a.ang + e * a.ang_stride);
  const f3 wb = matT_mul(R, ww);
  bad = bad || !(lc_finite(b) && lc_finite(v) && lc_finite(ww));
  const int body = K.foot_body[f];
  const float* dq = a.dofs + e * (2 * WBC_NDOF);
  float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  f3 o = mk3(0.f, 0.f, 0.f);                                       // in trunk axes, relative to the trunk
  f3 ax[LC_LEG_JOINTS], og[LC_LEG_JOINTS];
  int dj[LC_LEG_JOINTS];
  float qd[LC_LEG_JOINTS];
#pragma unroll
  for (int k = 0; k < LC_LEG_JOINTS; ++k) {
    const int j = K.path[body][k];
    dj[k] = K.dof[j];
    qd[k] = dq[2 * dj[k] + 1];
    float Q[9];
    const f3 u = tree_joint_rot(K.axis[j], dq[2 * dj[k]], Q);
    ax[k] = tree_frame_step(E, o, Q, K.joint_xyz[j], u);
    og[k] = o;
  }
  bad = bad || !(lc_finite(qd[0]) && lc_finite(qd[1]) && lc_finite(qd[2]));
  const f3 fk = o + mat_mul(E, mk3(K.foot_off[f][0], K.foot_off[f][1], K.foot_off[f][2]));
  const f3 c0 = cross(ax[0], fk - og[0]), c1 = cross(ax[1], fk - og[1]), c2 = cross(ax[2], fk - og[2]);
  const f3 p = b + mat_mul(R, fk);
  const f3 pd = v + mat_mul(R, cross(wb, fk) + ((c0 * qd[0] + c1 * qd[1]) + c2 * qd[2]));
  const f3 w0 = mat_mul(R, c0), w1 = mat_mul(R, c1), w2 = mat_mul(R, c2);      // the columns of J_i
  bad = bad || !(lc_finite(p) && lc_finite(pd));

  // 2 weight
  float w = 1.f;
  if (a.stance) {
    const float s = a.stance[ef];
    bad = bad || !lc_finite(s);
    w = lc_clamp(s, 0.f, 1.f);
  }

  // 3 stance force
  f3 fs = mk3(0.f, 0.f, 0.f);
  if (a.forces) {
    const f3 fin = ld3(a.forces + ef * 3);
    bad = bad || !lc_finite(fin);
    fs = fin;
    if (a.clip) {
      fs.z = lc_clamp(fin.z, cfg.fz_min, cfg.fz_max);
      const float lim = cfg.mu * fs.z;
      fs.x = lc_clamp(fin.x, -lim, lim);
      fs.y = lc_clamp(fin.y, -lim, lim);
      if (w > 0.f && (fs.x != fin.x || fs.y != fin.y || fs.z != fin.z)) bits |= WBC_LEGCTL_INFO_FORCE_CLIPPED << f;
    }
  }

  // 4 swing force, 5 feedback torque
  f3 F = mk3(0.f, 0.f, 0.f), aref = F;
  if (a.swing_ref) {
    const float* sr = a.swing_ref + ef * 9;
    const f3 rp = ld3(sr), rv = ld3(sr + 3);
    bad = bad || !(lc_finite(rp) && lc_finite(rv));
    F = mk3(cfg.kp[0] * (rp.x - p.x) + cfg.kd[0] * (rv.x - pd.x), cfg.kp[1] * (rp.y - p.y) + cfg.kd[1] * (rv.y - pd.y),
            cfg.kp[2] * (rp.z - p.z) + cfg.kd[2] * (rv.z - pd.z));
    if (a.mass_matrix) { aref = ld3(sr + 6); bad = bad || !lc_finite(aref); }
  }
  const float sw = 1.f - w;
  const f3 G = F * sw - fs * w;
  float t0 = dot(w0, G), t1 = dot(w1, G), t2 = dot(w2, G);

  // 6 feed-forward
  if (a.mass_matrix) {
    f3 acc = aref;
    if (a.acc_bias) {
      const f3 ab = ld3(a.acc_bias + e * a.acc_stride + a.foot_rb[f] * 6);
      bad = bad || !lc_finite(ab);
      acc = aref - ab;
    }
    const float* M = a.mass_matrix + e * a.mm_stride;
    float Mi[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Mi[r * 3 + c] = M[(6 + dj[r]) * WBC_NCOL + 6 + dj[c]];
        bad = bad || !lc_finite(Mi[r * 3 + c]);
      }
    const float r0 = dot(w0, acc), r1 = dot(w1, acc), r2 = dot(w2, acc);
    const float d2 = cfg.damping * cfg.damping;
    const float a00 = dot(w0, w0) + d2, a10 = dot(w1, w0), a11 = dot(w1, w1) + d2, a20 = dot(w2, w0), a21 = dot(w2, w1), a22 = dot(w2, w2) + d2;
    const float l00 = sqrtf(a00), l10 = a10 / l00;
    const float p1 = a11 - l10 * l10, l11 = sqrtf(p1);
    const float l20 = a20 / l00, l21 = (a21 - l20 * l10) / l11;
    const float p2 = a22 - l20 * l20 - l21 * l21, l22 = sqrtf(p2);
    const float z0 = r0 / l00, z1 = (r1 - l10 * z0) / l11, z2 = (r2 - l20 * z0 - l21 * z1) / l22;
    const float y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = (z0 - l10 * y1 - l20 * y2) / l00;
    if (lc_pivot(a00) && lc_pivot(p1) && lc_pivot(p2) && lc_finite(y0) && lc_finite(y1) && lc_finite(y2)) {
      t0 += sw * ((Mi[0] * y0 + Mi[1] * y1) + Mi[2] * y2);
      t1 += sw * ((Mi[3] * y0 + Mi[4] * y1) + Mi[5] * y2);
      t2 += sw * ((Mi[6] * y0 + Mi[7] * y1) + Mi[8] * y2);
    } else bits |= WBC_LEGCTL_INFO_FF_SINGULAR << f;
  }

  // 7 leg joints
  if (a.tau_bias) {
    const float* tb = a.tau_bias + e * a.bias_stride + 6;
    const float b0 = tb[dj[0]], b1 = tb[dj[1]], b2 = tb[dj[2]];
    bad = bad || !(lc_finite(b0) && lc_finite(b1) && lc_finite(b2));
    t0 += b0; t1 += b1; t2 += b2;
  }
  const float kds = w * cfg.kd_stance;
  t0 -= kds * qd[0]; t1 -= kds * qd[1]; t2 -= kds * qd[2];

  // 8 arm: joints f and f + 4 of the six
  float ta[2] = {0.f, 0.f};
  int da[2] = {0, 0};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int j = f + 4 * r;
    if (j < LC_ARM_DOFS) {
      const int d = a.arm_dof[j];
      da[r] = d;
      const float q = dq[2 * d], qdot = dq[2 * d + 1];
      const float qdes = a.arm_q_des ? a.arm_q_des[e * LC_ARM_DOFS + j] : cfg.arm_q_default[j];
      const float tb = a.tau_bias ? a.tau_bias[e * a.bias_stride + 6 + d] : 0.f;
      bad = bad || !(lc_finite(q) && lc_finite(qdot) && lc_finite(qdes) && lc_finite(tb));
      ta[r] = (tb + cfg.kp_arm[j] * (qdes - q)) - cfg.kd_arm[j] * qdot;
      // 9 limit
      if (lc_limit(a, e, d, ta[r], bad)) bits |= WBC_LEGCTL_INFO_SATURATED << 4;
    }
  }
  // 9 limit, the leg
  bool sat = lc_limit(a, e, dj[0], t0, bad);
  sat = lc_limit(a, e, dj[1], t1, bad) || sat;
  sat = lc_limit(a, e, dj[2], t2, bad) || sat;
  if (sat) bits |= WBC_LEGCTL_INFO_SATURATED << f;
  bad = bad || !(lc_finite(t0) && lc_finite(t1) && lc_finite(t2) && lc_finite(ta[0]) && lc_finite(ta[1]) && lc_finite(G));

  // what the env's four feet share
  int vote = bad ? 1 : 0;
  vote |= __shfl_xor(vote, 1); vote |= __shfl_xor(vote, 2);
  bits |= __shfl_xor(bits, 1); bits |= __shfl_xor(bits, 2);
  const bool failed = vote != 0;
  if (!live) return;

  if (a.tau) {
    float* to = a.tau + e * WBC_NDOF;
    to[dj[0]] = failed ? 0.f : t0; to[dj[1]] = failed ? 0.f : t1; to[dj[2]] = failed ? 0.f : t2;
    to[da[0]] = failed ? 0.f : ta[0];
    if (f + 4 < LC_ARM_DOFS) to[da[1]] = failed ? 0.f : ta[1];
    else to[a.finger_dof[f + 4 - LC_ARM_DOFS]] = 0.f;
  }
  if (a.leg_force) st3(a.leg_force + ef * 3, failed ? mk3(0.f, 0.f, 0.f) : G);
  if (a.foot) {
    st3(a.foot + ef * 6, failed ? mk3(0.f, 0.f, 0.f) : p);
    st3(a.foot + ef * 6 + 3, failed ? mk3(0.f, 0.f, 0.f) : pd);
  }
  if (a.info && f == 0) a.info[e] = failed ? WBC_LEGCTL_INFO_FAILED : bits;
}

void wbc_legctl_launch(const EstConst& K, const wbc_leg_control_cfg& cfg, const LcArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_leg_control_kernel, dim3((a.n + LC_EPW - 1) / LC_EPW), dim3(64), 0, (hipStream_t)stream, K, cfg, a);
}
