// wbc_contact_kernel.hip -- the kernel of wbc_sim_contact_detect (include/wbc_sim.h, whose comment is the text this kernel and
// tests/contact_reference.py both implement); its entry point and argument checks are with the other whole-body calls in wbc_arm_kernel.hip.
// A translation unit of its own: tests/test_identification.py pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_contact.h"

// ---- contact detection from proprioception -----------------------------------------------------------------------------------------------
// All the work is per foot, so lane = (env, foot): CT_EPW = 16 envs per 64-lane workgroup, a single wavefront, env `grp` on lanes
// 4 grp .. 4 grp + 3 (a launch whose env count is no multiple of CT_EPW repeats the last env on the idle groups and stores nothing from
// them). Each lane walks its own leg (tree_frame_step per joint, the three joints unrolled so that their axes and origins stay in
// registers), solves its own 3 x 3 system and owns its foot's four floats of state. What an env shares -- the non-finite vote and the OR of
// the feet's event bits into info -- goes through two xor shuffles inside the 4-lane group. No LDS, no barrier, no scratch.
// CT_EPW = 2 is the estimator's layout (the feet on lanes 0..3 of each 32-lane group, 56 lanes idle), kept for the measurement in DESIGN.md.
// Control flow around the shuffles is uniform; a failed env runs the same instructions and stores zeros. Every store follows the lane's
// last read of the state.

#define CT_SQRT2 1.41421356237309504880f

__device__ __forceinline__ bool ct_finite(float v) { return fabsf(v) <= 3.4e38f; }        // false for a NaN
__device__ __forceinline__ bool ct_finite(f3 v) { return ct_finite(v.x) && ct_finite(v.y) && ct_finite(v.z); }
__device__ __forceinline__ bool ct_pivot(float v) { return v > 0.f && v <= 3.4e38f; }
__device__ __forceinline__ float ct_Phi(float x) { return 0.5f * (1.f + erff(x / CT_SQRT2)); }

extern "C" __global__ void __launch_bounds__(64) wbc_contact_detect_kernel(EstConst K, wbc_contact_cfg cfg, CtArgs a) {
  const int lane = threadIdx.x, grp = lane / CT_LPE, l = lane - grp * CT_LPE;
  const int eu = blockIdx.x * CT_EPW + grp;
  const bool live = eu < a.n, act = l < WBC_NFEET;
  const size_t e = live ? eu : a.n - 1;
  const int f = l & (WBC_NFEET - 1);
  const size_t ef = e * WBC_NFEET + f;
  const bool reset = a.reset_all || (a.reset_mask && a.reset_mask[e] != 0);

  int bits = 0;
  bool bad = false, stance = false;
  float p = 0.f, c = 0.f, t = 0.f, Pphi = 0.f, Pz = 0.f, Pf = 0.f, P = 0.f;
  f3 force = mk3(0.f, 0.f, 0.f);
  if (act) {
    // 1 reset
    const float* st = a.state + ef * 4;
    if (reset) { p = a.p_init ? a.p_init[ef] : 1.f; c = p >= 0.5f ? 1.f : 0.f; t = cfg.t_dwell; }
    else { p = st[0]; c = st[1] != 0.f ? 1.f : 0.f; t = st[2]; bad = !ct_finite(st[1]); }
    bad = bad || !(ct_finite(p) && ct_finite(t));

    // 2 kinematics: the trunk's rotation from the quaternion, normalised; the leg walk with every joint's axis and origin kept
    const float* qr = a.quat + e * a.quat_stride;
    const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
    const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
    float R[9];
    quat_to_mat(qu, R);
    const f3 b = ld3(a.pos + e * a.pos_stride);
    const int body = K.foot_body[f];
    const float* dq = a.dofs + e * (2 * WBC_NDOF);
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 o = mk3(0.f, 0.f, 0.f);                                     // in trunk axes, relative to the trunk
    f3 ax[CT_LEG_JOINTS], og[CT_LEG_JOINTS];
    int dj[CT_LEG_JOINTS];
#pragma unroll
    for (int k = 0; k < CT_LEG_JOINTS; ++k) {
      const int j = K.path[body][k];
      dj[k] = K.dof[j];
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[j], dq[2 * dj[k]], Q);
      ax[k] = tree_frame_step(E, o, Q, K.joint_xyz[j], u);
      og[k] = o;
    }
    const f3 fk = o + mat_mul(E, mk3(K.foot_off[f][0], K.foot_off[f][1], K.foot_off[f][2]));
    const f3 pw = b + mat_mul(R, fk);
    bad = bad || !ct_finite(pw);

    // 3 force
    bool have_force = false;
    if (a.foot_force) {
      force = ld3(a.foot_force + ef * 3);
      bad = bad || !ct_finite(force);
      have_force = true;
    } else if (a.tau_ext) {
      const float* tr = a.tau_ext + e * a.tau_stride + 6;
      const float t0 = tr[dj[0]], t1 = tr[dj[1]], t2 = tr[dj[2]];
      bad = bad || !(ct_finite(t0) && ct_finite(t1) && ct_finite(t2));
      const f3 w0 = mat_mul(R, cross(ax[0], fk - og[0])), w1 = mat_mul(R, cross(ax[1], fk - og[1])), w2 = mat_mul(R, cross(ax[2], fk - og[2]));
      const float d2 = cfg.damping * cfg.damping;
      const float a00 = dot(w0, w0) + d2, a10 = dot(w1, w0), a11 = dot(w1, w1) + d2, a20 = dot(w2, w0), a21 = dot(w2, w1), a22 = dot(w2, w2) + d2;
      const float l00 = sqrtf(a00), l10 = a10 / l00;
      const float p1 = a11 - l10 * l10, l11 = sqrtf(p1);
      const float l20 = a20 / l00, l21 = (a21 - l20 * l10) / l11;
      const float p2 = a22 - l20 * l20 - l21 * l21, l22 = sqrtf(p2);
      const float z0 = t0 / l00, z1 = (t1 - l10 * z0) / l11, z2 = (t2 - l20 * z0 - l21 * z1) / l22;
      const float y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = (z0 - l10 * y1 - l20 * y2) / l00;
      const f3 fs = (w0 * y0 + w1 * y1) + w2 * y2;
      if (ct_pivot(a00) && ct_pivot(p1) && ct_pivot(p2) && ct_finite(fs)) force = fs;
      else bits |= WBC_CONTACT_INFO_FORCE_SINGULAR << f;
      have_force = true;
    }

    // 4 terms, 5 fusion
    float num = 0.f, den = 0.f, s = 0.f;
    bool sched = true;
    if (a.phase) {
      const float ph = a.phase[e * a.phase_stride];
      bad = bad || !ct_finite(ph);
      const float x0 = ph + cfg.offset[f];
      const float phi = x0 - floorf(x0);
      sched = cfg.duty >= 1.f || phi < cfg.duty;
      s = sched ? phi / cfg.duty : (phi - cfg.duty) / (1.f - cfg.duty);
      const float k = cfg.sigma_phase * CT_SQRT2;
      const float G = 0.5f * (erff(s / k) + erff((1.f - s) / k));
      Pphi = sched ? G : 1.f - G;
      num += Pphi / cfg.var_phase; den += 1.f / cfg.var_phase;
    }
    if (a.ground) {
      const float g = a.ground[ef];
      bad = bad || !ct_finite(g);
      Pz = ct_Phi((cfg.mu_z - (pw.z - g)) / cfg.sigma_z);
      num += Pz / cfg.var_z; den += 1.f / cfg.var_z;
    }
    if (have_force) {
      f3 nrm = mk3(0.f, 0.f, 1.f);
      if (a.normal) {
        const f3 nn = ld3(a.normal + ef * 3);
        nrm = nn * (1.f / sqrtf(dot(nn, nn)));
        bad = bad || !ct_finite(nrm);
      }
      Pf = ct_Phi((dot(force, nrm) - cfg.mu_f) / cfg.sigma_f);
      num += Pf / cfg.var_f; den += 1.f / cfg.var_f;
    }
    P = num / den;
    p = p + cfg.alpha * (P - p);

    // 6 flag
    t = t + cfg.dt;
    if (c == 0.f && p >= cfg.p_on && t >= cfg.t_dwell) { c = 1.f; t = 0.f; bits |= WBC_CONTACT_INFO_TOUCHDOWN << f; }
    else if (c != 0.f && p <= cfg.p_off && t >= cfg.t_dwell) { c = 0.f; t = 0.f; bits |= WBC_CONTACT_INFO_LIFTOFF << f; }

    // 7 events
    stance = c != 0.f;
    if (a.phase) {
      const bool early = !sched && s >= cfg.early_min && c != 0.f, late = sched && s >= cfg.late_min && c == 0.f;
      if (early) bits |= WBC_CONTACT_INFO_EARLY << f;
      if (late) bits |= WBC_CONTACT_INFO_LATE << f;
      stance = (sched || early) && !late;
    }
  }

  // what the env's four feet share
  int vote = bad ? 1 : 0;
  vote |= __shfl_xor(vote, 1); vote |= __shfl_xor(vote, 2);
  bits |= __shfl_xor(bits, 1); bits |= __shfl_xor(bits, 2);
  const bool failed = vote != 0;
  if (!live || !act) return;

  if (failed) { p = 0.f; c = 0.f; stance = false; force = mk3(0.f, 0.f, 0.f); Pphi = 0.f; Pz = 0.f; Pf = 0.f; P = 0.f; }
  else {
    float* st = a.state + ef * 4;
    st[0] = p; st[1] = c; st[2] = t; st[3] = 0.f;
  }
  if (a.prob) a.prob[ef] = p;
  if (a.contact) a.contact[ef] = c != 0.f ? 1 : 0;
  if (a.stance) a.stance[ef] = stance ? 1 : 0;
  if (a.force) st3(a.force + ef * 3, force);
  if (a.terms) { float* tm = a.terms + ef * 4; tm[0] = Pphi; tm[1] = Pz; tm[2] = Pf; tm[3] = P; }
  if (a.info && f == 0) a.info[e] = failed ? WBC_CONTACT_INFO_FAILED : ((reset ? WBC_CONTACT_INFO_RESET : 0) | bits);
}

void wbc_contact_launch(const EstConst& K, const wbc_contact_cfg& cfg, const CtArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_contact_detect_kernel, dim3((a.n + CT_EPW - 1) / CT_EPW), dim3(64), 0, (hipStream_t)stream, K, cfg, a);
}
