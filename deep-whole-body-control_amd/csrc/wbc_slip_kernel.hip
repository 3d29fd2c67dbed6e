// wbc_slip_kernel.hip -- the kernel of wbc_sim_slip_detect (include/wbc_sim.h, whose comment is the text this kernel and
// tests/slip_reference.py both implement); its entry point and argument checks are with the other whole-body calls in wbc_arm_kernel.hip.
// A translation unit of its own: tests/test_identification.py pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_slip.h"

// ---- foot slip detection and friction estimate --------------------------------------------------------------------------------------------
// The contact detector's layout: all the work but two small sums is per foot, so lane = (env, foot): SL_EPW = 16 envs per 64-lane
// workgroup, a single wavefront, env `grp` on lanes 4 grp .. 4 grp + 3 (a launch whose env count is no multiple of SL_EPW repeats the last
// env on the idle groups and stores nothing from them). Each lane walks its own leg (tree_frame_step per joint, the three joints unrolled
// so that their axes and origins stay in registers) and owns its foot's eight floats of state. What an env shares -- the common-mode
// mean, W, sum w_i mu_i, the non-finite vote and the OR of the event bits -- goes through xor shuffles inside the 4-lane group, which
// leave every lane of the group with the same bits ((x_0 + x_1) + (x_2 + x_3) whichever lane adds). No LDS, no barrier, no scratch.
// SL_EPW = 64 is lane = env with the four legs walked in sequence (the same code, the per-foot values in unrolled arrays of four and
// the sums written out), kept for the measurement in DESIGN.md.
// Control flow around the shuffles is uniform; a failed env runs the same instructions and stores zeros. Every store follows the lane's
// last read of the state.

#define SL_SQRT2 1.41421356237309504880f

__device__ __forceinline__ bool sl_finite(float v) { return fabsf(v) <= 3.4e38f; }        // false for a NaN
__device__ __forceinline__ bool sl_finite(f3 v) { return sl_finite(v.x) && sl_finite(v.y) && sl_finite(v.z); }
__device__ __forceinline__ float sl_Phi(float x) { return 0.5f * (1.f + erff(x / SL_SQRT2)); }
__device__ __forceinline__ float sl_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// (x_0 + x_1) + (x_2 + x_3) over the env's four feet, the same bits on every lane of the env
__device__ __forceinline__ float sl_sum(const float (&v)[SL_FPL]) {
#if SL_FPL == 1
  float s = v[0];
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  return s;
#else
  return (v[0] + v[1]) + (v[2] + v[3]);
#endif
}
__device__ __forceinline__ int sl_or(int v) {
#if SL_FPL == 1
  v |= __shfl_xor(v, 1);
  v |= __shfl_xor(v, 2);
#endif
  return v;
}

extern "C" __global__ void __launch_bounds__(64) wbc_slip_detect_kernel(EstConst K, wbc_slip_cfg cfg, SlArgs a) {
  const int lane = threadIdx.x, grp = lane / SL_LPE, l = lane - grp * SL_LPE;
  const int eu = blockIdx.x * SL_EPW + grp;
  const bool live = eu < a.n;
  const size_t e = live ? eu : a.n - 1;
  const bool reset = a.reset_all || (a.reset_mask && a.reset_mask[e] != 0);

  // 1 kinematics: the trunk's rotation from the quaternion, normalised; the trunk's velocities; per foot the leg walk with every joint's
  // axis and origin kept, and the foot origin's world velocity
  const float* qr = a.quat + e * a.quat_stride;
  const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
  const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
  float R[9];
  quat_to_mat(qu, R);
  const f3 v = ld3(a.vel + e * a.vel_stride), wr = ld3(a.ang + e * a.ang_stride);
  const f3 wb = a.ang_world ? matT_mul(R, wr) : wr;
  const float* dq = a.dofs + e * (2 * WBC_NDOF);

  int bits = 0;
  bool bad = !(sl_finite(v) && sl_finite(wr));

  float ux[SL_FPL], uy[SL_FPL], uz[SL_FPL], cc[SL_FPL], cw[SL_FPL], one[SL_FPL];
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) {
    const int f = l + j;
    const int body = K.foot_body[f];
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 o = mk3(0.f, 0.f, 0.f);                                     // in trunk axes, relative to the trunk
    f3 ax[SL_LEG_JOINTS], og[SL_LEG_JOINTS];
    float qd[SL_LEG_JOINTS];
#pragma unroll
    for (int k = 0; k < SL_LEG_JOINTS; ++k) {
      const int jn = K.path[body][k];
      const int d = K.dof[jn];
      qd[k] = dq[2 * d + 1];
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[jn], dq[2 * d], Q);
      ax[k] = tree_frame_step(E, o, Q, K.joint_xyz[jn], u);
      og[k] = o;
    }
    bad = bad || !(sl_finite(qd[0]) && sl_finite(qd[1]) && sl_finite(qd[2]));
    const f3 fk = o + mat_mul(E, mk3(K.foot_off[f][0], K.foot_off[f][1], K.foot_off[f][2]));
    const f3 c0 = cross(ax[0], fk - og[0]), c1 = cross(ax[1], fk - og[1]), c2 = cross(ax[2], fk - og[2]);
    const f3 u = v + mat_mul(R, cross(wb, fk) + ((c0 * qd[0] + c1 * qd[1]) + c2 * qd[2]));
    bad = bad || !sl_finite(u);
    ux[j] = u.x; uy[j] = u.y; uz[j] = u.z;

    // 3 standing
    const float cr = a.contact[e * WBC_NFEET + f];
    bad = bad || !sl_finite(cr);
    cc[j] = sl_clamp(cr, 0.f, 1.f);
    const bool stand = cc[j] >= cfg.c_on;
    cw[j] = stand ? cc[j] : 0.f;
    one[j] = stand ? 1.f : 0.f;
  }

  // 4 common mode: the mean velocity of the standing feet, weighted by their contact
  const float Sw = sl_sum(cw), cnt = sl_sum(one);
  float tmp[SL_FPL];
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) tmp[j] = cw[j] * ux[j];
  const float sx = sl_sum(tmp);
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) tmp[j] = cw[j] * uy[j];
  const float sy = sl_sum(tmp);
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) tmp[j] = cw[j] * uz[j];
  const float sz = sl_sum(tmp);
  const bool cm = cnt >= 2.f && Sw > 0.f;
  const f3 ub = cm ? mk3(sx / Sw, sy / Sw, sz / Sw) : mk3(0.f, 0.f, 0.f);

  // per foot: 2 reset, 3 touchdown, 4 the tangential speed, 5 evidence, 6 flag, 7 friction
  float p[SL_FPL], s[SL_FPL], t[SL_FPL], cp[SL_FPL], d[SL_FPL], mu[SL_FPL], w[SL_FPL], m[SL_FPL], sp[SL_FPL];
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) {
    const int f = l + j;
    const size_t ef = e * WBC_NFEET + f;
    const float* st = a.state + ef * WBC_SLIP_NS;
    const bool stand = one[j] != 0.f;
    if (reset) {
      p[j] = 0.f; s[j] = 0.f; t[j] = cfg.t_dwell; cp[j] = 0.f; d[j] = 0.f; w[j] = 0.f; m[j] = 0.f; mu[j] = cfg.mu_prior;
      if (a.mu_init) { mu[j] = a.mu_init[ef]; bad = bad || !sl_finite(mu[j]); }
    } else {
      const float s1 = st[1], s3 = st[3];
      p[j] = st[0]; s[j] = s1 != 0.f ? 1.f : 0.f; t[j] = st[2]; cp[j] = s3 != 0.f ? 1.f : 0.f;
      d[j] = st[4]; mu[j] = st[5]; w[j] = st[6]; m[j] = st[7];
      bad = bad || !(sl_finite(p[j]) && sl_finite(s1) && sl_finite(t[j]) && sl_finite(s3) && sl_finite(d[j]) && sl_finite(mu[j]) &&
                     sl_finite(w[j]) && sl_finite(m[j]));
    }
    if (stand && cp[j] == 0.f) d[j] = 0.f;

    f3 nrm = mk3(0.f, 0.f, 1.f);
    if (a.normal) {
      const f3 nn = ld3(a.normal + ef * 3);
      nrm = nn * (1.f / sqrtf(dot(nn, nn)));
      bad = bad || !sl_finite(nrm);
    }
    const f3 g = mk3(ux[j], uy[j], uz[j]) - ub * cfg.common_mode;
    const f3 gt = g - nrm * dot(nrm, g);
    sp[j] = sqrtf(dot(gt, gt));

    const float P = stand ? cc[j] * sl_Phi((sp[j] - cfg.v_slip) / cfg.sigma_v) : 0.f;
    p[j] = p[j] + cfg.alpha * (P - p[j]);

    t[j] = t[j] + cfg.dt;
    if (!stand && s[j] != 0.f) { s[j] = 0.f; t[j] = 0.f; bits |= WBC_SLIP_INFO_END << f; }
    else if (stand && s[j] == 0.f && p[j] >= cfg.p_on && t[j] >= cfg.t_dwell) { s[j] = 1.f; t[j] = 0.f; bits |= WBC_SLIP_INFO_START << f; }
    else if (s[j] != 0.f && p[j] <= cfg.p_off && t[j] >= cfg.t_dwell) { s[j] = 0.f; t[j] = 0.f; bits |= WBC_SLIP_INFO_END << f; }
    d[j] = d[j] + (s[j] != 0.f ? sp[j] * cfg.dt : 0.f);
    cp[j] = stand ? 1.f : 0.f;
    if (s[j] != 0.f) bits |= WBC_SLIP_INFO_SLIPPING << f;

    if (a.foot_force) {
      const f3 ff = ld3(a.foot_force + ef * 3);
      bad = bad || !sl_finite(ff);
      const float fn = dot(nrm, ff);
      const f3 fv = ff - nrm * fn;
      const float ft = sqrtf(dot(fv, fv));
      const bool valid = stand && fn >= cfg.fn_min;
      const float rho = ft / fn;
      m[j] = cfg.gamma * m[j];
      if (valid && s[j] == 0.f) m[j] = fmaxf(m[j], rho);
      w[j] = cfg.gamma * w[j];
      if (valid && s[j] != 0.f && p[j] > 0.f) {
        w[j] = w[j] + p[j];
        mu[j] = mu[j] + (p[j] / w[j]) * (rho - mu[j]);
      }
    }
    if (w[j] >= cfg.w_min) bits |= WBC_SLIP_INFO_MU_VALID << f;
    bad = bad || !(sl_finite(p[j]) && sl_finite(t[j]) && sl_finite(d[j]) && sl_finite(mu[j]) && sl_finite(w[j]) && sl_finite(m[j]));
  }

  // 8 fuse
  const float W = sl_sum(w);
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) tmp[j] = w[j] * mu[j];
  const float Swm = sl_sum(tmp);
  const float mue = W >= cfg.w_min ? Swm / W : cfg.mu_prior;

  // what the env's feet share
  const bool failed = sl_or(bad ? 1 : 0) != 0;
  bits = sl_or(bits);
  if (!live) return;

  // 9 outputs
#pragma unroll
  for (int j = 0; j < SL_FPL; ++j) {
    const int f = l + j;
    const size_t ef = e * WBC_NFEET + f;
    if (!failed) {
      float* st = a.state + ef * WBC_SLIP_NS;
      st[0] = p[j]; st[1] = s[j]; st[2] = t[j]; st[3] = cp[j]; st[4] = d[j]; st[5] = mu[j]; st[6] = w[j]; st[7] = m[j];
    }
    const float mraw = w[j] >= cfg.w_min ? mu[j] : mue;
    if (a.prob) a.prob[ef] = failed ? 0.f : p[j];
    if (a.slip) a.slip[ef] = (!failed && s[j] != 0.f) ? 1 : 0;
    if (a.weight) a.weight[ef] = failed ? 0.f : cc[j] * (1.f - p[j]);
    if (a.foot_vel) st3(a.foot_vel + ef * 3, failed ? mk3(0.f, 0.f, 0.f) : mk3(ux[j], uy[j], uz[j]));
    if (a.speed) a.speed[ef] = failed ? 0.f : sp[j];
    if (a.distance) a.distance[ef] = failed ? 0.f : d[j];
    if (a.mu) a.mu[ef] = failed ? 0.f : sl_clamp(cfg.mu_scale * mraw, cfg.mu_min, cfg.mu_max);
    if (a.mu_lower) a.mu_lower[ef] = failed ? 0.f : m[j];
  }
  if (l != 0) return;
  if (a.mu_env) { a.mu_env[e * 2] = failed ? 0.f : mue; a.mu_env[e * 2 + 1] = failed ? 0.f : W; }
  if (a.info) a.info[e] = failed ? WBC_SLIP_INFO_FAILED : ((reset ? WBC_SLIP_INFO_RESET : 0) | (a.foot_force ? 0 : WBC_SLIP_INFO_NO_FORCE) | bits);
}

void wbc_slip_launch(const EstConst& K, const wbc_slip_cfg& cfg, const SlArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_slip_detect_kernel, dim3((a.n + SL_EPW - 1) / SL_EPW), dim3(64), 0, (hipStream_t)stream, K, cfg, a);
}
