// wbc_footstep_kernel.hip -- the kernel of wbc_sim_footstep_plan (include/wbc_sim.h, whose comment is the text this kernel and
// tests/footstep_reference.py both implement); its entry point and argument checks are with the other whole-body calls in wbc_arm_kernel.hip.
// A translation unit of its own: tests/test_identification.py pins the number of kernels in wbc_arm_kernel.hip's code object.
#include "wbc_footstep.h"

// ---- gait clock, footholds and swing references ----------------------------------------------------------------------------------------
// One env per 64-lane workgroup, a single wavefront:
//  1) lane i < 4 walks leg i as wbc_leg_odometry_kernel does, applies the reset, the clock and the flag transitions of foot i, and forms its
//     nominal foothold (a standing foot also queries h(nom) there); lanes < 32 test the state's floats, every lane the env's other inputs;
//  2) the terrain search (fs_search): up to 16 candidates (search_radius <= 1) the four feet at once on 16 lanes each; more, the searching
//     feet in sequence, lane = candidate. Five terrain queries per candidate, then the argmin on (cost, index) by xor shuffles;
//  3) lane i < 4 forms the swing reference and stores foot i's outputs and state; lane 0 the phase and info;
//  4) lane = stage * 4 + foot: the schedule and the per-stage foot positions; a swing stage finds its source stage in a ballot of the stance flags.
// Control flow around the shuffles and barriers is uniform; a failed env runs the same instructions and stores zeros. Every store follows the
// last read of the state.

#define FS_INF __builtin_huge_valf()

// The step kernel's terrain_query (wbc_step_kernel.hip) on this kernel's constants: the same triangle choice, clamping and plane fallback. A
// copy, so that the step kernel's instructions stay the parent's; keep the two in step.
__device__ __forceinline__ void fs_terrain_query(const FsConst& K, float x, float y, float* h, f3* n) {
  if (!K.hf) { *h = K.ground_z; *n = mk3(0.f, 0.f, 1.f); return; }
  const float fx = (x - K.hf_t[0]) / K.hf_hs, fy = (y - K.hf_t[1]) / K.hf_hs;
  long long ix = (long long)fx, iy = (long long)fy;
  ix = ix < 0 ? 0 : ix; iy = iy < 0 ? 0 : iy;
  ix = ix > K.hf_rows - 2 ? K.hf_rows - 2 : ix;
  iy = iy > K.hf_cols - 2 ? K.hf_cols - 2 : iy;
  const float u = clampf(fx - (float)ix, 0.f, 1.f), v = clampf(fy - (float)iy, 0.f, 1.f);
  const int16_t* H = K.hf;
  const int cols = K.hf_cols;
  const float h00 = H[ix * cols + iy] * K.hf_vs, h10 = H[(ix + 1) * cols + iy] * K.hf_vs;
  const float h01 = H[ix * cols + iy + 1] * K.hf_vs, h11 = H[(ix + 1) * cols + iy + 1] * K.hf_vs;
  float dhdx, dhdy;
  if (u >= v) { dhdx = h10 - h00; dhdy = h11 - h10; } else { dhdy = h01 - h00; dhdx = h11 - h01; }
  *h = h00 + u * dhdx + v * dhdy + K.hf_t[2];
  const float gx = dhdx / K.hf_hs, gy = dhdy / K.hf_hs;
  const float inv = 1.f / sqrtf(gx * gx + gy * gy + 1.f);
  *n = mk3(-gx * inv, -gy * inv, inv);
}

__device__ __forceinline__ bool fs_finite(float v) { return fabsf(v) <= 3.4e38f; }        // false for a NaN
__device__ __forceinline__ bool fs_finite(f3 v) { return fs_finite(v.x) && fs_finite(v.y) && fs_finite(v.z); }

// b(s) = s^3 (10 - 15 s + 6 s^2) and its first two derivatives.
__device__ __forceinline__ void fs_bump(float s, float& b, float& b1, float& b2) {
  b = s * s * s * (10.f - 15.f * s + 6.f * s * s);
  b1 = 30.f * s * s * (1.f - s) * (1.f - s);
  b2 = 60.f * s * (1.f - s) * (1.f - 2.f * s);
}

// The cost of candidate c of a search around (nx, ny); FS_INF where it is rejected. Its position and height by reference.
__device__ __forceinline__ float fs_candidate(const FsConst& K, const wbc_footstep_cfg& cfg, int c, float nx, float ny, float& cx, float& cy, float& h) {
  const int side = 2 * cfg.search_radius + 1;
  const int ia = c / side, ib = c - ia * side;
  const float dx = (float)(ia - cfg.search_radius) * cfg.search_step, dy = (float)(ib - cfg.search_radius) * cfg.search_step;
  cx = nx + dx; cy = ny + dy;
  f3 n, nn;
  fs_terrain_query(K, cx, cy, &h, &n);
  float h1, h2, h3, h4;
  fs_terrain_query(K, cx + cfg.probe_radius, cy, &h1, &nn);
  fs_terrain_query(K, cx - cfg.probe_radius, cy, &h2, &nn);
  fs_terrain_query(K, cx, cy + cfg.probe_radius, &h3, &nn);
  fs_terrain_query(K, cx, cy - cfg.probe_radius, &h4, &nn);
  const float rough = fmaxf(fmaxf(fabsf(h1 - h), fabsf(h2 - h)), fmaxf(fabsf(h3 - h), fabsf(h4 - h)));
  if (rough > cfg.rough_max || n.z < cfg.nz_min) return FS_INF;
  return cfg.w_dist * (dx * dx + dy * dy) + cfg.w_rough * (rough * rough) + cfg.w_slope * (1.f - n.z);
}

// The terrain search of every foot flagged in sSearch around its nominal foothold sN, LPF lanes per foot: LPF = 64 the searching feet in
// sequence, lane = candidate; LPF = 16 the four feet at once, a lane taking candidates l, l + 16, ... . The argmin on (cost, index) by xor
// shuffles inside the LPF-lane group carries the winner's position and height along, so they are the bits its own lane computed. Leaves the
// target in sT and sNoSafe = 1 where every candidate was rejected. Every lane of a group takes the same path around the shuffles.
template <int LPF>
__device__ __forceinline__ void fs_search(const FsConst& K, const wbc_footstep_cfg& cfg, int lane, const int* sSearch, const float (*sN)[2],
                                          float (*sT)[3], int* sNoSafe) {
  constexpr int GROUPS = 64 / LPF;
  const int g = lane / LPF, l = lane - g * LPF;
  const int side = 2 * cfg.search_radius + 1, ncand = side * side;
#pragma nounroll
  for (int f0 = 0; f0 < WBC_NFEET; f0 += GROUPS) {
    const int f = f0 + g;
    const bool does = sSearch[f] != 0;
    if (GROUPS == 1 && !does) continue;                            // uniform: one foot per round
    const float nx = sN[f][0], ny = sN[f][1];
    float best = FS_INF, bx = nx, by = ny, bh = 0.f;
    int bi = ncand;
    if (does) {
#pragma nounroll
      for (int c = l; c < ncand; c += LPF) {
        float cx, cy, h;
        const float cost = fs_candidate(K, cfg, c, nx, ny, cx, cy, h);
        if (cost < best) { best = cost; bi = c; bx = cx; by = cy; bh = h; }
      }
    }
#pragma unroll
    for (int off = LPF / 2; off >= 1; off >>= 1) {
      const float ob = __shfl_xor(best, off), ox = __shfl_xor(bx, off), oy = __shfl_xor(by, off), oh = __shfl_xor(bh, off);
      const int oi = __shfl_xor(bi, off);
      if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; bx = ox; by = oy; bh = oh; }
    }
    if (l == 0 && does) {
      if (best < FS_INF) {
        sT[f][0] = bx; sT[f][1] = by; sT[f][2] = bh;
      } else {                                                     // no safe candidate: the nominal on the terrain
        float h;
        f3 nn;
        fs_terrain_query(K, nx, ny, &h, &nn);
        sT[f][0] = nx; sT[f][1] = ny; sT[f][2] = h;
        sNoSafe[f] = 1;
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(64) wbc_footstep_plan_kernel(FsConst K, wbc_footstep_cfg cfg, FsArgs a) {
  __shared__ float sP[WBC_NFEET][6];                               // p_i, pd_i
  __shared__ float sN[WBC_NFEET][2];                               // the nominal foothold's xy
  __shared__ int sSearch[WBC_NFEET];                               // the foot searches in this call
  __shared__ float sT[WBC_NFEET][3];                               // what the search chose
  __shared__ int sNoSafe[WBC_NFEET];
  __shared__ float sF[WBC_NFEET][3];                               // the foothold output
  const int lane = threadIdx.x;
  const size_t e = blockIdx.x;
  const int H = cfg.horizon;

  // uniform: the trunk's state, the command, the phase
  const f3 b = ld3(a.pos + e * a.pos_stride), v = ld3(a.vel + e * a.vel_stride);
  const float* qr = a.quat + e * a.quat_stride;
  const float qn = 1.f / sqrtf(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
  const float qu[4] = {qr[0] * qn, qr[1] * qn, qr[2] * qn, qr[3] * qn};
  float R[9];
  quat_to_mat(qu, R);
  const f3 ww = ld3(a.root + e * 26 + 10);
  const f3 wb = matT_mul(R, ww);
  const float cmdx = a.vel_cmd ? a.vel_cmd[e * 2] : 0.f, cmdy = a.vel_cmd ? a.vel_cmd[e * 2 + 1] : 0.f;
  const float wz = a.yaw_rate ? a.yaw_rate[e] : 0.f;
  const bool reset = a.reset_all || (a.reset_mask && a.reset_mask[e] != 0);
  float* st = a.state + e * WBC_FOOTSTEP_NS;
  const float phase = reset ? (a.phase_init ? a.phase_init[e] : 0.f) : st[0];
  bool bad = !(fs_finite(b) && fs_finite(v) && fs_finite(ww) && fs_finite(qn) && fs_finite(qu[0]) && fs_finite(qu[1]) && fs_finite(qu[2]) &&
               fs_finite(qu[3]) && fs_finite(cmdx) && fs_finite(cmdy) && fs_finite(wz) && fs_finite(phase));
  if (!reset && lane < WBC_FOOTSTEP_NS) bad = bad || !fs_finite(st[lane]);

  const bool always = cfg.duty >= 1.f;
  const float Tst = cfg.duty * cfg.period, Tsw = (1.f - cfg.duty) * cfg.period;
  const float hn = sqrtf(R[0] * R[0] + R[3] * R[3]);
  const float ch = hn > 0.f ? R[0] / hn : 1.f, sh = hn > 0.f ? R[3] / hn : 0.f;
  const float vcx = ch * cmdx - sh * cmdy, vcy = sh * cmdx + ch * cmdy;

  // per foot, lanes 0..3
  f3 p = mk3(0.f, 0.f, 0.f), pd = p, lift = p, target = p;
  float flag = 0.f, s = 0.f, nomx = 0.f, nomy = 0.f, nomh = 0.f;
  bool stand = true, lifted = false, search = false;
  if (lane < WBC_NFEET) {
    const int body = K.foot_body[lane];
    const float* dq = a.dofs + e * (2 * WBC_NDOF);
    float E[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    f3 o = mk3(0.f, 0.f, 0.f), w = o, vo = o;                      // in trunk axes, relative to the trunk: origin, angular velocity, the origin's velocity
#pragma nounroll
    for (int k = 0; k < WBC_MAX_DEPTH; ++k) {
      const int j = K.path[body][k];
      if (j < 0) break;
      const int d = K.dof[j];
      vo = vo + cross(w, mat_mul(E, mk3(K.joint_xyz[j][0], K.joint_xyz[j][1], K.joint_xyz[j][2])));
      float Q[9];
      const f3 u = tree_joint_rot(K.axis[j], dq[2 * d], Q);
      const f3 Sw = tree_frame_step(E, o, Q, K.joint_xyz[j], u);
      w = w + Sw * dq[2 * d + 1];
    }
    const f3 off = mat_mul(E, mk3(K.foot_off[lane][0], K.foot_off[lane][1], K.foot_off[lane][2]));
    const f3 fk = o + off;
    p = b + mat_mul(R, fk);
    pd = v + mat_mul(R, cross(wb, fk) + (vo + cross(w, off)));
    bad = bad || !(fs_finite(p) && fs_finite(pd));
    st3(sP[lane], p); st3(sP[lane] + 3, pd);
    // reset, clock, transitions
    const float* sf = st + 4 + 7 * lane;
    if (reset) { lift = p; target = p; flag = 0.f; }
    else { lift = ld3(sf); target = ld3(sf + 3); flag = sf[6]; }
    const float x0 = phase + cfg.offset[lane];
    const float phi = x0 - floorf(x0);
    stand = always || phi < cfg.duty;
    s = stand ? 0.f : (phi - cfg.duty) / (1.f - cfg.duty);
    if (!stand && flag == 0.f) { lift = p; flag = 1.f; lifted = true; }
    if (stand && flag != 0.f) { flag = 0.f; target = p; }
    // the nominal foothold
    const float t = stand ? (always ? 0.f : (cfg.duty - phi) * cfg.period + Tsw) : (1.f - s) * Tsw;
    float sa, ca;
    sincosf(wz * t, &sa, &ca);
    const float ct = ch * ca - sh * sa, stt = sh * ca + ch * sa;
    const float ox = cfg.stance_offset[lane][0], oy = cfg.stance_offset[lane][1];
    const float hipx = b.x + vcx * t + (ct * ox - stt * oy), hipy = b.y + vcy * t + (stt * ox + ct * oy);
    float ax = 0.5f * Tst * v.x + cfg.k_v * (v.x - vcx) + K.k_c * (v.y * wz);
    float ay = 0.5f * Tst * v.y + cfg.k_v * (v.y - vcy) - K.k_c * (v.x * wz);
    const float len = sqrtf(ax * ax + ay * ay);
    if (len > cfg.max_reach) { const float sc = cfg.max_reach / len; ax *= sc; ay *= sc; }
    nomx = hipx + ax; nomy = hipy + ay;
    search = !stand && s < cfg.latch;
    sN[lane][0] = nomx; sN[lane][1] = nomy;
  }
  const bool failed = __ballot(bad) != 0ull;
  if (lane < WBC_NFEET) {
    sSearch[lane] = (search && !failed) ? 1 : 0;
    sNoSafe[lane] = 0;
    if (stand && !failed) {                                       // a standing foot's foothold: the nominal on the terrain, one query
      f3 nn;
      fs_terrain_query(K, nomx, nomy, &nomh, &nn);
    }
  }
  __syncthreads();

  // the terrain search
  {
    const int side = 2 * cfg.search_radius + 1;
#if FS_LPF == 0
    if (side * side <= 16) fs_search<16>(K, cfg, lane, sSearch, sN, sT, sNoSafe);
    else fs_search<64>(K, cfg, lane, sSearch, sN, sT, sNoSafe);
#else
    fs_search<FS_LPF>(K, cfg, lane, sSearch, sN, sT, sNoSafe);
#endif
  }
  __syncthreads();

  // the swing reference, foot i's outputs and its state
  bool nosafe = false;
  if (lane < WBC_NFEET) {
    if (sSearch[lane]) { target = ld3(sT[lane]); nosafe = sNoSafe[lane] != 0; }
    f3 rp = p, rv = mk3(0.f, 0.f, 0.f), ra = rv, sacc = rv;
    if (!stand) {
      const float sd = 1.f / Tsw;
      float bb, b1, b2;
      fs_bump(s, bb, b1, b2);
      const float dx = target.x - lift.x, dy = target.y - lift.y;
      rp.x = lift.x + dx * bb; rp.y = lift.y + dy * bb;
      rv.x = dx * (b1 * sd); rv.y = dy * (b1 * sd);
      ra.x = dx * (b2 * sd * sd); ra.y = dy * (b2 * sd * sd);
      const float za = fmaxf(lift.z, target.z) + cfg.swing_height;
      const bool up = s < 0.5f;
      fs_bump(up ? 2.f * s : 2.f * s - 1.f, bb, b1, b2);
      const float z0 = up ? lift.z : za, dz = up ? za - lift.z : target.z - za;
      rp.z = z0 + dz * bb;
      rv.z = dz * (b1 * (2.f * sd));
      ra.z = dz * (b2 * (2.f * sd) * (2.f * sd));
      sacc = ra + (rp - p) * cfg.kp + (rv - pd) * cfg.kd;
    }
    f3 fh = stand ? mk3(nomx, nomy, nomh) : target;
    if (failed) { rv = mk3(0.f, 0.f, 0.f); rp = rv; ra = rv; sacc = rv; fh = rv; }
    st3(sF[lane], fh);
    const size_t ef = e * WBC_NFEET + lane;
    if (a.stance) a.stance[ef] = (stand && !failed) ? 1 : 0;
    if (a.contact) a.contact[ef] = (stand && !failed) ? 1.f : 0.f;
    if (a.swing_ref) { st3(a.swing_ref + ef * 9, rp); st3(a.swing_ref + ef * 9 + 3, rv); st3(a.swing_ref + ef * 9 + 6, ra); }
    if (a.swing_acc) st3(a.swing_acc + ef * 3, sacc);
    if (a.foothold) st3(a.foothold + ef * 3, fh);
    if (!failed) {
      float* sf = st + 4 + 7 * lane;
      st3(sf, lift); st3(sf + 3, target); sf[6] = flag;
    }
  }
  const unsigned lift_bits = (unsigned)(__ballot(lifted) & 0xFull), safe_bits = (unsigned)(__ballot(nosafe) & 0xFull);
  if (lane == 0) {
    if (!failed) {
      const float adv = phase + cfg.dt / cfg.period;
      st[0] = a.hold ? phase : adv - floorf(adv);
      st[1] = 0.f; st[2] = 0.f; st[3] = 0.f;
    }
    if (a.info) a.info[e] = failed ? WBC_FOOTSTEP_INFO_FAILED
                                   : ((reset ? WBC_FOOTSTEP_INFO_RESET : 0) | (int)(safe_bits * WBC_FOOTSTEP_INFO_NO_SAFE) | (int)(lift_bits * WBC_FOOTSTEP_INFO_LIFT));
  }
  __syncthreads();

  // the per-stage outputs: lane = stage * 4 + foot
  {
    const int k = lane >> 2, i = lane & 3;
    const bool active = k < H;
    const float x0 = phase + cfg.offset[i];
    const float xk = (phase + ((float)k + 0.5f) * (cfg.mpc_dt / cfg.period)) + cfg.offset[i];
    const float flk = floorf(xk);
    const bool sk = always || (xk - flk) < cfg.duty;
    const int m = always ? 0 : (int)(flk - floorf(x0));
    const unsigned long long mm = __ballot(active && sk) & (0x1111111111111111ull << i);
    int src = lane;
    if (!sk) {
      const unsigned long long later = mm & ~((2ull << lane) - 1ull), earlier = mm & ((1ull << lane) - 1ull);
      src = later ? __ffsll((long long)later) - 1 : (earlier ? 63 - __clzll((long long)earlier) : -1);
    }
    const int ms = __shfl(m, src < 0 ? lane : src);
    if (active) {
      const size_t ek = (e * H + k) * WBC_NFEET + i;
      if (a.schedule) a.schedule[ek] = (sk && !failed) ? 1 : 0;
      if (a.foot_pos) {
        f3 val = ld3(sF[i]);
        if (src >= 0) {
          if (ms <= 0) val = ld3(sP[i]);
          else { const float adv = (float)(ms - 1) * cfg.period; val.x += adv * vcx; val.y += adv * vcy; }
        }
        if (failed) val = mk3(0.f, 0.f, 0.f);
        st3(a.foot_pos + ek * 3, val);
      }
    }
  }
}

void wbc_footstep_launch(const FsConst& K, const wbc_footstep_cfg& cfg, const FsArgs& a, void* stream) {
  hipLaunchKernelGGL(wbc_footstep_plan_kernel, dim3(a.n), dim3(64), 0, (hipStream_t)stream, K, cfg, a);
}
