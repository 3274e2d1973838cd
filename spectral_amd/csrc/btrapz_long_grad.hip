// btrapz_long_grad.hip -- btrapz_solve_long_vjp_device / btrapz_solve_long_jvp_device (include/btrapz_hip_long_grad.h):
// the vector-Jacobian and Jacobian-vector products of a batched solve whose candidates have 65..256 segments.
//
// The method is vjp_kernel's (btrapz_vjp.hip) and jvp_kernel's (btrapz_jvp.hip), restated statement for statement in
// everything a lane does on its own: the record, the bounds and their provenance, P and q, the active-row rule (the
// NaN-multiplier rule included), rho, three passes of the method of multipliers on one block LDL^T, the chaining to
// the inputs, the defined cases.  What is new is what crosses lanes.
//
// Mapping: the long solve's (btrapz_kernels.hip, MULTI) -- one axis problem per WORKGROUP of W = ceil(seg_stride / 64)
// wavefronts, the lane K = 64 wv + lane holds segment K, lanes with K >= count are decoupled identities; 2 B workgroups,
// axis = blockIdx.x & 1.  Every index into seg, ctrl, lam and the outputs is the 64-segment kernels' with k = K.
//   * neighbour reads (K + 1, K - 1): DPP inside a wavefront; the wavefronts' edge lanes publish their values in LDS
//     (edge[wv][..]), one barrier, the edge lane on the other side of the seam reads;
//   * the seven sequential sweeps run wavefront by wavefront: in turn w only wavefront w runs its (at most 64) steps,
//     then hands the carried value (Z, fw or y) on through LDS and all wavefronts meet at one barrier;
//   * per-candidate sums: every lane publishes, wavefront 0 adds the entries 0 .. count - 1 in that order (the result
//     depends on the count only, not on W or the stride);
//   * cost_dot: the two axes of a candidate are two workgroups, so each writes its share to a [2][T][B] workspace and
//     long_cost_dot_kernel, launched behind on the same stream, adds s + l.  No atomics.
//
// Barriers: every __syncthreads() below stands in straight-line code or in a loop over W, GRAD_PASSES or
// a.T -- kernel arguments and constants.  ok, act and the segment count select DATA (and the trip count of the
// barrier-free inner step loops); nothing returns before the last barrier.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "btrapz_grad_rule.h"
#include "btrapz_long_grad.h"

namespace btrapz {

enum { LG_EDGE = 9, LG_LANES = 256 };

// A lane's place in its workgroup and the workgroup's LDS.
struct Wg {
  int lane, wv, W, K;          // lane of the wavefront, wavefront of the workgroup, wavefronts, segment 64 wv + lane
  int steps;                   // real segments of this wavefront: min(64, count - 64 wv), 0 without any
  double (*edge)[LG_EDGE];     // [4][9] values of a wavefront's edge lane, for the lane across the seam
  double *carry;               // [6] what a sweep hands from one wavefront to the next
  double (*rm)[LG_LANES];      // [4][256] per-candidate sums
};

// o = x of lane K + 1 (0 for the workgroup's last lane).  Two barriers, reached by every thread.
template <int N> __device__ __forceinline__ void from_next(const Wg &g, const double (&x)[N], double (&o)[N]) {
  static_assert(N <= LG_EDGE, "edge slots");
  if (g.lane == 0) { UNROLL for (int i = 0; i < N; i++) g.edge[g.wv][i] = x[i]; }
  __syncthreads();
  const bool has = g.wv + 1 < g.W;
  const int nw = has ? g.wv + 1 : g.wv;
  UNROLL for (int i = 0; i < N; i++) {
    const double v = dpp_next(x[i]);
    const double s = g.edge[nw][i];
    o[i] = g.lane == 63 ? (has ? s : 0.0) : v;
  }
  __syncthreads();
}
// o = x of lane K - 1 (0 for lane 0 of the workgroup).  Two barriers, reached by every thread.
template <int N> __device__ __forceinline__ void from_prev(const Wg &g, const double (&x)[N], double (&o)[N]) {
  static_assert(N <= LG_EDGE, "edge slots");
  if (g.lane == 63) { UNROLL for (int i = 0; i < N; i++) g.edge[g.wv][i] = x[i]; }
  __syncthreads();
  const bool has = g.wv > 0;
  const int pw = has ? g.wv - 1 : 0;
  UNROLL for (int i = 0; i < N; i++) {
    const double v = dpp_prev(x[i]);
    const double s = g.edge[pw][i];
    o[i] = g.lane == 0 ? (has ? s : 0.0) : v;
  }
  __syncthreads();
}

// Sums over the segments 0 .. n - 1, added in that order; the result is valid in wavefront 0.  Two barriers.
__device__ __forceinline__ Red4 sum4(const Wg &g, int n, double v0, double v1, double v2, double v3) {
  __syncthreads();   // (the readers of the call before are done)
  g.rm[0][g.K] = v0; g.rm[1][g.K] = v1; g.rm[2][g.K] = v2; g.rm[3][g.K] = v3;
  __syncthreads();
  Red4 r = {0.0, 0.0, 0.0, 0.0};
  if (g.wv == 0)
    for (int j = 0; j < n; j++) { r.a += g.rm[0][j]; r.b += g.rm[1][j]; r.c += g.rm[2][j]; r.d += g.rm[3][j]; }
  return r;
}
__device__ __forceinline__ double sum1(const Wg &g, int n, double v0) {
  __syncthreads();
  g.rm[0][g.K] = v0;
  __syncthreads();
  double r = 0.0;
  if (g.wv == 0)
    for (int j = 0; j < n; j++) r += g.rm[0][j];
  return r;
}

// ---- block LDL^T, downwards: S_k = T_k - Z_(k-1), K_k = S_k^-1 Mc, Z_k = Mc' K_k.  W turns, one barrier each. ----
__device__ __forceinline__ void factor_down(const Wg &g, const double (&T)[6], const double (&Mc)[9], double (&F)[6], double (&K)[9]) {
  double Z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < g.W; ++w) {
    if (g.wv == w) {
      double cin[6];
      UNROLL for (int i = 0; i < 6; i++) { const double v = g.carry[i]; cin[i] = w > 0 ? v : 0.0; }
      for (int s = 0; s < g.steps; ++s) {
        double pZ[6];
        UNROLL for (int i = 0; i < 6; i++) { const double v = dpp_prev(Z[i]); pZ[i] = g.lane == 0 ? cin[i] : v; }
        if (g.lane == s) {
          double Sk[6];
          UNROLL for (int i = 0; i < 6; i++) Sk[i] = T[i] - pZ[i];
          ldl3(Sk, F);
          UNROLL for (int j = 0; j < 3; j++) ldl3_solve(F, Mc[j], Mc[3 + j], Mc[6 + j], K[j], K[3 + j], K[6 + j]);
          Z[0] = Mc[0] * K[0] + Mc[3] * K[3] + Mc[6] * K[6];
          Z[1] = Mc[0] * K[1] + Mc[3] * K[4] + Mc[6] * K[7];
          Z[2] = Mc[0] * K[2] + Mc[3] * K[5] + Mc[6] * K[8];
          Z[3] = Mc[1] * K[1] + Mc[4] * K[4] + Mc[7] * K[7];
          Z[4] = Mc[1] * K[2] + Mc[4] * K[5] + Mc[7] * K[8];
          Z[5] = Mc[2] * K[2] + Mc[5] * K[5] + Mc[8] * K[8];
        }
      }
      if (g.lane == 63) { UNROLL for (int i = 0; i < 6; i++) g.carry[i] = Z[i]; }
    }
    __syncthreads();
  }
}
// ---- forward: u_k -= K_(k-1)' u_(k-1).  W turns, one barrier each. ----
__device__ __forceinline__ void sweep_forward(const Wg &g, const double (&K)[9], double (&u)[3]) {
  double fw[3] = {0.0, 0.0, 0.0};
  for (int w = 0; w < g.W; ++w) {
    if (g.wv == w) {
      double cin[3];
      UNROLL for (int i = 0; i < 3; i++) { const double v = g.carry[i]; cin[i] = w > 0 ? v : 0.0; }
      for (int s = 0; s < g.steps; ++s) {
        double pw[3];
        UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_prev(fw[i]); pw[i] = g.lane == 0 ? cin[i] : vv; }
        if (g.lane == s) {
          UNROLL for (int i = 0; i < 3; i++) u[i] -= pw[i];
          fw[0] = K[0] * u[0] + K[3] * u[1] + K[6] * u[2];
          fw[1] = K[1] * u[0] + K[4] * u[1] + K[7] * u[2];
          fw[2] = K[2] * u[0] + K[5] * u[1] + K[8] * u[2];
        }
      }
      if (g.lane == 63) { UNROLL for (int i = 0; i < 3; i++) g.carry[i] = fw[i]; }
    }
    __syncthreads();
  }
}
// ---- backward: X_k = S_k^-1 u_k - K_k X_(k+1).  W turns from the last wavefront up, one barrier each. ----
__device__ __forceinline__ void sweep_backward(const Wg &g, const double (&F)[6], const double (&K)[9], const double (&u)[3], bool last,
                                               double (&X)[3]) {
  ldl3_solve(F, u[0], u[1], u[2], X[0], X[1], X[2]);
  double y[3] = {0.0, 0.0, 0.0};
  for (int w = g.W - 1; w >= 0; --w) {
    if (g.wv == w) {
      double cin[3];
      UNROLL for (int i = 0; i < 3; i++) { const double v = g.carry[i]; cin[i] = w + 1 < g.W ? v : 0.0; }
      for (int s = g.steps - 1; s >= 0; --s) {
        double ny[3];
        UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_next(y[i]); ny[i] = last ? 0.0 : (g.lane == 63 ? cin[i] : vv); }
        if (g.lane == s) {
          UNROLL for (int i = 0; i < 3; i++) X[i] -= K[3 * i] * ny[0] + K[3 * i + 1] * ny[1] + K[3 * i + 2] * ny[2];
          UNROLL for (int i = 0; i < 3; i++) y[i] = X[i];
        }
      }
      if (g.lane == 0) { UNROLL for (int i = 0; i < 3; i++) g.carry[i] = y[i]; }
    }
    __syncthreads();
  }
}

// The body of both kernels.  Args: VjpArgs (backward) or JvpArgs (forward mode, cost_ws its second argument).
template <class Args> __device__ __forceinline__ void long_grad_body(const Args &a, double *cost_ws, const Wg &g0) {
  constexpr bool FWD = std::is_same<Args, JvpArgs>::value;
  Wg g = g0;
  const int k = g.K;                        // this lane's segment
  const int axis = blockIdx.x & 1;
  const long long cand = (long long)(blockIdx.x >> 1);
  const int Sg = a.S;                       // slots per candidate (seg_stride)
  const bool cand_in = cand < a.B;
  const int b = cand < a.B ? (int)cand : a.B - 1;
  const int n = a.seg_count ? a.seg_count[b] : Sg;
  const int set = a.set_index ? a.set_index[b] : 0;
  const int st = a.status[b];
  // the candidate is differentiated: solved (1 or 2), with a usable segment count and set
  const bool ok = cand_in && n >= 1 && n <= Sg && set >= 0 && set < a.n_sets && (st == BTRAPZ_SOLVED || st == BTRAPZ_SOLVED_INACCURATE);
  const bool act = ok && k < n;             // this lane holds a real segment
  const bool slot = cand_in && k < Sg;      // this lane owns a slot of the candidate's output rows
  const bool first = k == 0, last = k == n - 1;
  const int ns = (n >= 1 && n <= Sg) ? n : Sg;   // (control-point offsets of the l axis)
  const int nn = ok ? n : 0;                // segments summed over and swept through
  {
    const int left = nn - 64 * g.wv;
    g.steps = left < 0 ? 0 : left > 64 ? 64 : left;
  }
  const size_t BS = (size_t)a.B * a.seg_stride;
  const size_t e = (size_t)b * a.seg_stride + k;
  const Shared &sh = a.sets[(set >= 0 && set < a.n_sets) ? set : 0];
  const double *mq = a.mqm + (size_t)((set >= 0 && set < a.n_sets) ? set : 0) * 168 + axis * 84;
  const double *mu = a.mqm_unit + axis * 84;
  const int variant = sh.variant;

  // ---- the record, the rows and their bounds (begin_candidate), with the derivative of every bound ----
  const double *sg = a.seg;
  double t = act ? sg[BTRAPZ_F_T * BS + e] : 1.0;
  if (!(t > 0.0)) t = 1.0;
  const double it = 1.0 / t, t2 = t * t, t3 = t2 * t, it3 = it * it * it;
  const NullMap nm = {it, t * 0.05};
  double lb = 0.0, ls = 0.0, ub = 0.0, us = 0.0, begl = 0.0, endl = 0.0, skew = 0.0, bias = 0.0, vlo_in[5], vhi_in[5];
  UNROLL for (int i = 0; i < 5; i++) { vlo_in[i] = 0.0; vhi_in[i] = 0.0; }
  if (act) {
    if (axis == 0) {
      lb = sg[BTRAPZ_F_DOWN_BIAS * BS + e]; ls = sg[BTRAPZ_F_DOWN_SKEW * BS + e];
      ub = sg[BTRAPZ_F_UPP_BIAS * BS + e];  us = sg[BTRAPZ_F_UPP_SKEW * BS + e];
      const double dlo = sg[BTRAPZ_F_DS_LO * BS + e], dhi = sg[BTRAPZ_F_DS_HI * BS + e];
      UNROLL for (int i = 0; i < 5; i++) { vlo_in[i] = dlo; vhi_in[i] = dhi; }
    } else {
      lb = sg[BTRAPZ_F_L_DOWN_BIAS * BS + e]; ls = sg[BTRAPZ_F_L_DOWN_SKEW * BS + e];
      ub = sg[BTRAPZ_F_L_UPP_BIAS * BS + e];  us = sg[BTRAPZ_F_L_UPP_SKEW * BS + e];
      if (variant == BTRAPZ_CUBOID) { begl = sg[BTRAPZ_F_BEG_L * BS + e]; endl = sg[BTRAPZ_F_END_L * BS + e]; }
      UNROLL for (int i = 0; i < 5; i++) { vlo_in[i] = a.dl_bounds[(size_t)b * 10 + 2 * i]; vhi_in[i] = a.dl_bounds[(size_t)b * 10 + 2 * i + 1]; }
    }
    skew = sg[(axis == 0 ? BTRAPZ_F_X_SKEW : BTRAPZ_F_Y_SKEW) * BS + e];
    bias = sg[(axis == 0 ? BTRAPZ_F_X_BIAS : BTRAPZ_F_Y_BIAS) * BS + e];
  }
  // position lines lo_i = plo0 + i dplo; d(plo0)/d(bias, skew) and d(dplo)/d(skew) of the lower (l*) and upper (u*) line
  double plo0 = lb, dplo = ls * 0.2 * t, phi0 = ub, dphi = us * 0.2 * t;
  double lo0_b = 1.0, lo0_s = 0.0, lod_s = 0.2 * t, hi0_b = 1.0, hi0_s = 0.0, hid_s = 0.2 * t;
  if (variant == BTRAPZ_CUBOID) {
    if (axis == 0) {   // inscribed interval: the derivative of the branch taken
      const double l1 = ls * 0.0 + lb, l2 = lb + ls * t, h1 = us * 0.0 + ub, h2 = ub + us * t;
      const double lin = fmax(l1, l2), hin = fmin(h1, h2);
      plo0 = fmax(0.0, lin); phi0 = fmin(100.0, hin);
      const bool lclamp = !(lin >= 0.0), hclamp = !(hin <= 100.0);
      const bool l2b = l2 > l1, h2b = h2 < h1;
      lo0_b = lclamp ? 0.0 : 1.0; lo0_s = (lclamp || !l2b) ? 0.0 : t;
      hi0_b = hclamp ? 0.0 : 1.0; hi0_s = (hclamp || !h2b) ? 0.0 : t;
    } else {
      plo0 = begl; phi0 = endl;   // (d/d BEG_L, END_L: 1, kept in lo0_b / hi0_b)
    }
    dplo = 0.0; dphi = 0.0; lod_s = 0.0; hid_s = 0.0;
  }
  double vlo[5], vhi[5];
  UNROLL for (int i = 0; i < 5; i++) { vlo[i] = vlo_in[i]; vhi[i] = vhi_in[i]; }
  // bounds that are no bounds: moved far out by the solve, never active, gradient 0 / tangent ignored
  const bool lo_far = far_bound(plo0) || far_bound(plo0 + 5.0 * dplo), hi_far = far_bound(phi0) || far_bound(phi0 + 5.0 * dphi);
  move_far_bounds(plo0, dplo, phi0, dphi, vlo, vhi);
  double vlo_f[5], vhi_f[5];   // 1: the velocity bound is the input's, 0: moved
  UNROLL for (int i = 0; i < 5; i++) { vlo_f[i] = far_bound(vlo_in[i]) ? 0.0 : 1.0; vhi_f[i] = far_bound(vhi_in[i]) ? 0.0 : 1.0; }
  if (lo_far) { lo0_b = 0.0; lo0_s = 0.0; lod_s = 0.0; }
  if (hi_far) { hi0_b = 0.0; hi0_s = 0.0; hid_s = 0.0; }
  // acceleration / jerk limits: the host's clamp (s axis, +-1000) and far limits (+-BTRAPZ_FAR_LIMIT) are no inputs
  const double acc_lo = axis == 0 ? sh.acc_s[0] : sh.acc_l[0], acc_hi = axis == 0 ? sh.acc_s[1] : sh.acc_l[1];
  const double jrk_lo = axis == 0 ? sh.jerk_s[0] : sh.jerk_l[0], jrk_hi = axis == 0 ? sh.jerk_s[1] : sh.jerk_l[1];
  const double alo = acc_lo * t, ahi = acc_hi * t, jlo = jrk_lo * t2, jhi = jrk_hi * t2;
  auto moved = [&](double v, bool clamped_s) { return fabs(v) == BTRAPZ_FAR_LIMIT || (clamped_s && fabs(v) == 1000.0); };
  const double alo_f = moved(acc_lo, axis == 0) ? 0.0 : t, ahi_f = moved(acc_hi, axis == 0) ? 0.0 : t;
  const double jlo_f = moved(jrk_lo, false) ? 0.0 : t2, jhi_f = moved(jrk_hi, false) ? 0.0 : t2;
  // the joint rows 5 / 10 carry the intersection with the next segment's rows 0 / 6: which side supplied each bound
  double mplo = plo0 + 5.0 * dplo, mphi = phi0 + 5.0 * dphi, mvlo = vlo[4], mvhi = vhi[4];
  bool nx_plo = false, nx_phi = false, nx_vlo = false, nx_vhi = false;   // true: the next segment's (ties: this one's)
  {
    const double own[4] = {plo0, phi0, vlo[0], vhi[0]};
    double nb[4];
    from_next(g, own, nb);
    const double nplo = nb[0], nphi = nb[1], nvlo = nb[2], nvhi = nb[3];
    if (!last) {
      nx_plo = nplo > mplo; nx_phi = nphi < mphi; nx_vlo = nvlo > mvlo; nx_vhi = nvhi < mvhi;
      mplo = fmax(mplo, nplo); mphi = fmin(mphi, nphi); mvlo = fmax(mvlo, nvlo); mvhi = fmin(mvhi, nvhi);
      if (mplo > mphi) { mplo = 0.5 * (mplo + mphi); mphi = mplo; }   // (a joint pinned to the common point)
      if (mvlo > mvhi) { mvlo = 0.5 * (mvlo + mvhi); mvhi = mvlo; }
    }
  }
#define VLO(r) ((r) < 6 ? ((r) == 5 ? mplo : plo0 + (double)(r) * dplo) : (r) < 11 ? ((r) == 10 ? mvlo : vlo[(r) >= 6 && (r) < 11 ? (r) - 6 : 0]) : (r) < 15 ? alo : jlo)
#define VUP(r) ((r) < 6 ? ((r) == 5 ? mphi : phi0 + (double)(r) * dphi) : (r) < 11 ? ((r) == 10 ? mvhi : vhi[(r) >= 6 && (r) < 11 ? (r) - 6 : 0]) : (r) < 15 ? ahi : jhi)

  // ---- P, q (begin_candidate) and the control points ----
  double Pk[21], q[6], c[6];
  {
    const double we = axis == 0 ? sh.weight_end_s : sh.weight_end_l;
    UNROLL for (int i = 0; i < 21; i++) Pk[i] = 2.0 * (t3 * mq[i] + t * mq[21 + i] + it * mq[42 + i] + it3 * mq[63 + i]);
    if (last) Pk[SYM(5, 5)] += 2.0 * we * t2;
  }
  const double wr = axis == 0 ? sh.w_s[0] : sh.w_l[0], wd = axis == 0 ? sh.w_s[1] : sh.w_l[1];
  const double dref = axis == 0 ? sh.ds_ref : sh.dl_ref;
  const double rend = act ? a.ref_end[(size_t)b * 2 + axis] : 0.0;
  {
    double qp[6];
    UNROLL for (int i = 0; i < 6; i++) {
      qp[i] = -2.0 * (t * t * t) * wr * skew / (double)(i + 2) - 2.0 * (t * t) * wr * bias / (double)(i + 1);
      if (i > 0) qp[i] += -2.0 * wd * dref * t;
    }
    q[0] = qp[0] - 5.0 * qp[1] + 10.0 * qp[2] - 10.0 * qp[3] + 5.0 * qp[4] - qp[5];
    q[1] = 5.0 * qp[1] - 20.0 * qp[2] + 30.0 * qp[3] - 20.0 * qp[4] + 5.0 * qp[5];
    q[2] = 10.0 * qp[2] - 30.0 * qp[3] + 30.0 * qp[4] - 10.0 * qp[5];
    q[3] = 10.0 * qp[3] - 20.0 * qp[4] + 10.0 * qp[5];
    q[4] = 5.0 * qp[4] - 5.0 * qp[5];
    q[5] = qp[5];
    if (last) q[5] -= dref * 2.0 * rend * t;
  }
  const size_t o_own = (size_t)axis * 6 * ns + (size_t)k * 6;   // k < ns: this segment's slots of a ctrl row
  {
    const size_t o = (size_t)b * 12 * a.seg_stride + o_own;
    UNROLL for (int i = 0; i < 6; i++) c[i] = act ? a.ctrl[o + i] : 0.0;
  }
  double Pc[6];   // P x
  UNROLL for (int i = 0; i < 6; i++) {
    double s = 0.0;
    UNROLL for (int j = 0; j < 6; j++) s += HSYM(Pk, i, j) * c[j];
    Pc[i] = s;
  }

  // ---- active rows: multiplier above slack (the solve's last multipliers classify; their values are not used) ----
  // side: -1 lower bound active, +1 upper, 0 inactive; rho: the row's penalty weight
  double pscale = 0.0;
  UNROLL for (int i = 0; i < 6; i++) pscale = fmax(pscale, Pk[SYM(i, i)]);
  if (!(pscale > 0.0) || !(pscale < 1e300)) pscale = 1.0;
  int side[15];
  double rho[15], w[15];
  {
    const size_t lam_row = BS;
    const size_t lam_e = (size_t)axis * 36 * lam_row + e;
    GRAD_ROWS(r)
      const double gc = row_dot<r>(c, t);
      const double ll = act ? a.lam[lam_e + (size_t)r * lam_row] : 0.0, lu = act ? a.lam[lam_e + (size_t)(18 + r) * lam_row] : 0.0;
      const double lo = VLO(r), up = VUP(r);
      const bool al = (fabs(ll) < 1e300 ? ll > gc - lo : gc - lo < GRAD_SLACK_ACTIVE) && !(fabs(lo) >= BTRAPZ_FAR);
      const bool au = (fabs(lu) < 1e300 ? lu > up - gc : up - gc < GRAD_SLACK_ACTIVE) && !(fabs(up) >= BTRAPZ_FAR);
      side[ri_] = (act && (al || au)) ? ((al && au) ? (ll >= lu ? -1 : 1) : (al ? -1 : 1)) : 0;
      rho[ri_] = side[ri_] != 0 ? GRAD_RHO * pscale / (r < 6 ? t2 : r < 11 ? 50.0 : r < 15 ? 2400.0 : 72000.0) : 0.0;
      w[ri_] = 0.0;
    GRAD_END
  }

  // ---- reduced matrix: T = M11_k + M00_(k+1), M01 couples X_(k-1) (rows) and X_k (cols) ----
  double T[6], M01[9];
  {
    double H[21];
    UNROLL for (int i = 0; i < 21; i++) H[i] = Pk[i];
    GRAD_ROWS(r)
      row_outer<r>(rho[ri_], t2, H);
    GRAD_END
    if (!act) {   // (a lane without a segment: a decoupled identity)
      UNROLL for (int i = 0; i < 21; i++) H[i] = 0.0;
      UNROLL for (int i = 0; i < 6; i++) H[SYM(i, i)] = 1.0;
    }
    double w0[3], w1[3], w2[3], col[3], M00[6];
    UT_apply(nm, H[SYM(0, 0)], H[SYM(0, 1)], H[SYM(0, 2)], w0);
    UT_apply(nm, H[SYM(0, 1)], H[SYM(1, 1)], H[SYM(1, 2)], w1);
    UT_apply(nm, H[SYM(0, 2)], H[SYM(1, 2)], H[SYM(2, 2)], w2);
    UT_apply(nm, w0[0], w1[0], w2[0], col); M00[0] = col[0]; M00[1] = col[1]; M00[2] = col[2];
    UT_apply(nm, w0[1], w1[1], w2[1], col); M00[3] = col[1]; M00[4] = col[2];
    UT_apply(nm, w0[2], w1[2], w2[2], col); M00[5] = col[2];
    VT_apply(nm, H[SYM(0, 3)], H[SYM(0, 4)], H[SYM(0, 5)], w0);
    VT_apply(nm, H[SYM(1, 3)], H[SYM(1, 4)], H[SYM(1, 5)], w1);
    VT_apply(nm, H[SYM(2, 3)], H[SYM(2, 4)], H[SYM(2, 5)], w2);
    UNROLL for (int j = 0; j < 3; j++) {
      UT_apply(nm, w0[j], w1[j], w2[j], col);
      M01[0 * 3 + j] = col[0]; M01[1 * 3 + j] = col[1]; M01[2 * 3 + j] = col[2];
    }
    VT_apply(nm, H[SYM(3, 3)], H[SYM(3, 4)], H[SYM(3, 5)], w0);
    VT_apply(nm, H[SYM(3, 4)], H[SYM(4, 4)], H[SYM(4, 5)], w1);
    VT_apply(nm, H[SYM(3, 5)], H[SYM(4, 5)], H[SYM(5, 5)], w2);
    VT_apply(nm, w0[0], w1[0], w2[0], col); T[0] = col[0]; T[1] = col[1]; T[2] = col[2];
    VT_apply(nm, w0[1], w1[1], w2[1], col); T[3] = col[1]; T[4] = col[2];
    VT_apply(nm, w0[2], w1[2], w2[2], col); T[5] = col[2];
    double nM00[6];
    from_next(g, M00, nM00);
    UNROLL for (int i = 0; i < 6; i++) T[i] += last ? 0.0 : nM00[i];
  }
  // ---- block LDL^T: Mc = M01_(k+1) (0 for the last segment) ----
  double F[6] = {0.0, 0.0, 0.0, 1.0, 1.0, 1.0}, K[9], Mc[9];
  {
    double nM01[9];
    from_next(g, M01, nM01);
    UNROLL for (int i = 0; i < 9; i++) { Mc[i] = last ? 0.0 : nM01[i]; K[i] = 0.0; }
    factor_down(g, T, Mc, F, K);
  }

  if constexpr (!FWD) {
    // ================= the vector-Jacobian product (vjp_kernel) =================
    double xb[6];
    const double cbar = (act && a.cost_bar) ? a.cost_bar[b] : 0.0;
    {
      const size_t o = (size_t)b * 12 * a.seg_stride + o_own;
      UNROLL for (int i = 0; i < 6; i++) xb[i] = (act && a.ctrl_bar) ? a.ctrl_bar[o + i] : 0.0;
    }
    UNROLL for (int i = 0; i < 6; i++) xb[i] += cbar * (Pc[i] + q[i]);   // xbar'

    // ---- passes of the method of multipliers ----
    double v[6];   // v in control-point space (this segment)
    for (int pass = 0; pass < GRAD_PASSES; ++pass) {
      double h[6];
      UNROLL for (int i = 0; i < 6; i++) h[i] = xb[i];
      GRAD_ROWS(r)
        row_scatter<r>(-w[ri_], t, h);
      GRAD_END
      if (!act) { UNROLL for (int i = 0; i < 6; i++) h[i] = 0.0; }
      double u[3];
      {
        double un[3], nun[3];
        VT_apply(nm, h[3], h[4], h[5], u);
        UT_apply(nm, h[0], h[1], h[2], un);
        from_next(g, un, nun);
        UNROLL for (int i = 0; i < 3; i++) u[i] += last ? 0.0 : nun[i];
      }
      sweep_forward(g, K, u);
      double X[3] = {0.0, 0.0, 0.0};
      sweep_backward(g, F, K, u, last, X);
      double Xp[3];
      from_prev(g, X, Xp);   // (the initial state is given: 0 for segment 0)
      U_apply(nm, Xp, v[0], v[1], v[2]);
      V_apply(nm, X, v[3], v[4], v[5]);
      GRAD_ROWS(r)
        w[ri_] += rho[ri_] * row_dot<r>(v, t);
      GRAD_END
    }
    if (!act) { UNROLL for (int i = 0; i < 6; i++) v[i] = 0.0; }

    // ---- bounds: an active row's w goes to the input that supplied its bound ----
    double g_lb = 0.0, g_ls = 0.0, g_ub = 0.0, g_us = 0.0, g_vlo = 0.0, g_vhi = 0.0;   // this segment's fields
    double g_dl[10];                                                                     // l axis: the candidate's dl bounds
    UNROLL for (int i = 0; i < 10; i++) g_dl[i] = 0.0;
    double g_alo = 0.0, g_ahi = 0.0, g_jlo = 0.0, g_jhi = 0.0;
    double to_next[4] = {0.0, 0.0, 0.0, 0.0};   // amounts for the next segment's plo0, phi0, vlo[0], vhi[0]
    double own0[4];                             // (this segment's own row-0 / row-6 amounts come from the previous lane)
    GRAD_ROWS(r)
      const double wl = side[ri_] < 0 ? w[ri_] : 0.0, wu = side[ri_] > 0 ? w[ri_] : 0.0;
      if constexpr (r < 6) {
        if (r == 5 && nx_plo) to_next[0] += wl; else { g_lb += wl * lo0_b; g_ls += wl * (lo0_s + (double)r * lod_s); }
        if (r == 5 && nx_phi) to_next[1] += wu; else { g_ub += wu * hi0_b; g_us += wu * (hi0_s + (double)r * hid_s); }
      } else if constexpr (r < 11) {
        constexpr int i = r - 6;
        if (r == 10 && nx_vlo) to_next[2] += wl; else { if (axis == 0) g_vlo += wl * vlo_f[i]; else g_dl[2 * i] += wl * vlo_f[i]; }
        if (r == 10 && nx_vhi) to_next[3] += wu; else { if (axis == 0) g_vhi += wu * vhi_f[i]; else g_dl[2 * i + 1] += wu * vhi_f[i]; }
      } else if constexpr (r < 15) {
        g_alo += wl * alo_f; g_ahi += wu * ahi_f;
      } else {
        g_jlo += wl * jlo_f; g_jhi += wu * jhi_f;
      }
    GRAD_END
    from_prev(g, to_next, own0);
    g_lb += own0[0] * lo0_b; g_ls += own0[0] * lo0_s;
    g_ub += own0[1] * hi0_b; g_us += own0[1] * hi0_s;
    if (axis == 0) { g_vlo += own0[2] * vlo_f[0]; g_vhi += own0[3] * vhi_f[0]; }
    else { g_dl[0] += own0[2] * vlo_f[0]; g_dl[1] += own0[3] * vhi_f[0]; }

    // ---- q: qbar = -v + cbar x, through q = M' qp to the reference line, the weights, d_ref and ref_end ----
    double g_skew = 0.0, g_bias = 0.0, g_wr = 0.0, g_wd = 0.0, g_dref = 0.0, g_rend = 0.0;
    {
      double qb[6], qpb[6];
      UNROLL for (int i = 0; i < 6; i++) qb[i] = -v[i] + cbar * c[i];
      qpb[0] = qb[0];
      qpb[1] = -5.0 * qb[0] + 5.0 * qb[1];
      qpb[2] = 10.0 * qb[0] - 20.0 * qb[1] + 10.0 * qb[2];
      qpb[3] = -10.0 * qb[0] + 30.0 * qb[1] - 30.0 * qb[2] + 10.0 * qb[3];
      qpb[4] = 5.0 * qb[0] - 20.0 * qb[1] + 30.0 * qb[2] - 20.0 * qb[3] + 5.0 * qb[4];
      qpb[5] = -qb[0] + 5.0 * qb[1] - 10.0 * qb[2] + 10.0 * qb[3] - 5.0 * qb[4] + qb[5];
      UNROLL for (int i = 0; i < 6; i++) {
        const double ds_ = -2.0 * t3 / (double)(i + 2), db_ = -2.0 * t2 / (double)(i + 1);
        g_skew += qpb[i] * ds_ * wr; g_bias += qpb[i] * db_ * wr;
        g_wr += qpb[i] * (ds_ * skew + db_ * bias);
        if (i > 0) { g_wd += qpb[i] * (-2.0 * dref * t); g_dref += qpb[i] * (-2.0 * wd * t); }
      }
      if (last) { g_dref += qb[5] * (-2.0 * rend * t); g_rend = qb[5] * (-2.0 * dref * t); }
    }
    // ---- P: Pbar = -(v x' + x v') / 2 + cbar x x' / 2 against dP / dw_d = 2 t^p_d (unit table d), and the end weight ----
    double g_w[4] = {0.0, 0.0, 0.0, 0.0}, g_we = 0.0;
    {
      double e4[4] = {0.0, 0.0, 0.0, 0.0};
      UNROLL for (int j = 0; j < 6; j++)
        UNROLL for (int i = 0; i <= j; i++) {
          const double cf = i == j ? (-v[i] * c[i] + 0.5 * cbar * c[i] * c[i]) : (-(v[i] * c[j] + v[j] * c[i]) + cbar * c[i] * c[j]);
          UNROLL for (int d = 0; d < 4; d++) e4[d] += mu[21 * d + SYM(i, j)] * cf;
        }
      g_w[0] = 2.0 * t3 * e4[0] + g_wr; g_w[1] = 2.0 * t * e4[1] + g_wd; g_w[2] = 2.0 * it * e4[2]; g_w[3] = 2.0 * it3 * e4[3];
      if (last) g_we = 2.0 * t2 * (-v[5] * c[5] + 0.5 * cbar * c[5] * c[5]);
    }
    // ---- the initial state: Xinit_bar = U' (xbar' - P v - G' w) of segment 0 ----
    double g_init[3] = {0.0, 0.0, 0.0};
    if (first) {
      double r6[6];
      UNROLL for (int i = 0; i < 6; i++) {
        double s = 0.0;
        UNROLL for (int j = 0; j < 6; j++) s += HSYM(Pk, i, j) * v[j];
        r6[i] = xb[i] - s;
      }
      GRAD_ROWS(r)
        row_scatter<r>(-w[ri_], t, r6);
      GRAD_END
      UT_apply(nm, r6[0], r6[1], r6[2], g_init);
    }

    // ---- per-candidate sums over the segments (fixed order), then the stores ----
    auto m0 = [&](double x) { return act ? x : 0.0; };
    const Red4 s0 = sum4(g, nn, m0(g_w[0]), m0(g_w[1]), m0(g_w[2]), m0(g_w[3]));
    const Red4 s1 = sum4(g, nn, m0(g_dref), m0(g_alo), m0(g_ahi), m0(g_jlo));
    const Red4 s2 = sum4(g, nn, m0(g_jhi), m0(g_dl[0]), m0(g_dl[1]), m0(g_dl[2]));
    const Red4 s3 = sum4(g, nn, m0(g_dl[3]), m0(g_dl[4]), m0(g_dl[5]), m0(g_dl[6]));
    const Red4 s4 = sum4(g, nn, m0(g_dl[7]), m0(g_dl[8]), m0(g_dl[9]), m0(g_we));
    // (the last barrier is behind: what follows only stores)
    if (slot && a.g_seg) {
      double *gs = a.g_seg;
      if (axis == 0) {
        gs[BTRAPZ_F_T * BS + e] = 0.0;
        gs[BTRAPZ_F_DOWN_BIAS * BS + e] = m0(g_lb); gs[BTRAPZ_F_DOWN_SKEW * BS + e] = m0(g_ls);
        gs[BTRAPZ_F_UPP_BIAS * BS + e] = m0(g_ub);  gs[BTRAPZ_F_UPP_SKEW * BS + e] = m0(g_us);
        gs[BTRAPZ_F_DS_LO * BS + e] = m0(g_vlo);    gs[BTRAPZ_F_DS_HI * BS + e] = m0(g_vhi);
        gs[BTRAPZ_F_X_SKEW * BS + e] = m0(g_skew);  gs[BTRAPZ_F_X_BIAS * BS + e] = m0(g_bias);
      } else {
        const bool cub = variant == BTRAPZ_CUBOID;
        gs[BTRAPZ_F_L_DOWN_BIAS * BS + e] = cub ? 0.0 : m0(g_lb); gs[BTRAPZ_F_L_DOWN_SKEW * BS + e] = cub ? 0.0 : m0(g_ls);
        gs[BTRAPZ_F_L_UPP_BIAS * BS + e] = cub ? 0.0 : m0(g_ub);  gs[BTRAPZ_F_L_UPP_SKEW * BS + e] = cub ? 0.0 : m0(g_us);
        gs[BTRAPZ_F_BEG_L * BS + e] = cub ? m0(g_lb) : 0.0;      gs[BTRAPZ_F_END_L * BS + e] = cub ? m0(g_ub) : 0.0;
        gs[BTRAPZ_F_Y_SKEW * BS + e] = m0(g_skew);  gs[BTRAPZ_F_Y_BIAS * BS + e] = m0(g_bias);
      }
    }
    if (cand_in && a.g_ref_end && k == ns - 1) a.g_ref_end[(size_t)b * 2 + axis] = ok ? g_rend : 0.0;
    if (cand_in && k == 0) {
      if (a.g_init) UNROLL for (int i = 0; i < 3; i++) a.g_init[(size_t)b * 6 + axis * 3 + i] = ok ? g_init[i] : 0.0;
      if (a.g_dl && axis == 1) {
        const double d10[10] = {s2.b, s2.c, s2.d, s3.a, s3.b, s3.c, s3.d, s4.a, s4.b, s4.c};
        UNROLL for (int i = 0; i < 10; i++) a.g_dl[(size_t)b * 10 + i] = ok ? d10[i] : 0.0;
      }
      if (a.g_shared) {
        double *gsh = a.g_shared + (size_t)b * 20;
        // layout.Shared.as_array order: w_s[4] w_l[4] weight_end_s weight_end_l ds_ref dl_ref dds[2] ddds[2] ddl[2] dddl[2]
        const double wv4[4] = {s0.a, s0.b, s0.c, s0.d};
        UNROLL for (int d = 0; d < 4; d++) gsh[4 * axis + d] = ok ? wv4[d] : 0.0;
        gsh[8 + axis] = ok ? s4.d : 0.0; gsh[10 + axis] = ok ? s1.a : 0.0;
        gsh[12 + 4 * axis] = ok ? s1.b : 0.0; gsh[13 + 4 * axis] = ok ? s1.c : 0.0;
        gsh[14 + 4 * axis] = ok ? s1.d : 0.0; gsh[15 + 4 * axis] = ok ? s2.a : 0.0;
      }
    }
  } else {
    // ================= the Jacobian-vector products (jvp_kernel) =================
    double gx[6];   // P x + q: the gradient of the cost in x
    UNROLL for (int i = 0; i < 6; i++) gx[i] = Pc[i] + q[i];
    const double tp[4] = {2.0 * t3, 2.0 * t, 2.0 * it, 2.0 * it3};
    const bool cub_l = variant == BTRAPZ_CUBOID && axis == 1;
    // fields of this axis in seg_dot
    const int f_lb = axis == 0 ? BTRAPZ_F_DOWN_BIAS : cub_l ? BTRAPZ_F_BEG_L : BTRAPZ_F_L_DOWN_BIAS;
    const int f_ub = axis == 0 ? BTRAPZ_F_UPP_BIAS : cub_l ? BTRAPZ_F_END_L : BTRAPZ_F_L_UPP_BIAS;
    const int f_ls = axis == 0 ? BTRAPZ_F_DOWN_SKEW : BTRAPZ_F_L_DOWN_SKEW, f_us = axis == 0 ? BTRAPZ_F_UPP_SKEW : BTRAPZ_F_L_UPP_SKEW;
    const int f_skew = axis == 0 ? BTRAPZ_F_X_SKEW : BTRAPZ_F_Y_SKEW, f_bias = axis == 0 ? BTRAPZ_F_X_BIAS : BTRAPZ_F_Y_BIAS;
    const size_t o_pad = (size_t)12 * ns + (size_t)axis * 6 * (Sg - ns) + (size_t)(k < ns ? 0 : k - ns) * 6;   // k >= ns: its share of the slots beyond 12 S_b
    const size_t o_ctrl = k < ns ? o_own : o_pad;

    // ---- the tangents, one after the other on the one factor ----
    for (int tau = 0; tau < a.T; ++tau) {
      const size_t tb = (size_t)tau * a.B + b;
      // input tangents of this lane
      double dlb = 0.0, dls = 0.0, dub = 0.0, dus = 0.0, dskew = 0.0, dbias = 0.0, dvlo_in[5], dvhi_in[5];
      UNROLL for (int i = 0; i < 5; i++) { dvlo_in[i] = 0.0; dvhi_in[i] = 0.0; }
      if (act && a.seg_dot) {
        const double *sd = a.seg_dot + (size_t)tau * BTRAPZ_NUM_SEG_FIELDS * BS + e;
        dlb = sd[f_lb * BS]; dub = sd[f_ub * BS];
        if (!cub_l) { dls = sd[f_ls * BS]; dus = sd[f_us * BS]; }
        dskew = sd[f_skew * BS]; dbias = sd[f_bias * BS];
        if (axis == 0) {
          const double dlo = sd[BTRAPZ_F_DS_LO * BS], dhi = sd[BTRAPZ_F_DS_HI * BS];
          UNROLL for (int i = 0; i < 5; i++) { dvlo_in[i] = dlo; dvhi_in[i] = dhi; }
        }
      }
      if (act && a.dl_dot && axis == 1) {
        UNROLL for (int i = 0; i < 5; i++) { dvlo_in[i] = a.dl_dot[tb * 10 + 2 * i]; dvhi_in[i] = a.dl_dot[tb * 10 + 2 * i + 1]; }
      }
      double dw[4] = {0.0, 0.0, 0.0, 0.0}, dwe = 0.0, ddref = 0.0, dacc_lo = 0.0, dacc_hi = 0.0, djrk_lo = 0.0, djrk_hi = 0.0;
      if (act && a.shared_dot) {
        // layout.Shared.as_array order: w_s[4] w_l[4] weight_end_s weight_end_l ds_ref dl_ref dds[2] ddds[2] ddl[2] dddl[2]
        const double *pd = a.shared_dot + tb * 20;
        UNROLL for (int d = 0; d < 4; d++) dw[d] = pd[4 * axis + d];
        dwe = pd[8 + axis]; ddref = pd[10 + axis];
        dacc_lo = pd[12 + 4 * axis]; dacc_hi = pd[13 + 4 * axis]; djrk_lo = pd[14 + 4 * axis]; djrk_hi = pd[15 + 4 * axis];
      }
      const double drend = (act && a.ref_end_dot) ? a.ref_end_dot[tb * 2 + axis] : 0.0;
      double xp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // dx_p: the initial state's tangent moves segment 0's first three points
      if (act && first && a.init_dot) {
        const double dXi[3] = {a.init_dot[tb * 6 + axis * 3], a.init_dot[tb * 6 + axis * 3 + 1], a.init_dot[tb * 6 + axis * 3 + 2]};
        U_apply(nm, dXi, xp[0], xp[1], xp[2]);
      }

      // ---- db: the tangent of every row's bounds, the active side's kept (minus G dx_p) ----
      double d[15];
      {
        const double dplo0 = lo0_b * dlb + lo0_s * dls, dplod = lod_s * dls, dphi0 = hi0_b * dub + hi0_s * dus, dphid = hid_s * dus;
        double dvl[5], dvh[5];
        UNROLL for (int i = 0; i < 5; i++) { dvl[i] = vlo_f[i] * dvlo_in[i]; dvh[i] = vhi_f[i] * dvhi_in[i]; }
        const double own[4] = {dplo0, dphi0, dvl[0], dvh[0]};
        double nb[4];
        from_next(g, own, nb);
        const double n_plo = nb[0], n_phi = nb[1], n_vlo = nb[2], n_vhi = nb[3];
        GRAD_ROWS(r)
          double dl, du;
          if constexpr (r < 6) {
            dl = (r == 5 && nx_plo) ? n_plo : dplo0 + (double)r * dplod;
            du = (r == 5 && nx_phi) ? n_phi : dphi0 + (double)r * dphid;
          } else if constexpr (r < 11) {
            constexpr int i = r - 6;
            dl = (r == 10 && nx_vlo) ? n_vlo : dvl[i];
            du = (r == 10 && nx_vhi) ? n_vhi : dvh[i];
          } else if constexpr (r < 15) {
            dl = alo_f * dacc_lo; du = ahi_f * dacc_hi;
          } else {
            dl = jlo_f * djrk_lo; du = jhi_f * djrk_hi;
          }
          d[ri_] = (side[ri_] < 0 ? dl : side[ri_] > 0 ? du : 0.0) - row_dot<r>(xp, t);
          w[ri_] = 0.0;
        GRAD_END
      }
      // ---- dq (q = M' qp, last segment's end term) and dP x ----
      double dq[6], dPc[6];
      {
        double qp[6];
        const double a_skew = wr * dskew + skew * dw[0], a_bias = wr * dbias + bias * dw[0], a_ref = -2.0 * t * (dw[1] * dref + wd * ddref);
        UNROLL for (int i = 0; i < 6; i++) {
          qp[i] = (-2.0 * t3 / (double)(i + 2)) * a_skew + (-2.0 * t2 / (double)(i + 1)) * a_bias;
          if (i > 0) qp[i] += a_ref;
        }
        dq[0] = qp[0] - 5.0 * qp[1] + 10.0 * qp[2] - 10.0 * qp[3] + 5.0 * qp[4] - qp[5];
        dq[1] = 5.0 * qp[1] - 20.0 * qp[2] + 30.0 * qp[3] - 20.0 * qp[4] + 5.0 * qp[5];
        dq[2] = 10.0 * qp[2] - 30.0 * qp[3] + 30.0 * qp[4] - 10.0 * qp[5];
        dq[3] = 10.0 * qp[3] - 20.0 * qp[4] + 10.0 * qp[5];
        dq[4] = 5.0 * qp[4] - 5.0 * qp[5];
        dq[5] = qp[5];
        if (last) dq[5] -= 2.0 * t * (ddref * rend + dref * drend);
        // dP x = sum_d 2 t^p_d dw_d MU_d x (unit table d; recomputed per tangent)
        UNROLL for (int i = 0; i < 6; i++) dPc[i] = 0.0;
        if (a.shared_dot) {
          UNROLL for (int dd = 0; dd < 4; dd++) {
            const double cf = tp[dd] * dw[dd];
            UNROLL for (int i = 0; i < 6; i++) {
              double s = 0.0;
              UNROLL for (int j = 0; j < 6; j++) s += mu[21 * dd + (i <= j ? SYM(i, j) : SYM(j, i))] * c[j];
              dPc[i] += cf * s;
            }
          }
        }
        if (last) dPc[5] += 2.0 * t2 * dwe * c[5];
      }
      // ---- right-hand side in control-point space: -(dP x + dq) - P dx_p ----
      double f[6];
      UNROLL for (int i = 0; i < 6; i++)
        f[i] = -(dPc[i] + dq[i]) - (HSYM(Pk, i, 0) * xp[0] + HSYM(Pk, i, 1) * xp[1] + HSYM(Pk, i, 2) * xp[2]);

      // ---- passes of the method of multipliers (the backward kernel's, with the constraint target d) ----
      double v[6];   // dx_h in control-point space (this segment)
      for (int pass = 0; pass < GRAD_PASSES; ++pass) {
        double h[6];
        UNROLL for (int i = 0; i < 6; i++) h[i] = f[i];
        GRAD_ROWS(r)
          row_scatter<r>(rho[ri_] * d[ri_] - w[ri_], t, h);
        GRAD_END
        if (!act) { UNROLL for (int i = 0; i < 6; i++) h[i] = 0.0; }
        double u[3];
        {
          double un[3], nun[3];
          VT_apply(nm, h[3], h[4], h[5], u);
          UT_apply(nm, h[0], h[1], h[2], un);
          from_next(g, un, nun);
          UNROLL for (int i = 0; i < 3; i++) u[i] += last ? 0.0 : nun[i];
        }
        sweep_forward(g, K, u);
        double X[3] = {0.0, 0.0, 0.0};
        sweep_backward(g, F, K, u, last, X);
        double Xp[3];
        from_prev(g, X, Xp);   // (dx_p carries the initial state: 0 for segment 0)
        U_apply(nm, Xp, v[0], v[1], v[2]);
        V_apply(nm, X, v[3], v[4], v[5]);
        GRAD_ROWS(r)
          w[ri_] += rho[ri_] * (row_dot<r>(v, t) - d[ri_]);
        GRAD_END
      }
      // ---- dx = dx_h + dx_p, dcost = (P x + q)' dx + x' dP x / 2 + dq' x ----
      double dc = 0.0;
      UNROLL for (int i = 0; i < 6; i++) {
        v[i] = act ? v[i] + xp[i] : 0.0;
        dc += gx[i] * v[i] + c[i] * (0.5 * dPc[i] + dq[i]);
      }
      const double sc = sum1(g, nn, act ? dc : 0.0);
      // this axis' share of cost_dot: long_cost_dot_kernel adds the two (s + l)
      if (cand_in && k == 0 && cost_ws) cost_ws[((size_t)axis * a.T + tau) * a.B + b] = ok ? sc : 0.0;
      if (slot && a.ctrl_dot) {
        double *o = a.ctrl_dot + tb * 12 * a.seg_stride + o_ctrl;
        UNROLL for (int i = 0; i < 6; i++) o[i] = v[i];
      }
    }
  }
#undef VLO
#undef VUP
}

#define LG_PLACE                                                                                          \
  __shared__ double rm[4][LG_LANES];                                                                      \
  __shared__ double edge[4][LG_EDGE];                                                                     \
  __shared__ double carry[6];                                                                             \
  Wg g;                                                                                                   \
  g.lane = threadIdx.x & 63;                                                                              \
  g.wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));                                         \
  g.W = (int)(blockDim.x >> 6);                                                                           \
  g.K = 64 * g.wv + g.lane;                                                                               \
  g.steps = 0;                                                                                            \
  g.edge = edge; g.carry = carry; g.rm = rm

__global__ __launch_bounds__(256) void long_vjp_kernel(const VjpArgs a) {
  LG_PLACE;
  long_grad_body<VjpArgs>(a, nullptr, g);
}

__global__ __launch_bounds__(256) void long_jvp_kernel(const JvpArgs a, double *cost_ws) {
  LG_PLACE;
  long_grad_body<JvpArgs>(a, cost_ws, g);
}

__global__ __launch_bounds__(256) void long_cost_dot_kernel(const double *cost_ws, double *cost_dot, unsigned n) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) cost_dot[i] = cost_ws[i] + cost_ws[(size_t)n + i];
}

}  // namespace btrapz
