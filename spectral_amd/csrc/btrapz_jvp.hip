// btrapz_jvp.hip -- btrapz_solve_jvp_device: Jacobian-vector products of a batched solve (include/btrapz_hip.h), the
// forward-mode mirror of btrapz_vjp.hip, for T tangents per candidate in one launch.
//
// Per axis problem, at the returned optimum x with the active rows of the solve (vjp_kernel's rule: multiplier above
// slack), the rows G do not depend on any differentiated input, so the tangent of the KKT conditions is
//     [ P  A' ] [dx ]   [-(dP x + dq)]
//     [ A  0  ] [dmu] = [    db_A    ]
// with dP, dq, db the assembly applied to the input tangents -- the partial derivatives vjp_kernel applies transposed --
// and dcost = (P x + q)' dx + x' dP x / 2 + dq' x.  The matrix is the VJP's (it is symmetric), so J here is the exact
// transpose of the VJP's J'.
//
// The equalities are eliminated as there: dx = Phi dX + dx_p, dX the tangents of the joint states and dx_p = U dX_init
// the particular solution's tangent (segment 0 only).  With dx_h = Phi dX and d = db_A - G dx_p the method of multipliers
// reads
//     (Phi' (P + G' D G) Phi) dX = Phi' (-(dP x + dq) - P dx_p + G' (D d - w)),   w += D (G dx_h - d),
// D = rho_r on active rows (the VJP's rho).  The record, the bounds, P, the active set and the penalised block-tridiagonal
// matrix are built ONCE and factorised ONCE per axis problem; the factor (K, F: 15 doubles per lane) stays in registers
// while the kernel loops over the T tangents: right-hand side, GRAD_PASSES passes, back-substitution, store.
//
// Mapping: vjp_kernel's -- one lane per segment, a group of S lanes per axis problem, floor(64 / S) problems per
// wavefront, one axis per wavefront; ragged lanes beyond a candidate's count decoupled.  A workgroup is the two wavefronts
// (s axis, l axis) of the same candidates, so that cost_dot -- the one output both axes contribute to -- is summed through
// LDS in a fixed order (s + l) and written by one lane.  Every other entry is written by the lane that owns it: no atomics.
#include <hip/hip_runtime.h>
#include "btrapz_grad_rule.h"

namespace btrapz {

__global__ __launch_bounds__(128) void jvp_kernel(const JvpArgs a) {
  __shared__ double red_[2][4][64];
  __shared__ double cst[2][BTRAPZ_MAX_TANGENTS][64];   // [axis][tangent][group]: the axes' shares of cost_dot
  const int lane = threadIdx.x & 63;
  const int axis = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double (*red)[64] = red_[axis];
  const int pair = blockIdx.x;
  const int Sg = a.S;                       // lanes per group
  const int gpw = 64 / Sg;
  const int g = lane / Sg, k = lane - g * Sg;
  const bool lane_in_group = g < gpw;
  const int gl = lane_in_group ? g : gpw - 1;
  const int gbase = gl * Sg;
  const long long cand = (long long)pair * gpw + gl;
  const bool cand_in = lane_in_group && cand < a.B;
  const int b = cand < a.B ? (int)cand : a.B - 1;
  const int n = a.seg_count ? a.seg_count[b] : Sg;
  const int set = a.set_index ? a.set_index[b] : 0;
  const int st = a.status[b];
  // the candidate is differentiated: solved (1 or 2), with a usable segment count and set
  const bool ok = cand_in && n >= 1 && n <= Sg && set >= 0 && set < a.n_sets && (st == BTRAPZ_SOLVED || st == BTRAPZ_SOLVED_INACCURATE);
  const bool act = ok && k < n;             // this lane holds a real segment
  const bool first = k == 0, last = k == n - 1;
  const int ns = (n >= 1 && n <= Sg) ? n : Sg;   // (control-point offsets of the l axis)
  const size_t BS = (size_t)a.B * a.seg_stride;
  const size_t e = (size_t)b * a.seg_stride + k;
  const Shared &sh = a.sets[(set >= 0 && set < a.n_sets) ? set : 0];
  const double *mq = a.mqm + (size_t)((set >= 0 && set < a.n_sets) ? set : 0) * 168 + axis * 84;
  const double *mu = a.mqm_unit + axis * 84;
  const int variant = sh.variant;

  // ---- the record, the rows and their bounds (begin_candidate), with the derivative of every bound: as vjp_kernel ----
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
  // bounds that are no bounds: moved far out by the solve, never active, their tangent ignored
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
    const double nplo = dpp_next(plo0), nphi = dpp_next(phi0), nvlo = dpp_next(vlo[0]), nvhi = dpp_next(vhi[0]);
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
  {
    const size_t o = (size_t)b * 12 * a.seg_stride + (size_t)axis * 6 * ns + (size_t)k * 6;
    UNROLL for (int i = 0; i < 6; i++) c[i] = act ? a.ctrl[o + i] : 0.0;
  }
  double gx[6];   // P x + q: the gradient of the cost in x
  UNROLL for (int i = 0; i < 6; i++) {
    double s = 0.0;
    UNROLL for (int j = 0; j < 6; j++) s += HSYM(Pk, i, j) * c[j];
    gx[i] = s + q[i];
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
    UNROLL for (int i = 0; i < 6; i++) { const double v = dpp_next(M00[i]); T[i] += last ? 0.0 : v; }
  }
  // ---- block LDL^T, downwards (step s: lane s of every group): S_k = T_k - Z_(k-1), K_k = S_k^-1 Mc, Z_k = Mc' K_k,
  //      Mc = M01_(k+1) (0 for the last segment) ----
  double F[6] = {0.0, 0.0, 0.0, 1.0, 1.0, 1.0}, K[9], Mc[9];
  {
    double Z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    UNROLL for (int i = 0; i < 9; i++) { const double v = dpp_next(M01[i]); Mc[i] = last ? 0.0 : v; K[i] = 0.0; }
    for (int s = 0; s < Sg; ++s) {
      double pZ[6];
      UNROLL for (int i = 0; i < 6; i++) { const double v = dpp_prev(Z[i]); pZ[i] = first ? 0.0 : v; }
      if (k == s) {
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
  }

  const double tp[4] = {2.0 * t3, 2.0 * t, 2.0 * it, 2.0 * it3};
  const bool cub_l = variant == BTRAPZ_CUBOID && axis == 1;
  // fields of this axis in seg_dot
  const int f_lb = axis == 0 ? BTRAPZ_F_DOWN_BIAS : cub_l ? BTRAPZ_F_BEG_L : BTRAPZ_F_L_DOWN_BIAS;
  const int f_ub = axis == 0 ? BTRAPZ_F_UPP_BIAS : cub_l ? BTRAPZ_F_END_L : BTRAPZ_F_L_UPP_BIAS;
  const int f_ls = axis == 0 ? BTRAPZ_F_DOWN_SKEW : BTRAPZ_F_L_DOWN_SKEW, f_us = axis == 0 ? BTRAPZ_F_UPP_SKEW : BTRAPZ_F_L_UPP_SKEW;
  const int f_skew = axis == 0 ? BTRAPZ_F_X_SKEW : BTRAPZ_F_Y_SKEW, f_bias = axis == 0 ? BTRAPZ_F_X_BIAS : BTRAPZ_F_Y_BIAS;
  const size_t o_own = (size_t)axis * 6 * ns + (size_t)k * 6;                                       // k < ns: this segment's slots
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
      const double n_plo = dpp_next(dplo0), n_phi = dpp_next(dphi0), n_vlo = dpp_next(dvl[0]), n_vhi = dpp_next(dvh[0]);
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
      // dP x = sum_d 2 t^p_d dw_d MU_d x (unit table d; recomputed per tangent: 24 more live doubles would not fit)
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

    // ---- passes of the method of multipliers (vjp_kernel's, with the constraint target d) ----
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
        double un[3];
        VT_apply(nm, h[3], h[4], h[5], u);
        UT_apply(nm, h[0], h[1], h[2], un);
        UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_next(un[i]); u[i] += last ? 0.0 : vv; }
      }
      // forward: u_k -= K_(k-1)' u_(k-1)
      {
        double fw[3] = {0.0, 0.0, 0.0};
        for (int s = 0; s < Sg; ++s) {
          double pw[3];
          UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_prev(fw[i]); pw[i] = first ? 0.0 : vv; }
          if (k == s) {
            UNROLL for (int i = 0; i < 3; i++) u[i] -= pw[i];
            fw[0] = K[0] * u[0] + K[3] * u[1] + K[6] * u[2];
            fw[1] = K[1] * u[0] + K[4] * u[1] + K[7] * u[2];
            fw[2] = K[2] * u[0] + K[5] * u[1] + K[8] * u[2];
          }
        }
      }
      // backward: X_k = S_k^-1 u_k - K_k X_(k+1)
      double X[3] = {0.0, 0.0, 0.0};
      {
        ldl3_solve(F, u[0], u[1], u[2], X[0], X[1], X[2]);
        double y[3] = {0.0, 0.0, 0.0};
        for (int s = Sg - 1; s >= 0; --s) {
          double ny[3];
          UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_next(y[i]); ny[i] = last ? 0.0 : vv; }
          if (k == s) {
            UNROLL for (int i = 0; i < 3; i++) X[i] -= K[3 * i] * ny[0] + K[3 * i + 1] * ny[1] + K[3 * i + 2] * ny[2];
            UNROLL for (int i = 0; i < 3; i++) y[i] = X[i];
          }
        }
      }
      double Xp[3];
      UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_prev(X[i]); Xp[i] = first ? 0.0 : vv; }   // (dx_p carries the initial state)
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
    const Red4 sc = group_reduce<0, 0, 0, 0>(red, lane, gbase, k, Sg, act ? dc : 0.0, 0.0, 0.0, 0.0);
    if (k == 0 && lane_in_group) cst[axis][tau][g] = sc.a;
    if (cand_in && a.ctrl_dot) {
      double *o = a.ctrl_dot + tb * 12 * a.seg_stride + o_ctrl;
      UNROLL for (int i = 0; i < 6; i++) o[i] = v[i];
    }
  }

  // ---- cost_dot: the s axis wavefront adds the l axis' share (fixed order) ----
  __syncthreads();
  if (axis == 0 && k == 0 && cand_in && a.cost_dot)
    for (int tau = 0; tau < a.T; ++tau) a.cost_dot[(size_t)tau * a.B + b] = ok ? cst[0][tau][g] + cst[1][tau][g] : 0.0;
#undef VLO
#undef VUP
}

}  // namespace btrapz
