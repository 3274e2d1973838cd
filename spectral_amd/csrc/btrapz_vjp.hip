// btrapz_vjp.hip -- btrapz_solve_vjp_device: the vector-Jacobian product of a batched solve (include/btrapz_hip.h).
//
// Per axis problem, at the returned optimum x (the control points of the solve), with cotangents xbar (of ctrl) and cbar
// (of cost): xbar' = xbar + cbar (P x + q), and the adjoint system of the KKT conditions restricted to the active rows
//     [ P  A' ] [v]   [xbar']
//     [ A  0  ] [w] = [  0  ]
// (A: the continuity / initial-state equalities and the active inequality rows).  Then qbar = -v + cbar x,
// Pbar = -(v x' + x v') / 2 + cbar x x' / 2, and an active row's bound gets w; everything is chained through the
// assembly to the inputs.
//
// The equalities are eliminated exactly, as the solve does: v = Phi vX, vX the joint states (btrapz_ipm.h NullMap), so
// the system is block tridiagonal with 3x3 blocks.  The active rows enter by the method of multipliers:
//     (Phi' (P + G' D G) Phi) vX = Phi' (xbar' - G' w),   w += D G Phi vX,
// D = rho_r on active rows, rho_r = GRAD_RHO times the lane's largest diagonal entry of P over |g_r|^2.  Every pass
// divides the constraint error G v by about rho / |P|, while rho stays small enough (1e6) that the penalised matrix
// loses no more than about six digits to its condition.  One factorisation serves all passes.
//
// Mapping: that of the packed solve -- one lane per segment, a group of S lanes per axis problem, floor(64 / S) problems
// per wavefront, one axis per wavefront.  Ragged batches run groups of seg_stride lanes, the lanes beyond a candidate's
// segment count decoupled (the results are those of the uniform layout, bit for bit).  Reductions over a group:
// group_reduce (fixed order).  Each axis writes its own entries of every output: no atomics.
#include <hip/hip_runtime.h>
#include "btrapz_grad_rule.h"

namespace btrapz {

__global__ __launch_bounds__(64) void vjp_kernel(const VjpArgs a) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x;
  const int axis = blockIdx.x & 1;
  const int pair = blockIdx.x >> 1;
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
  // bounds that are no bounds: moved far out by the solve, never active, gradient 0
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

  // ---- P, q (begin_candidate), the control points and the cotangents ----
  double Pk[21], q[6], c[6], xb[6];
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
  const double cbar = (act && a.cost_bar) ? a.cost_bar[b] : 0.0;
  {
    const size_t o = (size_t)b * 12 * a.seg_stride + (size_t)axis * 6 * ns + (size_t)k * 6;
    UNROLL for (int i = 0; i < 6; i++) {
      c[i] = act ? a.ctrl[o + i] : 0.0;
      xb[i] = (act && a.ctrl_bar) ? a.ctrl_bar[o + i] : 0.0;
    }
  }
  double Pc[6];   // P x
  UNROLL for (int i = 0; i < 6; i++) {
    double s = 0.0;
    UNROLL for (int j = 0; j < 6; j++) s += HSYM(Pk, i, j) * c[j];
    Pc[i] = s;
  }
  UNROLL for (int i = 0; i < 6; i++) xb[i] += cbar * (Pc[i] + q[i]);   // xbar'

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
    UNROLL for (int i = 0; i < 3; i++) { const double vv = dpp_prev(X[i]); Xp[i] = first ? 0.0 : vv; }   // (the initial state is given)
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
  double own0[4] = {0.0, 0.0, 0.0, 0.0};      // (this segment's own row-0 / row-6 amounts come from the previous lane)
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
  UNROLL for (int i = 0; i < 4; i++) { const double vv = dpp_prev(to_next[i]); own0[i] = first ? 0.0 : vv; }
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

  // ---- per-candidate sums over the group (fixed order), then the stores ----
  auto m0 = [&](double x) { return act ? x : 0.0; };
  const Red4 s0 = group_reduce<0, 0, 0, 0>(red, lane, gbase, k, Sg, m0(g_w[0]), m0(g_w[1]), m0(g_w[2]), m0(g_w[3]));
  const Red4 s1 = group_reduce<0, 0, 0, 0>(red, lane, gbase, k, Sg, m0(g_dref), m0(g_alo), m0(g_ahi), m0(g_jlo));
  const Red4 s2 = group_reduce<0, 0, 0, 0>(red, lane, gbase, k, Sg, m0(g_jhi), m0(g_dl[0]), m0(g_dl[1]), m0(g_dl[2]));
  const Red4 s3 = group_reduce<0, 0, 0, 0>(red, lane, gbase, k, Sg, m0(g_dl[3]), m0(g_dl[4]), m0(g_dl[5]), m0(g_dl[6]));
  const Red4 s4 = group_reduce<0, 0, 0, 0>(red, lane, gbase, k, Sg, m0(g_dl[7]), m0(g_dl[8]), m0(g_dl[9]), m0(g_we));
  if (!cand_in) return;
  if (a.g_seg) {
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
  if (a.g_ref_end && k == (ns - 1 < Sg ? ns - 1 : Sg - 1)) a.g_ref_end[(size_t)b * 2 + axis] = ok ? g_rend : 0.0;
  if (k != 0) return;
  if (a.g_init) UNROLL for (int i = 0; i < 3; i++) a.g_init[(size_t)b * 6 + axis * 3 + i] = ok ? g_init[i] : 0.0;
  if (a.g_dl && axis == 1) {
    const double d10[10] = {s2.b, s2.c, s2.d, s3.a, s3.b, s3.c, s3.d, s4.a, s4.b, s4.c};
    UNROLL for (int i = 0; i < 10; i++) a.g_dl[(size_t)b * 10 + i] = ok ? d10[i] : 0.0;
  }
  if (a.g_shared) {
    double *gsh = a.g_shared + (size_t)b * 20;
    // layout.Shared.as_array order: w_s[4] w_l[4] weight_end_s weight_end_l ds_ref dl_ref dds[2] ddds[2] ddl[2] dddl[2]
    const double wv[4] = {s0.a, s0.b, s0.c, s0.d};
    UNROLL for (int d = 0; d < 4; d++) gsh[4 * axis + d] = ok ? wv[d] : 0.0;
    gsh[8 + axis] = ok ? s4.d : 0.0; gsh[10 + axis] = ok ? s1.a : 0.0;
    gsh[12 + 4 * axis] = ok ? s1.b : 0.0; gsh[13 + 4 * axis] = ok ? s1.c : 0.0;
    gsh[14 + 4 * axis] = ok ? s1.d : 0.0; gsh[15 + 4 * axis] = ok ? s2.a : 0.0;
  }
#undef VLO
#undef VUP
}

}  // namespace btrapz
