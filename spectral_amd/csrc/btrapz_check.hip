// btrapz_check.hip -- btrapz_check_rows_device: the audit of given control points against every row of their QP
// (include/btrapz_hip_check.h).
//
// The rows are the reference's own, row by row, as the oracle's assembly states them from a batch record (solve_3d.cc:
// 779-1129, cuboid_3d.cc:632-988): 18 inequality rows per segment and axis, 3 initial-state rows, 3 continuity rows per
// joint.  NOT the solve's merged form (begin_candidate, btrapz_kernels.hip): the joint rows are not intersected with the
// next segment's, no bound is moved (move_far_bounds) -- a side of a row is dropped where its own bound is at least
// BTRAPZ_FAR in size, and nowhere else --, and the s axis' velocity interval is clipped to [0, 1000] as the reference
// clips it (solve_3d.cc:835-845).
//
// Mapping: vjp_kernel's -- one lane per segment slot, a group of seg_stride lanes per candidate, floor(64 / seg_stride)
// candidates per wavefront, the record read field-major -- but both axes in the same lane, one after the other, so that
// obj (a sum over both) needs no second wavefront.  Beyond 64 slots: one candidate per wavefront, lane k takes the
// segments k, k + 64, ...; the same per-segment statements.  A lane reads its own six control points and the first three
// of the next segment straight from ctrl: no cross-lane traffic before the per-candidate reduction.
//
// Reduction: lane k <- lane k + d, d = 1, 2, 4, ..., over the lanes that hold a segment.  The margins travel as (value,
// row) pairs under the total order "smaller value, then lower row", the residuals as maxima: neither depends on the
// order.  obj is a sum: its tree is over the segment index alone (a lane beyond the candidate's count takes no part), so
// a candidate's bits do not depend on the group's width or on its place in the wavefront.
#include <hip/hip_runtime.h>
#include "btrapz_ipm.h"

namespace btrapz {

#define CHECK_NO_ROW 0x7fffffff

// a value that is no number fails every test a caller writes: the margin of such a row is -inf, such a residual +inf
__device__ __forceinline__ double nan_to(double v, double w) { return v != v ? w : v; }
// a side of a row is there unless its own bound is at least BTRAPZ_FAR in size (a NaN bound stays, and poisons the row)
__device__ __forceinline__ bool side_kept(double bound) { return !(fabs(bound) >= BTRAPZ_FAR); }
// a header limit the host moved to +-BTRAPZ_FAR_LIMIT (fill_parameters) was at least BTRAPZ_FAR in size: no limit
__device__ __forceinline__ bool limit_kept(double lim, double bound) { return fabs(lim) != BTRAPZ_FAR_LIMIT && side_kept(bound); }

struct RowMin { double m; int row; };
__device__ __forceinline__ void row_take(RowMin &w, double gx, double lo, bool has_lo, double up, bool has_up, double scale, int row) {
  const double inf = __builtin_huge_val();
  double m = fmin(has_lo ? nan_to(gx - lo, -inf) : inf, has_up ? nan_to(up - gx, -inf) : inf) * scale;
  m = nan_to(m, -inf);
  if (m < w.m) { w.m = m; w.row = row; }   // (rows come in rising order: the lowest row keeps a tie)
}
__device__ __forceinline__ void row_merge(RowMin &w, double m, int row) {
  if (m < w.m || (m == w.m && row < w.row)) { w.m = m; w.row = row; }
}

__global__ __launch_bounds__(64) void check_rows_kernel(const CheckArgs a) {
  const double inf = __builtin_huge_val();
  const int lane = threadIdx.x;
  const int Sg = a.seg_stride < 64 ? a.seg_stride : 64;   // lanes per group
  const int gpw = 64 / Sg;
  const int g = lane / Sg, k0 = lane - g * Sg;
  const bool lane_in_group = g < gpw;
  const long long cand = (long long)blockIdx.x * gpw + (lane_in_group ? g : gpw - 1);
  const bool cand_in = lane_in_group && cand < a.B;
  const int b = cand < a.B ? (int)cand : a.B - 1;
  const int n = a.seg_count ? a.seg_count[b] : a.seg_stride;
  const int set = a.set_index ? a.set_index[b] : 0;
  const bool usable = n >= 1 && n <= a.seg_stride && set >= 0 && set < a.n_sets;
  const bool act = cand_in && usable;
  const int nn = act ? (n < 64 ? n : 64) : 0;             // lanes of the group that hold a segment
  const size_t BS = (size_t)a.B * a.seg_stride;
  const Shared &sh = a.sets[usable ? set : 0];
  const int variant = sh.variant;
  const double *sg = a.seg;
  const double unit_c[3] = {a.unit ? 0.1414213562373095 : 1.0,      // 1 / sqrt(50)
                            a.unit ? 0.02041241452319315 : 1.0,     // 1 / sqrt(2400)
                            a.unit ? 0.003726779962499649 : 1.0};   // 1 / sqrt(72000)

  bool bad = false;      // this lane met a non-finite control point or a duration that is none
  double obj = 0.0;
  for (int axis = 0; axis < 2; ++axis) {
    const double *mq = a.mqm + (size_t)(usable ? set : 0) * 168 + axis * 84;
    const double acc_lo = axis == 0 ? sh.acc_s[0] : sh.acc_l[0], acc_hi = axis == 0 ? sh.acc_s[1] : sh.acc_l[1];
    const double jrk_lo = axis == 0 ? sh.jerk_s[0] : sh.jerk_l[0], jrk_hi = axis == 0 ? sh.jerk_s[1] : sh.jerk_l[1];
    const double we = axis == 0 ? sh.weight_end_s : sh.weight_end_l;
    const double wr = axis == 0 ? sh.w_s[0] : sh.w_l[0], wd = axis == 0 ? sh.w_s[1] : sh.w_l[1];
    const double dref = axis == 0 ? sh.ds_ref : sh.dl_ref;
    RowMin w[4] = {{inf, CHECK_NO_ROW}, {inf, CHECK_NO_ROW}, {inf, CHECK_NO_ROW}, {inf, CHECK_NO_ROW}};
    double eq_init = 0.0, eq_joint = 0.0;
    for (int k = k0; act && k < n; k += 64) {   // (one pass unless seg_stride > 64)
      const bool first = k == 0, last = k == n - 1;
      const size_t e = (size_t)b * a.seg_stride + k;
      const double t = sg[BTRAPZ_F_T * BS + e];
      const double tn = last ? 1.0 : sg[BTRAPZ_F_T * BS + e + 1];
      if (!(t > 0.0) || !(t < inf)) bad = true;
      // ---- control points: this segment's six, the next one's first three (16-byte loads: the offsets are even) ----
      double c[6], cn[3] = {0.0, 0.0, 0.0};
      {
        const double *p = a.ctrl + (size_t)b * 12 * a.seg_stride + (size_t)axis * 6 * n + (size_t)k * 6;
        const double2 c01 = *reinterpret_cast<const double2 *>(p), c23 = *reinterpret_cast<const double2 *>(p + 2),
                      c45 = *reinterpret_cast<const double2 *>(p + 4);
        c[0] = c01.x; c[1] = c01.y; c[2] = c23.x; c[3] = c23.y; c[4] = c45.x; c[5] = c45.y;
        if (!last) {
          const double2 n01 = *reinterpret_cast<const double2 *>(p + 6);
          cn[0] = n01.x; cn[1] = n01.y; cn[2] = p[8];
        }
        UNROLL for (int i = 0; i < 6; i++) if (!(fabs(c[i]) < inf)) bad = true;
      }
      // ---- the record ----
      double lb, ls, ub, us, begl = 0.0, endl = 0.0, vlo[5], vhi[5];
      if (axis == 0) {
        lb = sg[BTRAPZ_F_DOWN_BIAS * BS + e]; ls = sg[BTRAPZ_F_DOWN_SKEW * BS + e];
        ub = sg[BTRAPZ_F_UPP_BIAS * BS + e];  us = sg[BTRAPZ_F_UPP_SKEW * BS + e];
        // solve_3d.cc:835-845: the knots' intervals cut into [0, 1000]
        const double dlo = fmax(sg[BTRAPZ_F_DS_LO * BS + e], 0.0), dhi = fmin(sg[BTRAPZ_F_DS_HI * BS + e], 1000.0);
        UNROLL for (int i = 0; i < 5; i++) { vlo[i] = dlo; vhi[i] = dhi; }
      } else {
        lb = sg[BTRAPZ_F_L_DOWN_BIAS * BS + e]; ls = sg[BTRAPZ_F_L_DOWN_SKEW * BS + e];
        ub = sg[BTRAPZ_F_L_UPP_BIAS * BS + e];  us = sg[BTRAPZ_F_L_UPP_SKEW * BS + e];
        if (variant == BTRAPZ_CUBOID) { begl = sg[BTRAPZ_F_BEG_L * BS + e]; endl = sg[BTRAPZ_F_END_L * BS + e]; }
        // :1003-1004: dy_bounds_ indexed by the control point
        UNROLL for (int i = 0; i < 5; i++) { vlo[i] = a.dl_bounds[(size_t)b * 10 + 2 * i]; vhi[i] = a.dl_bounds[(size_t)b * 10 + 2 * i + 1]; }
      }
      const double skew = sg[(axis == 0 ? BTRAPZ_F_X_SKEW : BTRAPZ_F_Y_SKEW) * BS + e];
      const double bias = sg[(axis == 0 ? BTRAPZ_F_X_BIAS : BTRAPZ_F_Y_BIAS) * BS + e];
      // ---- position rows: lo_i = bias + skew (i / 5) t (:827-828, 965-966); cuboid: the inscribed s interval in [0, 100]
      //      (cuboid_3d.cc:677-697), beg_l / end_l (:826-827) ----
      double plo[6], phi[6];
      UNROLL for (int i = 0; i < 6; i++) { plo[i] = lb + ls * ((double)i / 5.0) * t; phi[i] = ub + us * ((double)i / 5.0) * t; }
      if (variant == BTRAPZ_CUBOID) {
        double lo = 0.0, hi = 100.0;
        UNROLL for (int i = 0; i < 6; i++) { lo = fmax(lo, plo[i]); hi = fmin(hi, phi[i]); }
        if (axis != 0) { lo = begl; hi = endl; }
        UNROLL for (int i = 0; i < 6; i++) { plo[i] = lo; phi[i] = hi; }
      }
      const double t2 = t * t;
      const double alo = acc_lo * t, ahi = acc_hi * t, jlo = jrk_lo * t * t, jhi = jrk_hi * t * t;
      const bool alo_k = limit_kept(acc_lo, alo), ahi_k = limit_kept(acc_hi, ahi);
      const bool jlo_k = limit_kept(jrk_lo, jlo), jhi_k = limit_kept(jrk_hi, jhi);
      const double pos_scale = a.unit ? 1.0 / t : 1.0;
      const int row0 = 18 * k;
      static_for<18>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const double gx = row_dot<r>(c, t);
        if constexpr (r < 6) row_take(w[0], gx, plo[r], side_kept(plo[r]), phi[r], side_kept(phi[r]), pos_scale, row0 + r);
        else if constexpr (r < 11) row_take(w[1], gx, vlo[r - 6], side_kept(vlo[r - 6]), vhi[r - 6], side_kept(vhi[r - 6]), unit_c[0], row0 + r);
        else if constexpr (r < 15) row_take(w[2], gx, alo, alo_k, ahi, ahi_k, unit_c[1], row0 + r);
        else row_take(w[3], gx, jlo, jlo_k, jhi, jhi_k, unit_c[2], row0 + r);
      });
      // ---- equality rows: the initial state (:896-912), the joint with the next segment (:918-949) ----
      if (first) {
        const double *in = a.init + (size_t)b * 6 + axis * 3;
        eq_init = fmax(eq_init, nan_to(fabs(t * c[0] - in[0]), inf));
        eq_init = fmax(eq_init, nan_to(fabs(5.0 * (c[1] - c[0]) - in[1]), inf));
        eq_init = fmax(eq_init, nan_to(fabs(20.0 * ((c[0] - 2.0 * c[1]) + c[2]) - in[2] * t), inf));
      }
      if (!last) {
        eq_joint = fmax(eq_joint, nan_to(fabs(tn * cn[0] - t * c[5]), inf));
        eq_joint = fmax(eq_joint, nan_to(fabs((c[5] - c[4]) + (cn[0] - cn[1])), inf));
        eq_joint = fmax(eq_joint, nan_to(fabs(tn * ((c[3] - 2.0 * c[4]) + c[5]) - t * ((cn[0] - 2.0 * cn[1]) + cn[2])), inf));
      }
      // ---- 0.5 x'Px + q'x of the segment: P from the set's M'QM tables, q as begin_candidate states it ----
      if (a.obj) {
        // 0.5 x'Px = sum_d t^p_d x' (M'QM)_d x, p = 3, 1, -1, -3, one table at a time (all four at once
        // cost the kernel its second wavefront per SIMD; two at a time measured 7 % slower), and the end weight on the last control point (:164-168)
        const double it = 1.0 / t, it3 = it * it * it;
        const double tp[4] = {t2 * t, t, it, it3};
        double o = 0.0;
        _Pragma("unroll 1") for (int d = 0; d < 4; d++) {
          const double *m = mq + 21 * d;
          double s = 0.0;
          UNROLL for (int j = 0; j < 6; j++) {
            double col = 0.5 * m[SYM(j, j)] * c[j];
            UNROLL for (int i = 0; i < j; i++) col += m[SYM(i, j)] * c[i];
            s += col * c[j];
          }
          o += (d == 0 ? tp[0] : d == 1 ? tp[1] : d == 2 ? tp[2] : tp[3]) * (2.0 * s);
        }
        if (last) o += we * t2 * (c[5] * c[5]);
        double q[6], qp[6];
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
        if (last) q[5] -= dref * 2.0 * a.ref_end[(size_t)b * 2 + axis] * t;
        UNROLL for (int i = 0; i < 6; i++) o += q[i] * c[i];
        obj += o;
      }
    }
    // ---- the axis' figures of every candidate of the wavefront: lane k <- lane k + d within a group ----
    for (int d = 1; d < Sg; d <<= 1) {
      double m4[4], e0, e1;
      int r4[4];
      UNROLL for (int i = 0; i < 4; i++) { m4[i] = __shfl_down(w[i].m, d); r4[i] = __shfl_down(w[i].row, d); }
      e0 = __shfl_down(eq_init, d); e1 = __shfl_down(eq_joint, d);
      if (k0 + d < nn) {
        UNROLL for (int i = 0; i < 4; i++) row_merge(w[i], m4[i], r4[i]);
        eq_init = fmax(eq_init, e0); eq_joint = fmax(eq_joint, e1);
      }
    }
    // (a candidate that turns out to be no candidate: overwritten below, by this lane)
    if (cand_in && k0 == 0) {
      const size_t o = (size_t)b * 8 + (size_t)axis * 4;
      if (a.margin) UNROLL for (int i = 0; i < 4; i++) a.margin[o + i] = w[i].m;
      if (a.worst) UNROLL for (int i = 0; i < 4; i++) a.worst[o + i] = w[i].row == CHECK_NO_ROW ? -1 : w[i].row;
      if (a.eq_res) { a.eq_res[(size_t)b * 4 + axis * 2] = eq_init; a.eq_res[(size_t)b * 4 + axis * 2 + 1] = eq_joint; }
    }
  }
  for (int d = 1; d < Sg; d <<= 1) {
    const double v = __shfl_down(obj, d);
    if (k0 + d < nn) obj += v;
  }
  // ---- the defined values of what is no candidate: a count or set out of range, a non-finite control point, t <= 0 ----
  const unsigned long long bad_lanes = __ballot(bad);
  const unsigned long long group = (Sg == 64 ? ~0ull : ((1ull << Sg) - 1ull)) << (lane_in_group ? g * Sg : 0);
  const bool none = !usable || (bad_lanes & group) != 0ull;
  if (!cand_in || k0 != 0) return;
  if (none) {
    if (a.margin) UNROLL for (int i = 0; i < 8; i++) a.margin[(size_t)b * 8 + i] = -inf;
    if (a.worst) UNROLL for (int i = 0; i < 8; i++) a.worst[(size_t)b * 8 + i] = -1;
    if (a.eq_res) UNROLL for (int i = 0; i < 4; i++) a.eq_res[(size_t)b * 4 + i] = inf;
  }
  if (a.obj) a.obj[b] = none ? inf : obj;
}

}  // namespace btrapz
