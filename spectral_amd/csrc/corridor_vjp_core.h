// corridor_vjp_core.h -- the backward pass of the corridor stage, the part compiled for host AND device.
//
// With its decisions frozen (where a segment opens, which segments the reference line selects, their order, the spans
// the overlap step leaves) the stage is a sparse linear map from the per-knot bounds and reference lines to the batch
// record: every differentiated field of output segment k is a copy, a difference quotient or a `bias + h * skew` of two
// or three knot values, the ds fields a max / min over a knot range.  What the transpose needs is the PROVENANCE of
// segment k: the obstacle o, the knot i0 at which its base segment opened (extract_segments_core) and the number h of
// one-second pieces CorridorSplit peeled in front of it.  It travels in Seg::count, which the stage sets at the selection,
// never compares (same_segment does not read it) and never stores in the record: 6 + 9 + 6 bits within the wave-wide
// kernels' limits (64 obstacles, 512 knots, hence at most 51 pieces).
// segment_adjoint() below is the whole per-segment transpose; corridor.cpp (btrapz_corridor_vjp_host) and
// corridor_vjp.hip (corridor_vjp_kernel) call it on the segments their -- identical -- decisions leave.
// segment_tangent() is the same map read forwards, one direction at a time (btrapz_corridor_jvp_host, corridor_jvp.hip).
#ifndef BTRAPZ_CORRIDOR_VJP_CORE_H
#define BTRAPZ_CORRIDOR_VJP_CORE_H

#include <stddef.h>

#include "../../include/btrapz_hip.h"
#include "corridor_core.h"

namespace btrapz {

// The capacities the wave-wide forward ends on (its retry pass, corridor_kernels.hip: MAX_ALL, MAX_SEL): a candidate
// beyond them has seg_count = -1 there and no gradient here.
enum { VJP_MAX_ALL = 160, VJP_MAX_SEL = 64, VJP_MAX_KNOTS = 512, VJP_MAX_OBS = 64 };

BTRAPZ_HD int provenance_pack(int o, int in_obstacle) { return (o << 15) | in_obstacle; }
BTRAPZ_HD int provenance_obstacle(int p) { return (p >> 15) & 63; }
BTRAPZ_HD int provenance_knot(int p) { return (p >> 6) & 511; }
BTRAPZ_HD int provenance_pieces(int p) { return p & 63; }
// extract_segments_core's note: (i0, h) of every segment it writes, left in the segment's count
struct ProvenanceNote {
  Seg *v;
  BTRAPZ_HD void operator()(int slot, int i0, int h) const { v[slot].count = (i0 << 6) | h; }
};

// The terms one output segment adds to the gradients, by output array; `p` numbers a segment's terms within an array
// (a compile-time constant at every call below).  An index is the entry's offset inside the candidate's block of the array.
enum { VJP_G_S = 0, VJP_G_L, VJP_G_DS, VJP_G_SREF, VJP_G_LREF, VJP_GROUPS };
enum { VJP_TERMS_S = 4, VJP_TERMS_L = 6, VJP_TERMS_DS = 2, VJP_TERMS_REF = 2 };

// Which knot of the span beg_t..end_t (clamped to the horizon, as the forward walks it) the ds_lo / ds_hi of a segment
// come from: the EARLIEST knot that attains the extreme; -1 when the default (0 below, 1000 above) attains it -- then
// nobody gets the gradient.  The extreme itself is the forward's walk, statement by statement.
BTRAPZ_HD void ds_extreme_knots(int N, int beg_t, int end_t, const double *dsb, int &at_lo, int &at_hi) {
  double lo = 0.0, hi = 1000.0;  // solve_3d.cc:835-841
  for (int i = beg_t; i <= end_t; i++) {
    const int ii = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    lo = fmax(dsb[2 * ii], lo);
    hi = fmin(dsb[2 * ii + 1], hi);
  }
  at_lo = -1; at_hi = -1;
  for (int i = end_t; i >= beg_t; i--) {
    const int ii = i < 0 ? 0 : (i > N - 1 ? N - 1 : i);
    if (lo > 0.0 && dsb[2 * ii] == lo) at_lo = ii;
    if (hi < 1000.0 && dsb[2 * ii + 1] == hi) at_hi = ii;
  }
}

// Transpose of the record of output segment k (c: the segment as the stage leaves it, provenance in c.count).
// bar: the cotangent of slot k, field f at bar[f * BS]; null: zero.  Field 0 (T) is an integer knot count times delta
// and is not differentiated.  sink.add(group, p, index, value): one term, index < 0 meaning "nobody".
template <class Sink>
BTRAPZ_HD void segment_adjoint(int variant, int N, double delta, int k, const Seg &c, const double *dsb, const double *bar,
                               size_t BS, Sink &sink) {
  const int o = provenance_obstacle(c.count), i0 = provenance_knot(c.count), h = provenance_pieces(c.count);
#define BAR_(f) (bar ? bar[(size_t)(f) * BS] : 0.0)
  // down_skew = (lo(i0 + 1) - lo(i0)) / delta, down_bias = lo(i0) + h additions of down_skew; upp_* with hi
  {
    const double db = BAR_(BTRAPZ_F_DOWN_BIAS), dk = BAR_(BTRAPZ_F_DOWN_SKEW), ub = BAR_(BTRAPZ_F_UPP_BIAS), uk = BAR_(BTRAPZ_F_UPP_SKEW);
    const double gd = ((double)h * db + dk) / delta, gu = ((double)h * ub + uk) / delta;   // to knot i0 + 1
    const int at = (o * N + i0) * 2;
    sink.add(VJP_G_S, 0, at, db - gd);
    sink.add(VJP_G_S, 1, at + 2, gd);
    sink.add(VJP_G_S, 2, at + 1, ub - gu);
    sink.add(VJP_G_S, 3, at + 3, gu);
  }
  // beg_l = llo(i0), end_l = lhi(i0); trapezoid: l_down_bias = llo(i0), l_down_skew the forward difference at knot 0 for
  // i0 = 0, else the backward difference at i0 (pieces inherit both); cuboid: the l lines are the defaults
  {
    const int i1 = i0 == 0 ? 1 : i0;
    const double ldb = variant == 0 ? BAR_(BTRAPZ_F_L_DOWN_BIAS) : 0.0, lub = variant == 0 ? BAR_(BTRAPZ_F_L_UPP_BIAS) : 0.0;
    const double ldk = variant == 0 ? BAR_(BTRAPZ_F_L_DOWN_SKEW) / delta : 0.0, luk = variant == 0 ? BAR_(BTRAPZ_F_L_UPP_SKEW) / delta : 0.0;
    const int at = (o * N + i0) * 2, at1 = (o * N + i1) * 2;
    sink.add(VJP_G_L, 0, at, ldb + BAR_(BTRAPZ_F_BEG_L));
    sink.add(VJP_G_L, 1, at + 1, lub + BAR_(BTRAPZ_F_END_L));
    sink.add(VJP_G_L, 2, variant == 0 ? at1 : -1, ldk);
    sink.add(VJP_G_L, 3, variant == 0 ? at1 - 2 : -1, -ldk);
    sink.add(VJP_G_L, 4, variant == 0 ? at1 + 1 : -1, luk);
    sink.add(VJP_G_L, 5, variant == 0 ? at1 - 1 : -1, -luk);
  }
  {
    int at_lo, at_hi;
    ds_extreme_knots(N, c.beg_t, c.end_t, dsb, at_lo, at_hi);
    sink.add(VJP_G_DS, 0, at_lo < 0 ? -1 : 2 * at_lo, BAR_(BTRAPZ_F_DS_LO));
    sink.add(VJP_G_DS, 1, at_hi < 0 ? -1 : 2 * at_hi + 1, BAR_(BTRAPZ_F_DS_HI));
  }
  {  // the reference line of second k: solve_3d.cc:1161-1165, clamped
    const int r0 = 10 * k > N - 1 ? N - 1 : 10 * k, r1 = 10 * k + 1 > N - 1 ? N - 1 : 10 * k + 1;
    const double xk = BAR_(BTRAPZ_F_X_SKEW) / delta, yk = BAR_(BTRAPZ_F_Y_SKEW) / delta;
    sink.add(VJP_G_SREF, 0, r0, BAR_(BTRAPZ_F_X_BIAS) - xk);
    sink.add(VJP_G_SREF, 1, r1, xk);
    sink.add(VJP_G_LREF, 0, r0, BAR_(BTRAPZ_F_Y_BIAS) - yk);
    sink.add(VJP_G_LREF, 1, r1, yk);
  }
#undef BAR_
}

// ---- forward mode (corridor_jvp.hip, btrapz_corridor_jvp_host): the same rules read forwards ----
// One direction's tangents of one candidate's six input arrays, laid out as the inputs; a null array is zero.
struct KnotTangentSource {
  const double *s, *l;        // [O][N][2]
  const double *ds;           // [N][2]
  const double *sref, *lref;  // [N]
  int N;
  BTRAPZ_HD double sb(int o, int i, int j) const { return s ? s[((size_t)o * N + i) * 2 + j] : 0.0; }
  BTRAPZ_HD double lb(int o, int i, int j) const { return l ? l[((size_t)o * N + i) * 2 + j] : 0.0; }
  BTRAPZ_HD double dsb(int i, int j) const { return ds ? ds[(size_t)i * 2 + j] : 0.0; }
  BTRAPZ_HD double sr(int i) const { return sref ? sref[i] : 0.0; }
  BTRAPZ_HD double lr(int i) const { return lref ? lref[i] : 0.0; }
};
// Where output segment k reads: the same for every direction, so found once per segment.
struct SegmentReads { int o, i0, h, i1, at_lo, at_hi, r0, r1; };
BTRAPZ_HD SegmentReads segment_reads(int N, int k, const Seg &c, const double *dsb) {
  SegmentReads r;
  r.o = provenance_obstacle(c.count); r.i0 = provenance_knot(c.count); r.h = provenance_pieces(c.count);
  r.i1 = r.i0 == 0 ? 1 : r.i0;
  ds_extreme_knots(N, c.beg_t, c.end_t, dsb, r.at_lo, r.at_hi);
  r.r0 = 10 * k > N - 1 ? N - 1 : 10 * k; r.r1 = 10 * k + 1 > N - 1 ? N - 1 : 10 * k + 1;
  return r;
}
// The tangents of the record of one output segment for one direction: out[f], f < BTRAPZ_NUM_SEG_FIELDS (field 0: 0).
template <class Source>
BTRAPZ_HD void segment_tangent(int variant, double delta, const SegmentReads &r, const Source &src, double *out) {
  out[BTRAPZ_F_T] = 0.0;
  {
    const double lo0 = src.sb(r.o, r.i0, 0), hi0 = src.sb(r.o, r.i0, 1);
    const double dk = (src.sb(r.o, r.i0 + 1, 0) - lo0) / delta, uk = (src.sb(r.o, r.i0 + 1, 1) - hi0) / delta;
    out[BTRAPZ_F_DOWN_SKEW] = dk; out[BTRAPZ_F_DOWN_BIAS] = lo0 + (double)r.h * dk;
    out[BTRAPZ_F_UPP_SKEW] = uk; out[BTRAPZ_F_UPP_BIAS] = hi0 + (double)r.h * uk;
  }
  {
    const double llo = src.lb(r.o, r.i0, 0), lhi = src.lb(r.o, r.i0, 1);
    out[BTRAPZ_F_BEG_L] = llo; out[BTRAPZ_F_END_L] = lhi;
    if (variant == 0) {
      out[BTRAPZ_F_L_DOWN_BIAS] = llo; out[BTRAPZ_F_L_UPP_BIAS] = lhi;
      out[BTRAPZ_F_L_DOWN_SKEW] = (src.lb(r.o, r.i1, 0) - src.lb(r.o, r.i1 - 1, 0)) / delta;
      out[BTRAPZ_F_L_UPP_SKEW] = (src.lb(r.o, r.i1, 1) - src.lb(r.o, r.i1 - 1, 1)) / delta;
    } else {
      out[BTRAPZ_F_L_DOWN_BIAS] = 0.0; out[BTRAPZ_F_L_UPP_BIAS] = 0.0; out[BTRAPZ_F_L_DOWN_SKEW] = 0.0; out[BTRAPZ_F_L_UPP_SKEW] = 0.0;
    }
  }
  out[BTRAPZ_F_DS_LO] = r.at_lo < 0 ? 0.0 : src.dsb(r.at_lo, 0);
  out[BTRAPZ_F_DS_HI] = r.at_hi < 0 ? 0.0 : src.dsb(r.at_hi, 1);
  {
    const double x0 = src.sr(r.r0), y0 = src.lr(r.r0);
    out[BTRAPZ_F_X_BIAS] = x0; out[BTRAPZ_F_X_SKEW] = (src.sr(r.r1) - x0) / delta;
    out[BTRAPZ_F_Y_BIAS] = y0; out[BTRAPZ_F_Y_SKEW] = (src.lr(r.r1) - y0) / delta;
  }
}

}  // namespace btrapz
#endif
