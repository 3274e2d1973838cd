// prism_vjp_core.h -- the backward pass of the prism stage (obstacle prisms -> per-knot bounds), the part compiled for
// host AND device: prism_vjp.hip (prism_bounds_vjp_kernel) and prism_vjp_host.cpp (btrapz_prism_bounds_vjp_host) call the
// statements below and nothing else, so the two make the same decisions and add the same terms in the same order.
//
// With its decisions frozen the stage is a sparse map that is at most bilinear in every parameter (include/btrapz_hip.h
// lists the rules).  The decisions are made again here, from the prisms and the road alone, with the forward's statements
// (prism_core.h: prism_tables, prism_strip_s, round2 -- which are __device__ only and keep their text, so that the forward
// kernels' code does not change; this is the backward's own variant, one element per call instead of one lane per element)
// and with the forward's rounded values.  What the backward needs beyond the forward's tables:
//   slot[c]  the edge that candidate c supplied (c = q: l_min of car q; P + q: l_max of car q; 2P, 2P + 1: the road), -1
//            when an earlier candidate has its value or it is off: the provenance of an edge;
//   the winner of each max / min of a strip's s bounds at a knot (prism_vjp_winners);
//   the raw parameters t0, vel_s, vel_l, T of a car for the chain rule (prism_vjp_car_out).
// The forward-mode derivative (prism_jvp.hip, prism_jvp_host.cpp) makes the same decisions with the same statements and
// reads the chain rule forwards: prism_jvp_edge_owner, prism_jvp_edge_dot, prism_jvp_face_dot at the end of this file.
// THE TWO-DECIMAL ROUNDING OF A FACE IS DIFFERENTIATED AS THE IDENTITY (straight-through): a face value at knot i counts as
// s0 -+ l_safe + vel_s (i / rate - t0).
#ifndef BTRAPZ_PRISM_VJP_CORE_H
#define BTRAPZ_PRISM_VJP_CORE_H

#include <stddef.h>

#include "../../include/btrapz_hip.h"

#ifndef BTRAPZ_HD
#if defined(__HIPCC__)
#define BTRAPZ_HD __host__ __device__ inline
#else
#define BTRAPZ_HD inline
#endif
#endif

// The forward's expressions, operation by operation (prism_core.h switches contraction off per function; here to the end
// of the translation unit, as corridor_core.h does).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace btrapz {

enum { PVJP_MAX_CARS = 16, PVJP_MAX_CAND = 2 * PVJP_MAX_CARS + 2, PVJP_MAX_STRIPS = 2 * PVJP_MAX_CARS + 1, PVJP_LANES = 64 };

// The tables of one scene (LDS on the device).  w0, w1: first and last knot of a car's window; y1, cc, ct0: the face
// line's offset, slope and slope * t0 as prism_tables leaves them; flags: bit 0 active, bit 1 ahead.
struct PrismVjpTab {
  double w0[PVJP_MAX_CARS], w1[PVJP_MAX_CARS], y1[PVJP_MAX_CARS], cc[PVJP_MAX_CARS], ct0[PVJP_MAX_CARS];
  double lmin[PVJP_MAX_CARS], lmax[PVJP_MAX_CARS];
  double t0[PVJP_MAX_CARS], vs[PVJP_MAX_CARS], vl[PVJP_MAX_CARS], T[PVJP_MAX_CARS];
  double cand[PVJP_MAX_CAND], edge[PVJP_MAX_CAND], edge_bar[PVJP_MAX_CAND];
  int flags[PVJP_MAX_CARS];
  int cand_on[PVJP_MAX_CAND], first[PVJP_MAX_CAND], slot[PVJP_MAX_CAND];
  int cover[PVJP_MAX_STRIPS];
  int strips;
};

// round2 of prism_core.h, word for word
BTRAPZ_HD double prism_vjp_round2(double x) {
  const double y = x * 100.0;
  const double e = __builtin_fma(x, 100.0, -y);
  double r = __builtin_rint(y);
  const double d = y - __builtin_trunc(y);
  if (d == 0.5 || d == -0.5) {
    const double lo = __builtin_floor(y), hi = lo + 1.0;
    if (e > 0.0) r = hi; else if (e < 0.0) r = lo;
  }
  return r / 100.0;
}

// ---- the tables, in the forward's phases; a barrier (device) or the end of a loop (host) between two phases ----
// phase 1, q < P: car q of scene p ([P][8])
BTRAPZ_HD void prism_vjp_car(PrismVjpTab &t, const btrapz_road &r, const double *p, int P, int q) {
  const double *c = p + (size_t)q * 8;
  const double s0 = c[0], l0 = c[1], t0 = c[2], vs = c[3], vl = c[4], T = c[5];
  const bool on = c[6] != 0.0;
  const double fl = l0 + vl * T;
  const double lmin = vl >= 0 ? l0 - r.w_safe : fl - r.w_safe;
  const double lmax = vl >= 0 ? fl + r.w_safe : l0 + r.w_safe;
  const bool ahead = t0 == 0.0;
  const double fs = s0 + vs * T;
  const double y1 = ahead ? s0 - r.l_safe : s0 + r.l_safe;
  const double y2 = ahead ? fs - r.l_safe : fs + r.l_safe;
  const double x1 = t0, x2 = t0 + T;
  const double cc = (y2 - y1) / (x2 - x1);
  t.w0[q] = t0 * r.knots_per_second; t.w1[q] = (t0 + T) * r.knots_per_second; t.y1[q] = y1; t.cc[q] = cc;
  t.lmin[q] = lmin; t.lmax[q] = lmax; t.ct0[q] = cc * t0;
  t.t0[q] = t0; t.vs[q] = vs; t.vl[q] = vl; t.T[q] = T;
  t.flags[q] = (on ? 1 : 0) | (ahead ? 2 : 0);
  t.cand[q] = lmin; t.cand[P + q] = lmax; t.cand_on[q] = on; t.cand_on[P + q] = on;
}
// phase 2, once: the road's own edges only where the cars leave room
BTRAPZ_HD void prism_vjp_road_edges(PrismVjpTab &t, const btrapz_road &r, int P) {
  double mn = 1e300, mx = -1e300;
  for (int j = 0; j < 2 * P; j++)
    if (t.cand_on[j]) { mn = t.cand[j] < mn ? t.cand[j] : mn; mx = t.cand[j] > mx ? t.cand[j] : mx; }
  t.cand[2 * P] = r.l_lo; t.cand_on[2 * P] = mn > r.l_lo;
  t.cand[2 * P + 1] = r.l_hi; t.cand_on[2 * P + 1] = mx < r.l_hi;
}
// phase 3, c < 2P + 2: a candidate counts if no earlier candidate has its value
BTRAPZ_HD void prism_vjp_first(PrismVjpTab &t, int c) {
  bool mine = false;
  if (t.cand_on[c]) {
    const double v = t.cand[c];
    mine = true;
    for (int j = 0; j < c; j++) if (t.cand_on[j] && t.cand[j] == v) mine = false;
  }
  t.first[c] = mine;
}
// phase 4, c < 2P + 2: its edge = the distinct values below it; that edge is the candidate's (its provenance)
BTRAPZ_HD void prism_vjp_rank(PrismVjpTab &t, int P, int c) {
  int slot = -1;
  if (t.first[c]) {
    const double v = t.cand[c];
    int rank = 0;
    for (int j = 0; j < 2 * P + 2; j++) if (t.first[j] && t.cand[j] < v) ++rank;
    t.edge[rank] = v;
    slot = rank;
  }
  t.slot[c] = slot;
}
BTRAPZ_HD int prism_vjp_strip_count(const PrismVjpTab &t, int P) {
  int E = 0;
  for (int c = 0; c < 2 * P + 2; c++) E += t.first[c] ? 1 : 0;
  return E > 0 ? E - 1 : 0;
}
// phase 5, j < strips: the cars whose lateral extent contains strip j
BTRAPZ_HD void prism_vjp_cover(PrismVjpTab &t, int P, int j) {
  const double e0 = t.edge[j], e1 = t.edge[j + 1];
  int m = 0;
  for (int q = 0; q < P; q++)
    if ((t.flags[q] & 1) && t.lmin[q] <= e0 && e1 <= t.lmax[q]) m |= 1 << q;
  t.cover[j] = m;
}

// prism_strip_s with the winners tracked: the car whose FACE is the strip's lower / upper s bound at knot i, -1 where the
// bound is the road's limit.  The first covering car replaces the limits; a later car only when strictly tighter.
BTRAPZ_HD void prism_vjp_winners(const PrismVjpTab &t, const btrapz_road &r, int j, int i, int &w_lo, int &w_hi) {
  double lo = r.s_lo, hi = r.s_hi;
  int wl = -1, wh = -1;
  bool first = true;
  for (int m = t.cover[j]; m; m &= m - 1) {
    const int q = __builtin_ctz(m);
    const bool ahead = (t.flags[q] & 2) != 0;
    const bool inside = !((double)i < t.w0[q] || (double)i > t.w1[q]);
    double c_lo = r.s_lo, c_hi = r.s_hi;
    int q_lo = -1, q_hi = -1;
    if (inside) {
      const double y = prism_vjp_round2(t.cc[q] * (double)i / r.knots_per_second - t.ct0[q] + t.y1[q]);
      if (ahead) { c_hi = y; q_hi = q; } else { c_lo = y; q_lo = q; }
    }
    if (first) { lo = c_lo; hi = c_hi; wl = q_lo; wh = q_hi; first = false; }
    else {
      if (c_lo > lo) { lo = c_lo; wl = q_lo; }
      if (c_hi < hi) { hi = c_hi; wh = q_hi; }
    }
  }
  w_lo = wl; w_hi = wh;
}

// The two running sums of a car, one column per lane: sum[(2 q) * 64 + lane] = sum of bar, sum[(2 q + 1) * 64 + lane] = sum
// of bar * (i / rate - t0), over the (strip, knot) pairs of the lane at which the car's face is the bound.
BTRAPZ_HD void prism_vjp_add(const PrismVjpTab &t, const btrapz_road &r, int j, int i, double bar_lo, double bar_hi, double *sum, int lane) {
  int w_lo, w_hi;
  prism_vjp_winners(t, r, j, i, w_lo, w_hi);
  const double at = (double)i / r.knots_per_second;
  if (w_lo >= 0) {
    double *s = sum + (size_t)(2 * w_lo) * PVJP_LANES + lane;
    s[0] += bar_lo; s[PVJP_LANES] += bar_lo * (at - t.t0[w_lo]);
  }
  if (w_hi >= 0) {
    double *s = sum + (size_t)(2 * w_hi) * PVJP_LANES + lane;
    s[0] += bar_hi; s[PVJP_LANES] += bar_hi * (at - t.t0[w_hi]);
  }
}

// The chain rule of car q: face_bar = sum of bar, face_at_bar = sum of bar * (i / rate - t0), the edges' cotangents in
// t.edge_bar.  out: the car's 8 entries of prisms_bar.
BTRAPZ_HD void prism_vjp_car_out(const PrismVjpTab &t, int P, int q, double face_bar, double face_at_bar, double *out) {
  double g[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t.flags[q] & 1) {
    const double lmin_bar = t.slot[q] >= 0 ? t.edge_bar[t.slot[q]] : 0.0;
    const double lmax_bar = t.slot[P + q] >= 0 ? t.edge_bar[t.slot[P + q]] : 0.0;
    const double moving = t.vl[q] >= 0 ? lmax_bar : lmin_bar;   // the end that is l0 + vel_l T -+ w_safe
    g[0] = face_bar;
    g[1] = lmin_bar + lmax_bar;
    g[2] = -(t.vs[q] * face_bar);
    g[3] = face_at_bar;
    g[4] = t.T[q] * moving;
    g[5] = t.vl[q] * moving;
  }
  for (int k = 0; k < 8; k++) out[k] = g[k];
}

// ---- forward mode (prism_jvp.hip, prism_jvp_host.cpp): the rules of prism_vjp_car_out read forwards, per element ----
// d: the tangents of one scene's cars for one direction, [P][6] = s0, l0, t0, vel_s, vel_l, T.
// after phase 4, c < 2P + 2: owner[j] = the candidate that supplied edge j (every edge 0..strips has exactly one)
BTRAPZ_HD void prism_jvp_edge_owner(const PrismVjpTab &t, int *owner, int c) {
  if (t.slot[c] >= 0) owner[t.slot[c]] = c;
}
// the tangent of the edge candidate c supplied: l0_dot for the stationary end, (l0_dot + T vel_l_dot) + vel_l T_dot for
// the end that is l0 + vel_l T -+ w_safe, 0 for the road's edges
BTRAPZ_HD double prism_jvp_edge_dot(const PrismVjpTab &t, int P, int c, const double *d) {
  if (c < 0 || c >= 2 * P) return 0.0;
  const int q = c < P ? c : c - P;
  const double *dq = d + (size_t)q * 6;
  const bool moving = (t.vl[q] >= 0) == (c >= P);
  if (!moving) return dq[1];
  return (dq[1] + t.T[q] * dq[4]) + t.vl[q] * dq[5];
}
// the tangent of car q's face at knot i (rounding straight-through)
BTRAPZ_HD double prism_jvp_face_dot(const PrismVjpTab &t, const btrapz_road &r, int q, int i, const double *d) {
  const double *dq = d + (size_t)q * 6;
  const double at = (double)i / r.knots_per_second;
  return (dq[0] + dq[3] * (at - t.t0[q])) - t.vs[q] * dq[2];
}

}  // namespace btrapz
#endif
