// clearance_core.h -- the per-pair statements of the clearance stage (include/btrapz_hip_clearance.h),
// shared by the kernels (btrapz_clearance.hip) and the host twins (clearance_host.cpp): the signed clearance of two
// rectangles with its winning feature, the derivative of a frozen feature, and the audit's order.  Plain C++: it compiles
// under hipcc for both sides and under g++ for the host alone.  The two sides differ in sin / cos only.
//
// Everything is formed in RELATIVE quantities -- d = c_B - c_A in both frames, c = cos and s = sin of the heading
// difference from the two rectangles' own cosines and sines -- so that no vertex is ever placed in the plane and
// subtracted again: the only cancellation is the one in d itself.
#ifndef BTRAPZ_CLEARANCE_CORE_H
#define BTRAPZ_CLEARANCE_CORE_H
#include <math.h>
#include <stddef.h>

#include "cartesian_core.h"

namespace btrapz {
namespace clr {

using cart::kNobody;
using cart::sin_cos;

struct Foot {
  double hl, hw, off;
};
// the ego at a sample: the pose's point, cos and sin of its heading
struct Ego {
  double x, y, ca, sa;
};
// an obstacle at a sample
struct Obs {
  double x, y, cb, sb, hl, hw;
};

CART_HD bool is_nan3(double a, double b, double c) { return a != a || b != b || c != c; }

// the pair in relative quantities
struct Rel {
  double dx, dy;     // d = c_B - c_A
  double dAu, dAn;   // d in A's frame
  double dBu, dBn;   // d in B's frame
  double c, s;       // u_A . u_B = n_A . n_B,   n_A . u_B = -(u_A . n_B)
};
CART_HD Rel relative(const Foot &ft, const Ego &e, const Obs &b) {
  Rel r;
  r.dx = b.x - (e.x + ft.off * e.ca);
  r.dy = b.y - (e.y + ft.off * e.sa);
  r.dAu = r.dx * e.ca + r.dy * e.sa;
  r.dAn = r.dy * e.ca - r.dx * e.sa;
  r.dBu = r.dx * b.cb + r.dy * b.sb;
  r.dBn = r.dy * b.cb - r.dx * b.sb;
  r.c = e.ca * b.cb + e.sa * b.sb;
  r.s = e.ca * b.sb - e.sa * b.cb;
  return r;
}

// the sign of vertex i, i = 0 .. 3: (+,+), (-,+), (-,-), (+,-)
CART_HD double vx_sign(int i) { return (i == 0 || i == 3) ? 1.0 : -1.0; }
CART_HD double vy_sign(int i) { return i < 2 ? 1.0 : -1.0; }

// vertex i of A in B's frame (relative to c_B), and of B in A's frame (relative to c_A)
CART_HD void vertex_a_in_b(const Foot &ft, const Rel &r, int i, double &pu, double &pn) {
  const double ax = vx_sign(i) * ft.hl, ay = vy_sign(i) * ft.hw;
  pu = ax * r.c + ay * r.s - r.dBu;
  pn = ay * r.c - ax * r.s - r.dBn;
}
CART_HD void vertex_b_in_a(const Obs &b, const Rel &r, int i, double &pu, double &pn) {
  const double bx = vx_sign(i) * b.hl, by = vy_sign(i) * b.hw;
  pu = bx * r.c - by * r.s + r.dAu;
  pn = bx * r.s + by * r.c + r.dAn;
}
// the distance of the point (pu, pn) to the box of half extents (hl, hw) in the box's frame; m = the offset's components
CART_HD double box_distance(double pu, double pn, double hl, double hw, double &m0, double &m1) {
  const double q0 = fabs(pu) - hl, q1 = fabs(pn) - hw;
  m0 = q0 > 0.0 ? q0 : 0.0;
  m1 = q1 > 0.0 ? q1 : 0.0;
  return sqrt(m0 * m0 + m1 * m1);
}

// The signed clearance of the pair and its feature (0 .. 11).  No argument is NaN.
CART_HD double pair_clearance(const Foot &ft, const Ego &e, const Obs &b, int &feature) {
  const Rel r = relative(ft, e, b);
  const double ac = fabs(r.c), as = fabs(r.s);
  const double g1 = fabs(r.dAn) - ft.hw - (b.hl * as + b.hw * ac);
  const double g2 = fabs(r.dBu) - (ft.hl * ac + ft.hw * as) - b.hl;
  const double g3 = fabs(r.dBn) - (ft.hl * as + ft.hw * ac) - b.hw;
  double g = fabs(r.dAu) - ft.hl - (b.hl * ac + b.hw * as);
  int k = 0;
  if (g1 > g) { g = g1; k = 1; }
  if (g2 > g) { g = g2; k = 2; }
  if (g3 > g) { g = g3; k = 3; }
  if (!(g > 0.0)) { feature = k; return g; }
  double best = HUGE_VAL;
  k = 4;
  CART_UNROLL for (int i = 0; i < 4; i++) {
    double pu, pn, m0, m1;
    vertex_a_in_b(ft, r, i, pu, pn);
    const double dist = box_distance(pu, pn, b.hl, b.hw, m0, m1);
    if (dist < best) { best = dist; k = 4 + i; }
  }
  CART_UNROLL for (int i = 0; i < 4; i++) {
    double pu, pn, m0, m1;
    vertex_b_in_a(b, r, i, pu, pn);
    const double dist = box_distance(pu, pn, ft.hl, ft.hw, m0, m1);
    if (dist < best) { best = dist; k = 8 + i; }
  }
  feature = k;
  return best;
}

// The derivative of the pair's clearance under the frozen feature: d clear = nx (dx_A - dx_B) + ny (dy_A - dy_B)
// + la dtheta_A - lb dtheta_B, with (x_A, y_A) the pose's point and (x_B, y_B) the obstacle's centre.  With W the
// witness point, la = (W - P_A) x n and lb = (W - c_B) x n; W is kept relative to c_A (wx, wy in the plane's axes).
struct Grad {
  double nx, ny, la, lb;
};
CART_HD double sign_pos(double v) { return v < 0.0 ? -1.0 : 1.0; }
// false: the derivative is 0 (no such feature, or a disjoint feature at distance exactly 0) and g is not to be used
CART_HD bool pair_gradient(const Foot &ft, const Ego &e, const Obs &b, int feature, Grad &g) {
  g.nx = g.ny = g.la = g.lb = 0.0;
  if (feature < 0 || feature > 11) return false;
  const Rel r = relative(ft, e, b);
  double nx, ny;   // the unit direction from B to A, in the plane
  double wx, wy;   // the witness relative to c_A, in the plane
  if (feature < 2) {
    // a face of A: n = -sigma e, the witness is B's support vertex towards A
    const double eu = feature == 0 ? 1.0 : 0.0, en = 1.0 - eu;   // e in A's frame
    const double sg = sign_pos(feature == 0 ? r.dAu : r.dAn);
    // e . u_B and e . n_B:  u_A . u_B = c, n_A . u_B = s, u_A . n_B = -s, n_A . n_B = c
    const double su = sign_pos(eu * r.c + en * r.s), sv = sign_pos(en * r.c - eu * r.s);
    const double bu = -sg * su * b.hl, bn = -sg * sv * b.hw;     // the vertex in B's frame
    wx = r.dx + bu * b.cb - bn * b.sb;
    wy = r.dy + bu * b.sb + bn * b.cb;
    nx = -sg * (eu * e.ca - en * e.sa);
    ny = -sg * (eu * e.sa + en * e.ca);
  } else if (feature < 4) {
    // a face of B: n = -sigma e, the witness is A's support vertex towards B
    const double eu = feature == 2 ? 1.0 : 0.0, en = 1.0 - eu;   // e in B's frame
    const double sg = sign_pos(feature == 2 ? r.dBu : r.dBn);
    // e . u_A and e . n_A
    const double su = sign_pos(eu * r.c - en * r.s), sv = sign_pos(eu * r.s + en * r.c);
    const double au = sg * su * ft.hl, an = sg * sv * ft.hw;     // the vertex in A's frame
    wx = au * e.ca - an * e.sa;
    wy = au * e.sa + an * e.ca;
    nx = -sg * (eu * b.cb - en * b.sb);
    ny = -sg * (eu * b.sb + en * b.cb);
  } else if (feature < 8) {
    // vertex i of A against the box B: n = the offset in B's frame, normalised
    const int i = feature - 4;
    double pu, pn, m0, m1;
    vertex_a_in_b(ft, r, i, pu, pn);
    const double dist = box_distance(pu, pn, b.hl, b.hw, m0, m1);
    if (!(dist > 0.0)) return false;
    const double nu = (pu < 0.0 ? -m0 : m0) / dist, nn = (pn < 0.0 ? -m1 : m1) / dist;
    nx = nu * b.cb - nn * b.sb;
    ny = nu * b.sb + nn * b.cb;
    const double au = vx_sign(i) * ft.hl, an = vy_sign(i) * ft.hw;
    wx = au * e.ca - an * e.sa;
    wy = au * e.sa + an * e.ca;
  } else {
    // vertex i of B against the box A: n = minus the offset in A's frame, normalised
    const int i = feature - 8;
    double pu, pn, m0, m1;
    vertex_b_in_a(b, r, i, pu, pn);
    const double dist = box_distance(pu, pn, ft.hl, ft.hw, m0, m1);
    if (!(dist > 0.0)) return false;
    const double nu = -(pu < 0.0 ? -m0 : m0) / dist, nn = -(pn < 0.0 ? -m1 : m1) / dist;
    nx = nu * e.ca - nn * e.sa;
    ny = nu * e.sa + nn * e.ca;
    const double bu = vx_sign(i) * b.hl, bn = vy_sign(i) * b.hw;
    wx = r.dx + bu * b.cb - bn * b.sb;
    wy = r.dy + bu * b.sb + bn * b.cb;
  }
  g.nx = nx;
  g.ny = ny;
  // W - P_A = W - c_A + off u_A;   W - c_B = W - c_A - d
  const double ax = wx + ft.off * e.ca, ay = wy + ft.off * e.sa;
  g.la = ax * ny - ay * nx;
  g.lb = (wx - r.dx) * ny - (wy - r.dy) * nx;
  return true;
}

// ---- a sample against its scene: the minimum over the obstacles present, lowest obstacle on a tie ----
// pose points at [O][3][n] of the scene, half at [O][2]; obstacles o < count.  Returns +inf and which = -1 when none is
// present.  The ego is not NaN.
CART_HD double sample_clearance(const Foot &ft, const Ego &e, const double *pose, const double *half, int count, int n, int j,
                                int &which) {
  double best = HUGE_VAL;
  which = -1;
  for (int o = 0; o < count; o++) {
    const double *p = pose + (size_t)o * 3 * (size_t)n + (size_t)j;
    const double ox = p[0], oy = p[n], oth = p[2 * (size_t)n];
    if (is_nan3(ox, oy, oth)) continue;
    Obs b;
    b.x = ox; b.y = oy; b.hl = half[2 * o]; b.hw = half[2 * o + 1];
    sin_cos(oth, b.sb, b.cb);
    int k;
    const double cl = pair_clearance(ft, e, b, k);
    if (cl < best) { best = cl; which = o * 16 + k; }
  }
  return best;
}

// the gradient of a sample under its frozen `which`; false: the derivative is 0 (nobody, an obstacle or a feature that does
// not exist, an absent obstacle) -- 0 whatever the cotangent or tangent holds there, NaN included
CART_HD bool sample_gradient(const Foot &ft, const Ego &e, const double *pose, const double *half, int count, int n, int j,
                             int which, int &o, Grad &g) {
  if (which < 0 || (which & 15) > 11) return false;
  o = which >> 4;
  if (o >= count) return false;
  const double *p = pose + (size_t)o * 3 * (size_t)n + (size_t)j;
  const double ox = p[0], oy = p[n], oth = p[2 * (size_t)n];
  if (is_nan3(ox, oy, oth)) return false;
  Obs b;
  b.x = ox; b.y = oy; b.hl = half[2 * o]; b.hw = half[2 * o + 1];
  sin_cos(oth, b.sb, b.cb);
  return pair_gradient(ft, e, b, which & 15, g);
}

// the scene's obstacle count, clamped to [0, O]
CART_HD int scene_count(const int *obs_count, int scene, int O) {
  if (!obs_count) return O;
  const int c = obs_count[scene] < O ? obs_count[scene] : O;
  return c > 0 ? c : 0;
}

// ---- the audit: the minimum with the sample that attains it and that sample's `which` ----
struct Least {
  double key;
  int idx, which, n_below, n_invalid;
};
CART_HD void least_init(Least &l) { l.key = HUGE_VAL; l.idx = kNobody; l.which = -1; l.n_below = 0; l.n_invalid = 0; }
// samples arrive in rising order: a strict comparison keeps the lowest on a tie; +inf and NaN enter nothing
CART_HD void least_take(Least &l, double clear, int which, int j, double d_safe) {
  if (clear < l.key) { l.key = clear; l.idx = j; l.which = which; }
  if (clear < d_safe) l.n_below++;
}
// the total order "smaller value, then lower sample"
CART_HD void least_merge(Least &l, double okey, int oidx, int owhich) {
  if (okey < l.key || (okey == l.key && oidx < l.idx)) { l.key = okey; l.idx = oidx; l.which = owhich; }
}

}  // namespace clr
}  // namespace btrapz
#endif
