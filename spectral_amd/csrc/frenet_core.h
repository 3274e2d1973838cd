// frenet_core.h -- the per-sample statements of the projection onto the reference line (include/btrapz_hip_frenet.h,
// DESIGN 3.20), shared by the kernels (btrapz_frenet.hip) and the host twins (frenet_host.cpp): the coarse pass's
// candidate rule, chord distance and order, the window's index range, the safeguarded Newton refinement, the map from
// (x, y, theta, kappa, v, a) to (s, ds, dds, l, dl, ddl) and its 6 x 6 Jacobian with the interval frozen.  Line,
// RefPoint, normalize_angle and sin_cos are cartesian_core.h's; ref_at() restates cart::lookup's statements for a given
// interval.  Plain C++: hipcc compiles it for both sides, g++ for the host alone.
#ifndef BTRAPZ_FRENET_CORE_H
#define BTRAPZ_FRENET_CORE_H
#include "cartesian_core.h"

namespace btrapz {
namespace frenet {

using cart::Line;
using cart::RefPoint;
using cart::normalize_angle;
using cart::sin_cos;

constexpr int kMaxSteps = 64;                      // the cap of the refinement
constexpr double kStepDone = 9.313225746154785e-10;  // 2^-30: a step of w this small ends the refinement (below)

// ---- coarse pass --------------------------------------------------------------------------------------------------
// g of the definition at one table point; c, s = cos, sin of the point's heading.  One fused multiply-add on both
// sides, so that host and device agree on its sign given the same c and s.
CART_HD double along(double x, double y, double rx, double ry, double c, double s) { return fma(x - rx, c, (y - ry) * s); }

// interval i (ga at point i, gb at point i + 1) is a candidate on a + -> - change; the last interval also on + -> 0
CART_HD bool candidate(double ga, double gb, bool last) { return ga >= 0.0 && (gb < 0.0 || (last && gb == 0.0)); }

// squared distance of p from the chord a -> b
CART_HD double chord_d2(double x, double y, double ax, double ay, double bx, double by) {
  const double ex = bx - ax, ey = by - ay, px = x - ax, py = y - ay;
  double t = (px * ex + py * ey) / (ex * ex + ey * ey);
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  const double qx = px - t * ex, qy = py - t * ey;
  return qx * qx + qy * qy;
}

// the winner so far.  Intervals arrive in rising order, so the strict comparison keeps the lowest on a tie (and a
// distance that is no number wins nothing).
struct Best {
  double d2, ga, gb;
  int i;
};
CART_HD void best_init(Best &b) { b.d2 = HUGE_VAL; b.ga = 0.0; b.gb = 0.0; b.i = -1; }
CART_HD void best_take(Best &b, int i, double d2, double ga, double gb) {
  if (d2 < b.d2) { b.d2 = d2; b.ga = ga; b.gb = gb; b.i = i; }
}

// the intervals a window [lo, hi] admits, rs[i + 1] >= lo and rs[i] <= hi: [first, last], empty when first > last.
// Every index read lies in [0, M - 1].
CART_HD void window_range(const double *rs, int M, double lo, double hi, int &first, int &last) {
  int a = 0, b = M;   // a: the first k with rs[k] >= lo, M when there is none
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (rs[mid] < lo) a = mid + 1; else b = mid;
  }
  int c = 0, d = M;   // c - 1: the last k with rs[k] <= hi, -1 when there is none
  while (c < d) {
    const int mid = (c + d) >> 1;
    if (rs[mid] <= hi) c = mid + 1; else d = mid;
  }
  first = a - 1 < 0 ? 0 : a - 1;
  last = c - 1 > M - 2 ? M - 2 : c - 1;
}

// ---- the line within interval i at w in [0, 1]: cart::lookup's statements with the interval given -------------------
CART_HD RefPoint ref_at(const Line &t, int i, double w) {
  const double h = t.rs[i + 1] - t.rs[i];
  RefPoint p;
  const double dx = t.rx[i + 1] - t.rx[i], dy = t.ry[i + 1] - t.ry[i];
  const double dth = normalize_angle(t.rtheta[i + 1] - t.rtheta[i]);
  const double dk = t.rkappa[i + 1] - t.rkappa[i], ddk = t.rdkappa[i + 1] - t.rdkappa[i];
  p.x = t.rx[i] + w * dx;            p.mx = dx / h;
  p.y = t.ry[i] + w * dy;            p.my = dy / h;
  p.theta = t.rtheta[i] + w * dth;   p.mtheta = dth / h;
  p.kappa = t.rkappa[i] + w * dk;    p.mkappa = dk / h;
  p.dkappa = t.rdkappa[i] + w * ddk; p.mdkappa = ddk / h;
  return p;
}
// the w of an s the forward returned (cart::lookup's statement)
CART_HD double weight_of(const Line &t, int i, double s) { return (s - t.rs[i]) / (t.rs[i + 1] - t.rs[i]); }

// ---- refinement: the root w in [0, 1] of g(w) = (p - r(w)) . (cos theta(w), sin theta(w)), g(0) = ga >= 0 >= gb = g(1).
// Newton from the secant point; the bracket [lo, hi] shrinks by the sign of g at every iterate, and a step that
// leaves it (a zero slope gives one) is replaced by its midpoint.  Newton doubles the correct digits, so a Newton
// step below 2^-30, once applied, leaves an error of the order 2^-60: the iteration ends there, far above the rounding
// noise of g (2^-53 (|x| + |y| + |rx| + |ry|) / |g'|), at which it would wander for ever.  Returns the steps taken.
CART_HD int refine(const Line &t, int i, double x, double y, double ga, double gb, double &w_out) {
  const double ax = t.rx[i], ay = t.ry[i], ex = t.rx[i + 1] - ax, ey = t.ry[i + 1] - ay;
  const double th = t.rtheta[i], dth = normalize_angle(t.rtheta[i + 1] - th);
  double lo = 0.0, hi = 1.0;
  double w = ga / (ga - gb);
  if (!(w >= 0.0 && w <= 1.0)) w = 0.5;
  int it = 0;
  while (it < kMaxSteps) {
    it++;
    double sn, cs;
    sin_cos(th + w * dth, sn, cs);
    const double px = x - (ax + w * ex), py = y - (ay + w * ey);
    const double g = fma(px, cs, py * sn);
    if (g == 0.0) break;
    if (g > 0.0) lo = w; else hi = w;
    const double l = py * cs - px * sn;
    const double slope = l * dth - (ex * cs + ey * sn);
    const double dw = g / slope;
    double wn = w - dw;
    if (fabs(dw) <= kStepDone) {   // (at the noise floor the last step may point out of the bracket by an ulp: it is not bisected)
      if (wn >= 0.0 && wn <= 1.0) w = wn;
      break;
    }
    if (!(wn > lo && wn < hi)) wn = 0.5 * (lo + hi);
    w = wn;
  }
  w_out = w;
  return it;
}

// ---- the map.  c = (x, y, theta, kappa, v, a) (rows above the order hold 0), p = the line at the root, sn, cs of
//      p.theta; out = (s, ds, dds, l, dl, ddl) but for s, which the caller forms from w ------------------------------
CART_HD void map(const RefPoint &p, double sn, double cs, const double c[6], int order, double out[6]) {
  const double l = (c[1] - p.y) * cs - (c[0] - p.x) * sn;
  out[3] = l;
  out[1] = 0.0; out[2] = 0.0; out[4] = 0.0; out[5] = 0.0;
  if (order < 1) return;
  double sD, cD;
  sin_cos(c[2] - p.theta, sD, cD);
  const double v = c[4], om = 1.0 - p.kappa * l;
  const double vt = v * cD, vn = v * sD;
  const double sd = vt / om;
  out[1] = sd;
  out[4] = vn;
  if (order < 2) return;
  const double kc = c[3], a = c[5], v2k = v * v * kc;
  const double at = a * cD - v2k * sD, an = a * sD + v2k * cD;
  out[2] = (at + sd * sd * p.dkappa * l + 2.0 * p.kappa * sd * vn) / om;
  out[5] = an - p.kappa * (sd * sd) * om;
}

// K[q][j] = d out_q / d c_j with the interval frozen (the slopes of p stand for the table), p = the line at the s the
// forward returned, l its l.  Rows q in the order (s, ds, dds, l, dl, ddl), columns (x, y, theta, kappa, v, a); block
// lower triangular in (s, l | ds, dl | dds, ddl) against (x, y | theta, v | kappa, a); rows above the order are 0.
// First G = d out / d (s, l, theta, v, kappa, a) with s and l as free variables, then s and l by the inverse of the
// forward's 2 x 2 block d (x, y) / d (s, l).
CART_HD void jacobian(const RefPoint &p, double l, const double c[6], int order, double K[6][6]) {
  CART_UNROLL for (int q = 0; q < 6; q++)
    CART_UNROLL for (int j = 0; j < 6; j++) K[q][j] = 0.0;
  double sn, cs;
  sin_cos(p.theta, sn, cs);
  const double x_s = p.mx - cs * p.mtheta * l, y_s = p.my - sn * p.mtheta * l;   // the forward's column s; column l = (-sn, cs)
  const double iD = 1.0 / (x_s * cs + y_s * sn);
  const double s_x = cs * iD, s_y = sn * iD, l_x = -y_s * iD, l_y = x_s * iD;
  K[0][0] = s_x; K[0][1] = s_y;
  K[3][0] = l_x; K[3][1] = l_y;
  if (order < 1) return;
  double sD, cD;
  sin_cos(c[2] - p.theta, sD, cD);
  const double v = c[4], k = p.kappa, kp = p.dkappa;
  const double om = 1.0 - k * l, iom = 1.0 / om;
  const double vt = v * cD, vn = v * sD, sd = vt * iom;
  // columns (s, l, theta, v, kappa, a)
  const double dom[6] = {-p.mkappa * l, -k, 0.0, 0.0, 0.0, 0.0};
  const double dvt[6] = {vn * p.mtheta, 0.0, -vn, cD, 0.0, 0.0};
  const double dvn[6] = {-vt * p.mtheta, 0.0, vt, sD, 0.0, 0.0};
  double G[4][6];   // rows ds, dl, dds, ddl
  CART_UNROLL for (int z = 0; z < 6; z++) {
    G[0][z] = (dvt[z] - sd * dom[z]) * iom;
    G[1][z] = dvn[z];
    G[2][z] = 0.0;
    G[3][z] = 0.0;
  }
  if (order >= 2) {
    const double kc = c[3], a = c[5], v2 = v * v;
    const double at = a * cD - v2 * kc * sD, an = a * sD + v2 * kc * cD;
    const double sdd = (at + sd * sd * kp * l + 2.0 * k * sd * vn) * iom;
    const double dat[6] = {an * p.mtheta, 0.0, -an, -2.0 * v * kc * sD, -v2 * sD, cD};
    const double dan[6] = {-at * p.mtheta, 0.0, at, 2.0 * v * kc * cD, v2 * cD, sD};
    const double dk[6] = {p.mkappa, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double dkp[6] = {p.mdkappa, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double dl[6] = {0.0, 1.0, 0.0, 0.0, 0.0, 0.0};
    CART_UNROLL for (int z = 0; z < 6; z++) {
      const double dsd = G[0][z], dld = G[1][z];
      const double dN = dat[z] + 2.0 * sd * kp * l * dsd + sd * sd * (dkp[z] * l + kp * dl[z]) +
                        2.0 * (dk[z] * sd * vn + k * dsd * vn + k * sd * dld);
      G[2][z] = (dN - sdd * dom[z]) * iom;
      G[3][z] = dan[z] - dk[z] * sd * sd * om - 2.0 * k * sd * om * dsd - k * sd * sd * dom[z];
    }
  }
  const int row[4] = {1, 4, 2, 5};
  CART_UNROLL for (int r = 0; r < 4; r++) {
    const int q = row[r];
    K[q][0] = G[r][0] * s_x + G[r][1] * l_x;
    K[q][1] = G[r][0] * s_y + G[r][1] * l_y;
    K[q][2] = G[r][2];
    K[q][4] = G[r][3];
    K[q][3] = G[r][4];
    K[q][5] = G[r][5];
  }
}

// what the derivatives do per sample: the Jacobian at the forward's result, or false (OUTSIDE: interval not in the
// table, which also keeps every index in bounds whatever `interval` holds)
CART_HD bool jacobian_at(const Line &t, int i, const double c[6], double s, double l, int order, double K[6][6]) {
  if (i < 0 || i > t.M - 2) return false;
  double cc[6] = {c[0], c[1], 0.0, 0.0, 0.0, 0.0};
  if (order >= 1) { cc[2] = c[2]; cc[4] = c[4]; }
  if (order >= 2) { cc[3] = c[3]; cc[5] = c[5]; }
  jacobian(ref_at(t, i, weight_of(t, i, s)), l, cc, order, K);
  return true;
}

}  // namespace frenet
}  // namespace btrapz
#endif
