// cartesian_core.h -- the per-sample statements of the Cartesian stage (include/btrapz_hip_cartesian.h),
// shared by the kernels (btrapz_cartesian.hip) and the host twins (cartesian_host.cpp): the lookup in the reference
// line's table, the map from a Frenet sample to (x, y, theta, kappa, v, a), its 6 x 6 Jacobian with the interval frozen,
// and the audit's order.  Plain C++: it compiles under hipcc for both sides and under g++ for the host alone.  The two
// sides differ in sin / cos only (one sincos per sample on the device).
#ifndef BTRAPZ_CARTESIAN_CORE_H
#define BTRAPZ_CARTESIAN_CORE_H
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define CART_HD __host__ __device__ inline __attribute__((always_inline))
#define CART_UNROLL _Pragma("unroll")
#else
#define CART_HD inline
#define CART_UNROLL
#endif

namespace btrapz {
namespace cart {

constexpr double kPi = 3.141592653589793;
constexpr int kNobody = 0x7fffffff;   // "no sample yet" while reducing; written as -1

// one line of the table (rs may live in LDS on the device)
struct Line {
  const double *rs, *rx, *ry, *rtheta, *rkappa, *rdkappa;
  int M;
};
// the line at one arc length, and its slopes within the interval (the frozen decision)
struct RefPoint {
  double x, y, theta, kappa, dkappa;
  double mx, my, mtheta, mkappa, mdkappa;
};

// the reference's NormalizeAngle (cart_frenet.py:193)
CART_HD double normalize_angle(double a) {
  a = fmod(a + kPi, 2.0 * kPi);
  if (a < 0.0) a += 2.0 * kPi;
  return a - kPi;
}

// OUTSIDE: below the first point, above the last, or no number
CART_HD bool outside(const Line &t, double s) { return !(s >= t.rs[0] && s <= t.rs[t.M - 1]); }

// the largest i with rs[i] <= s, clamped to M - 2; s is not OUTSIDE.  Every index it reads or returns lies in the
// table whatever the table holds.
CART_HD int interval(const Line &t, double s) {
  int lo = 0, hi = t.M - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.rs[mid] <= s) lo = mid; else hi = mid;
  }
  return lo;
}

CART_HD RefPoint lookup(const Line &t, double s) {
  const int i = interval(t, s);
  const double h = t.rs[i + 1] - t.rs[i];
  const double w = (s - t.rs[i]) / h;
  RefPoint p;
  const double dx = t.rx[i + 1] - t.rx[i], dy = t.ry[i + 1] - t.ry[i];
  const double dth = normalize_angle(t.rtheta[i + 1] - t.rtheta[i]);
  const double dk = t.rkappa[i + 1] - t.rkappa[i], ddk = t.rdkappa[i + 1] - t.rdkappa[i];
  p.x = t.rx[i] + w * dx;           p.mx = dx / h;
  p.y = t.ry[i] + w * dy;           p.my = dy / h;
  p.theta = t.rtheta[i] + w * dth;  p.mtheta = dth / h;
  p.kappa = t.rkappa[i] + w * dk;   p.mkappa = dk / h;
  p.dkappa = t.rdkappa[i] + w * ddk; p.mdkappa = ddk / h;
  return p;
}

CART_HD void sin_cos(double a, double &sn, double &cs) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(a, &sn, &cs);
#else
  sn = sin(a); cs = cos(a);
#endif
}

// what the map and its Jacobian share: the velocity and acceleration along and across the line
struct Moving {
  double sn, cs, w, vt, vn, at, an;
};
CART_HD Moving moving(const RefPoint &p, const double f[6]) {
  Moving m;
  sin_cos(p.theta, m.sn, m.cs);
  const double sd = f[1], sdd = f[2], l = f[3], ld = f[4], ldd = f[5];
  m.w = 1.0 - p.kappa * l;
  m.vt = sd * m.w;
  m.vn = ld;
  m.at = sdd * m.w - sd * sd * p.dkappa * l - 2.0 * p.kappa * sd * ld;
  m.an = ldd + p.kappa * (sd * sd) * m.w;
  return m;
}

// out = (x, y, theta, kappa, v, a) of f = (s, ds, dds, l, dl, ddl) at p
CART_HD void map(const RefPoint &p, const Moving &m, const double f[6], double out[6]) {
  const double l = f[3];
  out[0] = p.x - m.sn * l;
  out[1] = p.y + m.cs * l;
  const double v2 = m.vt * m.vt + m.vn * m.vn;
  const double v = sqrt(v2);
  out[4] = v;
  if (v == 0.0) {
    out[2] = normalize_angle(p.theta);
    out[3] = 0.0;
    out[5] = m.at;
    return;
  }
  out[2] = normalize_angle(p.theta + atan2(m.vn, m.vt));
  out[3] = (m.vt * m.an - m.vn * m.at) / (v2 * v);
  out[5] = (m.vt * m.at + m.vn * m.an) / v;
}

// J[i][q] = d out_i / d f_q with the interval frozen (the slopes of p stand for the table)
CART_HD void jacobian(const RefPoint &p, const Moving &m, const double f[6], double J[6][6]) {
  const double sd = f[1], sdd = f[2], l = f[3], ld = f[4];
  CART_UNROLL for (int i = 0; i < 6; i++)
    CART_UNROLL for (int q = 0; q < 6; q++) J[i][q] = 0.0;
  J[0][0] = p.mx - m.cs * p.mtheta * l;  J[0][3] = -m.sn;
  J[1][0] = p.my - m.sn * p.mtheta * l;  J[1][3] = m.cs;
  const double v2 = m.vt * m.vt + m.vn * m.vn;
  const double v = sqrt(v2);
  if (v == 0.0) return;
  const double k = p.kappa, kp = p.dkappa;
  const double w_s = -p.mkappa * l, w_l = -k;
  // columns s, ds, dds, l, dl, ddl of vt, vn, at, an
  const double dvt[6] = {sd * w_s, m.w, 0.0, sd * w_l, 0.0, 0.0};
  const double dvn[6] = {0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  const double dat[6] = {sdd * w_s - sd * sd * p.mdkappa * l - 2.0 * p.mkappa * sd * ld,
                         -2.0 * sd * kp * l - 2.0 * k * ld,
                         m.w,
                         sdd * w_l - sd * sd * kp,
                         -2.0 * k * sd,
                         0.0};
  const double dan[6] = {(sd * sd) * (p.mkappa * m.w + k * w_s), 2.0 * k * sd * m.w, 0.0, (sd * sd) * (k * w_l), 0.0, 1.0};
  const double iv = 1.0 / v, iv2 = 1.0 / v2;
  const double a = (m.vt * m.at + m.vn * m.an) * iv;
  const double kap = (m.vt * m.an - m.vn * m.at) * (iv2 * iv);
  CART_UNROLL for (int q = 0; q < 6; q++) {
    const double dv = (m.vt * dvt[q] + m.vn * dvn[q]) * iv;
    const double dN = m.at * dvt[q] + m.vt * dat[q] + m.an * dvn[q] + m.vn * dan[q];
    const double dC = m.an * dvt[q] + m.vt * dan[q] - m.at * dvn[q] - m.vn * dat[q];
    J[2][q] = (m.vt * dvn[q] - m.vn * dvt[q]) * iv2;
    J[3][q] = dC * (iv2 * iv) - 3.0 * kap * dv * iv;
    J[4][q] = dv;
    J[5][q] = (dN - a * dv) * iv;
  }
  J[2][0] += p.mtheta;
}

// ---- the layouts: where component q (s, ds, dds, l, dl, ddl) of sample j of row r lies ----
CART_HD size_t frenet_offset(int layout, size_t r, int n, int j, int q) {
  return layout == 0 ? (r * 6 + (size_t)q) * (size_t)n + (size_t)j
                     : ((r * 2 + (size_t)(q / 3)) * (size_t)n + (size_t)j) * 3 + (size_t)(q % 3);
}

// ---- the audit: six extremes as maxima of a key (the minima negated, which is exact), with the sample that attains
//      them; order of the fields: kappa_abs_max, alat_abs_max, a_min, a_max, v_max, frame_min ----
struct Extremes {
  double key[6];
  int idx[6];
  int n_outside;
};
CART_HD void extremes_init(Extremes &e) {
  CART_UNROLL for (int i = 0; i < 6; i++) { e.key[i] = -HUGE_VAL; e.idx[i] = kNobody; }
  e.n_outside = 0;
}
// the values as written to cart; samples arrive in rising order, so a strict comparison keeps the lowest on a tie (and
// a value that is no number, or a key of -inf, enters nothing)
CART_HD void extremes_take(Extremes &e, const double out[6], double w, int j) {
  const double ak = fabs(out[3]);
  const double key[6] = {ak, out[4] * out[4] * ak, -out[5], out[5], out[4], -w};
  CART_UNROLL for (int i = 0; i < 6; i++)
    if (key[i] > e.key[i]) { e.key[i] = key[i]; e.idx[i] = j; }
}
// the total order "better value, then lower sample"
CART_HD void extremes_merge(double &key, int &idx, double okey, int oidx) {
  if (okey > key || (okey == key && oidx < idx)) { key = okey; idx = oidx; }
}
CART_HD double extremes_value(const Extremes &e, int i) { return (i == 2 || i == 5) ? -e.key[i] : e.key[i]; }

}  // namespace cart
}  // namespace btrapz
#endif
