// frenet_host.cpp -- btrapz_frenet_host / _vjp_host / _jvp_host (include/btrapz_hip_frenet.h): the projection onto the
// reference line on the host, query by query with the statements of frenet_core.h that the kernels run.  No GPU, no
// context.  Plain C++ (g++ builds it for the sanitizer program, host_check/frenet_check.cpp).
#include <math.h>

#include <vector>

#include "../../include/btrapz_hip_frenet.h"
#include "frenet_core.h"

#define FRENET_EXPORT extern "C" __attribute__((visibility("default")))

using namespace btrapz::frenet;
using btrapz::cart::frenet_offset;

namespace {

bool bad_common(const btrapz_refline *t, int R, int n, int layout, int order, const double *cart, const double *frenet) {
  if (!t || !cart || !frenet || !t->rs || !t->rx || !t->ry || !t->rtheta || !t->rkappa || !t->rdkappa) return true;
  if (R < 1 || n < 1 || t->n_lines < 1 || t->M < 2) return true;
  if (order < 0 || order > 2) return true;
  return layout != BTRAPZ_FRENET_SAMPLES && layout != BTRAPZ_FRENET_STATES;
}

// the row's line: its index, -1 when the whole row is OUTSIDE
int row_line(const btrapz_refline *t, const int *line_index, int r, Line &ln) {
  const int li = line_index ? line_index[r] : 0;
  if (li < 0 || li >= t->n_lines) return -1;
  const size_t o = (size_t)li * (size_t)t->M;
  ln.rs = t->rs + o; ln.rx = t->rx + o; ln.ry = t->ry + o; ln.rtheta = t->rtheta + o; ln.rkappa = t->rkappa + o;
  ln.rdkappa = t->rdkappa + o; ln.M = t->M;
  return li;
}
int row_count(const int *count, int r, int n) {
  if (!count) return n;
  const int c = count[r] < n ? count[r] : n;
  return c > 0 ? c : 0;
}
// the rows of cart up to the order; the others are not read
void read_cart(const double *cart, size_t r, int n, int j, int order, double c[6]) {
  const double *cr = cart + r * 6 * (size_t)n + j;
  for (int i = 0; i < 6; i++) c[i] = 0.0;
  c[0] = cr[0]; c[1] = cr[(size_t)n];
  if (order >= 1) { c[2] = cr[2 * (size_t)n]; c[4] = cr[4 * (size_t)n]; }
  if (order >= 2) { c[3] = cr[3 * (size_t)n]; c[5] = cr[5 * (size_t)n]; }
}

}  // namespace

FRENET_EXPORT int btrapz_frenet_host(const btrapz_refline *t, const int *line_index, int R, int n, int layout, int order,
                                     const double *cart, const int *count, const double *s_window, double *frenet,
                                     int *interval, int *n_outside) {
  if (bad_common(t, R, n, layout, order, cart, frenet)) return BTRAPZ_EINVAL;
  const int M = t->M;
  std::vector<double> cs_((size_t)M), sn_((size_t)M);
  int have = -1;   // the line whose cosines and sines are in cs_, sn_
  for (int r = 0; r < R; r++) {
    Line ln;
    const int li = row_line(t, line_index, r, ln);
    const int cnt = row_count(count, r, n);
    if (li >= 0 && li != have && cnt > 0) {
      for (int k = 0; k < M; k++) sin_cos(ln.rtheta[k], sn_[(size_t)k], cs_[(size_t)k]);
      have = li;
    }
    int first = 0, last = M - 2;
    bool row_ok = li >= 0;
    if (row_ok && s_window) {
      const double lo = s_window[2 * (size_t)r], hi = s_window[2 * (size_t)r + 1];
      row_ok = lo <= hi;
      if (row_ok) window_range(ln.rs, M, lo, hi, first, last);
    }
    int outside = 0;
    for (int j = 0; j < cnt; j++) {
      double c[6], out[6];
      read_cart(cart, (size_t)r, n, j, order, c);
      Best b;
      best_init(b);
      if (row_ok && c[0] == c[0] && c[1] == c[1] && first <= last) {
        double ga = along(c[0], c[1], ln.rx[first], ln.ry[first], cs_[(size_t)first], sn_[(size_t)first]);
        for (int i = first; i <= last; i++) {
          const double gb = along(c[0], c[1], ln.rx[i + 1], ln.ry[i + 1], cs_[(size_t)i + 1], sn_[(size_t)i + 1]);
          if (candidate(ga, gb, i == M - 2))
            best_take(b, i, chord_d2(c[0], c[1], ln.rx[i], ln.ry[i], ln.rx[i + 1], ln.ry[i + 1]), ga, gb);
          ga = gb;
        }
      }
      if (b.i < 0) {
        outside++;
        for (int q = 0; q < 6; q++) out[q] = NAN;
      } else {
        double w, sn, cs;
        refine(ln, b.i, c[0], c[1], b.ga, b.gb, w);
        const RefPoint p = ref_at(ln, b.i, w);
        sin_cos(p.theta, sn, cs);
        map(p, sn, cs, c, order, out);
        out[0] = ln.rs[b.i] + w * (ln.rs[b.i + 1] - ln.rs[b.i]);
      }
      for (int q = 0; q < 6; q++) frenet[frenet_offset(layout, (size_t)r, n, j, q)] = out[q];
      if (interval) interval[(size_t)r * n + j] = b.i;
    }
    if (n_outside) n_outside[r] = outside;
  }
  return BTRAPZ_OK;
}

FRENET_EXPORT int btrapz_frenet_vjp_host(const btrapz_refline *t, const int *line_index, int R, int n, int layout, int order,
                                         const double *cart, const double *frenet, const int *interval, const int *count,
                                         const double *frenet_bar, double *cart_bar) {
  if (bad_common(t, R, n, layout, order, cart, frenet) || !interval || !frenet_bar || !cart_bar) return BTRAPZ_EINVAL;
  for (int r = 0; r < R; r++) {
    Line ln;
    const bool has_line = row_line(t, line_index, r, ln) >= 0;
    const int cnt = row_count(count, r, n);
    for (int j = 0; j < n; j++) {
      double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (j < cnt && has_line) {
        double c[6], K[6][6];
        read_cart(cart, (size_t)r, n, j, order, c);
        const double s = frenet[frenet_offset(layout, (size_t)r, n, j, 0)], l = frenet[frenet_offset(layout, (size_t)r, n, j, 3)];
        if (jacobian_at(ln, interval[(size_t)r * n + j], c, s, l, order, K)) {
          for (int q = 0; q < 6; q++) {
            if (q % 3 > order) continue;   // a row above the order is 0: what frenet_bar holds there is not read
            const double fb = frenet_bar[frenet_offset(layout, (size_t)r, n, j, q)];
            for (int i = 0; i < 6; i++) g[i] += fb * K[q][i];
          }
        }
      }
      for (int i = 0; i < 6; i++) cart_bar[((size_t)r * 6 + i) * n + j] = g[i];
    }
  }
  return BTRAPZ_OK;
}

FRENET_EXPORT int btrapz_frenet_jvp_host(const btrapz_refline *t, const int *line_index, int R, int n, int layout, int order,
                                         const double *cart, const double *frenet, const int *interval, const int *count, int T,
                                         const double *cart_dot, double *frenet_dot) {
  if (bad_common(t, R, n, layout, order, cart, frenet) || !interval || !cart_dot || !frenet_dot) return BTRAPZ_EINVAL;
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) return BTRAPZ_EINVAL;
  const size_t slab = (size_t)R * 6 * (size_t)n;
  for (int r = 0; r < R; r++) {
    Line ln;
    const bool has_line = row_line(t, line_index, r, ln) >= 0;
    const int cnt = row_count(count, r, n);
    for (int j = 0; j < cnt; j++) {
      double c[6], K[6][6];
      bool in = false;
      if (has_line) {
        read_cart(cart, (size_t)r, n, j, order, c);
        const double s = frenet[frenet_offset(layout, (size_t)r, n, j, 0)], l = frenet[frenet_offset(layout, (size_t)r, n, j, 3)];
        in = jacobian_at(ln, interval[(size_t)r * n + j], c, s, l, order, K);
      }
      for (int k = 0; k < T; k++) {
        double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (in) {
          double cd[6];
          read_cart(cart_dot + (size_t)k * slab, (size_t)r, n, j, order, cd);
          for (int q = 0; q < 6; q++)
            for (int i = 0; i < 6; i++) d[q] += K[q][i] * cd[i];
        }
        for (int q = 0; q < 6; q++) frenet_dot[(size_t)k * slab + frenet_offset(layout, (size_t)r, n, j, q)] = d[q];
      }
    }
  }
  return BTRAPZ_OK;
}
