// cartesian_host.cpp -- btrapz_cartesian_host / _vjp_host / _jvp_host (include/btrapz_hip_cartesian.h): the Cartesian
// stage on the host, sample by sample with the statements of cartesian_core.h that the kernels run.  No GPU, no context.
// Plain C++ (g++ builds it for the sanitizer program, host_check/cartesian_check.cpp).
#include <math.h>

#include "../../include/btrapz_hip_cartesian.h"
#include "cartesian_core.h"

#define CART_EXPORT extern "C" __attribute__((visibility("default")))

using namespace btrapz::cart;

namespace {

bool bad_common(const btrapz_refline *t, int R, int n, int layout, const double *f) {
  if (!t || !f || !t->rs || !t->rx || !t->ry || !t->rtheta || !t->rkappa || !t->rdkappa) return true;
  if (R < 1 || n < 1 || t->n_lines < 1 || t->M < 2) return true;
  return layout != BTRAPZ_FRENET_SAMPLES && layout != BTRAPZ_FRENET_STATES;
}

// the row's line (false: the whole row is OUTSIDE) and its sample count
bool row_line(const btrapz_refline *t, const int *line_index, int r, Line &ln) {
  const int li = line_index ? line_index[r] : 0;
  if (li < 0 || li >= t->n_lines) return false;
  const size_t o = (size_t)li * (size_t)t->M;
  ln.rs = t->rs + o; ln.rx = t->rx + o; ln.ry = t->ry + o; ln.rtheta = t->rtheta + o; ln.rkappa = t->rkappa + o;
  ln.rdkappa = t->rdkappa + o; ln.M = t->M;
  return true;
}
int row_count(const int *count, int r, int n) {
  if (!count) return n;
  const int c = count[r] < n ? count[r] : n;
  return c > 0 ? c : 0;
}
void read_sample(int layout, const double *f, size_t r, int n, int j, double u[6]) {
  for (int q = 0; q < 6; q++) u[q] = f[frenet_offset(layout, r, n, j, q)];
}

}  // namespace

CART_EXPORT int btrapz_cartesian_host(const btrapz_refline *t, const int *line_index, int R, int n, int layout, const double *f,
                                      const int *count, double *cart, const btrapz_kin_audit *au) {
  if (bad_common(t, R, n, layout, f)) return BTRAPZ_EINVAL;
  if (!cart && !au) return BTRAPZ_EINVAL;
  if (au && !au->kappa_abs_max && !au->alat_abs_max && !au->a_min && !au->a_max && !au->v_max && !au->frame_min &&
      !au->n_outside && !au->worst)
    return BTRAPZ_EINVAL;
  for (int r = 0; r < R; r++) {
    Line ln;
    const bool has_line = row_line(t, line_index, r, ln);
    const int cnt = row_count(count, r, n);
    Extremes e;
    extremes_init(e);
    for (int j = 0; j < cnt; j++) {
      double u[6], out[6];
      read_sample(layout, f, (size_t)r, n, j, u);
      if (!has_line || outside(ln, u[0])) {
        e.n_outside++;
        if (cart) for (int i = 0; i < 6; i++) cart[((size_t)r * 6 + i) * n + j] = NAN;
        continue;
      }
      const RefPoint p = lookup(ln, u[0]);
      const Moving m = moving(p, u);
      map(p, m, u, out);
      if (cart) for (int i = 0; i < 6; i++) cart[((size_t)r * 6 + i) * n + j] = out[i];
      extremes_take(e, out, m.w, j);
    }
    if (au) {
      double *const val[6] = {au->kappa_abs_max, au->alat_abs_max, au->a_min, au->a_max, au->v_max, au->frame_min};
      for (int i = 0; i < 6; i++) {
        if (val[i]) val[i][r] = extremes_value(e, i);
        if (au->worst) au->worst[(size_t)r * 6 + i] = e.idx[i] == kNobody ? -1 : e.idx[i];
      }
      if (au->n_outside) au->n_outside[r] = e.n_outside;
    }
  }
  return BTRAPZ_OK;
}

CART_EXPORT int btrapz_cartesian_vjp_host(const btrapz_refline *t, const int *line_index, int R, int n, int layout,
                                          const double *f, const int *count, const double *cart_bar, double *f_bar) {
  if (bad_common(t, R, n, layout, f) || !cart_bar || !f_bar) return BTRAPZ_EINVAL;
  for (int r = 0; r < R; r++) {
    Line ln;
    const bool has_line = row_line(t, line_index, r, ln);
    const int cnt = row_count(count, r, n);
    for (int j = 0; j < n; j++) {
      double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (j < cnt && has_line) {
        double u[6];
        read_sample(layout, f, (size_t)r, n, j, u);
        if (!outside(ln, u[0])) {
          const RefPoint p = lookup(ln, u[0]);
          const Moving m = moving(p, u);
          double J[6][6];
          jacobian(p, m, u, J);
          for (int i = 0; i < 6; i++) {
            const double cb = cart_bar[((size_t)r * 6 + i) * n + j];
            for (int q = 0; q < 6; q++) g[q] += cb * J[i][q];
          }
        }
      }
      for (int q = 0; q < 6; q++) f_bar[frenet_offset(layout, (size_t)r, n, j, q)] = g[q];
    }
  }
  return BTRAPZ_OK;
}

CART_EXPORT int btrapz_cartesian_jvp_host(const btrapz_refline *t, const int *line_index, int R, int n, int layout,
                                          const double *f, const int *count, int T, const double *f_dot, double *cart_dot) {
  if (bad_common(t, R, n, layout, f) || !f_dot || !cart_dot) return BTRAPZ_EINVAL;
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) return BTRAPZ_EINVAL;
  const size_t slab = (size_t)R * 6 * (size_t)n;
  for (int r = 0; r < R; r++) {
    Line ln;
    const bool has_line = row_line(t, line_index, r, ln);
    const int cnt = row_count(count, r, n);
    for (int j = 0; j < cnt; j++) {
      double u[6], J[6][6];
      read_sample(layout, f, (size_t)r, n, j, u);
      const bool in = has_line && !outside(ln, u[0]);
      if (in) {
        const RefPoint p = lookup(ln, u[0]);
        const Moving m = moving(p, u);
        jacobian(p, m, u, J);
      }
      for (int k = 0; k < T; k++) {
        double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (in) {
          double ud[6];
          read_sample(layout, f_dot + (size_t)k * slab, (size_t)r, n, j, ud);
          for (int i = 0; i < 6; i++)
            for (int q = 0; q < 6; q++) d[i] += J[i][q] * ud[q];
        }
        for (int i = 0; i < 6; i++) cart_dot[(size_t)k * slab + ((size_t)r * 6 + i) * n + j] = d[i];
      }
    }
  }
  return BTRAPZ_OK;
}
