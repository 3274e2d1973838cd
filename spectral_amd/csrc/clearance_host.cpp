// clearance_host.cpp -- btrapz_clearance_host / _vjp_host / _jvp_host (include/btrapz_hip_clearance.h): the clearance
// stage on the host, sample by sample with the statements of clearance_core.h that the kernels run.  No GPU, no context.
// Plain C++ (g++ builds it for the sanitizer program, host_check/clearance_check.cpp).
#include <math.h>

#include "../../include/btrapz_hip_clearance.h"
#include "clearance_core.h"

#define CLR_EXPORT extern "C" __attribute__((visibility("default")))

using namespace btrapz::clr;

namespace {

bool good_extent(double v) { return v > 0.0 && v < HUGE_VAL; }

bool bad_common(const btrapz_footprint *ft, const btrapz_obstacles *ob, int R, int n, const double *cart) {
  if (!ft || !ob || !ob->pose || !ob->half || !cart) return true;
  if (R < 1 || n < 1 || ob->O < 1 || ob->n_scenes < 1 || ob->n != n) return true;
  if (!good_extent(ft->half_length) || !good_extent(ft->half_width) || !(fabs(ft->centre_offset) < HUGE_VAL)) return true;
  const size_t halves = (size_t)ob->n_scenes * (size_t)ob->O * 2;
  for (size_t i = 0; i < halves; i++)
    if (!good_extent(ob->half[i])) return true;
  return false;
}

struct Row {
  const double *pose, *half;
  int scene, obs, cnt;
};
Row open_row(const btrapz_obstacles *ob, const int *scene_index, const int *count, int r, int n) {
  Row row;
  int sc = scene_index ? scene_index[r] : 0;
  if (sc < 0 || sc >= ob->n_scenes) sc = -1;
  row.scene = sc;
  const size_t k = (size_t)(sc < 0 ? 0 : sc);
  row.pose = ob->pose + k * (size_t)ob->O * 3 * (size_t)n;
  row.half = ob->half + k * (size_t)ob->O * 2;
  row.obs = sc < 0 ? 0 : scene_count(ob->obs_count, sc, ob->O);
  int c = n;
  if (count) { c = count[r] < n ? count[r] : n; if (c < 0) c = 0; }
  row.cnt = c;
  return row;
}
bool load_ego(const double *cart, int r, int n, int j, Ego &e) {
  const double *cr = cart + (size_t)r * 6 * (size_t)n + (size_t)j;
  const double x = cr[(size_t)BTRAPZ_CART_X * n], y = cr[(size_t)BTRAPZ_CART_Y * n], th = cr[(size_t)BTRAPZ_CART_THETA * n];
  if (is_nan3(x, y, th)) return false;
  e.x = x; e.y = y;
  sin_cos(th, e.sa, e.ca);
  return true;
}
Foot foot_of(const btrapz_footprint *ft) {
  Foot f;
  f.hl = ft->half_length; f.hw = ft->half_width; f.off = ft->centre_offset;
  return f;
}

}  // namespace

CLR_EXPORT int btrapz_clearance_host(const btrapz_footprint *ft, const btrapz_obstacles *ob, const int *scene_index, int R, int n,
                                     const double *cart, const int *count, double d_safe, double *clear, int *which,
                                     const btrapz_clear_audit *au) {
  if (bad_common(ft, ob, R, n, cart)) return BTRAPZ_EINVAL;
  if (!clear && !which && !au) return BTRAPZ_EINVAL;
  if (au && !au->clear_min && !au->worst && !au->n_below && !au->n_invalid) return BTRAPZ_EINVAL;
  const Foot foot = foot_of(ft);
  for (int r = 0; r < R; r++) {
    const Row row = open_row(ob, scene_index, count, r, n);
    Least l;
    least_init(l);
    for (int j = 0; j < row.cnt; j++) {
      Ego e;
      double cl = NAN;
      int wh = -1;
      if (row.scene >= 0 && load_ego(cart, r, n, j, e)) {
        cl = sample_clearance(foot, e, row.pose, row.half, row.obs, n, j, wh);
        least_take(l, cl, wh, j, d_safe);
      } else {
        l.n_invalid++;
      }
      if (clear) clear[(size_t)r * n + j] = cl;
      if (which) which[(size_t)r * n + j] = wh;
    }
    if (au) {
      const bool nobody = l.idx == kNobody;
      if (au->clear_min) au->clear_min[r] = l.key;
      if (au->worst) {
        au->worst[(size_t)r * 2] = nobody ? -1 : l.idx;
        au->worst[(size_t)r * 2 + 1] = nobody ? -1 : (l.which >> 4);
      }
      if (au->n_below) au->n_below[r] = l.n_below;
      if (au->n_invalid) au->n_invalid[r] = l.n_invalid;
    }
  }
  return BTRAPZ_OK;
}

CLR_EXPORT int btrapz_clearance_vjp_host(const btrapz_footprint *ft, const btrapz_obstacles *ob, const int *scene_index, int R,
                                         int n, const double *cart, const int *count, const int *which, const double *clear_bar,
                                         double *cart_bar) {
  if (bad_common(ft, ob, R, n, cart) || !which || !clear_bar || !cart_bar) return BTRAPZ_EINVAL;
  const Foot foot = foot_of(ft);
  for (int r = 0; r < R; r++) {
    const Row row = open_row(ob, scene_index, count, r, n);
    for (int j = 0; j < n; j++) {
      Ego e;
      Grad g;
      int o = 0;
      bool in = false;
      if (j < row.cnt && row.scene >= 0 && load_ego(cart, r, n, j, e))
        in = sample_gradient(foot, e, row.pose, row.half, row.obs, n, j, which[(size_t)r * n + j], o, g);
      double *cb = cart_bar + (size_t)r * 6 * (size_t)n + j;
      for (int i = 0; i < 6; i++) cb[(size_t)i * n] = 0.0;
      if (in) {
        const double w = clear_bar[(size_t)r * n + j];
        cb[(size_t)BTRAPZ_CART_X * n] = w * g.nx;
        cb[(size_t)BTRAPZ_CART_Y * n] = w * g.ny;
        cb[(size_t)BTRAPZ_CART_THETA * n] = w * g.la;
      }
    }
  }
  return BTRAPZ_OK;
}

CLR_EXPORT int btrapz_clearance_jvp_host(const btrapz_footprint *ft, const btrapz_obstacles *ob, const int *scene_index, int R,
                                         int n, const double *cart, const int *count, const int *which, int T,
                                         const double *cart_dot, const double *obs_dot, double *clear_dot) {
  if (bad_common(ft, ob, R, n, cart) || !which || !cart_dot || !clear_dot) return BTRAPZ_EINVAL;
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) return BTRAPZ_EINVAL;
  const Foot foot = foot_of(ft);
  const size_t cslab = (size_t)R * 6 * (size_t)n, oslab = (size_t)ob->n_scenes * ob->O * 3 * (size_t)n;
  for (int r = 0; r < R; r++) {
    const Row row = open_row(ob, scene_index, count, r, n);
    for (int j = 0; j < row.cnt; j++) {
      Ego e;
      Grad g;
      int o = 0;
      bool in = false;
      if (row.scene >= 0 && load_ego(cart, r, n, j, e))
        in = sample_gradient(foot, e, row.pose, row.half, row.obs, n, j, which[(size_t)r * n + j], o, g);
      for (int t = 0; t < T; t++) {
        double d = 0.0;
        if (in) {
          const double *cd = cart_dot + (size_t)t * cslab + (size_t)r * 6 * (size_t)n + j;
          double vx = cd[(size_t)BTRAPZ_CART_X * n], vy = cd[(size_t)BTRAPZ_CART_Y * n];
          d = g.la * cd[(size_t)BTRAPZ_CART_THETA * n];
          if (obs_dot) {
            const double *od = obs_dot + (size_t)t * oslab + ((size_t)row.scene * ob->O + o) * 3 * (size_t)n + j;
            vx -= od[0]; vy -= od[n];
            d -= g.lb * od[2 * (size_t)n];
          }
          d += g.nx * vx + g.ny * vy;
        }
        clear_dot[((size_t)t * R + (size_t)r) * n + j] = d;
      }
    }
  }
  return BTRAPZ_OK;
}
