// btrapz_clearance.hip -- btrapz_clearance_device / _vjp_device / _jvp_device (include/btrapz_hip_clearance.h, DESIGN
// 3.21): the signed clearance of the ego's rectangle against a scene's obstacle rectangles per sample, the audit of a
// row, and the derivatives under the frozen feature.  The per-pair statements are clearance_core.h's, shared with the
// host twins.
//
// Mapping: that of btrapz_cartesian.hip -- one wavefront per row, kClrWaves wavefronts per workgroup, lane q takes the
// samples q, q + 64, ... in rising order, so the three pose rows of cart, every obstacle's three pose rows and the
// outputs are read and written contiguously along the samples.  A workgroup walks the rows base, base + gridDim.x
// kClrWaves, ...  There is no barrier and no LDS: rows of one scene sit next to each other, so the obstacle columns a
// wavefront reads are the ones its neighbours just read, and they come from the caches.
//
// The ego's sincos is taken once per sample, an obstacle's once per (row, sample, obstacle) -- recomputed, not staged
// (DESIGN 3.21 says what that costs).  The obstacle loop has no chunking: one obstacle per trip, scene_count trips.
//
// Audit: each lane keeps (least clearance, sample, which) over its own samples, then a butterfly over xor 32 ... 1 under
// the total order "smaller value, then lower sample".  No atomics: repeated calls are bit-identical, and the audit's bits
// do not depend on which of clear and which are written (the template arguments remove stores, no arithmetic).
//
// The derivative kernels read `which` and one obstacle per sample: no obstacle loop.  An obstacle index that `which`
// names is checked against the scene's count before anything is read through it.
#include <hip/hip_runtime.h>

#include <string>

#include "btrapz_device.h"
#include "../../include/btrapz_hip_clearance.h"
#include "clearance_core.h"

#define UNROLL _Pragma("unroll")

namespace btrapz {

namespace {

using namespace clr;

constexpr int kClrWaves = 4;
constexpr int kClrMaxBlocks = 4096;

struct ClrArgs {
  int R, n, O, n_scenes, T;
  Foot foot;
  const double *pose, *half;
  const int *obs_count, *scene_index;
  const double *cart;
  const int *count;
  double d_safe;
  double *clear;
  int *which_out;
  btrapz_clear_audit audit;
  const int *which;
  const double *clear_bar;
  double *cart_bar;
  const double *cart_dot, *obs_dot;
  double *clear_dot;
};

// what every kernel knows of a row before its samples: the scene's arrays and counts
struct Row {
  const double *pose, *half;   // the scene's [O][3][n] and [O][2]
  int scene;                   // -1: no such scene, the whole row is invalid
  int obs;                     // obstacles of the scene
  int cnt;                     // samples read
};
__device__ __forceinline__ Row open_row(const ClrArgs &a, long long r) {
  Row row;
  int sc = a.scene_index ? a.scene_index[r] : 0;
  if (sc < 0 || sc >= a.n_scenes) sc = -1;
  row.scene = sc;
  const size_t k = (size_t)(sc < 0 ? 0 : sc);
  row.pose = a.pose + k * (size_t)a.O * 3 * (size_t)a.n;
  row.half = a.half + k * (size_t)a.O * 2;
  row.obs = sc < 0 ? 0 : scene_count(a.obs_count, sc, a.O);
  int c = a.n;
  if (a.count) { c = a.count[r] < a.n ? a.count[r] : a.n; if (c < 0) c = 0; }
  row.cnt = c;
  return row;
}
// the ego at sample j of row r; false: its pose holds a NaN
__device__ __forceinline__ bool load_ego(const double *cart, long long r, int n, int j, Ego &e) {
  const double *cr = cart + (size_t)r * 6 * (size_t)n + (size_t)j;
  const double x = cr[(size_t)BTRAPZ_CART_X * n], y = cr[(size_t)BTRAPZ_CART_Y * n], th = cr[(size_t)BTRAPZ_CART_THETA * n];
  if (is_nan3(x, y, th)) return false;
  e.x = x; e.y = y;
  sin_cos(th, e.sa, e.ca);
  return true;
}

template <bool CLEAR, bool WHICH, bool AUDIT>
__global__ __launch_bounds__(64 * kClrWaves) void clearance_kernel(const ClrArgs a) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const double nan = __builtin_nan("");
  for (long long base = (long long)blockIdx.x * kClrWaves; base < a.R; base += (long long)gridDim.x * kClrWaves) {
    const long long r = base + wave;
    if (r >= a.R) continue;
    const Row row = open_row(a, r);
    Least l;
    least_init(l);
    for (int j = lane; j < row.cnt; j += 64) {
      Ego e;
      double cl = nan;
      int wh = -1;
      if (row.scene >= 0 && load_ego(a.cart, r, a.n, j, e)) {
        cl = sample_clearance(a.foot, e, row.pose, row.half, row.obs, a.n, j, wh);
        if (AUDIT) least_take(l, cl, wh, j, a.d_safe);
      } else {
        l.n_invalid++;
      }
      if (CLEAR) a.clear[(size_t)r * a.n + j] = cl;
      if (WHICH) a.which_out[(size_t)r * a.n + j] = wh;
    }
    if (AUDIT) {
      UNROLL for (int d = 32; d >= 1; d >>= 1) {
        const double ok = __shfl_xor(l.key, d);
        const int oi = __shfl_xor(l.idx, d);
        const int ow = __shfl_xor(l.which, d);
        least_merge(l, ok, oi, ow);
        l.n_below += __shfl_xor(l.n_below, d);
        l.n_invalid += __shfl_xor(l.n_invalid, d);
      }
      if (lane == 0) {
        const bool nobody = l.idx == kNobody;
        if (a.audit.clear_min) a.audit.clear_min[r] = l.key;
        if (a.audit.worst) {
          a.audit.worst[(size_t)r * 2] = nobody ? -1 : l.idx;
          a.audit.worst[(size_t)r * 2 + 1] = nobody ? -1 : (l.which >> 4);
        }
        if (a.audit.n_below) a.audit.n_below[r] = l.n_below;
        if (a.audit.n_invalid) a.audit.n_invalid[r] = l.n_invalid;
      }
    }
  }
}

// MODE 0: cart_bar = J' clear_bar (every sample of the row is written, all six rows); MODE 1: clear_dot[t] = J (cart_dot[t],
// obs_dot[t]) for the samples read
template <int MODE>
__global__ __launch_bounds__(64 * kClrWaves) void clearance_grad_kernel(const ClrArgs a) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const size_t cslab = (size_t)a.R * 6 * (size_t)a.n, oslab = (size_t)a.n_scenes * a.O * 3 * (size_t)a.n;
  for (long long base = (long long)blockIdx.x * kClrWaves; base < a.R; base += (long long)gridDim.x * kClrWaves) {
    const long long r = base + wave;
    if (r >= a.R) continue;
    const Row row = open_row(a, r);
    const int last = MODE == 0 ? a.n : row.cnt;
    for (int j = lane; j < last; j += 64) {
      Ego e;
      Grad g;
      int o = 0;
      bool in = false;
      if (j < row.cnt && row.scene >= 0 && load_ego(a.cart, r, a.n, j, e))
        in = sample_gradient(a.foot, e, row.pose, row.half, row.obs, a.n, j, a.which[(size_t)r * a.n + j], o, g);
      if (MODE == 0) {
        double *cb = a.cart_bar + (size_t)r * 6 * (size_t)a.n + j;
        double bx = 0.0, by = 0.0, bt = 0.0;
        if (in) {
          const double w = a.clear_bar[(size_t)r * a.n + j];
          bx = w * g.nx; by = w * g.ny; bt = w * g.la;
        }
        cb[(size_t)BTRAPZ_CART_X * a.n] = bx;
        cb[(size_t)BTRAPZ_CART_Y * a.n] = by;
        cb[(size_t)BTRAPZ_CART_THETA * a.n] = bt;
        cb[(size_t)BTRAPZ_CART_KAPPA * a.n] = 0.0;
        cb[(size_t)BTRAPZ_CART_V * a.n] = 0.0;
        cb[(size_t)BTRAPZ_CART_A * a.n] = 0.0;
      } else {
        for (int t = 0; t < a.T; t++) {
          double d = 0.0;
          if (in) {
            const double *cd = a.cart_dot + (size_t)t * cslab + (size_t)r * 6 * (size_t)a.n + j;
            double vx = cd[(size_t)BTRAPZ_CART_X * a.n], vy = cd[(size_t)BTRAPZ_CART_Y * a.n];
            d = g.la * cd[(size_t)BTRAPZ_CART_THETA * a.n];
            if (a.obs_dot) {
              const double *od = a.obs_dot + (size_t)t * oslab + ((size_t)row.scene * a.O + o) * 3 * (size_t)a.n + j;
              vx -= od[0]; vy -= od[a.n];
              d -= g.lb * od[2 * (size_t)a.n];
            }
            d += g.nx * vx + g.ny * vy;
          }
          a.clear_dot[((size_t)t * a.R + (size_t)r) * a.n + j] = d;
        }
      }
    }
  }
}

int refuse(btrapz_ctx *c, const char *what) {
  btrapz_ctx_set_error(c, what);
  return BTRAPZ_EINVAL;
}
bool good_extent(double v) { return v > 0.0 && v < HUGE_VAL; }
// the checks the three entry points share; nullptr: none failed
const char *bad_common(const btrapz_footprint *ft, const btrapz_obstacles *ob, int R, int n, const double *cart) {
  if (!ft) return "invalid argument: footprint (null)";
  if (!ob) return "invalid argument: obstacles (null)";
  if (!ob->pose || !ob->half) return "invalid argument: obstacles (pose or half is null)";
  if (!cart) return "invalid argument: cart (null)";
  if (R < 1) return "invalid argument: R (< 1)";
  if (n < 1) return "invalid argument: n (< 1)";
  if (ob->O < 1) return "invalid argument: obstacles.O (< 1)";
  if (ob->n_scenes < 1) return "invalid argument: obstacles.n_scenes (< 1)";
  if (ob->n != n) return "invalid argument: obstacles.n (differs from n)";
  if (!good_extent(ft->half_length) || !good_extent(ft->half_width))
    return "invalid argument: footprint (a half extent is not > 0 and finite)";
  if (!(fabs(ft->centre_offset) < HUGE_VAL)) return "invalid argument: footprint.centre_offset (not finite)";
  return nullptr;
}
ClrArgs common_args(const btrapz_footprint *ft, const btrapz_obstacles *ob, const int *scene_index, int R, int n,
                    const double *cart, const int *count) {
  ClrArgs a = {};
  a.R = R; a.n = n; a.O = ob->O; a.n_scenes = ob->n_scenes;
  a.foot.hl = ft->half_length; a.foot.hw = ft->half_width; a.foot.off = ft->centre_offset;
  a.pose = ob->pose; a.half = ob->half; a.obs_count = ob->obs_count;
  a.scene_index = scene_index; a.cart = cart; a.count = count;
  return a;
}
template <class K>
int launch(btrapz_ctx *c, K kernel, const ClrArgs &a, void *stream, const char *what) {
  hipError_t e = hipSetDevice(btrapz_ctx_device(c));
  if (e == hipSuccess) {
    const long long groups = ((long long)a.R + kClrWaves - 1) / kClrWaves;
    const unsigned blocks = (unsigned)(groups < kClrMaxBlocks ? groups : kClrMaxBlocks);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * kClrWaves), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) return BTRAPZ_OK;
  btrapz_ctx_set_error(c, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return BTRAPZ_EHIP;
}

}  // namespace

}  // namespace btrapz

using namespace btrapz;

BTRAPZ_EXPORT int btrapz_clearance_device(btrapz_ctx *c, const btrapz_footprint *ft, const btrapz_obstacles *ob,
                                          const int *scene_index, int R, int n, const double *cart, const int *count,
                                          double d_safe, double *clear, int *which, const btrapz_clear_audit *au, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(ft, ob, R, n, cart)) return refuse(c, why);
  if (!clear && !which && !au) return refuse(c, "invalid argument: clear, which and audit are all null");
  if (au && !au->clear_min && !au->worst && !au->n_below && !au->n_invalid)
    return refuse(c, "invalid argument: audit (every field is null)");
  ClrArgs a = common_args(ft, ob, scene_index, R, n, cart, count);
  a.d_safe = d_safe; a.clear = clear; a.which_out = which;
  if (au) a.audit = *au;
  const char *what = "btrapz_clearance_device";
  const int form = (clear ? 4 : 0) | (which ? 2 : 0) | (au ? 1 : 0);
  switch (form) {
    case 7: return launch(c, clearance_kernel<true, true, true>, a, stream, what);
    case 6: return launch(c, clearance_kernel<true, true, false>, a, stream, what);
    case 5: return launch(c, clearance_kernel<true, false, true>, a, stream, what);
    case 4: return launch(c, clearance_kernel<true, false, false>, a, stream, what);
    case 3: return launch(c, clearance_kernel<false, true, true>, a, stream, what);
    case 2: return launch(c, clearance_kernel<false, true, false>, a, stream, what);
    default: return launch(c, clearance_kernel<false, false, true>, a, stream, what);
  }
}

BTRAPZ_EXPORT int btrapz_clearance_vjp_device(btrapz_ctx *c, const btrapz_footprint *ft, const btrapz_obstacles *ob,
                                              const int *scene_index, int R, int n, const double *cart, const int *count,
                                              const int *which, const double *clear_bar, double *cart_bar, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(ft, ob, R, n, cart)) return refuse(c, why);
  if (!which) return refuse(c, "invalid argument: which (null)");
  if (!clear_bar) return refuse(c, "invalid argument: clear_bar (null)");
  if (!cart_bar) return refuse(c, "invalid argument: cart_bar (null)");
  ClrArgs a = common_args(ft, ob, scene_index, R, n, cart, count);
  a.which = which; a.clear_bar = clear_bar; a.cart_bar = cart_bar;
  return launch(c, clearance_grad_kernel<0>, a, stream, "btrapz_clearance_vjp_device");
}

BTRAPZ_EXPORT int btrapz_clearance_jvp_device(btrapz_ctx *c, const btrapz_footprint *ft, const btrapz_obstacles *ob,
                                              const int *scene_index, int R, int n, const double *cart, const int *count,
                                              const int *which, int T, const double *cart_dot, const double *obs_dot,
                                              double *clear_dot, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(ft, ob, R, n, cart)) return refuse(c, why);
  if (!which) return refuse(c, "invalid argument: which (null)");
  if (!cart_dot) return refuse(c, "invalid argument: cart_dot (null)");
  if (!clear_dot) return refuse(c, "invalid argument: clear_dot (null)");
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) return refuse(c, "invalid argument: T (1 .. BTRAPZ_MAX_TANGENTS = 32)");
  ClrArgs a = common_args(ft, ob, scene_index, R, n, cart, count);
  a.which = which; a.T = T; a.cart_dot = cart_dot; a.obs_dot = obs_dot; a.clear_dot = clear_dot;
  return launch(c, clearance_grad_kernel<1>, a, stream, "btrapz_clearance_jvp_device");
}
