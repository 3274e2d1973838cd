// btrapz_cartesian.hip -- btrapz_cartesian_device / _vjp_device / _jvp_device (include/btrapz_hip_cartesian.h, DESIGN
// 3.19): Frenet samples to Cartesian states, the kinematic audit of a row, and the map's derivatives.  The per-sample
// statements -- lookup, map, 6 x 6 Jacobian, the audit's order -- are cartesian_core.h's, shared with the host twins.
//
// Mapping: one wavefront per row, kCartWaves wavefronts per workgroup (as btrapz_states.hip), lane q takes the samples
// q, q + 64, ... in rising order: the reads and writes of the SAMPLES layout and of cart are contiguous per row.  A
// workgroup walks the rows base, base + gridDim.x kCartWaves, ...; every wavefront of it passes the same barriers (a
// surplus wavefront stages nothing and skips the row).
//
// The row's rs line is staged in the wavefront's own slice of LDS while it fits (M <= kCartLdsM) and stays there for
// the next row when that row uses the same line; beyond that the binary search reads global memory.  The other five
// arrays are read at the interval's two ends only.
//
// Audit: each lane keeps six (key, sample) pairs over its own samples, then a butterfly over xor 32 ... 1 under the
// total order "better key, then lower sample".  No atomics: repeated calls are bit-identical, and the audit's bits do
// not depend on whether cart is written (the template argument removes stores, no arithmetic).
#include <hip/hip_runtime.h>

#include <string>

#include "btrapz_device.h"
#include "../../include/btrapz_hip_cartesian.h"
#include "cartesian_core.h"

#define UNROLL _Pragma("unroll")

namespace btrapz {

namespace {

using namespace cart;

constexpr int kCartWaves = 4;
constexpr int kCartLdsM = 1024;     // doubles of rs per wavefront: 32 KiB per workgroup
constexpr int kCartMaxBlocks = 2048;

struct CartArgs {
  int R, n, M, n_lines, T;
  const double *rs, *rx, *ry, *rtheta, *rkappa, *rdkappa;
  const int *line_index;
  const double *f;
  const int *count;
  double *cart;
  btrapz_kin_audit audit;
  const double *cart_bar;
  double *f_bar;
  const double *f_dot;
  double *cart_dot;
};

template <int LAYOUT>
__device__ __forceinline__ void load_sample(const double *f, size_t r, int n, int j, double u[6]) {
  UNROLL for (int q = 0; q < 6; q++) u[q] = f[frenet_offset(LAYOUT, r, n, j, q)];
}

// What every kernel does per row before its samples: the row's line (staged), its count.  Returns false for a
// surplus wavefront -- after the barrier.
struct Row {
  Line ln;
  bool has_line;
  int cnt;
};
__device__ __forceinline__ bool open_row(const CartArgs &a, long long r, double *lds, int &staged, int lane, Row &row) {
  const bool active = r < a.R;
  int li = -1;
  if (active) {
    li = a.line_index ? a.line_index[r] : 0;
    if (li < 0 || li >= a.n_lines) li = -1;
  }
  const bool stage = a.M <= kCartLdsM;
  const size_t o = (size_t)(li < 0 ? 0 : li) * (size_t)a.M;
  if (stage) {
    if (li >= 0 && li != staged) {
      for (int k = lane; k < a.M; k += 64) lds[k] = a.rs[o + k];
      staged = li;
    }
    __syncthreads();   // (the slice is the wavefront's own: what this orders is its writes before its reads)
  }
  if (!active) return false;
  row.ln.rs = stage ? lds : a.rs + o;
  row.ln.rx = a.rx + o; row.ln.ry = a.ry + o; row.ln.rtheta = a.rtheta + o; row.ln.rkappa = a.rkappa + o;
  row.ln.rdkappa = a.rdkappa + o; row.ln.M = a.M;
  row.has_line = li >= 0;
  int c = a.n;
  if (a.count) { c = a.count[r] < a.n ? a.count[r] : a.n; if (c < 0) c = 0; }
  row.cnt = c;
  return true;
}

template <int LAYOUT, bool CART, bool AUDIT>
__global__ __launch_bounds__(64 * kCartWaves) void cartesian_kernel(const CartArgs a) {
  __shared__ double rs_[kCartWaves][kCartLdsM];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const double nan = __builtin_nan("");
  int staged = -1;
  for (long long base = (long long)blockIdx.x * kCartWaves; base < a.R; base += (long long)gridDim.x * kCartWaves) {
    const long long r = base + wave;
    Row row;
    if (!open_row(a, r, rs_[wave], staged, lane, row)) continue;
    double *cr = CART ? a.cart + (size_t)r * 6 * a.n : nullptr;
    Extremes e;
    extremes_init(e);
    for (int j = lane; j < row.cnt; j += 64) {
      double u[6], out[6];
      load_sample<LAYOUT>(a.f, (size_t)r, a.n, j, u);
      if (!row.has_line || outside(row.ln, u[0])) {
        e.n_outside++;
        if (CART) UNROLL for (int i = 0; i < 6; i++) cr[(size_t)i * a.n + j] = nan;
        continue;
      }
      const RefPoint p = lookup(row.ln, u[0]);
      const Moving m = moving(p, u);
      map(p, m, u, out);
      if (CART) UNROLL for (int i = 0; i < 6; i++) cr[(size_t)i * a.n + j] = out[i];
      if (AUDIT) extremes_take(e, out, m.w, j);
    }
    if (AUDIT) {
      UNROLL for (int d = 32; d >= 1; d >>= 1) {
        UNROLL for (int i = 0; i < 6; i++) {
          const double ok = __shfl_xor(e.key[i], d);
          const int oi = __shfl_xor(e.idx[i], d);
          extremes_merge(e.key[i], e.idx[i], ok, oi);
        }
        e.n_outside += __shfl_xor(e.n_outside, d);
      }
      if (lane == 0) {
        double *const val[6] = {a.audit.kappa_abs_max, a.audit.alat_abs_max, a.audit.a_min, a.audit.a_max, a.audit.v_max,
                                a.audit.frame_min};
        UNROLL for (int i = 0; i < 6; i++) {
          if (val[i]) val[i][r] = extremes_value(e, i);
          if (a.audit.worst) a.audit.worst[(size_t)r * 6 + i] = e.idx[i] == kNobody ? -1 : e.idx[i];
        }
        if (a.audit.n_outside) a.audit.n_outside[r] = e.n_outside;
      }
    }
  }
}

// MODE 0: f_bar = J' cart_bar (every sample of the row is written); MODE 1: cart_dot[t] = J f_dot[t] for the samples read
template <int LAYOUT, int MODE>
__global__ __launch_bounds__(64 * kCartWaves) void cartesian_grad_kernel(const CartArgs a) {
  __shared__ double rs_[kCartWaves][kCartLdsM];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const size_t slab = (size_t)a.R * 6 * (size_t)a.n;
  int staged = -1;
  for (long long base = (long long)blockIdx.x * kCartWaves; base < a.R; base += (long long)gridDim.x * kCartWaves) {
    const long long r = base + wave;
    Row row;
    if (!open_row(a, r, rs_[wave], staged, lane, row)) continue;
    const int last = MODE == 0 ? a.n : row.cnt;
    for (int j = lane; j < last; j += 64) {
      double u[6], J[6][6];
      bool in = false;
      if (j < row.cnt && row.has_line) {
        load_sample<LAYOUT>(a.f, (size_t)r, a.n, j, u);
        in = !outside(row.ln, u[0]);
      }
      if (in) {
        const RefPoint p = lookup(row.ln, u[0]);
        const Moving m = moving(p, u);
        jacobian(p, m, u, J);
      }
      if (MODE == 0) {
        double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (in) {
          UNROLL for (int i = 0; i < 6; i++) {
            const double cb = a.cart_bar[((size_t)r * 6 + i) * a.n + j];
            UNROLL for (int q = 0; q < 6; q++) g[q] += cb * J[i][q];
          }
        }
        UNROLL for (int q = 0; q < 6; q++) a.f_bar[frenet_offset(LAYOUT, (size_t)r, a.n, j, q)] = g[q];
      } else {
        for (int t = 0; t < a.T; t++) {
          double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          if (in) {
            double ud[6];
            load_sample<LAYOUT>(a.f_dot + (size_t)t * slab, (size_t)r, a.n, j, ud);
            UNROLL for (int i = 0; i < 6; i++)
              UNROLL for (int q = 0; q < 6; q++) d[i] += J[i][q] * ud[q];
          }
          UNROLL for (int i = 0; i < 6; i++) a.cart_dot[(size_t)t * slab + ((size_t)r * 6 + i) * a.n + j] = d[i];
        }
      }
    }
  }
}

int refuse(btrapz_ctx *c, const char *what) {
  btrapz_ctx_set_error(c, what);
  return BTRAPZ_EINVAL;
}
// the checks the three entry points share; nullptr: none failed
const char *bad_common(const btrapz_refline *t, int R, int n, int layout, const double *f) {
  if (!t) return "invalid argument: refline (null)";
  if (!t->rs || !t->rx || !t->ry || !t->rtheta || !t->rkappa || !t->rdkappa) return "invalid argument: refline (an array is null)";
  if (!f) return "invalid argument: f (null)";
  if (R < 1) return "invalid argument: R (< 1)";
  if (n < 1) return "invalid argument: n (< 1)";
  if (t->n_lines < 1) return "invalid argument: refline.n_lines (< 1)";
  if (t->M < 2) return "invalid argument: refline.M (< 2)";
  if (layout != BTRAPZ_FRENET_SAMPLES && layout != BTRAPZ_FRENET_STATES) return "invalid argument: layout (unknown)";
  return nullptr;
}
CartArgs common_args(const btrapz_refline *t, const int *line_index, int R, int n, const double *f, const int *count) {
  CartArgs a = {};
  a.R = R; a.n = n; a.M = t->M; a.n_lines = t->n_lines;
  a.rs = t->rs; a.rx = t->rx; a.ry = t->ry; a.rtheta = t->rtheta; a.rkappa = t->rkappa; a.rdkappa = t->rdkappa;
  a.line_index = line_index; a.f = f; a.count = count;
  return a;
}
template <class K>
int launch(btrapz_ctx *c, K kernel, const CartArgs &a, void *stream, const char *what) {
  hipError_t e = hipSetDevice(btrapz_ctx_device(c));
  if (e == hipSuccess) {
    const long long groups = ((long long)a.R + kCartWaves - 1) / kCartWaves;
    const unsigned blocks = (unsigned)(groups < kCartMaxBlocks ? groups : kCartMaxBlocks);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * kCartWaves), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) return BTRAPZ_OK;
  btrapz_ctx_set_error(c, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return BTRAPZ_EHIP;
}

}  // namespace

}  // namespace btrapz

using namespace btrapz;

BTRAPZ_EXPORT int btrapz_cartesian_device(btrapz_ctx *c, const btrapz_refline *t, const int *line_index, int R, int n, int layout,
                                          const double *f, const int *count, double *cart, const btrapz_kin_audit *au,
                                          void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(t, R, n, layout, f)) return refuse(c, why);
  if (!cart && !au) return refuse(c, "invalid argument: cart and audit are both null");
  if (au && !au->kappa_abs_max && !au->alat_abs_max && !au->a_min && !au->a_max && !au->v_max && !au->frame_min &&
      !au->n_outside && !au->worst)
    return refuse(c, "invalid argument: audit (every field is null)");
  CartArgs a = common_args(t, line_index, R, n, f, count);
  a.cart = cart;
  if (au) a.audit = *au;
  const char *what = "btrapz_cartesian_device";
  const bool samples = layout == BTRAPZ_FRENET_SAMPLES;
  if (cart && au) return samples ? launch(c, cartesian_kernel<0, true, true>, a, stream, what) : launch(c, cartesian_kernel<1, true, true>, a, stream, what);
  if (cart) return samples ? launch(c, cartesian_kernel<0, true, false>, a, stream, what) : launch(c, cartesian_kernel<1, true, false>, a, stream, what);
  return samples ? launch(c, cartesian_kernel<0, false, true>, a, stream, what) : launch(c, cartesian_kernel<1, false, true>, a, stream, what);
}

BTRAPZ_EXPORT int btrapz_cartesian_vjp_device(btrapz_ctx *c, const btrapz_refline *t, const int *line_index, int R, int n,
                                              int layout, const double *f, const int *count, const double *cart_bar,
                                              double *f_bar, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(t, R, n, layout, f)) return refuse(c, why);
  if (!cart_bar) return refuse(c, "invalid argument: cart_bar (null)");
  if (!f_bar) return refuse(c, "invalid argument: f_bar (null)");
  CartArgs a = common_args(t, line_index, R, n, f, count);
  a.cart_bar = cart_bar; a.f_bar = f_bar;
  const char *what = "btrapz_cartesian_vjp_device";
  return layout == BTRAPZ_FRENET_SAMPLES ? launch(c, cartesian_grad_kernel<0, 0>, a, stream, what)
                                         : launch(c, cartesian_grad_kernel<1, 0>, a, stream, what);
}

BTRAPZ_EXPORT int btrapz_cartesian_jvp_device(btrapz_ctx *c, const btrapz_refline *t, const int *line_index, int R, int n,
                                              int layout, const double *f, const int *count, int T, const double *f_dot,
                                              double *cart_dot, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(t, R, n, layout, f)) return refuse(c, why);
  if (!f_dot) return refuse(c, "invalid argument: f_dot (null)");
  if (!cart_dot) return refuse(c, "invalid argument: cart_dot (null)");
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) return refuse(c, "invalid argument: T (1 .. BTRAPZ_MAX_TANGENTS = 32)");
  CartArgs a = common_args(t, line_index, R, n, f, count);
  a.T = T; a.f_dot = f_dot; a.cart_dot = cart_dot;
  const char *what = "btrapz_cartesian_jvp_device";
  return layout == BTRAPZ_FRENET_SAMPLES ? launch(c, cartesian_grad_kernel<0, 1>, a, stream, what)
                                         : launch(c, cartesian_grad_kernel<1, 1>, a, stream, what);
}
