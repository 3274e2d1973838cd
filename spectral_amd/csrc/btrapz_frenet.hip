// btrapz_frenet.hip -- btrapz_frenet_device / _vjp_device / _jvp_device (include/btrapz_hip_frenet.h):
// Cartesian states projected onto the reference line, and the derivatives of that map.  The per-sample statements --
// candidate rule, chord distance, window range, refinement, map, 6 x 6 Jacobian -- are frenet_core.h's, shared with the
// host twins.
//
// Forward.  A workgroup of 256 threads owns whole rows: kThreads / n of them while n < kThreads (thread = one query),
// else one row in slices of kThreads queries; workgroups walk the row groups with a grid stride.  The coarse pass is
// the hot path, O(M) per query: the line's (rx, ry, cos rtheta, sin rtheta) are staged in LDS, kLdsM points at a time
// (32 KiB; the cosines and sines are formed while staging, one sincos per point and workgroup, so the sweep itself
// holds no transcendental), and every thread sweeps the staged points for its own query.  All lanes of a wavefront read
// the same LDS address per step (a broadcast, no bank conflict) and keep the winner so far in registers: the order
// (d^2, then index) is total and each thread meets its intervals in rising order, so no reduction across lanes is
// needed.  A window shrinks the sweep of a wavefront to the union of its lanes' index ranges (two binary searches per
// row, a min / max butterfly per wavefront).  Rows of one group that use different lines are served line by line:
// one pass per distinct line in row order, the threads of other lines idle meanwhile.  A line that is already staged
// is not staged again (M <= kLdsM).  Then every thread refines and maps its own query.
//
// n_outside of a row is summed by the row's first thread from the group's flags in LDS (n < kThreads), or counted by
// the barrier (one row per workgroup).  No atomics anywhere: repeated calls are bit-identical.
//
// Derivatives: per-sample maps over the flat index r n + j, one kernel template for VJP and JVP; the table is read at the
// interval's two ends from global memory.
#include <hip/hip_runtime.h>

#include <string>

#include "btrapz_device.h"
#include "../../include/btrapz_hip_frenet.h"
#include "frenet_core.h"

#define UNROLL _Pragma("unroll")

namespace btrapz {

namespace {

using namespace frenet;
using cart::frenet_offset;

constexpr int kThreads = 256;
constexpr int kLdsM = 1024;       // table points staged at a time: 4 arrays of doubles, 32 KiB
constexpr int kMaxBlocks = 4096;
constexpr int kNone = 0x7fffffff;

struct FrenetArgs {
  int R, n, M, n_lines, T, order;
  const double *rs, *rx, *ry, *rtheta, *rkappa, *rdkappa;
  const int *line_index;
  const double *cart;
  const int *count;
  const double *s_window;
  double *frenet;
  int *interval;
  int *n_outside;
  const double *frenet_in;
  const int *interval_in;
  const double *frenet_bar;
  double *cart_bar;
  const double *cart_dot;
  double *frenet_dot;
};

__device__ __forceinline__ int line_of(const FrenetArgs &a, long long r) {
  const int li = a.line_index ? a.line_index[r] : 0;
  return (li < 0 || li >= a.n_lines) ? -1 : li;
}
__device__ __forceinline__ Line line_at(const FrenetArgs &a, int li) {
  const size_t o = (size_t)li * (size_t)a.M;
  Line ln;
  ln.rs = a.rs + o; ln.rx = a.rx + o; ln.ry = a.ry + o; ln.rtheta = a.rtheta + o; ln.rkappa = a.rkappa + o;
  ln.rdkappa = a.rdkappa + o; ln.M = a.M;
  return ln;
}
__device__ __forceinline__ int row_count(const FrenetArgs &a, long long r) {
  if (!a.count) return a.n;
  const int c = a.count[r] < a.n ? a.count[r] : a.n;
  return c > 0 ? c : 0;
}
// the rows of cart up to the order; the others are not read
__device__ __forceinline__ void read_cart(const double *cart, size_t r, int n, int j, int order, double c[6]) {
  const double *cr = cart + r * 6 * (size_t)n + j;
  UNROLL for (int i = 0; i < 6; i++) c[i] = 0.0;
  c[0] = cr[0]; c[1] = cr[(size_t)n];
  if (order >= 1) { c[2] = cr[2 * (size_t)n]; c[4] = cr[4 * (size_t)n]; }
  if (order >= 2) { c[3] = cr[3 * (size_t)n]; c[5] = cr[5 * (size_t)n]; }
}

template <int LAYOUT>
__global__ __launch_bounds__(kThreads) void frenet_kernel(const FrenetArgs a) {
  __shared__ double px_[kLdsM], py_[kLdsM], pc_[kLdsM], ps_[kLdsM];
  __shared__ int flag_[kThreads];
  const int tid = (int)threadIdx.x;
  const bool one_row = a.n >= kThreads;
  const int rpb = one_row ? 1 : kThreads / a.n;                          // rows of a group
  const int slices = one_row ? (a.n + kThreads - 1) / kThreads : 1;      // slices of a row
  const int lr = one_row ? 0 : tid / a.n;                                // this thread's row within the group
  const int jl = one_row ? tid : tid - lr * a.n;
  const long long groups = ((long long)a.R + rpb - 1) / rpb;
  const double nan = __builtin_nan("");
  int staged_line = -1, staged_c0 = -1;

  for (long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const long long r0 = grp * rpb;
    const int rows = (long long)rpb < a.R - r0 ? rpb : (int)(a.R - r0);
    const long long r = r0 + lr;
    const bool mine = lr < rows;
    // the row's facts: its line, its count, the intervals its window admits
    int li = -1, cnt = 0, first = 0, last = -1;
    if (mine) {
      li = line_of(a, r);
      cnt = row_count(a, r);
      if (li >= 0) {
        last = a.M - 2;
        if (a.s_window) {
          const double lo = a.s_window[2 * (size_t)r], hi = a.s_window[2 * (size_t)r + 1];
          if (lo <= hi) window_range(a.rs + (size_t)li * (size_t)a.M, a.M, lo, hi, first, last);
          else last = -1;
        }
      }
    }
    int row_out = 0;
    for (int sl = 0; sl < slices; sl++) {
      const int j = sl * kThreads + jl;
      const bool read = mine && j < cnt;
      double c[6];
      UNROLL for (int i = 0; i < 6; i++) c[i] = 0.0;
      if (read) read_cart(a.cart, (size_t)r, a.n, j, a.order, c);
      const double x = c[0], y = c[1];
      const bool valid = read && li >= 0 && x == x && y == y && first <= last;
      // the points this wavefront sweeps: the union of its lanes' ranges
      int kmin = valid ? first : kNone, kmax = valid ? last + 1 : -1;
      UNROLL for (int d = 32; d >= 1; d >>= 1) {
        const int omin = __shfl_xor(kmin, d), omax = __shfl_xor(kmax, d);
        kmin = omin < kmin ? omin : kmin;
        kmax = omax > kmax ? omax : kmax;
      }
      Best b;
      best_init(b);
      double gprev = 0.0, prx = 0.0, pry = 0.0;
      bool done = !valid;
      int seen = -1;
      for (int q = 0; q < rows; q++) {   // one pass per distinct line of the group, in row order
        const int lq = line_of(a, r0 + q);
        if (lq < 0 || lq == seen) continue;
        seen = lq;
        const bool sweep = !done && li == lq;
        if (!__syncthreads_or(sweep)) continue;
        for (int c0 = 0; c0 < a.M; c0 += kLdsM) {
          const int cm = a.M - c0 < kLdsM ? a.M - c0 : kLdsM;
          if (staged_line != lq || staged_c0 != c0) {
            __syncthreads();   // the sweeps of what is staged are over
            const size_t o = (size_t)lq * (size_t)a.M + (size_t)c0;
            for (int k = tid; k < cm; k += kThreads) {
              double sn, cs;
              sincos(a.rtheta[o + k], &sn, &cs);
              px_[k] = a.rx[o + k]; py_[k] = a.ry[o + k]; pc_[k] = cs; ps_[k] = sn;
            }
            staged_line = lq; staged_c0 = c0;
            __syncthreads();
          }
          if (sweep) {
            const int ka = kmin > c0 ? kmin : c0, kb = kmax < c0 + cm - 1 ? kmax : c0 + cm - 1;
            for (int k = ka; k <= kb; k++) {
              const double rxk = px_[k - c0], ryk = py_[k - c0];
              const double g = along(x, y, rxk, ryk, pc_[k - c0], ps_[k - c0]);
              const int i = k - 1;
              if (i >= first && i <= last && candidate(gprev, g, i == a.M - 2))
                best_take(b, i, chord_d2(x, y, prx, pry, rxk, ryk), gprev, g);
              gprev = g; prx = rxk; pry = ryk;
            }
          }
        }
        if (sweep) done = true;
      }
      if (read) {
        double out[6];
        if (b.i < 0) {
          UNROLL for (int q = 0; q < 6; q++) out[q] = nan;
        } else {
          const Line ln = line_at(a, li);
          double w, sn, cs;
          refine(ln, b.i, x, y, b.ga, b.gb, w);
          const RefPoint p = ref_at(ln, b.i, w);
          sin_cos(p.theta, sn, cs);
          map(p, sn, cs, c, a.order, out);
          out[0] = ln.rs[b.i] + w * (ln.rs[b.i + 1] - ln.rs[b.i]);
        }
        UNROLL for (int q = 0; q < 6; q++) a.frenet[frenet_offset(LAYOUT, (size_t)r, a.n, j, q)] = out[q];
        if (a.interval) a.interval[(size_t)r * a.n + j] = b.i;
      }
      if (a.n_outside) {
        const int flag = read && b.i < 0;
        if (one_row) {
          row_out += __syncthreads_count(flag);
        } else {
          flag_[tid] = flag;
          __syncthreads();
          if (mine && jl == 0)
            for (int k = 0; k < a.n; k++) row_out += flag_[tid + k];
          __syncthreads();
        }
      }
    }
    if (a.n_outside && mine && jl == 0) a.n_outside[r] = row_out;
  }
}

// MODE 0: cart_bar = K' frenet_bar (every sample of the row is written); MODE 1: frenet_dot[t] = K cart_dot[t] for the
// samples read
template <int LAYOUT, int MODE>
__global__ __launch_bounds__(kThreads) void frenet_grad_kernel(const FrenetArgs a) {
  const long long total = (long long)a.R * a.n;
  const size_t slab = (size_t)a.R * 6 * (size_t)a.n;
  for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (long long)gridDim.x * kThreads) {
    const long long r = idx / a.n;
    const int j = (int)(idx - r * a.n);
    const int cnt = row_count(a, r);
    if (MODE == 1 && j >= cnt) continue;
    double c[6], K[6][6];
    bool in = false;
    const int li = line_of(a, r);
    if (j < cnt && li >= 0) {
      read_cart(a.cart, (size_t)r, a.n, j, a.order, c);
      const double s = a.frenet_in[frenet_offset(LAYOUT, (size_t)r, a.n, j, 0)];
      const double l = a.frenet_in[frenet_offset(LAYOUT, (size_t)r, a.n, j, 3)];
      in = jacobian_at(line_at(a, li), a.interval_in[(size_t)r * a.n + j], c, s, l, a.order, K);
    }
    if (MODE == 0) {
      double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (in) {
        UNROLL for (int q = 0; q < 6; q++) {
          if (q % 3 > a.order) continue;   // a row above the order is 0: what frenet_bar holds there is not read
          const double fb = a.frenet_bar[frenet_offset(LAYOUT, (size_t)r, a.n, j, q)];
          UNROLL for (int i = 0; i < 6; i++) g[i] += fb * K[q][i];
        }
      }
      UNROLL for (int i = 0; i < 6; i++) a.cart_bar[((size_t)r * 6 + i) * a.n + j] = g[i];
    } else {
      for (int t = 0; t < a.T; t++) {
        double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (in) {
          double cd[6];
          read_cart(a.cart_dot + (size_t)t * slab, (size_t)r, a.n, j, a.order, cd);
          UNROLL for (int q = 0; q < 6; q++)
            UNROLL for (int i = 0; i < 6; i++) d[q] += K[q][i] * cd[i];
        }
        UNROLL for (int q = 0; q < 6; q++) a.frenet_dot[(size_t)t * slab + frenet_offset(LAYOUT, (size_t)r, a.n, j, q)] = d[q];
      }
    }
  }
}

int refuse(btrapz_ctx *c, const char *what) {
  btrapz_ctx_set_error(c, what);
  return BTRAPZ_EINVAL;
}
// the checks the three entry points share; nullptr: none failed
const char *bad_common(const btrapz_refline *t, int R, int n, int layout, int order, const double *cart) {
  if (!t) return "invalid argument: refline (null)";
  if (!t->rs || !t->rx || !t->ry || !t->rtheta || !t->rkappa || !t->rdkappa) return "invalid argument: refline (an array is null)";
  if (!cart) return "invalid argument: cart (null)";
  if (R < 1) return "invalid argument: R (< 1)";
  if (n < 1) return "invalid argument: n (< 1)";
  if (t->n_lines < 1) return "invalid argument: refline.n_lines (< 1)";
  if (t->M < 2) return "invalid argument: refline.M (< 2)";
  if (layout != BTRAPZ_FRENET_SAMPLES && layout != BTRAPZ_FRENET_STATES) return "invalid argument: layout (unknown)";
  if (order < 0 || order > 2) return "invalid argument: order (0, 1 or 2)";
  return nullptr;
}
FrenetArgs common_args(const btrapz_refline *t, const int *line_index, int R, int n, int order, const double *cart, const int *count) {
  FrenetArgs a = {};
  a.R = R; a.n = n; a.M = t->M; a.n_lines = t->n_lines; a.order = order;
  a.rs = t->rs; a.rx = t->rx; a.ry = t->ry; a.rtheta = t->rtheta; a.rkappa = t->rkappa; a.rdkappa = t->rdkappa;
  a.line_index = line_index; a.cart = cart; a.count = count;
  return a;
}
template <class K>
int launch(btrapz_ctx *c, K kernel, const FrenetArgs &a, long long work, void *stream, const char *what) {
  hipError_t e = hipSetDevice(btrapz_ctx_device(c));
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)(work < kMaxBlocks ? work : kMaxBlocks);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) return BTRAPZ_OK;
  btrapz_ctx_set_error(c, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return BTRAPZ_EHIP;
}
long long grad_blocks(int R, int n) { return ((long long)R * n + kThreads - 1) / kThreads; }

}  // namespace

}  // namespace btrapz

using namespace btrapz;

BTRAPZ_EXPORT int btrapz_frenet_device(btrapz_ctx *c, const btrapz_refline *t, const int *line_index, int R, int n, int layout,
                                       int order, const double *cart, const int *count, const double *s_window, double *frenet,
                                       int *interval, int *n_outside, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(t, R, n, layout, order, cart)) return refuse(c, why);
  if (!frenet) return refuse(c, "invalid argument: frenet (null)");
  FrenetArgs a = common_args(t, line_index, R, n, order, cart, count);
  a.s_window = s_window; a.frenet = frenet; a.interval = interval; a.n_outside = n_outside;
  const int rpb = n >= kThreads ? 1 : kThreads / n;
  const long long groups = ((long long)R + rpb - 1) / rpb;
  const char *what = "btrapz_frenet_device";
  return layout == BTRAPZ_FRENET_SAMPLES ? launch(c, frenet_kernel<0>, a, groups, stream, what)
                                         : launch(c, frenet_kernel<1>, a, groups, stream, what);
}

BTRAPZ_EXPORT int btrapz_frenet_vjp_device(btrapz_ctx *c, const btrapz_refline *t, const int *line_index, int R, int n,
                                           int layout, int order, const double *cart, const double *frenet, const int *interval,
                                           const int *count, const double *frenet_bar, double *cart_bar, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(t, R, n, layout, order, cart)) return refuse(c, why);
  if (!frenet) return refuse(c, "invalid argument: frenet (null)");
  if (!interval) return refuse(c, "invalid argument: interval (null)");
  if (!frenet_bar) return refuse(c, "invalid argument: frenet_bar (null)");
  if (!cart_bar) return refuse(c, "invalid argument: cart_bar (null)");
  FrenetArgs a = common_args(t, line_index, R, n, order, cart, count);
  a.frenet_in = frenet; a.interval_in = interval; a.frenet_bar = frenet_bar; a.cart_bar = cart_bar;
  const char *what = "btrapz_frenet_vjp_device";
  return layout == BTRAPZ_FRENET_SAMPLES ? launch(c, frenet_grad_kernel<0, 0>, a, grad_blocks(R, n), stream, what)
                                         : launch(c, frenet_grad_kernel<1, 0>, a, grad_blocks(R, n), stream, what);
}

BTRAPZ_EXPORT int btrapz_frenet_jvp_device(btrapz_ctx *c, const btrapz_refline *t, const int *line_index, int R, int n,
                                           int layout, int order, const double *cart, const double *frenet, const int *interval,
                                           const int *count, int T, const double *cart_dot, double *frenet_dot, void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (const char *why = bad_common(t, R, n, layout, order, cart)) return refuse(c, why);
  if (!frenet) return refuse(c, "invalid argument: frenet (null)");
  if (!interval) return refuse(c, "invalid argument: interval (null)");
  if (!cart_dot) return refuse(c, "invalid argument: cart_dot (null)");
  if (!frenet_dot) return refuse(c, "invalid argument: frenet_dot (null)");
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) return refuse(c, "invalid argument: T (1 .. BTRAPZ_MAX_TANGENTS = 32)");
  FrenetArgs a = common_args(t, line_index, R, n, order, cart, count);
  a.T = T; a.frenet_in = frenet; a.interval_in = interval; a.cart_dot = cart_dot; a.frenet_dot = frenet_dot;
  const char *what = "btrapz_frenet_jvp_device";
  return layout == BTRAPZ_FRENET_SAMPLES ? launch(c, frenet_grad_kernel<0, 1>, a, grad_blocks(R, n), stream, what)
                                         : launch(c, frenet_grad_kernel<1, 1>, a, grad_blocks(R, n), stream, what);
}
