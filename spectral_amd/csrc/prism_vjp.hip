// prism_vjp.hip -- the backward pass of the prism stage (btrapz_prism_bounds_vjp_device): cotangents of s_bounds / l_bounds
// [B][O][N][2] in, gradients w.r.t. the prisms [B][P][8] out.
//
// prism_bounds_vjp_kernel: one wavefront per scene, the mirror image of the write-bound forward (prism_kernels.hip): it
// READS O * N * 32 bytes per scene, one 16-byte load per lane, knot and array, coalesced along the knots.  The scene's
// tables are made again in LDS with the statements of prism_vjp_core.h (lane per car, per candidate, per strip).  Then strip
// by strip, the lanes strided over the knots, so that the strip's cover mask and edges are wave-uniform:
//   l_bar: two sums per strip (lower edge, upper edge) in registers, reduced with the butterfly at the end of the strip;
//          lane 0 adds them into the edges' cotangents;
//   s_bar: the winner of the strip's max / min at the knot (prism_vjp_winners) gets the term -- two running sums per car,
//          `bar` and `bar * (i / rate - t0)`, in lane-private LDS columns (the car varies from knot to knot: no dynamically
//          indexed registers), reduced with the butterfly at the end.
// Lane q then writes the 8 entries of car q (prism_vjp_car_out).  Fixed order, no atomics: a lane adds its terms over
// strips and knots ascending, the butterfly adds across the lanes with xor 32, 16, .. 1 -- btrapz_prism_bounds_vjp_host
// (prism_vjp_host.cpp) walks the same order and gives the same bits.
#include <hip/hip_runtime.h>

#include "btrapz_device.h"
#include "prism_vjp_core.h"

namespace btrapz {

struct PrismVjpArgs {
  int B, P, N, O;
  btrapz_road road;
  const double *prisms;                   // [B][P][8]
  const double *s_bar, *l_bar;            // [B][O][N][2]; either may be null (zero)
  double *prisms_bar;                     // [B][P][8]
};

namespace {
constexpr size_t kTabBytes = (sizeof(PrismVjpTab) + 15) / 16 * 16;
__device__ __forceinline__ double butterfly_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
}  // namespace

__global__ __launch_bounds__(64) void prism_bounds_vjp_kernel(const PrismVjpArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];   // the tables | sums [2 P][64]; no static LDS in front of it
  PrismVjpTab &t = *reinterpret_cast<PrismVjpTab *>(lds);
  double *sums = reinterpret_cast<double *>(lds + kTabBytes);
  const int lane = threadIdx.x, b = blockIdx.x;
  const int N = a.N, O = a.O, P = a.P, nc = 2 * P + 2;
  const double *p = a.prisms + (size_t)b * P * 8;
  if (lane < P) prism_vjp_car(t, a.road, p, P, lane);
  for (int k = 0; k < 2 * P; k++) sums[k * PVJP_LANES + lane] = 0.0;
  __syncthreads();
  if (lane == 0) prism_vjp_road_edges(t, a.road, P);
  __syncthreads();
  if (lane < nc) prism_vjp_first(t, lane);
  __syncthreads();
  if (lane < nc) prism_vjp_rank(t, P, lane);
  __syncthreads();
  const int strips = prism_vjp_strip_count(t, P);
  if (lane < strips) prism_vjp_cover(t, P, lane);
  if (lane <= strips) t.edge_bar[lane] = 0.0;
  __syncthreads();
  double *out = a.prisms_bar + ((size_t)b * P + lane) * 8;
  if (strips > O) {   // the forward's n_strips = -1
    if (lane < P) for (int k = 0; k < 8; k++) out[k] = 0.0;
    return;
  }
  const double2 *sb = a.s_bar ? reinterpret_cast<const double2 *>(a.s_bar) + (size_t)b * O * N : nullptr;
  const double2 *lb = a.l_bar ? reinterpret_cast<const double2 *>(a.l_bar) + (size_t)b * O * N : nullptr;
  double carry = 0.0;   // the upper-edge sum of the strip below
  for (int j = 0; j < strips; j++) {
    const bool covered = sb && t.cover[j] != 0;
    double e0 = 0.0, e1 = 0.0;
    for (int i = lane; i < N; i += PVJP_LANES) {
      const size_t at = (size_t)j * N + i;
      if (lb) { const double2 l = lb[at]; e0 += l.x; e1 += l.y; }
      if (covered) { const double2 s = sb[at]; prism_vjp_add(t, a.road, j, i, s.x, s.y, sums, lane); }
    }
    if (lb) {
      e0 = butterfly_sum(e0); e1 = butterfly_sum(e1);
      if (lane == 0) t.edge_bar[j] = carry + e0;
      carry = e1;
    }
  }
  if (lane == 0) t.edge_bar[strips] = carry;
  double face_bar = 0.0, face_at_bar = 0.0;
  for (int q = 0; q < P; q++) {
    if (!(t.flags[q] & 1)) continue;
    const double s0 = butterfly_sum(sums[(2 * q) * PVJP_LANES + lane]);
    const double s1 = butterfly_sum(sums[(2 * q + 1) * PVJP_LANES + lane]);
    if (lane == q) { face_bar = s0; face_at_bar = s1; }
  }
  __syncthreads();   // edge_bar is complete
  if (lane < P) prism_vjp_car_out(t, P, lane, face_bar, face_at_bar, out);
}

}  // namespace btrapz

using namespace btrapz;

BTRAPZ_EXPORT int btrapz_prism_bounds_vjp_device(btrapz_ctx *c, int B, int P, int N, const btrapz_road *road, const double *prisms,
                                              int O, const double *s_bounds_bar, const double *l_bounds_bar, double *prisms_bar,
                                              void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  const char *why = nullptr;
  if (B < 1 || P < 1 || N < 1 || O < 1) why = "invalid argument: B, P, N and O must be >= 1";
  else if (P > PVJP_MAX_CARS) why = "invalid argument: P > 16 cars per scene";
  else if (!road || !prisms || !prisms_bar) why = "invalid argument: road, prisms and prisms_bar must be non-null";
  else if (!s_bounds_bar && !l_bounds_bar) why = "invalid argument: s_bounds_bar and l_bounds_bar are both null";
  else if (!(road->knots_per_second > 0)) why = "invalid argument: road.knots_per_second must be > 0";
  if (why) { btrapz_ctx_set_error(c, why); return BTRAPZ_EINVAL; }
  if (hipSetDevice(btrapz_ctx_device(c)) != hipSuccess) { btrapz_ctx_set_error(c, "hipSetDevice failed"); return BTRAPZ_EHIP; }
  PrismVjpArgs a;
  a.B = B; a.P = P; a.N = N; a.O = O; a.road = *road;
  a.prisms = prisms; a.s_bar = s_bounds_bar; a.l_bar = l_bounds_bar; a.prisms_bar = prisms_bar;
  hipLaunchKernelGGL(prism_bounds_vjp_kernel, dim3(B), dim3(64), kTabBytes + sizeof(double) * 2 * P * PVJP_LANES, (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) { btrapz_ctx_set_error(c, "prism_bounds_vjp_kernel: launch failed"); return BTRAPZ_EHIP; }
  return BTRAPZ_OK;
}
