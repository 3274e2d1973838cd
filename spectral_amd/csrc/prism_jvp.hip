// prism_jvp.hip -- the forward-mode derivative of the prism stage (btrapz_prism_bounds_jvp_device): tangents of the prisms
// [T][B][P][8] in, tangents of s_bounds / l_bounds [T][B][O][N][2] out.
//
// prism_bounds_jvp_kernel: one wavefront per scene, the forward's write pattern (prism_kernels.hip) T times over: it WRITES
// T * O * N * 32 bytes per scene, one 16-byte store per lane, tangent, knot and array, coalesced along the knots.  The
// scene's tables are made again in LDS with the statements of prism_vjp_core.h (lane per car, per candidate, per strip), the
// scene's prisms_dot ([T][P][6], at most 24 KB) is staged behind them.  Then strip by strip, the lanes strided over the
// knots, so that the strip's cover mask and edge owners are wave-uniform; the winners of the strip's max / min at a knot
// (prism_vjp_winners) are evaluated once, the inner loop over the tangents reads the winners' rows from LDS and stores.
// Every output entry is written exactly once (padding strips and overflowing scenes: zeros): no atomics, no sums -- the
// host twin (prism_jvp_host.cpp) evaluates the same statements and gives the same bits.
#include <hip/hip_runtime.h>

#include "../../include/btrapz_hip_stage_jvp.h"
#include "btrapz_device.h"
#include "prism_vjp_core.h"

namespace btrapz {

struct PrismJvpArgs {
  int B, P, N, O, T;
  btrapz_road road;
  const double *prisms;                   // [B][P][8]
  const double *prisms_dot;               // [T][B][P][8]
  double *s_dot, *l_dot;                  // [T][B][O][N][2]; either may be null (not wanted)
};

namespace {
constexpr size_t kTabBytes = (sizeof(PrismVjpTab) + 15) / 16 * 16;
constexpr size_t kOwnerBytes = (sizeof(int) * PVJP_MAX_CAND + 15) / 16 * 16;
}  // namespace

__global__ __launch_bounds__(64) void prism_bounds_jvp_kernel(const PrismJvpArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];   // the tables | owner[2 P + 2] | prisms_dot [T][P][6]
  PrismVjpTab &t = *reinterpret_cast<PrismVjpTab *>(lds);
  int *owner = reinterpret_cast<int *>(lds + kTabBytes);
  double *pd = reinterpret_cast<double *>(lds + kTabBytes + kOwnerBytes);
  const int lane = threadIdx.x, b = blockIdx.x;
  const int N = a.N, O = a.O, P = a.P, T = a.T, B = a.B, nc = 2 * P + 2;
  const double *p = a.prisms + (size_t)b * P * 8;
  if (lane < P) prism_vjp_car(t, a.road, p, P, lane);
  for (int e = lane; e < T * P * 6; e += PVJP_LANES) {
    const int d = e / (P * 6), r = e - d * (P * 6), q = r / 6, k = r - q * 6;
    pd[e] = a.prisms_dot[(((size_t)d * B + b) * P + q) * 8 + k];
  }
  __syncthreads();
  if (lane == 0) prism_vjp_road_edges(t, a.road, P);
  __syncthreads();
  if (lane < nc) prism_vjp_first(t, lane);
  __syncthreads();
  if (lane < nc) prism_vjp_rank(t, P, lane);
  __syncthreads();
  const int strips = prism_vjp_strip_count(t, P);
  if (lane < strips) prism_vjp_cover(t, P, lane);
  if (lane < nc) prism_jvp_edge_owner(t, owner, lane);
  __syncthreads();
  const bool overflow = strips > O;   // the forward's n_strips = -1: zeros everywhere
  double2 *sd = reinterpret_cast<double2 *>(a.s_dot), *ld = reinterpret_cast<double2 *>(a.l_dot);
  const size_t per_tangent = (size_t)B * O * N;
  for (int j = 0; j < O; j++) {
    const bool live = !overflow && j < strips;
    const int c0 = live ? owner[j] : -1, c1 = live ? owner[j + 1] : -1;
    const bool covered = live && sd && t.cover[j] != 0;
    for (int i = lane; i < N; i += PVJP_LANES) {
      int w_lo = -1, w_hi = -1;
      if (covered) prism_vjp_winners(t, a.road, j, i, w_lo, w_hi);
      size_t at = ((size_t)b * O + j) * N + i;
      for (int d = 0; d < T; d++, at += per_tangent) {
        const double *dd = pd + (size_t)d * P * 6;
        if (ld) ld[at] = make_double2(prism_jvp_edge_dot(t, P, c0, dd), prism_jvp_edge_dot(t, P, c1, dd));
        if (sd) sd[at] = make_double2(w_lo >= 0 ? prism_jvp_face_dot(t, a.road, w_lo, i, dd) : 0.0,
                                      w_hi >= 0 ? prism_jvp_face_dot(t, a.road, w_hi, i, dd) : 0.0);
      }
    }
  }
}

}  // namespace btrapz

using namespace btrapz;

BTRAPZ_EXPORT int btrapz_prism_bounds_jvp_device(btrapz_ctx *c, int B, int P, int N, const btrapz_road *road, const double *prisms,
                                              int O, int T, const double *prisms_dot, double *s_bounds_dot, double *l_bounds_dot,
                                              void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  const char *why = nullptr;
  if (B < 1 || P < 1 || N < 1 || O < 1) why = "invalid argument: B, P, N and O must be >= 1";
  else if (P > PVJP_MAX_CARS) why = "invalid argument: P > 16 cars per scene";
  else if (T < 1 || T > BTRAPZ_MAX_TANGENTS) why = "invalid argument: T must be in 1..BTRAPZ_MAX_TANGENTS";
  else if (!road || !prisms || !prisms_dot) why = "invalid argument: road, prisms and prisms_dot must be non-null";
  else if (!s_bounds_dot && !l_bounds_dot) why = "invalid argument: s_bounds_dot and l_bounds_dot are both null";
  else if (!(road->knots_per_second > 0)) why = "invalid argument: road.knots_per_second must be > 0";
  if (why) { btrapz_ctx_set_error(c, why); return BTRAPZ_EINVAL; }
  if (hipSetDevice(btrapz_ctx_device(c)) != hipSuccess) { btrapz_ctx_set_error(c, "hipSetDevice failed"); return BTRAPZ_EHIP; }
  PrismJvpArgs a;
  a.B = B; a.P = P; a.N = N; a.O = O; a.T = T; a.road = *road;
  a.prisms = prisms; a.prisms_dot = prisms_dot; a.s_dot = s_bounds_dot; a.l_dot = l_bounds_dot;
  hipLaunchKernelGGL(prism_bounds_jvp_kernel, dim3(B), dim3(64), kTabBytes + kOwnerBytes + sizeof(double) * 6 * P * T, (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) { btrapz_ctx_set_error(c, "prism_bounds_jvp_kernel: launch failed"); return BTRAPZ_EHIP; }
  return BTRAPZ_OK;
}
