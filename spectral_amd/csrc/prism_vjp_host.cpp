// prism_vjp_host.cpp -- btrapz_prism_bounds_vjp_host: the backward pass of the prism stage on the host (no GPU, no
// context).  The statements are prism_vjp_core.h's, the order of every sum is prism_bounds_vjp_kernel's (prism_vjp.hip):
// 64 "lanes", lane L adding the knots L, L + 64, .. of strip after strip, then the butterfly across the lanes (xor 32, 16,
// .. 1).  Same inputs, same bits as the device call.
#include "prism_vjp_core.h"

#include <vector>

namespace {

using namespace btrapz;

double butterfly_sum(const double *column) {
  double v[PVJP_LANES], w[PVJP_LANES];
  for (int l = 0; l < PVJP_LANES; l++) v[l] = column[l];
  for (int d = 32; d >= 1; d >>= 1) {
    for (int l = 0; l < PVJP_LANES; l++) w[l] = v[l] + v[l ^ d];
    for (int l = 0; l < PVJP_LANES; l++) v[l] = w[l];
  }
  return v[0];
}

void scene_vjp(int P, int N, int O, const btrapz_road &road, const double *p, const double *s_bar, const double *l_bar,
               double *out, PrismVjpTab &t, double *sums) {
  const int nc = 2 * P + 2;
  for (int q = 0; q < P; q++) prism_vjp_car(t, road, p, P, q);
  prism_vjp_road_edges(t, road, P);
  for (int c = 0; c < nc; c++) prism_vjp_first(t, c);
  for (int c = 0; c < nc; c++) prism_vjp_rank(t, P, c);
  const int strips = t.strips = prism_vjp_strip_count(t, P);
  for (int j = 0; j < strips; j++) prism_vjp_cover(t, P, j);
  for (int j = 0; j <= strips; j++) t.edge_bar[j] = 0.0;
  for (int k = 0; k < 8 * P; k++) out[k] = 0.0;
  if (strips > O) return;
  for (int k = 0; k < 2 * P * PVJP_LANES; k++) sums[k] = 0.0;
  double carry = 0.0;
  for (int j = 0; j < strips; j++) {
    const bool covered = s_bar && t.cover[j] != 0;
    double e0[PVJP_LANES], e1[PVJP_LANES];
    for (int lane = 0; lane < PVJP_LANES; lane++) {
      e0[lane] = 0.0; e1[lane] = 0.0;
      for (int i = lane; i < N; i += PVJP_LANES) {
        const size_t at = ((size_t)j * N + i) * 2;
        if (l_bar) { e0[lane] += l_bar[at]; e1[lane] += l_bar[at + 1]; }
        if (covered) prism_vjp_add(t, road, j, i, s_bar[at], s_bar[at + 1], sums, lane);
      }
    }
    if (l_bar) {
      t.edge_bar[j] = carry + butterfly_sum(e0);
      carry = butterfly_sum(e1);
    }
  }
  t.edge_bar[strips] = carry;
  for (int q = 0; q < P; q++) {
    double face_bar = 0.0, face_at_bar = 0.0;
    if (t.flags[q] & 1) {
      face_bar = butterfly_sum(sums + (size_t)(2 * q) * PVJP_LANES);
      face_at_bar = butterfly_sum(sums + (size_t)(2 * q + 1) * PVJP_LANES);
    }
    prism_vjp_car_out(t, P, q, face_bar, face_at_bar, out + (size_t)q * 8);
  }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int btrapz_prism_bounds_vjp_host(
    int B, int P, int N, const btrapz_road *road, const double *prisms, int O, const double *s_bounds_bar,
    const double *l_bounds_bar, double *prisms_bar) {
  if (B < 1 || P < 1 || P > PVJP_MAX_CARS || N < 1 || O < 1 || !road || !prisms || !prisms_bar ||
      (!s_bounds_bar && !l_bounds_bar) || !(road->knots_per_second > 0))
    return BTRAPZ_EINVAL;
  PrismVjpTab t;
  std::vector<double> sums((size_t)2 * P * PVJP_LANES);
  const size_t per_scene = (size_t)O * N * 2;
  for (int b = 0; b < B; b++)
    scene_vjp(P, N, O, *road, prisms + (size_t)b * P * 8, s_bounds_bar ? s_bounds_bar + b * per_scene : nullptr,
              l_bounds_bar ? l_bounds_bar + b * per_scene : nullptr, prisms_bar + (size_t)b * P * 8, t, sums.data());
  return BTRAPZ_OK;
}
