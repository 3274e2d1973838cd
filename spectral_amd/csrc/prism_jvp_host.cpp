// prism_jvp_host.cpp -- btrapz_prism_bounds_jvp_host: the forward-mode derivative of the prism stage on the host (no GPU,
// no context).  The statements are prism_vjp_core.h's, walked as prism_bounds_jvp_kernel walks them (prism_jvp.hip); every
// output entry is one expression of them, so the order of the walk does not matter: same inputs, the device call's bits.
#include "../../include/btrapz_hip_stage_jvp.h"
#include "prism_vjp_core.h"

#include <vector>

namespace {

using namespace btrapz;

void scene_jvp(int B, int b, int P, int N, int O, int T, const btrapz_road &road, const double *p, const double *prisms_dot,
               double *s_dot, double *l_dot, PrismVjpTab &t, double *pd) {
  const int nc = 2 * P + 2;
  int owner[PVJP_MAX_CAND];
  for (int q = 0; q < P; q++) prism_vjp_car(t, road, p, P, q);
  for (int d = 0; d < T; d++)
    for (int q = 0; q < P; q++)
      for (int k = 0; k < 6; k++) pd[((size_t)d * P + q) * 6 + k] = prisms_dot[(((size_t)d * B + b) * P + q) * 8 + k];
  prism_vjp_road_edges(t, road, P);
  for (int c = 0; c < nc; c++) prism_vjp_first(t, c);
  for (int c = 0; c < nc; c++) prism_vjp_rank(t, P, c);
  const int strips = t.strips = prism_vjp_strip_count(t, P);
  for (int j = 0; j < strips; j++) prism_vjp_cover(t, P, j);
  for (int c = 0; c < nc; c++) prism_jvp_edge_owner(t, owner, c);
  const bool overflow = strips > O;
  const size_t per_tangent = (size_t)B * O * N;
  for (int j = 0; j < O; j++) {
    const bool live = !overflow && j < strips;
    const int c0 = live ? owner[j] : -1, c1 = live ? owner[j + 1] : -1;
    const bool covered = live && s_dot && t.cover[j] != 0;
    for (int i = 0; i < N; i++) {
      int w_lo = -1, w_hi = -1;
      if (covered) prism_vjp_winners(t, road, j, i, w_lo, w_hi);
      size_t at = ((size_t)b * O + j) * N + i;
      for (int d = 0; d < T; d++, at += per_tangent) {
        const double *dd = pd + (size_t)d * P * 6;
        if (l_dot) { l_dot[2 * at] = prism_jvp_edge_dot(t, P, c0, dd); l_dot[2 * at + 1] = prism_jvp_edge_dot(t, P, c1, dd); }
        if (s_dot) {
          s_dot[2 * at] = w_lo >= 0 ? prism_jvp_face_dot(t, road, w_lo, i, dd) : 0.0;
          s_dot[2 * at + 1] = w_hi >= 0 ? prism_jvp_face_dot(t, road, w_hi, i, dd) : 0.0;
        }
      }
    }
  }
}

}  // namespace

extern "C" __attribute__((visibility("default"))) int btrapz_prism_bounds_jvp_host(
    int B, int P, int N, const btrapz_road *road, const double *prisms, int O, int T, const double *prisms_dot,
    double *s_bounds_dot, double *l_bounds_dot) {
  if (B < 1 || P < 1 || P > PVJP_MAX_CARS || N < 1 || O < 1 || T < 1 || T > BTRAPZ_MAX_TANGENTS || !road || !prisms || !prisms_dot ||
      (!s_bounds_dot && !l_bounds_dot) || !(road->knots_per_second > 0))
    return BTRAPZ_EINVAL;
  PrismVjpTab t;
  std::vector<double> pd((size_t)T * P * 6);
  for (int b = 0; b < B; b++)
    scene_jvp(B, b, P, N, O, T, *road, prisms + (size_t)b * P * 8, prisms_dot, s_bounds_dot, l_bounds_dot, t, pd.data());
  return BTRAPZ_OK;
}
