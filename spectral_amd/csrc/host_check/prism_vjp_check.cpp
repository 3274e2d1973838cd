// prism_vjp_check.cpp -- btrapz_prism_bounds_vjp_host (prism_vjp_host.cpp, prism_vjp_core.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone host program (g++, no HIP, no GPU; `make host_asan_prism_vjp`).  Synthetic
// scenes over the shapes' edges -- 1 knot, 1 car, 16 distinct cars (33 strips, O = 33 and 34), O one short of the strips
// (zeros), inactive slots, coinciding extents, either cotangent missing -- and the refusals.  Prints one line per case and "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../../include/btrapz_hip.h"

static unsigned long long rs = 12345;
static double urand() { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (double)(rs >> 11) / 9007199254740992.0; }

static const btrapz_road kRoad = {0.0, 50.0, -2.0, 8.0, 5.0 / 3 + 5.0 / 3, 2.0 / 3 + 2.0 / 3, 10.0};

// kind 0: random cars; 1: sixteen-style distinct extents inside the road; 2: every car the same
static int run_case(int B, int P, int N, int O, int kind, int inactive_every, int mask, int expect_nonzero) {
  std::vector<double> pr((size_t)B * P * 8, 0.0), sbar((size_t)B * O * N * 2), lbar(sbar.size()), out((size_t)B * P * 8, NAN);
  for (int b = 0; b < B; b++)
    for (int q = 0; q < P; q++) {
      double *c = &pr[((size_t)b * P + q) * 8];
      c[0] = 5.0 + 35.0 * urand();
      c[1] = kind == 1 ? -0.6 + 0.45 * q + 0.01 * urand() : kind == 2 ? 3.0 : -3.0 + 12.0 * urand();
      c[2] = (q + b) % 2 ? 0.0 : 0.1 + 2.9 * urand();
      c[3] = 8.0 * urand();
      c[4] = kind == 1 ? 0.0 : (q % 3 == 0 ? 0.25 : q % 3 == 1 ? -0.25 : 0.0);
      c[5] = q % 2 ? 3.0 : 4.0;
      c[6] = (inactive_every > 0 && (q + b) % inactive_every == 0) ? 0.0 : 1.0;
    }
  for (double &v : sbar) v = urand() - 0.5;
  for (double &v : lbar) v = urand() - 0.5;
  const int rc = btrapz_prism_bounds_vjp_host(B, P, N, &kRoad, pr.data(), O, mask & 1 ? sbar.data() : nullptr,
                                              mask & 2 ? lbar.data() : nullptr, out.data());
  double sum = 0.0;
  int nan = 0;
  for (double v : out) { if (std::isnan(v)) ++nan; else sum += std::fabs(v); }
  printf("B %d P %d N %d O %d kind %d inactive %d mask %d -> rc %d sum %.6g nan %d\n", B, P, N, O, kind, inactive_every, mask, rc, sum, nan);
  if (rc != BTRAPZ_OK) return rc;
  if (nan) return -100;
  if (expect_nonzero >= 0 && (sum > 0.0) != (expect_nonzero != 0)) return -101;
  return 0;
}

int main() {
  int bad = 0;
  bad += run_case(1, 1, 1, 3, 0, 0, 3, -1) != 0;
  bad += run_case(3, 2, 3, 5, 0, 0, 3, 1) != 0;
  bad += run_case(4, 4, 71, 9, 0, 0, 3, 1) != 0;
  bad += run_case(4, 4, 71, 9, 0, 0, 1, -1) != 0;
  bad += run_case(4, 4, 71, 9, 0, 0, 2, 1) != 0;
  bad += run_case(4, 4, 129, 9, 0, 3, 3, 1) != 0;
  bad += run_case(2, 16, 65, 33, 1, 0, 3, 1) != 0;     // sixteen distinct cars inside the road: 33 strips
  bad += run_case(2, 16, 64, 34, 1, 0, 3, 1) != 0;     // one padding strip
  bad += run_case(2, 16, 63, 32, 1, 0, 3, 0) != 0;     // one strip too many for O: zeros
  bad += run_case(2, 16, 200, 40, 0, 0, 3, -1) != 0;
  bad += run_case(2, 3, 71, 5, 2, 0, 3, 1) != 0;       // identical cars
  bad += run_case(2, 3, 71, 5, 0, 1, 3, 0) != 0;       // every slot inactive: the road alone, zeros
  bad += run_case(1, 17, 71, 40, 0, 0, 3, -1) != BTRAPZ_EINVAL;
  bad += run_case(1, 2, 71, 5, 0, 0, 0, -1) != BTRAPZ_EINVAL;
  bad += btrapz_prism_bounds_vjp_host(0, 1, 1, &kRoad, nullptr, 1, nullptr, nullptr, nullptr) != BTRAPZ_EINVAL;
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
