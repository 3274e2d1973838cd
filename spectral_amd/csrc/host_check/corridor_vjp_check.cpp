// corridor_vjp_check.cpp -- btrapz_corridor_vjp_host (corridor.cpp, corridor_vjp_core.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone host program (g++, no HIP, no GPU; `make host_asan_vjp`).  Synthetic candidates
// over the shapes' edges -- 3 knots, 512 knots, 64 obstacles, bounds that kink every few knots (lists that overflow: -1),
// a reference outside every corridor (0) -- every output wanted, then subsets.  Prints one line per case and "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../../include/btrapz_hip.h"

static unsigned long long rs = 12345;
static double urand() { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (double)(rs >> 11) / 9007199254740992.0; }

static int run_case(int variant, int N, int O, int kink, double l_ref_at, int seg_stride, int mask) {
  const double delta = 0.1;
  std::vector<double> sb((size_t)O * N * 2), lb((size_t)O * N * 2), ds((size_t)N * 2), dl((size_t)N * 2), sr(N), lr(N);
  for (int o = 0; o < O; o++) {
    double lo = 0.0, slope = 0.5;
    for (int i = 0; i < N; i++) {
      if (kink > 0 && i % kink == 0) slope = 0.2 + 1.5 * urand();
      lo += slope * delta;
      sb[((size_t)o * N + i) * 2] = lo; sb[((size_t)o * N + i) * 2 + 1] = lo + 20.0 + o;
      lb[((size_t)o * N + i) * 2] = -2.0 + 0.01 * i; lb[((size_t)o * N + i) * 2 + 1] = 4.0 + o;
    }
  }
  for (int i = 0; i < N; i++) { ds[2 * i] = urand(); ds[2 * i + 1] = 20.0 + urand(); dl[2 * i] = -3.0; dl[2 * i + 1] = 3.0; sr[i] = 5.0 + 0.08 * i; lr[i] = l_ref_at; }
  std::vector<double> seg_bar((size_t)BTRAPZ_NUM_SEG_FIELDS * seg_stride), re_bar(2, 1.0), dl_bar(10, 1.0);
  for (double &v : seg_bar) v = urand() - 0.5;
  std::vector<double> g_s(sb.size()), g_l(lb.size()), g_ds(ds.size()), g_dl(dl.size()), g_sr(N), g_lr(N);
  btrapz_knot_grads out = {mask & 1 ? g_s.data() : nullptr, mask & 2 ? g_l.data() : nullptr, mask & 4 ? g_ds.data() : nullptr,
                           mask & 8 ? g_dl.data() : nullptr, mask & 16 ? g_sr.data() : nullptr, mask & 32 ? g_lr.data() : nullptr};
  int count = -2;
  const int rc = btrapz_corridor_vjp_host(variant, N, O, delta, sb.data(), lb.data(), ds.data(), dl.data(), sr.data(), lr.data(), seg_stride,
                                          seg_bar.data(), re_bar.data(), dl_bar.data(), &out, &count);
  double sum = 0.0;
  for (double v : g_s) sum += std::fabs(v);
  printf("variant %d N %d O %d kink %d stride %d mask %d -> rc %d seg_count %d |g_s| %.6g\n", variant, N, O, kink, seg_stride, mask, rc, count, sum);
  return rc;
}

int main() {
  int bad = 0;
  for (int variant = 0; variant < 2; variant++) {
    bad += run_case(variant, 3, 1, 0, 0.0, 16, 63) != 0;
    bad += run_case(variant, 4, 2, 0, 0.0, 16, 63) != 0;
    bad += run_case(variant, 71, 3, 0, 0.0, 16, 63) != 0;
    bad += run_case(variant, 71, 3, 17, 0.0, 16, 21) != 0;
    bad += run_case(variant, 201, 2, 40, 0.0, 64, 42) != 0;
    bad += run_case(variant, 512, 2, 0, 0.0, 64, 63) != 0;
    bad += run_case(variant, 512, 64, 0, 0.0, 64, 63) != 0;     // two segments per obstacle at most: overflow
    bad += run_case(variant, 101, 3, 2, 0.0, 16, 63) != 0;      // a kink every other knot: the lists overflow
    bad += run_case(variant, 71, 3, 0, 50.0, 16, 63) != 0;      // the reference outside every corridor
    bad += run_case(variant, 71, 3, 0, 0.0, 2, 63) != 0;        // more segments than the stride
  }
  bad += run_case(0, 513, 1, 0, 0.0, 16, 63) != BTRAPZ_EINVAL;
  bad += run_case(0, 71, 65, 0, 0.0, 16, 63) != BTRAPZ_EINVAL;
  bad += run_case(0, 71, 1, 0, 0.0, 16, 0) != BTRAPZ_EINVAL;
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
