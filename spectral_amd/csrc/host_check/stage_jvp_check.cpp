// stage_jvp_check.cpp -- btrapz_prism_bounds_jvp_host (prism_jvp_host.cpp, prism_vjp_core.h) and btrapz_corridor_jvp_host
// (corridor.cpp, corridor_vjp_core.h) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program (g++,
// no HIP, no GPU; `make host_asan_stage_jvp`).  The synthetic inputs of prism_vjp_check.cpp and corridor_vjp_check.cpp over
// the shapes' edges, with 1, 2 and 32 directions, every output wanted and subsets, outputs pre-filled with NaN (they must
// come back without one), and the refusals.  Prints one line per case and "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../../include/btrapz_hip_stage_jvp.h"

static unsigned long long rs = 12345;
static double urand() { rs = rs * 6364136223846793005ull + 1442695040888963407ull; return (double)(rs >> 11) / 9007199254740992.0; }

static const btrapz_road kRoad = {0.0, 50.0, -2.0, 8.0, 5.0 / 3 + 5.0 / 3, 2.0 / 3 + 2.0 / 3, 10.0};

static int count_nan(const std::vector<double> &v, double &sum) {
  int nan = 0;
  for (double x : v) { if (std::isnan(x)) ++nan; else sum += std::fabs(x); }
  return nan;
}

// kind 0: random cars; 1: sixteen-style distinct extents inside the road; 2: every car the same.  mask: 1 s, 2 l wanted.
static int prism_case(int B, int P, int N, int O, int T, int kind, int inactive_every, int mask, int expect_nonzero) {
  std::vector<double> pr((size_t)B * P * 8, 0.0), pd((size_t)(T > 0 ? T : 1) * B * P * 8);
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
  for (size_t e = 0; e < pd.size(); e++) pd[e] = e % 8 >= 6 ? NAN : urand() - 0.5;   // entries 6 and 7 are never read
  const size_t n_out = (size_t)(T > 0 ? T : 1) * B * O * N * 2;
  std::vector<double> s(mask & 1 ? n_out : 0, NAN), l(mask & 2 ? n_out : 0, NAN);
  const int rc = btrapz_prism_bounds_jvp_host(B, P, N, &kRoad, pr.data(), O, T, pd.data(), mask & 1 ? s.data() : nullptr,
                                              mask & 2 ? l.data() : nullptr);
  double sum = 0.0;
  const int nan = rc == BTRAPZ_OK ? count_nan(s, sum) + count_nan(l, sum) : 0;
  printf("prism B %d P %d N %d O %d T %d kind %d inactive %d mask %d -> rc %d sum %.6g nan %d\n", B, P, N, O, T, kind, inactive_every, mask, rc, sum, nan);
  if (rc != BTRAPZ_OK) return rc;
  if (nan) return -100;
  if (expect_nonzero >= 0 && (sum > 0.0) != (expect_nonzero != 0)) return -101;
  return 0;
}

// tmask: bit per tangent array (s, l, ds, dl, s_ref, l_ref); omask: 1 seg_dot, 2 ref_end_dot, 4 dl_bounds_dot
static int corridor_case(int variant, int N, int O, int kink, double l_ref_at, int seg_stride, int T, int tmask, int omask) {
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
  const size_t Tn = T > 0 ? T : 1;
  std::vector<double> t_s(Tn * sb.size()), t_l(Tn * lb.size()), t_ds(Tn * ds.size()), t_dl(Tn * dl.size()), t_sr(Tn * N), t_lr(Tn * N);
  for (std::vector<double> *v : {&t_s, &t_l, &t_ds, &t_dl, &t_sr, &t_lr}) for (double &x : *v) x = urand() - 0.5;
  const btrapz_knot_tangents tan = {tmask & 1 ? t_s.data() : nullptr, tmask & 2 ? t_l.data() : nullptr, tmask & 4 ? t_ds.data() : nullptr,
                                    tmask & 8 ? t_dl.data() : nullptr, tmask & 16 ? t_sr.data() : nullptr, tmask & 32 ? t_lr.data() : nullptr};
  std::vector<double> seg(omask & 1 ? Tn * BTRAPZ_NUM_SEG_FIELDS * seg_stride : 0, NAN), re(omask & 2 ? Tn * 2 : 0, NAN), d10(omask & 4 ? Tn * 10 : 0, NAN);
  int count = -2;
  const int rc = btrapz_corridor_jvp_host(variant, N, O, delta, sb.data(), lb.data(), ds.data(), dl.data(), sr.data(), lr.data(), seg_stride, T,
                                          &tan, omask & 1 ? seg.data() : nullptr, omask & 2 ? re.data() : nullptr, omask & 4 ? d10.data() : nullptr, &count);
  double sum = 0.0;
  const int nan = rc == BTRAPZ_OK ? count_nan(seg, sum) + count_nan(re, sum) + count_nan(d10, sum) : 0;
  printf("corridor variant %d N %d O %d kink %d stride %d T %d tangents %d outputs %d -> rc %d seg_count %d sum %.6g nan %d\n", variant, N, O, kink,
         seg_stride, T, tmask, omask, rc, count, sum, nan);
  if (rc != BTRAPZ_OK) return rc;
  if (nan) return -100;
  if (count < 1 && sum != 0.0) return -101;     // no corridor: zeros in every entry
  return 0;
}

int main() {
  int bad = 0;
  bad += prism_case(1, 1, 1, 3, 1, 0, 0, 3, -1) != 0;
  bad += prism_case(3, 2, 3, 5, 2, 0, 0, 3, 1) != 0;
  bad += prism_case(4, 4, 71, 9, 32, 0, 0, 3, 1) != 0;
  bad += prism_case(4, 4, 71, 9, 3, 0, 0, 1, -1) != 0;
  bad += prism_case(4, 4, 71, 9, 3, 0, 0, 2, 1) != 0;
  bad += prism_case(4, 4, 129, 9, 2, 0, 3, 3, 1) != 0;
  bad += prism_case(2, 16, 65, 33, 32, 1, 0, 3, 1) != 0;     // sixteen distinct cars inside the road: 33 strips
  bad += prism_case(2, 16, 64, 34, 2, 1, 0, 3, 1) != 0;      // one padding strip
  bad += prism_case(2, 16, 63, 32, 2, 1, 0, 3, 0) != 0;      // one strip too many for O: zeros
  bad += prism_case(2, 16, 200, 40, 1, 0, 0, 3, -1) != 0;
  bad += prism_case(2, 3, 71, 5, 2, 2, 0, 3, 1) != 0;        // identical cars
  bad += prism_case(2, 3, 71, 5, 2, 0, 1, 3, 0) != 0;        // every slot inactive: the road alone, zeros
  bad += prism_case(1, 17, 71, 40, 1, 0, 0, 3, -1) != BTRAPZ_EINVAL;
  bad += prism_case(1, 2, 71, 5, 1, 0, 0, 0, -1) != BTRAPZ_EINVAL;
  bad += prism_case(1, 2, 71, 5, 0, 0, 0, 3, -1) != BTRAPZ_EINVAL;
  bad += prism_case(1, 2, 71, 5, 33, 0, 0, 3, -1) != BTRAPZ_EINVAL;
  bad += btrapz_prism_bounds_jvp_host(1, 1, 1, &kRoad, nullptr, 1, 1, nullptr, nullptr, nullptr) != BTRAPZ_EINVAL;
  for (int variant = 0; variant < 2; variant++) {
    bad += corridor_case(variant, 3, 1, 0, 0.0, 16, 1, 63, 7) != 0;
    bad += corridor_case(variant, 4, 2, 0, 0.0, 16, 2, 63, 7) != 0;
    bad += corridor_case(variant, 71, 3, 0, 0.0, 16, 32, 63, 7) != 0;
    bad += corridor_case(variant, 71, 3, 17, 0.0, 16, 3, 21, 1) != 0;
    bad += corridor_case(variant, 71, 1, 0, 0.0, 16, 32, 63, 7) != 0;
    bad += corridor_case(variant, 71, 2, 30, 0.0, 32, 32, 63, 7) != 0;
    bad += corridor_case(variant, 201, 2, 40, 0.0, 64, 2, 42, 6) != 0;
    bad += corridor_case(variant, 512, 2, 0, 0.0, 64, 2, 63, 7) != 0;
    bad += corridor_case(variant, 512, 64, 0, 0.0, 64, 1, 63, 7) != 0;     // two segments per obstacle at most: overflow
    bad += corridor_case(variant, 101, 3, 2, 0.0, 16, 2, 63, 7) != 0;      // a kink every other knot: the lists overflow
    bad += corridor_case(variant, 71, 3, 0, 50.0, 16, 2, 63, 7) != 0;      // the reference outside every corridor
    bad += corridor_case(variant, 71, 3, 0, 0.0, 2, 2, 63, 7) != 0;        // more segments than the stride
  }
  bad += corridor_case(0, 513, 1, 0, 0.0, 16, 1, 63, 7) != BTRAPZ_EINVAL;
  bad += corridor_case(0, 71, 65, 0, 0.0, 16, 1, 63, 7) != BTRAPZ_EINVAL;
  bad += corridor_case(0, 71, 1, 0, 0.0, 65, 1, 63, 7) != BTRAPZ_EINVAL;
  bad += corridor_case(0, 71, 1, 0, 0.0, 16, 0, 63, 7) != BTRAPZ_EINVAL;
  bad += corridor_case(0, 71, 1, 0, 0.0, 16, 33, 63, 7) != BTRAPZ_EINVAL;
  bad += corridor_case(0, 71, 1, 0, 0.0, 16, 1, 0, 7) != BTRAPZ_EINVAL;
  bad += corridor_case(0, 71, 1, 0, 0.0, 16, 1, 63, 0) != BTRAPZ_EINVAL;
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
