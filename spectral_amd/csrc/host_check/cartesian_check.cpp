// cartesian_check.cpp -- btrapz_cartesian_host, _vjp_host and _jvp_host (cartesian_host.cpp, cartesian_core.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program (g++, no HIP, no GPU; `make host_asan_cartesian`).
// Every buffer has exactly the size the header states, so a read or write past a row, a table or a tangent is caught.
// Shapes over the edges -- 1 row, 1 sample, tables of 2 and 3 points, both layouts, counts 0, 1, n and beyond n, two lines
// with a line_index that is out of range for one row, samples on table points, at both ends, one ulp outside them and
// NaN, a table that is not increasing (meaningless values, but no access outside it) -- and the refusals.  It also checks
// the adjoint identity <cart_bar, J f_dot> = <J' cart_bar, f_dot> of every case.  Prints one line per case and "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../../include/btrapz_hip_cartesian.h"

static unsigned long long seed = 2468;
static double urand() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; }

struct Table {
  std::vector<double> rs, rx, ry, rth, rk, rdk;
  btrapz_refline view(int n_lines, int M) const { return btrapz_refline{n_lines, M, rs.data(), rx.data(), ry.data(), rth.data(), rk.data(), rdk.data()}; }
};
// arcs of radius 20 + 15 line (a clothoid's curvature slope on odd lines), sampled every h metres; shuffled: not increasing
static Table make_table(int n_lines, int M, double h, bool shuffled) {
  Table t;
  for (int li = 0; li < n_lines; li++)
    for (int i = 0; i < M; i++) {
      const double s = h * i, k0 = 1.0 / (20.0 + 15.0 * li), dk = li % 2 ? 1e-3 : 0.0;
      const double th = k0 * s + 0.5 * dk * s * s + 3.0 * li;   // (beyond pi on the second line: the wrap is taken)
      t.rs.push_back(shuffled && i % 3 == 1 ? h * (M - i) : s);
      t.rx.push_back(std::sin(k0 * s) / k0); t.ry.push_back((1.0 - std::cos(k0 * s)) / k0);
      t.rth.push_back(th); t.rk.push_back(k0 + dk * s); t.rdk.push_back(dk);
    }
  return t;
}

static int run_case(int R, int n, int M, int n_lines, int layout, int count_kind, bool with_index, bool shuffled, int T) {
  const double h = 0.5, s_end = h * (M - 1);
  const Table tab = make_table(n_lines, M, h, shuffled);
  const btrapz_refline t = tab.view(n_lines, M);
  const size_t sz = (size_t)R * 6 * n;
  std::vector<double> f(sz), cart(sz, -7.0), cbar(sz), fbar(sz, -7.0), fdot((size_t)T * sz), cdot((size_t)T * sz, -7.0);
  std::vector<int> count(R), index(R);
  for (int r = 0; r < R; r++) {
    count[r] = count_kind == 0 ? 0 : count_kind == 1 ? 1 : count_kind == 2 ? n : count_kind == 3 ? n + 5 : (r * 7) % (n + 2) - 1;
    index[r] = r % (n_lines + 1) == n_lines && r > 0 ? n_lines : r % n_lines;   // some rows: out of range
    for (int j = 0; j < n; j++) {
      double u[6] = {s_end * urand(), 0.5 + 10.0 * urand(), 4.0 * urand() - 2.0, 6.0 * urand() - 3.0, 2.0 * urand() - 1.0, 2.0 * urand() - 1.0};
      switch ((r + j) % 11) {
        case 1: u[0] = h * (j % M); break;                       // on a table point
        case 2: u[0] = 0.0; break;
        case 3: u[0] = s_end; break;
        case 4: u[0] = std::nextafter(0.0, -1.0); break;         // one ulp outside either end
        case 5: u[0] = std::nextafter(s_end, 1e9); break;
        case 6: u[0] = NAN; break;
        case 7: u[1] = 0.0; u[4] = 0.0; break;                   // v == 0
        default: break;
      }
      for (int q = 0; q < 6; q++) {
        const size_t o = layout == 0 ? ((size_t)r * 6 + q) * n + j : (((size_t)r * 2 + q / 3) * n + j) * 3 + q % 3;
        f[o] = u[q];
      }
    }
  }
  for (double &v : cbar) v = urand() - 0.5;
  for (double &v : fdot) v = urand() - 0.5;
  std::vector<double> e6[6];
  for (auto &v : e6) v.assign(R, -7.0);
  std::vector<int> nout(R, -7), worst((size_t)R * 6, -7);
  btrapz_kin_audit au = {e6[0].data(), e6[1].data(), e6[2].data(), e6[3].data(), e6[4].data(), e6[5].data(), nout.data(), worst.data()};
  const int *cnt = count_kind == 2 ? nullptr : count.data(), *idx = with_index ? index.data() : nullptr;
  int rc = btrapz_cartesian_host(&t, idx, R, n, layout, f.data(), cnt, cart.data(), &au);
  if (rc == BTRAPZ_OK) rc = btrapz_cartesian_host(&t, idx, R, n, layout, f.data(), cnt, nullptr, &au);
  if (rc == BTRAPZ_OK) rc = btrapz_cartesian_vjp_host(&t, idx, R, n, layout, f.data(), cnt, cbar.data(), fbar.data());
  if (rc == BTRAPZ_OK) rc = btrapz_cartesian_jvp_host(&t, idx, R, n, layout, f.data(), cnt, T, fdot.data(), cdot.data());
  // the adjoint identity over the samples that were read, per tangent; the counts of what was written
  double worst_gap = 0.0;
  long outside = 0, kept = 0;
  if (rc == BTRAPZ_OK) {
    for (int r = 0; r < R; r++) {
      const int c = cnt ? (cnt[r] < n ? (cnt[r] > 0 ? cnt[r] : 0) : n) : n;
      outside += nout[r];
      for (int j = c; j < n; j++) kept += cart[(size_t)r * 6 * n + j] == -7.0;
    }
    for (int k = 0; k < T; k++) {
      double lhs = 0.0, rhs = 0.0, scale = 0.0;
      for (int r = 0; r < R; r++) {
        const int c = cnt ? (cnt[r] < n ? (cnt[r] > 0 ? cnt[r] : 0) : n) : n;
        for (int i = 0; i < 6; i++)
          for (int j = 0; j < c; j++) {
            const size_t o = ((size_t)r * 6 + i) * n + j;
            lhs += cbar[o] * cdot[(size_t)k * sz + o];
            scale += std::fabs(cbar[o] * cdot[(size_t)k * sz + o]);
          }
      }
      for (size_t o = 0; o < sz; o++) rhs += fbar[o] * fdot[(size_t)k * sz + o];
      if (!shuffled && scale > 0.0) worst_gap = std::fmax(worst_gap, std::fabs(lhs - rhs) / scale);
    }
  }
  printf("R %d n %d M %d lines %d layout %d count %d index %d shuffled %d T %d -> rc %d outside %ld kept %ld adjoint gap %.3g\n", R, n, M,
         n_lines, layout, count_kind, (int)with_index, (int)shuffled, T, rc, outside, kept, worst_gap);
  if (rc != BTRAPZ_OK) return rc;
  return worst_gap < 1e-12 ? 0 : -100;
}

int main() {
  int bad = 0;
  for (int layout = 0; layout < 2; layout++) {
    bad += run_case(1, 1, 2, 1, layout, 2, false, false, 1) != 0;
    bad += run_case(3, 63, 3, 1, layout, 2, false, false, 2) != 0;
    bad += run_case(5, 64, 65, 2, layout, 4, true, false, 3) != 0;
    bad += run_case(4, 65, 1000, 2, layout, 3, true, false, 12) != 0;
    bad += run_case(7, 130, 65, 3, layout, 4, true, false, 1) != 0;
    bad += run_case(2, 9, 3, 1, layout, 0, false, false, 1) != 0;
    bad += run_case(2, 9, 3, 1, layout, 1, false, false, 1) != 0;
    bad += run_case(3, 40, 17, 2, layout, 2, true, true, 2) != 0;       // a table that is not increasing
  }
  // the refusals
  const Table tab = make_table(1, 2, 1.0, false);
  btrapz_refline t = tab.view(1, 2);
  double f[6] = {0.5, 1, 0, 0, 0, 0}, out[6], d[6];
  double v = 0;
  btrapz_kin_audit none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  btrapz_kin_audit one = none;
  one.v_max = &v;
  int refused = 0, calls = 0;
  auto expect = [&](int rc) { ++calls; refused += rc == BTRAPZ_EINVAL; printf("refusal %d -> rc %d\n", calls, rc); };
  expect(btrapz_cartesian_host(nullptr, nullptr, 1, 1, 0, f, nullptr, out, nullptr));
  expect(btrapz_cartesian_host(&t, nullptr, 0, 1, 0, f, nullptr, out, nullptr));
  expect(btrapz_cartesian_host(&t, nullptr, 1, 0, 0, f, nullptr, out, nullptr));
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 2, f, nullptr, out, nullptr));
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 0, nullptr, nullptr, out, nullptr));
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 0, f, nullptr, nullptr, nullptr));
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 0, f, nullptr, out, &none));
  expect(btrapz_cartesian_vjp_host(&t, nullptr, 1, 1, 0, f, nullptr, nullptr, d));
  expect(btrapz_cartesian_vjp_host(&t, nullptr, 1, 1, 0, f, nullptr, out, nullptr));
  expect(btrapz_cartesian_jvp_host(&t, nullptr, 1, 1, 0, f, nullptr, 0, f, d));
  expect(btrapz_cartesian_jvp_host(&t, nullptr, 1, 1, 0, f, nullptr, BTRAPZ_MAX_TANGENTS + 1, f, d));
  expect(btrapz_cartesian_jvp_host(&t, nullptr, 1, 1, 0, f, nullptr, 1, nullptr, d));
  t.M = 1;
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 0, f, nullptr, out, nullptr));
  t.M = 2; t.n_lines = 0;
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 0, f, nullptr, out, nullptr));
  t.n_lines = 1; t.rkappa = nullptr;
  expect(btrapz_cartesian_host(&t, nullptr, 1, 1, 0, f, nullptr, out, nullptr));
  t.rkappa = tab.rk.data();
  bad += refused != calls;
  bad += btrapz_cartesian_host(&t, nullptr, 1, 1, 0, f, nullptr, nullptr, &one) != BTRAPZ_OK || !(v == 1.0);
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
