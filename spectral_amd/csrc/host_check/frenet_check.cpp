// frenet_check.cpp -- btrapz_frenet_host, _vjp_host and _jvp_host (frenet_host.cpp, frenet_core.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program (g++, no HIP, no GPU; `make host_asan_frenet`).
// Every buffer has exactly the size the header states, so a read or write past a row, a table, a window or a tangent is
// caught.  Shapes over the edges -- 1 row, 1 query, tables of 2 and 3 points, both layouts, the three orders, counts 0, 1,
// n and beyond n, lines with a line_index that is out of range for some rows, windows (whole, narrow, NaN, lo > hi),
// queries on table normals, before and beyond the line and NaN, an interval array of wild values handed to the
// derivatives, a table that is not increasing (meaningless values, but no access outside it) -- and the refusals.  It
// also checks the adjoint identity <frenet_bar, K cart_dot> = <K' frenet_bar, cart_dot> of every case.  Prints one line
// per case and "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../../include/btrapz_hip_frenet.h"

static unsigned long long seed = 13579;
static double urand() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; }

struct Table {
  std::vector<double> rs, rx, ry, rth, rk, rdk;
  btrapz_refline view(int n_lines, int M) const { return btrapz_refline{n_lines, M, rs.data(), rx.data(), ry.data(), rth.data(), rk.data(), rdk.data()}; }
};
// arcs of radius 30 + 15 line, sampled every h metres; shuffled: rs is not increasing
static Table make_table(int n_lines, int M, double h, bool shuffled) {
  Table t;
  for (int li = 0; li < n_lines; li++)
    for (int i = 0; i < M; i++) {
      const double s = h * i, k0 = 1.0 / (30.0 + 15.0 * li);
      t.rs.push_back(shuffled && i % 3 == 1 ? h * (M - i) : s);
      t.rx.push_back(std::sin(k0 * s) / k0); t.ry.push_back((1.0 - std::cos(k0 * s)) / k0);
      t.rth.push_back(k0 * s + 3.0 * li); t.rk.push_back(k0); t.rdk.push_back(li % 2 ? 1e-3 : 0.0);
    }
  // the lines after the first are the first one turned by 3 li radians about the origin
  for (int li = 1; li < n_lines; li++)
    for (int i = 0; i < M; i++) {
      const double c = std::cos(3.0 * li), s = std::sin(3.0 * li), x = t.rx[(size_t)li * M + i], y = t.ry[(size_t)li * M + i];
      t.rx[(size_t)li * M + i] = c * x - s * y; t.ry[(size_t)li * M + i] = s * x + c * y;
    }
  return t;
}

static int run_case(int R, int n, int M, int n_lines, int layout, int order, int count_kind, bool with_index, int window_kind,
                    bool shuffled, int T) {
  const double h = 40.0 / (M - 1);
  const Table tab = make_table(n_lines, M, h, shuffled);
  const btrapz_refline t = tab.view(n_lines, M);
  const size_t sz = (size_t)R * 6 * n;
  std::vector<double> cart(sz), fr(sz, -7.0), fbar(sz), cbar(sz, -7.0), cdot((size_t)T * sz), fdot((size_t)T * sz, -7.0), win((size_t)R * 2);
  std::vector<int> count(R), index(R), iv((size_t)R * n, -7), nout(R, -7);
  for (int r = 0; r < R; r++) {
    count[r] = count_kind == 0 ? 0 : count_kind == 1 ? 1 : count_kind == 2 ? n : count_kind == 3 ? n + 5 : (r * 7) % (n + 2) - 1;
    index[r] = r % (n_lines + 1) == n_lines && r > 0 ? n_lines : r % n_lines;   // some rows: out of range
    const int li = with_index ? (index[r] < n_lines ? index[r] : 0) : 0;
    win[2 * (size_t)r] = window_kind == 1 ? 10.0 : 0.0; win[2 * (size_t)r + 1] = window_kind == 1 ? 30.0 : 40.0;
    if (window_kind == 2 && r % 3 == 1) win[2 * (size_t)r] = NAN;
    if (window_kind == 2 && r % 3 == 2) { win[2 * (size_t)r] = 30.0; win[2 * (size_t)r + 1] = 10.0; }
    for (int j = 0; j < n; j++) {
      const int k = (int)(urand() * (M - 1));
      const double w = urand(), l = 6.0 * urand() - 3.0;
      const size_t a = (size_t)li * M + k;
      const double th = tab.rth[a] + w * (tab.rth[a + 1] - tab.rth[a]);
      double x = tab.rx[a] + w * (tab.rx[a + 1] - tab.rx[a]) - std::sin(th) * l, y = tab.ry[a] + w * (tab.ry[a + 1] - tab.ry[a]) + std::cos(th) * l;
      switch ((r + j) % 9) {
        case 1: x = tab.rx[a] - std::sin(tab.rth[a]) * l; y = tab.ry[a] + std::cos(tab.rth[a]) * l; break;   // on a table normal
        case 2: x = tab.rx[(size_t)li * M] - 5.0 * std::cos(tab.rth[(size_t)li * M]); y = tab.ry[(size_t)li * M] - 5.0 * std::sin(tab.rth[(size_t)li * M]); break;
        case 3: x = NAN; break;
        case 4: y = NAN; break;
        case 5: x = 1e6; y = -1e6; break;
        default: break;
      }
      const double u[6] = {x, y, th + 2.0 * urand() - 1.0, 0.1 * urand() - 0.05, (r + j) % 9 == 6 ? 0.0 : 0.5 + 10.0 * urand(), 4.0 * urand() - 2.0};
      for (int q = 0; q < 6; q++) cart[((size_t)r * 6 + q) * n + j] = u[q];
    }
  }
  for (double &v : fbar) v = urand() - 0.5;
  for (double &v : cdot) v = urand() - 0.5;
  const int *cnt = count_kind == 2 ? nullptr : count.data(), *idx = with_index ? index.data() : nullptr;
  const double *wn = window_kind ? win.data() : nullptr;
  int rc = btrapz_frenet_host(&t, idx, R, n, layout, order, cart.data(), cnt, wn, fr.data(), iv.data(), nout.data());
  if (rc == BTRAPZ_OK) rc = btrapz_frenet_host(&t, idx, R, n, layout, order, cart.data(), cnt, wn, fr.data(), nullptr, nullptr);
  if (rc == BTRAPZ_OK) rc = btrapz_frenet_vjp_host(&t, idx, R, n, layout, order, cart.data(), fr.data(), iv.data(), cnt, fbar.data(), cbar.data());
  if (rc == BTRAPZ_OK) rc = btrapz_frenet_jvp_host(&t, idx, R, n, layout, order, cart.data(), fr.data(), iv.data(), cnt, T, cdot.data(), fdot.data());
  double worst_gap = 0.0;
  long outside = 0, kept = 0;
  if (rc == BTRAPZ_OK) {
    for (int r = 0; r < R; r++) {
      const int c = cnt ? (cnt[r] < n ? (cnt[r] > 0 ? cnt[r] : 0) : n) : n;
      outside += nout[r];
      for (int j = c; j < n; j++) kept += iv[(size_t)r * n + j] == -7;
    }
    for (int k = 0; k < T; k++) {
      double lhs = 0.0, rhs = 0.0, scale = 0.0;
      for (int r = 0; r < R; r++) {
        const int c = cnt ? (cnt[r] < n ? (cnt[r] > 0 ? cnt[r] : 0) : n) : n;
        for (int q = 0; q < 6; q++)
          for (int j = 0; j < c; j++) {
            if (q % 3 > order) continue;
            const size_t o = layout == 0 ? ((size_t)r * 6 + q) * n + j : (((size_t)r * 2 + q / 3) * n + j) * 3 + q % 3;
            lhs += fbar[o] * fdot[(size_t)k * sz + o];
            scale += std::fabs(fbar[o] * fdot[(size_t)k * sz + o]);
          }
      }
      for (size_t o = 0; o < sz; o++) rhs += cbar[o] * cdot[(size_t)k * sz + o];
      if (!shuffled && std::isfinite(scale) && scale > 0.0) worst_gap = std::fmax(worst_gap, std::fabs(lhs - rhs) / scale);
    }
    // an interval array of wild values: OUTSIDE to the derivatives, no access outside the table
    for (size_t o = 0; o < iv.size(); o++) iv[o] = (o % 3 == 0) ? 2147483647 : (o % 3 == 1) ? -2147483647 - 1 : M - 1;
    rc = btrapz_frenet_vjp_host(&t, idx, R, n, layout, order, cart.data(), fr.data(), iv.data(), cnt, fbar.data(), cbar.data());
    for (double v : cbar) if (v != 0.0) rc = -200;
  }
  printf("R %d n %d M %d lines %d layout %d order %d count %d index %d window %d shuffled %d T %d -> rc %d outside %ld kept %ld adjoint gap %.3g\n",
         R, n, M, n_lines, layout, order, count_kind, (int)with_index, window_kind, (int)shuffled, T, rc, outside, kept, worst_gap);
  if (rc != BTRAPZ_OK) return rc;
  return worst_gap < 1e-11 ? 0 : -100;
}

int main() {
  int bad = 0;
  for (int layout = 0; layout < 2; layout++) {
    bad += run_case(1, 1, 2, 1, layout, 2, 2, false, 0, false, 1) != 0;
    bad += run_case(3, 63, 3, 1, layout, 0, 2, false, 0, false, 2) != 0;
    bad += run_case(5, 64, 65, 2, layout, 1, 4, true, 1, false, 3) != 0;
    bad += run_case(4, 65, 1000, 2, layout, 2, 3, true, 2, false, 12) != 0;
    bad += run_case(7, 130, 65, 3, layout, 2, 4, true, 1, false, 1) != 0;
    bad += run_case(2, 9, 3, 1, layout, 2, 0, false, 0, false, 1) != 0;
    bad += run_case(2, 9, 3, 1, layout, 1, 1, false, 2, false, 1) != 0;
    bad += run_case(3, 40, 17, 2, layout, 2, 2, true, 1, true, 2) != 0;       // a table that is not increasing
  }
  // the refusals
  const Table tab = make_table(1, 2, 1.0, false);
  btrapz_refline t = tab.view(1, 2);
  double c[6] = {0.5, 0.1, 0, 0, 1, 0}, out[6], d[6];
  int iv[1] = {0};
  int refused = 0, calls = 0;
  auto expect = [&](int rc) { ++calls; refused += rc == BTRAPZ_EINVAL; printf("refusal %d -> rc %d\n", calls, rc); };
  expect(btrapz_frenet_host(nullptr, nullptr, 1, 1, 0, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 0, 1, 0, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 1, 0, 0, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 2, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, 3, c, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, -1, c, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, 2, nullptr, nullptr, nullptr, out, nullptr, nullptr));
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, 2, c, nullptr, nullptr, nullptr, nullptr, nullptr));
  expect(btrapz_frenet_vjp_host(&t, nullptr, 1, 1, 0, 2, c, out, nullptr, nullptr, out, d));
  expect(btrapz_frenet_vjp_host(&t, nullptr, 1, 1, 0, 2, c, out, iv, nullptr, nullptr, d));
  expect(btrapz_frenet_vjp_host(&t, nullptr, 1, 1, 0, 2, c, out, iv, nullptr, out, nullptr));
  expect(btrapz_frenet_jvp_host(&t, nullptr, 1, 1, 0, 2, c, out, iv, nullptr, 0, c, d));
  expect(btrapz_frenet_jvp_host(&t, nullptr, 1, 1, 0, 2, c, out, iv, nullptr, BTRAPZ_MAX_TANGENTS + 1, c, d));
  expect(btrapz_frenet_jvp_host(&t, nullptr, 1, 1, 0, 2, c, out, iv, nullptr, 1, nullptr, d));
  t.M = 1;
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  t.M = 2; t.n_lines = 0;
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  t.n_lines = 1; t.rkappa = nullptr;
  expect(btrapz_frenet_host(&t, nullptr, 1, 1, 0, 2, c, nullptr, nullptr, out, nullptr, nullptr));
  t.rkappa = tab.rk.data();
  bad += refused != calls;
  bad += btrapz_frenet_host(&t, nullptr, 1, 1, 0, 2, c, nullptr, nullptr, out, iv, nullptr) != BTRAPZ_OK || iv[0] != 0;
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
