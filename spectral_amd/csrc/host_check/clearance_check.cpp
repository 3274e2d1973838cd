// clearance_check.cpp -- btrapz_clearance_host, _vjp_host and _jvp_host (clearance_host.cpp, clearance_core.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program (g++, no HIP, no GPU; `make host_asan_clearance`).
// Every buffer has exactly the size the header states, so a read or write past a row, a scene or a tangent is caught.
// Shapes over the edges -- 1 row, 1 sample, 1 obstacle, 17 obstacles, counts 0, 1, n and beyond n, three scenes with a
// scene_index that is out of range for one row, obs_count 0, ragged and beyond O, NaN ego and obstacle poses, a `which`
// that names an obstacle or a feature that does not exist -- and the refusals.  It also checks the adjoint identity
// <clear_bar, J cart_dot> = <J' clear_bar, cart_dot> of every case.  Prints one line per case and "ok".
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../../include/btrapz_hip_clearance.h"

static unsigned long long seed = 1357;
static double urand() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; }

static int run_case(int R, int n, int O, int n_scenes, int count_kind, int obs_kind, bool with_index, bool with_obs_dot, int T) {
  const size_t csz = (size_t)R * 6 * n, osz = (size_t)n_scenes * O * 3 * n, rn = (size_t)R * n;
  std::vector<double> cart(csz), pose(osz), half((size_t)n_scenes * O * 2), clear(rn, -7.0), cbar(rn), cartbar(csz, -7.0);
  std::vector<double> cdot((size_t)T * csz), odot(with_obs_dot ? (size_t)T * osz : 0), cleardot((size_t)T * rn, -7.0);
  std::vector<int> which(rn, -7), count(R), index(R), obs_count(n_scenes);
  for (double &v : cart) v = 40.0 * urand() - 20.0;
  for (double &v : pose) v = 40.0 * urand() - 20.0;
  for (double &v : half) v = 0.5 + 2.0 * urand();
  for (int r = 0; r < R; r++) {
    count[r] = count_kind == 0 ? 0 : count_kind == 1 ? 1 : count_kind == 2 ? n : count_kind == 3 ? n + 5 : (r * 7) % (n + 2) - 1;
    index[r] = r % (n_scenes + 1) == n_scenes && r > 0 ? n_scenes : r % n_scenes;   // some rows: out of range
    for (int j = 0; j < n; j++)
      if ((r + j) % 9 == 4) cart[((size_t)r * 6 + (r + j) % 3) * n + j] = NAN;      // a NaN in x, y or theta
  }
  for (int k = 0; k < n_scenes; k++) {
    obs_count[k] = obs_kind == 0 ? 0 : obs_kind == 1 ? O + 3 : (k * 5 + 1) % (O + 1);
    for (int o = 0; o < O; o++)
      for (int j = 0; j < n; j++)
        if ((k + o + j) % 7 == 3) pose[(((size_t)k * O + o) * 3 + (o + j) % 3) * n + j] = NAN;   // absent there
  }
  for (double &v : cbar) v = urand() - 0.5;
  for (double &v : cdot) v = urand() - 0.5;
  for (double &v : odot) v = urand() - 0.5;
  const btrapz_footprint ft = {2.4, 0.95, 1.3};
  const btrapz_obstacles ob = {n_scenes, O, n, pose.data(), half.data(), obs_kind == 3 ? nullptr : obs_count.data()};
  std::vector<double> cmin(R, -7.0);
  std::vector<int> worst((size_t)R * 2, -7), below(R, -7), invalid(R, -7);
  btrapz_clear_audit au = {cmin.data(), worst.data(), below.data(), invalid.data()};
  const int *cnt = count_kind == 2 ? nullptr : count.data(), *idx = with_index ? index.data() : nullptr;
  int rc = btrapz_clearance_host(&ft, &ob, idx, R, n, cart.data(), cnt, 0.5, clear.data(), which.data(), &au);
  if (rc == BTRAPZ_OK) rc = btrapz_clearance_host(&ft, &ob, idx, R, n, cart.data(), cnt, 0.5, nullptr, nullptr, &au);
  if (rc == BTRAPZ_OK) rc = btrapz_clearance_host(&ft, &ob, idx, R, n, cart.data(), cnt, 0.5, nullptr, which.data(), nullptr);
  if (rc == BTRAPZ_OK) rc = btrapz_clearance_vjp_host(&ft, &ob, idx, R, n, cart.data(), cnt, which.data(), cbar.data(), cartbar.data());
  if (rc == BTRAPZ_OK)
    rc = btrapz_clearance_jvp_host(&ft, &ob, idx, R, n, cart.data(), cnt, which.data(), T, cdot.data(),
                                   with_obs_dot ? odot.data() : nullptr, cleardot.data());
  double worst_gap = 0.0;
  long invalid_sum = 0, kept = 0, nobody = 0;
  if (rc == BTRAPZ_OK) {
    for (int r = 0; r < R; r++) {
      const int c = cnt ? (cnt[r] < n ? (cnt[r] > 0 ? cnt[r] : 0) : n) : n;
      invalid_sum += invalid[r];
      for (int j = c; j < n; j++) kept += clear[(size_t)r * n + j] == -7.0 && which[(size_t)r * n + j] == -7;
      for (int j = 0; j < c; j++) nobody += which[(size_t)r * n + j] == -1;
    }
    // the adjoint identity over the samples read, without the obstacles' tangents (they have no reverse mode)
    if (!with_obs_dot)
      for (int k = 0; k < T; k++) {
        double lhs = 0.0, rhs = 0.0, scale = 0.0;
        for (int r = 0; r < R; r++) {
          const int c = cnt ? (cnt[r] < n ? (cnt[r] > 0 ? cnt[r] : 0) : n) : n;
          for (int j = 0; j < c; j++) {
            const double t = cbar[(size_t)r * n + j] * cleardot[((size_t)k * R + r) * n + j];
            lhs += t; scale += std::fabs(t);
          }
        }
        for (size_t o = 0; o < csz; o++) rhs += cartbar[o] * cdot[(size_t)k * csz + o];
        if (scale > 0.0) worst_gap = std::fmax(worst_gap, std::fabs(lhs - rhs) / scale);
      }
    // a `which` that names nothing: no access outside the arrays, derivative 0
    for (size_t i = 0; i < rn; i++) which[i] = (int)(i % 5 == 0 ? O * 16 + 3 : i % 5 == 1 ? 15 : i % 5 == 2 ? 0x7fffffff : which[i]);
    rc = btrapz_clearance_vjp_host(&ft, &ob, idx, R, n, cart.data(), cnt, which.data(), cbar.data(), cartbar.data());
  }
  printf("R %d n %d O %d scenes %d count %d obs %d index %d obs_dot %d T %d -> rc %d invalid %ld nobody %ld kept %ld adjoint gap %.3g\n", R, n,
         O, n_scenes, count_kind, obs_kind, (int)with_index, (int)with_obs_dot, T, rc, invalid_sum, nobody, kept, worst_gap);
  if (rc != BTRAPZ_OK) return rc;
  return worst_gap < 1e-12 ? 0 : -100;
}

int main() {
  int bad = 0;
  bad += run_case(1, 1, 1, 1, 2, 3, false, false, 1) != 0;
  bad += run_case(3, 63, 2, 1, 2, 3, false, true, 2) != 0;
  bad += run_case(5, 64, 16, 3, 4, 2, true, false, 3) != 0;
  bad += run_case(4, 65, 17, 3, 3, 1, true, true, 12) != 0;
  bad += run_case(7, 130, 17, 3, 4, 2, true, false, BTRAPZ_MAX_TANGENTS) != 0;
  bad += run_case(2, 9, 3, 1, 0, 3, false, false, 1) != 0;
  bad += run_case(2, 9, 3, 1, 1, 3, false, false, 1) != 0;
  bad += run_case(3, 40, 4, 2, 2, 0, true, false, 2) != 0;        // no obstacle anywhere
  // the refusals
  double cart[6] = {0, 0, 0, 0, 0, 0}, pose[3] = {5, 0, 0}, half[2] = {1, 1}, out[6], v = -7.0;
  int wh = -7;
  btrapz_footprint ft = {2.0, 1.0, 0.0};
  btrapz_obstacles ob = {1, 1, 1, pose, half, nullptr};
  btrapz_clear_audit none = {nullptr, nullptr, nullptr, nullptr};
  btrapz_clear_audit one = none;
  one.clear_min = &v;
  int refused = 0, calls = 0;
  auto expect = [&](int rc) { ++calls; refused += rc == BTRAPZ_EINVAL; printf("refusal %d -> rc %d\n", calls, rc); };
  expect(btrapz_clearance_host(nullptr, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  expect(btrapz_clearance_host(&ft, nullptr, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 0, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 0, cart, nullptr, 0.0, out, &wh, nullptr));
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 2, cart, nullptr, 0.0, out, &wh, nullptr));   // obstacles.n != n
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, nullptr, nullptr, 0.0, out, &wh, nullptr));
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, nullptr, nullptr, nullptr));
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, nullptr, nullptr, &none));
  expect(btrapz_clearance_vjp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, nullptr, out, out));
  expect(btrapz_clearance_vjp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, &wh, nullptr, out));
  expect(btrapz_clearance_vjp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, &wh, out, nullptr));
  expect(btrapz_clearance_jvp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, &wh, 0, cart, nullptr, out));
  expect(btrapz_clearance_jvp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, &wh, BTRAPZ_MAX_TANGENTS + 1, cart, nullptr, out));
  expect(btrapz_clearance_jvp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, &wh, 1, nullptr, nullptr, out));
  expect(btrapz_clearance_jvp_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, &wh, 1, cart, nullptr, nullptr));
  ob.O = 0;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  ob.O = 1; ob.n_scenes = 0;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  ob.n_scenes = 1; ob.pose = nullptr;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  ob.pose = pose; half[1] = 0.0;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  half[1] = INFINITY;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  half[1] = 1.0; ft.half_length = -1.0;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  ft.half_length = NAN;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  ft.half_length = 2.0; ft.centre_offset = INFINITY;
  expect(btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, out, &wh, nullptr));
  ft.centre_offset = 0.0;
  bad += refused != calls;
  // boxes 2 x 1 and 1 x 1 half extents, centres 5 apart along x: clearance 2 by a face, exactly
  bad += btrapz_clearance_host(&ft, &ob, nullptr, 1, 1, cart, nullptr, 0.0, nullptr, nullptr, &one) != BTRAPZ_OK || !(v == 2.0);
  if (bad) { printf("FAILED: %d\n", bad); return 1; }
  printf("ok\n");
  return 0;
}
