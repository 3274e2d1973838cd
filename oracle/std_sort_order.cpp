// std_sort_order.cpp -- the order the C++ library's std::sort gives tied keys (test infrastructure only, see
// btrapz_oracle.h).
//
// The reference orders the selected corridor segments with std::sort and a comparator that looks at beg_t alone
// (src/solve_3d.cc:630).  std::sort is not stable: libstdc++'s introsort keeps tied keys in input order up to 16
// elements only, so for longer corridors the order of two segments that open at the same knot is whatever that
// algorithm leaves -- and the order decides the corridor (the l-continuity reorder and the overlap walk see it).
// The oracle therefore does not restate the algorithm: it calls the real one.  The permutation depends on the outcomes
// of the comparisons only, so sorting (beg_t, index) pairs gives the permutation of the cubes.
#include <algorithm>
#include <utility>
#include <vector>

extern "C" {

// perm[r] = index (into beg_t) of the element std::sort leaves at position r.
void orc_std_sort_order(const int *beg_t, int n, int *perm) {
  std::vector<std::pair<int, int>> v((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) v[(size_t)i] = std::make_pair(beg_t[i], i);
  std::sort(v.begin(), v.end(),
            [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
  for (int i = 0; i < n; i++) perm[i] = v[(size_t)i].second;
}

// The same with std::stable_sort: ties in input order for every n (the tests count with it how many inputs depend on
// the tie order at all).
void orc_stable_sort_order(const int *beg_t, int n, int *perm) {
  std::vector<std::pair<int, int>> v((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) v[(size_t)i] = std::make_pair(beg_t[i], i);
  std::stable_sort(v.begin(), v.end(),
                   [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
  for (int i = 0; i < n; i++) perm[i] = v[(size_t)i].second;
}

// McIlroy's adversary ("A Killer Adversary for Quicksort", 1999) run against the live std::sort: every key starts as
// "gas" (larger than any fixed value, its own value undecided); when two gas keys are compared, one of them -- the
// current pivot candidate if it takes part -- is frozen to the next small value.  Whatever pivot the sort picks is thus
// among the smallest keys of its range, every partition is lopsided, and the depth limit runs out: the key array
// written to `keys` drives this very std::sort into its heap-sort fallback.  Returns the number of comparisons made.
long orc_std_sort_adversary(int n, int *keys) {
  if (n < 1) return 0;
  const int gas = n - 1;
  std::vector<int> val((size_t)n, gas), idx((size_t)n);
  for (int i = 0; i < n; i++) idx[(size_t)i] = i;
  int nsolid = 0, candidate = 0;
  long ncmp = 0;
  std::sort(idx.begin(), idx.end(), [&](int x, int y) {
    ncmp++;
    if (val[(size_t)x] == gas && val[(size_t)y] == gas) {
      if (x == candidate) val[(size_t)x] = nsolid++; else val[(size_t)y] = nsolid++;
    }
    if (val[(size_t)x] == gas) candidate = x; else if (val[(size_t)y] == gas) candidate = y;
    return val[(size_t)x] < val[(size_t)y];
  });
  for (int i = 0; i < n; i++) keys[i] = val[(size_t)i];
  return ncmp;
}

}  // extern "C"
