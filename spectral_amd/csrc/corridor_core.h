// corridor_core.h -- the corridor stage on fixed-capacity arrays, compiled for host AND device.
//
// One implementation serves both the C++ find_traj driver (corridor.cpp) and the batched device
// pipeline (corridor_kernels.hip).  Restates (file:line in /root/reference)
//   CorridorGeneration  src/solve_3d.cc:323-486   src/cuboid_3d.cc:301-407
//   CorridorSplit       src/solve_3d.cc:729-772   src/cuboid_3d.cc:588-625
//   CollisionCheck      src/solve_3d.cc:488-714   src/cuboid_3d.cc:409-573
// with the reference's arithmetic kept expression by expression (several factors of its edge
// functions are identically zero; `(k*d + b) - b` is NOT simplified: it is not k*d in floating point).
#ifndef BTRAPZ_CORRIDOR_CORE_H
#define BTRAPZ_CORRIDOR_CORE_H

#if defined(__HIPCC__)
#define BTRAPZ_HD __host__ __device__ inline
#else
#define BTRAPZ_HD inline
#endif

#include <math.h>

// Expression by expression means operation by operation: a fused multiply-add rounds once where the reference rounds
// twice, and the signs of the edge functions below decide membership on degenerate quads (collapsed or crossing
// bounds).  hipcc contracts device code by default; from here to the end of the translation unit it does not.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace btrapz {

// One corridor segment == the reference's Cube (include/btrapz/cube_type.h:2-24).  POD: usable in LDS.
struct Seg {
  int beg_t, end_t;
  double t;
  double beg_l, end_l;
  double upp_skew, upp_bias, down_skew, down_bias;
  double l_upp_skew, l_upp_bias, l_down_skew, l_down_bias;
  int count;
};

BTRAPZ_HD Seg seg_default() {  // Cube::Cube(), cube_type.h:12-21
  Seg s;
  s.beg_t = 0; s.end_t = 0; s.t = 0.0; s.beg_l = 0.0; s.end_l = 0.0;
  s.upp_skew = 0.0; s.upp_bias = 1000.0; s.down_skew = 0.0; s.down_bias = 0.0;
  s.l_upp_skew = 0.0; s.l_upp_bias = 1000.0; s.l_down_skew = 0.0; s.l_down_bias = 0.0;
  s.count = 0;
  return s;
}

// Per-knot bounds as interleaved (lower, upper) pairs with an element stride, so the same code reads
// a std::vector<pair>, a file-ordered [N][2] block or an LDS staging buffer.
struct BoundsView {
  const double *p;
  BTRAPZ_HD double lo(int i) const { return p[2 * i]; }
  BTRAPZ_HD double hi(int i) const { return p[2 * i + 1]; }
};

// Per-knot slopes of the s bounds, (b(i) - b(i-1)) / delta for i = 1..N-1: computed on the fly on the host, read
// from a table the lanes filled in parallel on the device (the divisions are the expensive part of the scan; the
// expression -- hence the rounding -- is the same).
struct SlopesOnTheFly {
  BoundsView sb;
  double delta;
  BTRAPZ_HD double down(int i) const { return (sb.lo(i) - sb.lo(i - 1)) / delta; }
  BTRAPZ_HD double up(int i) const { return (sb.hi(i) - sb.hi(i - 1)) / delta; }
};
struct SlopeTable {  // interleaved (down, up) pairs, entry i at p[2 i]
  const double *p;
  BTRAPZ_HD double down(int i) const { return p[2 * i]; }
  BTRAPZ_HD double up(int i) const { return p[2 * i + 1]; }
};

// ---- CorridorGeneration + CorridorSplit for one obstacle.  Returns the number of segments written,
// or -1 when `cap` is too small.
// (SB, LB: anything with lo(i) / hi(i) -- BoundsView, or the strips of the fused prism + corridor kernel)
// note(slot, i0, h): told, for every segment written, the knot i0 at which its base segment opened and the number h of
// one-second pieces in front of it -- what the stage's backward pass (corridor_vjp_core.h) needs to know and cannot read
// off the segment.  The default does nothing and leaves no code behind.
struct NoSegmentNote { BTRAPZ_HD void operator()(int, int, int) const {} };
template <class SB, class LB, class Slopes, class Note = NoSegmentNote>
BTRAPZ_HD int extract_segments_core(int variant, int N, double delta, SB sb, LB lb, Slopes sk, Seg *v, int cap, Note note = Note()) {
  if (cap < 1 || N < 3) return -1;
  int n = 0;
  {
    Seg s = seg_default();
    s.beg_t = 0;
    s.down_skew = sk.down(1); s.down_bias = sb.lo(0);
    s.upp_skew = sk.up(1); s.upp_bias = sb.hi(0);
    if (variant == 0) {  // solve_3d.cc:338-341
      s.l_down_skew = (lb.lo(1) - lb.lo(0)) / delta; s.l_down_bias = lb.lo(0);
      s.l_upp_skew = (lb.hi(1) - lb.hi(0)) / delta; s.l_upp_bias = lb.hi(0);
    }
    s.beg_l = lb.lo(0); s.end_l = lb.hi(0);
    v[n++] = s;
  }
  const double threshold = 0.2;  // solve_3d.cc:372
  double cur_down = v[0].down_skew, cur_up = v[0].upp_skew;  // slopes of the open segment
  for (int i = 2; i < N - 1; i++) {
    const double dskew = sk.down(i), uskew = sk.up(i);
    if (fabs(dskew - cur_down) > threshold || fabs(uskew - cur_up) > threshold) {
      if (n + 1 > cap) return -1;
      v[n - 1].end_t = i;
      Seg s = seg_default();
      s.beg_t = i;
      s.down_skew = sk.down(i + 1); s.down_bias = sb.lo(i);
      s.upp_skew = sk.up(i + 1); s.upp_bias = sb.hi(i);
      cur_down = s.down_skew; cur_up = s.upp_skew;
      s.beg_l = lb.lo(i); s.end_l = lb.hi(i);
      if (variant == 0) {  // solve_3d.cc:358-367: the l line of a later segment is the backward difference at i
        s.l_down_bias = lb.lo(i); s.l_upp_bias = lb.hi(i);
        s.l_down_skew = (lb.lo(i) - lb.lo(i - 1)) / delta; s.l_upp_skew = (lb.hi(i) - lb.hi(i - 1)) / delta;
      }
      v[n++] = s;
    }
  }
  v[n - 1].end_t = N - 1;
  for (int i = 0; i < n; i++) v[i].t = (v[i].end_t - v[i].beg_t) * delta;
  // CorridorSplit: peel 1.0 s / 10-knot pieces off the front of every segment while its t > 1 (the reference
  // hard-codes delta = 0.1: solve_3d.cc:735-746; it inserts each piece with vector::insert).  Same pieces, same
  // arithmetic, but written straight to their final slots: count first, then fill from the back (the slots of
  // segment k start at k + the pieces peeled before it, so unread segments are never overwritten).
  int total = 0;
  for (int k = 0; k < n; k++) {
    double t = v[k].t;
    int h = 0;
    while (t > 1) { t = t - 1; if (++h > cap) return -1; }   // bounded: a huge (or infinite) t must not spin
    total += h + 1;
  }
  if (total > cap) return -1;
  int pos = total;
  for (int k = n - 1; k >= 0; k--) {
    Seg rest = v[k];
    int h = 0;
    { double t = rest.t; while (t > 1) { t = t - 1; h++; } }
    pos -= h + 1;
    int w = pos;
    const int opened_at = rest.beg_t;
    int pieces = 0;
    while (rest.t > 1) {
      rest.t = rest.t - 1;
      Seg head = seg_default();
      head.beg_t = rest.beg_t;
      head.end_t = head.beg_t + 10;
      head.t = 1.0;
      head.down_skew = rest.down_skew; head.down_bias = rest.down_bias;
      head.upp_skew = rest.upp_skew; head.upp_bias = rest.upp_bias;
      if (variant == 0) {
        head.l_down_skew = rest.l_down_skew; head.l_down_bias = rest.l_down_bias;
        head.l_upp_skew = rest.l_upp_skew; head.l_upp_bias = rest.l_upp_bias;
      }
      head.beg_l = rest.beg_l; head.end_l = rest.end_l;
      rest.beg_t = rest.beg_t + 10;
      rest.down_bias = head.down_bias + 1.0 * head.down_skew;
      rest.upp_bias = head.upp_bias + 1.0 * head.upp_skew;
      v[w++] = head;
      note(w - 1, opened_at, pieces++);
    }
    v[w] = rest;
    note(w, opened_at, pieces);
  }
  return total;
}

BTRAPZ_HD bool same_segment(const Seg &a, const Seg &b) {  // solve_3d.cc:621
  return a.beg_t == b.beg_t && a.end_t == b.end_t && a.down_bias == b.down_bias && a.down_skew == b.down_skew &&
         a.upp_bias == b.upp_bias && a.upp_skew == b.upp_skew && a.beg_l == b.beg_l && a.end_l == b.end_l;
}

// Point-in-quadrilateral by the signs of four edge functions (solve_3d.cc:534-581).
BTRAPZ_HD bool knot_inside(const Seg &c, double s, double l, double knot, double delta) {
  if (!(l <= c.end_l && l >= c.beg_l)) return false;
  const double d0 = (s - c.down_bias) * (c.beg_t - c.beg_t) - (knot - c.beg_t) * (c.upp_bias - c.down_bias);
  const double d1 = (s - c.upp_bias) * (c.end_t - c.beg_t) - (knot - c.beg_t) * (c.upp_skew * delta + c.upp_bias - c.upp_bias);
  const double d2 = (s - c.upp_bias - c.upp_skew * delta) * (c.end_t - c.end_t) -
                    (knot - c.end_t) * (c.down_skew * delta + c.down_bias - c.upp_skew * delta - c.upp_bias);
  const double d3 = (s - c.down_bias - c.down_skew * delta) * (c.beg_t - c.end_t) -
                    (knot - c.end_t) * (c.down_bias - c.down_skew * delta - c.down_bias);
  const bool pos = d0 > 0 || d1 > 0 || d2 > 0 || d3 > 0;
  const bool neg = d0 < 0 || d1 < 0 || d2 < 0 || d3 < 0;
  return !(pos && neg);
}

// knot_inside for a knot of the segment's OWN span, beg_t <= knot <= end_t, of a segment with finite fields and
//   gap0 = upp_bias - down_bias in (0, 1e300),  gap1 = down_skew delta + down_bias - upp_skew delta - upp_bias in (-1e300, 0)
// and a finite reference -- what the device's selection establishes before it restricts a segment's walk to its own knots
// (corridor_kernels.hip).  There the first products of d0 and d2 are (finite) * (t - t) = +-0 exactly, and their second
// ones are (knot - beg_t) * gap0 >= 0 and (knot - end_t) * gap1 >= 0, zero only at the span's ends and never rounded to
// zero elsewhere (an integer of magnitude >= 1 times a non-zero double): d0 and d2 are never positive, d0 < 0 iff
// knot > beg_t, d2 < 0 iff knot < end_t.  Same decision as knot_inside, bit for bit, without the two edge functions.
BTRAPZ_HD bool knot_inside_own_span(const Seg &c, double s, double l, int knot_i, double delta) {
  if (!(l <= c.end_l && l >= c.beg_l)) return false;
  const double knot = (double)knot_i;
  const double d1 = (s - c.upp_bias) * (c.end_t - c.beg_t) - (knot - c.beg_t) * (c.upp_skew * delta + c.upp_bias - c.upp_bias);
  const double d3 = (s - c.down_bias - c.down_skew * delta) * (c.beg_t - c.end_t) -
                    (knot - c.end_t) * (c.down_bias - c.down_skew * delta - c.down_bias);
  const bool pos = d1 > 0 || d3 > 0;
  const bool neg = knot_i > c.beg_t || knot_i < c.end_t || d1 < 0 || d3 < 0;
  return !(pos && neg);
}

// The reference takes a segment each time a running hit counter reaches 3; the counter is shared by all
// segments of all obstacles and reset only when a segment is taken (solve_3d.cc:584-596).  Given the
// number of reference knots inside a segment and the counter carried in, this returns how many copies the
// reference pushes (>= 1 means the segment is selected; later copies are exact duplicates, removed by its
// de-dup pass) and updates the counter.
BTRAPZ_HD int selection_pushes(int hits_inside, int &carry) {
  const int total = carry + hits_inside;
  carry = total % 3;
  return total / 3;
}

// How many of those copies survive the reference's de-dup pass: one -- unless the segment does not compare equal to
// itself (a NaN among the fields same_segment compares: garbage input, but the count is the reference's), then all.
BTRAPZ_HD int selection_copies(int pushes, bool equals_itself) {
  return pushes < 1 ? 0 : (pushes >= 2 && !equals_itself ? pushes : 1);
}
BTRAPZ_HD int selection_copies(int pushes, const Seg &c) { return selection_copies(pushes, same_segment(c, c)); }

// De-dup (keep first), then ordering and time-overlap resolution: solve_3d.cc:617-703 (trapezoid),
// cuboid_3d.cc:538-567 (cuboid: no sort, no reorder, every later twin, a third of the span).  Separate steps so that
// the device can run all but the overlap walk across the lanes (corridor_kernels.hip).
// (S: Seg, or a type derived from it that copies itself another way -- corridor_vjp.hip)
template <class S>
BTRAPZ_HD int dedup_segments_core(S *v, int n) {
  for (int i = 0; i + 1 < n; i++)
    for (int j = i + 1; j < n;) {
      if (same_segment(v[i], v[j])) { for (int m = j; m + 1 < n; m++) v[m] = v[m + 1]; n--; } else j++;
    }
  return n;
}
// ---- The order of the reference's std::sort (solve_3d.cc:630: comparator on beg_t alone).  std::sort is not stable: two
// segments that open at the same knot end in whatever order the algorithm leaves them, and the order decides the corridor
// (reorder and overlap below see it).  The reference is built against libstdc++, whose std::sort is this introsort
// (bits/stl_algo.h, unchanged from GCC 4 to 13): median of (first + 1, middle, last - 1) swapped to the front, an unguarded
// Hoare partition around it, the right part first, ranges of 16 or fewer left alone, heap sort when 2 floor(lg n) levels
// are used up, and one final insertion pass -- guarded on the first 16 elements, unguarded behind them.  Restated here
// comparison by comparison and move by move in plain C++ (no library on the device): only `key(a) < key(b)` on integers
// decides anything, so the permutation is the library's for every input.  Up to 16 elements the whole of it is the guarded
// insertion pass, which keeps ties in input order.
// T: what is moved (a Seg; on the device's wave-wide path a packed (beg_t, lane) pair).  Key: T -> the int compared.
enum { STD_SORT_THRESHOLD = 16 };
struct SegBegT { BTRAPZ_HD int operator()(const Seg &s) const { return s.beg_t; } };

template <class T, class Key>
BTRAPZ_HD void std_sort_linear_insert(T *v, int last, Key key) {  // __unguarded_linear_insert: no test for the front
  const T val = v[last];
  int next = last - 1;
  while (key(val) < key(v[next])) { v[last] = v[next]; last = next; --next; }
  v[last] = val;
}
template <class T, class Key>
BTRAPZ_HD void std_sort_insertion(T *v, int first, int last, Key key) {  // __insertion_sort
  if (first == last) return;
  for (int i = first + 1; i != last; ++i) {
    if (key(v[i]) < key(v[first])) {
      const T val = v[i];
      for (int m = i; m > first; --m) v[m] = v[m - 1];   // move_backward(first, i, i + 1)
      v[first] = val;
    } else {
      std_sort_linear_insert(v, i, key);
    }
  }
}
template <class T, class Key>
BTRAPZ_HD void std_sort_adjust_heap(T *f, int hole, int len, T value, Key key) {  // __adjust_heap + __push_heap (stl_heap.h)
  const int top = hole;
  int child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (key(f[child]) < key(f[child - 1])) child--;
    f[hole] = f[child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    f[hole] = f[child - 1];
    hole = child - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && key(f[parent]) < key(value)) { f[hole] = f[parent]; hole = parent; parent = (hole - 1) / 2; }
  f[hole] = value;
}
template <class T, class Key>
BTRAPZ_HD void std_sort_heap_sort(T *f, int len, Key key) {  // __partial_sort(first, last, last): __make_heap, __sort_heap
  if (len < 2) return;
  for (int parent = (len - 2) / 2;; parent--) {
    const T value = f[parent];
    std_sort_adjust_heap(f, parent, len, value, key);
    if (parent == 0) break;
  }
  for (int last = len; last > 1;) {   // __pop_heap(first, last, last)
    --last;
    const T value = f[last];
    f[last] = f[0];
    std_sort_adjust_heap(f, 0, last, value, key);
  }
}
template <class T, class Key>
BTRAPZ_HD int std_sort_partition_pivot(T *v, int first, int last, Key key) {  // __unguarded_partition_pivot
  const int mid = first + (last - first) / 2;
  {  // __move_median_to_first(first, first + 1, mid, last - 1)
    const int a = first + 1, b = mid, c = last - 1;
    int m;
    if (key(v[a]) < key(v[b])) m = key(v[b]) < key(v[c]) ? b : (key(v[a]) < key(v[c]) ? c : a);
    else m = key(v[a]) < key(v[c]) ? a : (key(v[b]) < key(v[c]) ? c : b);
    const T x = v[first]; v[first] = v[m]; v[m] = x;
  }
  int lo = first + 1, hi = last;  // __unguarded_partition(first + 1, last, pivot = first)
  for (;;) {
    while (key(v[lo]) < key(v[first])) ++lo;
    --hi;
    while (key(v[first]) < key(v[hi])) --hi;
    if (!(lo < hi)) return lo;
    const T x = v[lo]; v[lo] = v[hi]; v[hi] = x;
    ++lo;
  }
}
BTRAPZ_HD int std_sort_depth_limit(int n) {  // 2 * __lg(n)
  int lg = 0;
  while ((n >> (lg + 1)) > 0) lg++;
  return 2 * lg;
}
// frames: room for 3 * std_sort_depth_limit(n) ints -- the (first, cut, depth) of every __introsort_loop call that waits
// for its recursive call on the right part to return (the recursion spelled out: no call stack on the device).
// Returns true when some range ran out of its depth limit and was heap-sorted.
template <class T, class Key>
BTRAPZ_HD bool std_sort_core(T *v, int n, Key key, int *frames) {
  bool heap_sorted = false;
  if (n <= 0) return false;
  int first = 0, last = n, depth = std_sort_depth_limit(n), sp = 0;
  for (;;) {   // __introsort_loop
    if (last - first > STD_SORT_THRESHOLD) {
      if (depth != 0) {
        --depth;
        const int cut = std_sort_partition_pivot(v, first, last, key);
        frames[3 * sp] = first; frames[3 * sp + 1] = cut; frames[3 * sp + 2] = depth; sp++;   // the caller goes on with [first, cut)
        first = cut;                                                                          // ... after [cut, last)
        continue;
      }
      std_sort_heap_sort(v + first, last - first, key);
      heap_sorted = true;
    }
    if (sp == 0) break;
    sp--;
    first = frames[3 * sp]; last = frames[3 * sp + 1]; depth = frames[3 * sp + 2];
  }
  if (n > STD_SORT_THRESHOLD) {   // __final_insertion_sort
    std_sort_insertion(v, 0, (int)STD_SORT_THRESHOLD, key);
    for (int i = STD_SORT_THRESHOLD; i != n; ++i) std_sort_linear_insert(v, i, key);
  } else {
    std_sort_insertion(v, 0, n, key);
  }
  return heap_sorted;
}
// Returns whether the heap-sort fallback ran (a fact about the input the tests ask for).
// (S: Seg, or a type derived from it; frames: std_sort_core's, from the caller where a local array would cost a stack)
template <class S>
BTRAPZ_HD bool sort_segments_core(S *v, int n, int *frames) {
  if (n <= STD_SORT_THRESHOLD) {  // the guarded insertion pass alone: a stable insertion sort by beg_t
    for (int i = 1; i < n; i++) {
      const S x = v[i];
      int j = i - 1;
      while (j >= 0 && x.beg_t < v[j].beg_t) { v[j + 1] = v[j]; j--; }
      v[j + 1] = x;
    }
    return false;
  }
  return std_sort_core(v, n, SegBegT(), frames);
}
BTRAPZ_HD bool sort_segments_core(Seg *v, int n) {
  int frames[3 * 2 * 31];
  return sort_segments_core(v, n, frames);
}
// Trapezoid variant, first half: pull a segment that continues segment i's lane next to it (solve_3d.cc:640-666).
// Only beg_l, beg_t and end_t are compared; the device runs the k search across the lanes (corridor_kernels.hip).
template <class S>
BTRAPZ_HD void reorder_segments_core(S *v, int n) {
  for (int i = 0; i + 1 < n; i++)
    for (int j = i + 1; j < n; j++) {
      if (v[i].beg_l == v[j].beg_l && j - i == 1) break;
      for (int k = j + 1; k < n; k++)
        if (v[i].beg_l == v[k].beg_l && v[i].end_t == v[k].beg_t) { const S x = v[j]; v[j] = v[k]; v[k] = x; break; }
    }
}
// Time overlaps: between neighbours (trapezoid, solve_3d.cc:678-703: its inner loop breaks after j = i + 1) or between every pair of twins (cuboid).
// Each step sees the spans the previous one left, so this stays a serial walk on the device too.
template <class S>
BTRAPZ_HD void overlap_segments_core(int variant, double delta, S *v, int n) {
  if (variant == 0) {
    for (int i = 0; i + 1 < n; i++) {
      S &a = v[i], &b = v[i + 1];
      if (a.beg_t == b.beg_t && a.end_t == b.end_t) {
        const int half = (a.end_t - a.beg_t) / 2;
        a.end_t -= half; a.t = (a.end_t - a.beg_t) * delta;
        b.beg_t += half; b.t = (b.end_t - b.beg_t) * delta;
      } else if (a.beg_t > b.beg_t && a.end_t <= b.end_t) {
        const int half = (a.end_t - a.beg_t) / 2;
        if (half > 1) { a.end_t -= half; a.t = (a.end_t - a.beg_t) * delta; }
        b.beg_t = a.end_t; b.t = (b.end_t - b.beg_t) * delta;
      }
    }
  } else {
    for (int i = 0; i + 1 < n; i++)
      for (int j = i + 1; j < n; j++)
        if (v[i].beg_t == v[j].beg_t && v[i].end_t == v[j].end_t) {
          const int third = (v[i].end_t - v[i].beg_t) / 3;
          v[i].end_t -= third; v[i].t = (v[i].end_t - v[i].beg_t) * delta;
          v[j].beg_t += third; v[j].t = (v[j].end_t - v[j].beg_t) * delta;
        }
  }
}
template <class S>
BTRAPZ_HD void resolve_segments_core(int variant, double delta, S *v, int n) {
  if (variant == 0) reorder_segments_core(v, n);
  overlap_segments_core(variant, delta, v, n);
}
BTRAPZ_HD int order_segments_core(int variant, double delta, Seg *v, int n) {
  n = dedup_segments_core(v, n);
  if (variant == 0) sort_segments_core(v, n);
  resolve_segments_core(variant, delta, v, n);
  return n;
}

}  // namespace btrapz
#endif
