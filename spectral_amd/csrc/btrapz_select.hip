// btrapz_select.hip -- deterministic K-best selection beside the arg-min (include/btrapz_hip_select.h):
// btrapz_topk_device, btrapz_topk_pairs_device, btrapz_gather_rows_device.
//
// The order is argmin_kernel's (btrapz_kernels.hip): cost ascending, equal costs -> lowest index.  It is a total order on
// the entries that take part (cost < +inf, index >= 0), so the K best of a set are the K best of the union of the K best
// of its parts -- whatever the parts are: the steps of a wavefront, the wavefronts of a block, the chunks of a group, the
// shards of the ranks.  One procedure serves all four.
//
// Mapping: a wavefront keeps its list sorted in registers, one entry per lane (lane r holds rank r; lanes >= K and
// slots nobody fills hold (+inf, -1)).  It reads 64 entries per step, coalesced, and a ballot against the list's worst
// entry decides whether any of them can enter: most steps end there, so the kernel streams.  A few survivors are placed
// one by one, at popcount(ballot(held entry is before the new one)), the lanes behind moving up by one (DPP
// wave_shr:1); a step with many -- the first steps of every list -- is sorted by a bitonic network over the lanes and
// merged: the 64 best of two sorted lists are min(a[l], b[63 - l]), a bitonic sequence that six exchanges put in order.
// That merge also joins the lists of a block's wavefronts, pairwise through LDS.  A group of 8 192 costs or more is
// split over blocks of about 1 024 costs (as the arg-min does); their sorted lists go to a workspace of the context and a
// second launch merges them the same way.
#include <hip/hip_runtime.h>

#include "btrapz_select.h"

#define UNROLL _Pragma("unroll")

namespace btrapz {

namespace {

constexpr int kMaxK = BTRAPZ_MAX_TOPK;
constexpr int kSplitGroup = 8192, kChunk = 1024, kMaxChunks = 256;   // argmin's split
constexpr int kWaveOnly = 256;                                        // entries up to which one wavefront takes a list alone
constexpr int kListsPerWave = 4;                                      // the merging launch: partial lists a wavefront takes (up to 16 wavefronts)
constexpr int kSerialMax = 8;                                         // entries of a step that enter one by one; more: sort and merge

__device__ __forceinline__ bool before(double c2, long long i2, double c1, long long i1) {
  return c2 < c1 || (c2 == c1 && i2 < i1);
}
// lane l <- lane l - 1 (lane 0 reads 0 and never keeps it)
__device__ __forceinline__ int prev32(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }   // wave_shr:1
__device__ __forceinline__ double prev_lane(double x) { return __hiloint2double(prev32(__double2hiint(x)), prev32(__double2loint(x))); }
__device__ __forceinline__ long long prev_lane(long long x) {
  return (long long)(((unsigned long long)(unsigned)prev32((int)(x >> 32)) << 32) | (unsigned)prev32((int)x));
}
// the value lane j holds (j the same in every lane)
__device__ __forceinline__ double of_lane(double x, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), j), __builtin_amdgcn_readlane(__double2loint(x), j));
}
__device__ __forceinline__ long long of_lane(long long x, int j) {
  return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(x >> 32), j) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)x, j));
}

// The sorted list of a wavefront: lane r holds the entry of rank r; lanes >= K and ranks nobody fills hold (+inf, -1).
struct List {
  double c;
  long long i;
  __device__ __forceinline__ void clear() { c = __builtin_huge_val(); i = -1; }
  // compare-exchange with lane ^ j: the lower lane of a pair keeps the earlier entry when `up`, the later one otherwise
  // (equal entries are empty ones: both lanes keep theirs)
  __device__ __forceinline__ void exchange(int lane, int j, bool up) {
    const double pc = __shfl_xor(c, j);
    const long long pi = __shfl_xor(i, j);
    const bool lower = (lane & j) == 0;
    if (lower == up ? before(pc, pi, c, i) : before(c, i, pc, pi)) { c = pc; i = pi; }
  }
  // 64 entries in any order -> ascending over the lanes (bitonic network, 21 exchanges)
  __device__ __forceinline__ void sort(int lane) {
    UNROLL for (int k = 2; k <= 64; k <<= 1)
      UNROLL for (int j = k >> 1; j > 0; j >>= 1) exchange(lane, j, (lane & k) == 0 || k == 64);
  }
  // The K best of this list and of ANOTHER SORTED list o (ascending over the lanes, empty entries last): lane l keeps the
  // earlier one of its entry and o's entry of lane 63 - l -- together the 64 best of both, a bitonic sequence -- and six
  // exchanges put them in order.
  __device__ __forceinline__ void merge_sorted(int K, int lane, const List &o) {
    const double rc = __shfl(o.c, 63 - lane);
    const long long ri = __shfl(o.i, 63 - lane);
    if (before(rc, ri, c, i)) { c = rc; i = ri; }
    UNROLL for (int j = 32; j > 0; j >>= 1) exchange(lane, j, true);
    if (lane >= K) clear();
  }
  // One step: every lane offers (nc, ni) when `take`.  A ballot against the list's worst entry says how many can enter at
  // all.  A few enter one by one, in lane order: at popcount(ballot(held entry is before the new one)), the lanes behind
  // moving up by one; many are sorted and merged.  Either way the result is the K best of the list and the step's
  // entries in the total order.
  __device__ __forceinline__ void offer(int K, int lane, bool take, double nc, long long ni) {
    double wc = of_lane(c, K - 1);
    long long wi = of_lane(i, K - 1);
    unsigned long long m = __ballot(take && before(nc, ni, wc, wi));
    if (__popcll(m) > kSerialMax) {
      List o;
      o.c = nc; o.i = ni;
      if (!take) o.clear();
      o.sort(lane);
      if (of_lane(i, 0) >= 0) { merge_sorted(K, lane, o); return; }
      c = o.c; i = o.i;                             // (the list was empty: a wavefront's first step)
      if (lane >= K) clear();
      return;
    }
    while (m) {
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      const double ec = of_lane(nc, j);
      const long long ei = of_lane(ni, j);
      if (!before(ec, ei, wc, wi)) continue;        // (the list has moved on since the ballot)
      const int pos = __popcll(__ballot(before(c, i, ec, ei)));   // < K: the worst entry is not before (ec, ei)
      const double pc = prev_lane(c);
      const long long pi = prev_lane(i);
      if (lane > pos) { c = pc; i = pi; }
      if (lane == pos) { c = ec; i = ei; }
      if (lane >= K) clear();
      wc = of_lane(c, K - 1);
      wi = of_lane(i, K - 1);
    }
  }
};

}  // namespace

enum { SRC_COST = 0, SRC_LISTS = 1, SRC_PAIRS = 2 };

struct SelectArgs {
  int K, count;                  // per output list: `group` costs (SRC_COST), world * K pairs (SRC_PAIRS), sorted lists of K (SRC_LISTS)
  long long index_base;          // added to the indices written to best_idx (SRC_COST, SRC_LISTS)
  const double *cost;            // SRC_COST: [groups][count]; SRC_LISTS: [groups][count][K] partial costs
  const long long *idx;          // SRC_LISTS: [groups][count][K] partial indices (without index_base); SRC_PAIRS: pairs
  int n;                         // SRC_PAIRS: lists per rank
  long long *best_idx; double *best_cost;   // [groups][K]
  double *part_cost; long long *part_idx;   // gridDim.y > 1: [groups][gridDim.y][K]
};

// Entry e of list g as (take, cost, index): SRC_COST, SRC_PAIRS.
template <int SRC> __device__ __forceinline__ bool entry(const SelectArgs &a, long long g, int e, double &c, long long &i) {
  if (SRC == SRC_COST) {
    i = g * a.count + e;
    c = a.cost[i];
    return c < __builtin_huge_val();
  }
  const int r = e / a.K, k = e - r * a.K;
  const long long at = ((((long long)r * a.n + g) * a.K) + k) * 2;
  c = __longlong_as_double(a.idx[at]);
  i = a.idx[at + 1];
  return i >= 0 && c < __builtin_huge_val();
}

// grid = (lists, chunks); block = 64 .. 1024.  Chunk y of list g takes entries [y per, (y + 1) per) (SRC_LISTS: one chunk).
template <int SRC> __global__ __launch_bounds__(1024) void select_kernel(const SelectArgs a) {
  __shared__ double sc[8 * 64];
  __shared__ long long si[8 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int K = a.K;
  const long long g = blockIdx.x;
  const int chunks = gridDim.y;
  List l;
  l.clear();
  if (SRC == SRC_LISTS) {
    // wavefront w merges the sorted lists w, w + waves, ...
    // (the next list is on its way while this one is merged)
    List o, n;
    o.clear();
    if (wave < a.count && lane < K) { o.c = a.cost[(g * a.count + wave) * K + lane]; o.i = a.idx[(g * a.count + wave) * K + lane]; }
    for (int s = wave; s < a.count; s += waves) {
      n.clear();
      if (s + waves < a.count && lane < K) {
        const long long at = (g * a.count + s + waves) * K + lane;
        n.c = a.cost[at]; n.i = a.idx[at];
      }
      l.merge_sorted(K, lane, o);
      o = n;
    }
  } else {
    const int per = (a.count + chunks - 1) / chunks;
    const int lo = blockIdx.y * per < a.count ? blockIdx.y * per : a.count;
    const int hi = lo + per < a.count ? lo + per : a.count;
    // wavefront w takes the steps w, w + waves, ...; the next step's entry is on its way while this one is offered
    const int stride = 64 * waves;
    int e = lo + 64 * wave + lane;
    double c = 0.0, nc = 0.0;
    long long i = -1, ni = -1;
    bool take = e < hi && entry<SRC>(a, g, e, c, i);
    for (int e0 = lo + 64 * wave; e0 < hi; e0 += stride) {
      const int en = e + stride;
      const bool ntake = en < hi && entry<SRC>(a, g, en, nc, ni);
      l.offer(K, lane, take, c, i);
      e = en; take = ntake; c = nc; i = ni;
    }
  }
  // the wavefronts' lists, pairwise through LDS: 1 -> 0, 3 -> 2, ...; then 2 -> 0, 6 -> 4, ...; ...
  for (int s = 1; s < waves; s <<= 1) {
    if ((wave & (2 * s - 1)) == s) { sc[(wave >> 1) * 64 + lane] = l.c; si[(wave >> 1) * 64 + lane] = l.i; }
    __syncthreads();
    if ((wave & (2 * s - 1)) == 0 && wave + s < waves) {
      List o;
      o.c = sc[((wave + s) >> 1) * 64 + lane]; o.i = si[((wave + s) >> 1) * 64 + lane];
      l.merge_sorted(K, lane, o);
    }
    __syncthreads();
  }
  if (wave == 0 && lane < K) {
    if (chunks == 1) {
      const long long at = g * K + lane;
      a.best_idx[at] = (SRC != SRC_PAIRS && l.i >= 0) ? l.i + a.index_base : l.i;
      a.best_cost[at] = l.c;
    } else {
      const long long at = (g * chunks + blockIdx.y) * K + lane;
      a.part_cost[at] = l.c;
      a.part_idx[at] = l.i;
    }
  }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(long long total, const long long *idx, long long index_base, int B,
                                                          int row_doubles, const double *src, double *rows) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const long long j = id / row_doubles, k = id - j * row_doubles;
  const long long at = idx[j];
  const unsigned long long r = (unsigned long long)at - (unsigned long long)index_base;
  const bool ok = at != -1 && at >= index_base && r < (unsigned long long)B;
  rows[id] = ok ? src[(long long)r * row_doubles + k] : __longlong_as_double(0x7ff8000000000000LL);
}

namespace {

int refuse(btrapz_ctx *c, const char *what) { btrapz_ctx_set_error(c, what); return BTRAPZ_EINVAL; }
int launched(btrapz_ctx *c, const char *what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return BTRAPZ_OK;
  btrapz_ctx_set_error(c, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return BTRAPZ_EHIP;
}
int set_device(btrapz_ctx *c) {
  const hipError_t e = hipSetDevice(btrapz_ctx_device(c));
  if (e == hipSuccess) return BTRAPZ_OK;
  btrapz_ctx_set_error(c, (std::string("hipSetDevice: ") + hipGetErrorString(e)).c_str());
  return BTRAPZ_EHIP;
}
bool bad_k(int K) { return K < 1 || K > kMaxK; }
int block_for(long long entries) { return entries <= kWaveOnly ? 64 : 256; }

}  // namespace

}  // namespace btrapz

using namespace btrapz;

BTRAPZ_EXPORT int btrapz_topk_device(btrapz_ctx *c, int B, int group, int K, long long index_base, const double *cost,
                                     long long *best_idx, double *best_cost, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (bad_k(K)) return refuse(c, "invalid argument: K (1 .. BTRAPZ_MAX_TOPK = 64)");
  if (B < 1) return refuse(c, "invalid argument: B (< 1)");
  if (group < 1 || B % group != 0) return refuse(c, "invalid argument: group (< 1, or B is not a multiple of it)");
  if (!cost) return refuse(c, "invalid argument: cost (null)");
  if (!best_idx) return refuse(c, "invalid argument: best_idx (null)");
  if (!best_cost) return refuse(c, "invalid argument: best_cost (null)");
  int rc = set_device(c);
  if (rc != BTRAPZ_OK) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int groups = B / group;
  int chunks = group >= kSplitGroup ? (group + kChunk - 1) / kChunk : 1;
  if (chunks > kMaxChunks) chunks = kMaxChunks;
  SelectArgs a = {};
  a.K = K; a.count = group; a.index_base = index_base; a.cost = cost; a.best_idx = best_idx; a.best_cost = best_cost;
  if (chunks == 1) {
    hipLaunchKernelGGL(select_kernel<SRC_COST>, dim3(groups), dim3(block_for(group)), 0, stream, a);
    return launched(c, "btrapz_topk_device");
  }
  // partial lists [groups][chunks][K] in the context's workspace, merged by a second launch
  rc = btrapz_ctx_select_workspace(c, (size_t)groups * chunks * K, stream_, &a.part_cost, &a.part_idx);
  if (rc != BTRAPZ_OK) return rc;
  hipLaunchKernelGGL(select_kernel<SRC_COST>, dim3(groups, chunks), dim3(256), 0, stream, a);
  SelectArgs m = {};
  m.K = K; m.count = chunks; m.index_base = index_base; m.cost = a.part_cost; m.idx = a.part_idx;
  m.best_idx = best_idx; m.best_cost = best_cost;
  const int merge_waves = (chunks + kListsPerWave - 1) / kListsPerWave;       // chunks >= 8: 2 .. 16 wavefronts
  hipLaunchKernelGGL(select_kernel<SRC_LISTS>, dim3(groups), dim3(64 * (merge_waves < 16 ? merge_waves : 16)), 0, stream, m);
  rc = launched(c, "btrapz_topk_device");
  const int rc2 = btrapz_ctx_workspace_close(c, stream_);
  return rc != BTRAPZ_OK ? rc : rc2;
}

BTRAPZ_EXPORT int btrapz_topk_pairs_device(btrapz_ctx *c, int world, int n, int K, const long long *pairs, double *best_cost,
                                           long long *best_idx, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (world < 1) return refuse(c, "invalid argument: world (< 1)");
  if (n < 1) return refuse(c, "invalid argument: n (< 1)");
  if (bad_k(K)) return refuse(c, "invalid argument: K (1 .. BTRAPZ_MAX_TOPK = 64)");
  if ((long long)world * K > 0x7fffffffLL) return refuse(c, "invalid argument: world (world * K does not fit an int)");
  if (!pairs) return refuse(c, "invalid argument: pairs (null)");
  if (!best_cost) return refuse(c, "invalid argument: best_cost (null)");
  if (!best_idx) return refuse(c, "invalid argument: best_idx (null)");
  const int rc = set_device(c);
  if (rc != BTRAPZ_OK) return rc;
  SelectArgs a = {};
  a.K = K; a.count = world * K; a.idx = pairs; a.n = n; a.best_idx = best_idx; a.best_cost = best_cost;
  hipLaunchKernelGGL(select_kernel<SRC_PAIRS>, dim3(n), dim3(block_for(a.count)), 0, (hipStream_t)stream_, a);
  return launched(c, "btrapz_topk_pairs_device");
}

BTRAPZ_EXPORT int btrapz_gather_rows_device(btrapz_ctx *c, int n, const long long *idx, long long index_base, int B,
                                            int row_doubles, const double *src, double *rows, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (n < 1) return refuse(c, "invalid argument: n (< 1)");
  if (B < 1) return refuse(c, "invalid argument: B (< 1)");
  if (row_doubles < 1) return refuse(c, "invalid argument: row_doubles (< 1)");
  if (!idx) return refuse(c, "invalid argument: idx (null)");
  if (!src) return refuse(c, "invalid argument: src (null)");
  if (!rows) return refuse(c, "invalid argument: rows (null)");
  const long long total = (long long)n * row_doubles, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return refuse(c, "invalid argument: n (n * row_doubles is beyond one launch)");
  const int rc = set_device(c);
  if (rc != BTRAPZ_OK) return rc;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, total, idx, index_base, B,
                     row_doubles, src, rows);
  return launched(c, "btrapz_gather_rows_device");
}
