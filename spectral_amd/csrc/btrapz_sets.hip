// btrapz_sets.hip -- btrapz_solve_sets_device: a batch in which every candidate names its parameter set (weights, ds_ref /
// dl_ref, acceleration and jerk limits).  The candidates are bucketed on the device by key = set (uniform batches) or
// 64 set + 64 - segment count (ragged batches), so that no wavefront holds two sets: the solve bodies then read the set's
// weights, limits and M'QM table through scalar loads, exactly as a one-set launch reads a.sh and its table.  Here: the
// bucket kernels for any number of keys and the lean instantiations (the packed ones are in btrapz_kernels.hip).
#include "btrapz_lean_body.h"

namespace btrapz {

LEAN_SETS_INSTANCE(ipm_solve_lean_sets_ordered_kernel, false)        // cold, uniform or ragged
LEAN_SETS_INSTANCE(ipm_solve_lean_sets_warm_ordered_kernel, true)    // + btrapz_warm

// Key of candidate b, -1 when it is not solved: a set index outside [0, n_sets), or (ragged) a segment count outside
// 1..min(64, seg_stride).  A uniform batch has seg_count == nullptr (the host checks S <= 64).
__device__ __forceinline__ int sets_key(int b, int seg_stride, const int *seg_count, const int *set_index, int n_sets) {
  const int set = set_index[b];
  if (set < 0 || set >= n_sets) return -1;
  if (!seg_count) return set;
  const int s = seg_count[b];
  if (s < 1 || s > 64 || s > seg_stride) return -1;
  return set * 64 + (64 - s);
}

// meta: cand_prefix [n_keys + 1], wave_prefix [n_keys + 1], counts / cursors [n_keys] (zeroed before this launch).
// One global atomic per distinct key and wavefront (ballots): a batch whose keys repeat does not serialise on one address.
__global__ __launch_bounds__(256) void sets_hist_kernel(int B, int seg_stride, const int *seg_count, const int *set_index,
                                                        int n_sets, int n_keys, int *meta) {
  int *hist = meta + 2 * ((size_t)n_keys + 1);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int key = i < B ? sets_key(i, seg_stride, seg_count, set_index, n_sets) : -1;
  unsigned long long remaining = __ballot(key >= 0);
  while (remaining) {
    const int leader = __ffsll((long long)remaining) - 1;
    const int k = __builtin_amdgcn_readlane(key, leader);
    const unsigned long long m = __ballot(key == k);
    if (lane == leader) atomicAdd(&hist[k], __popcll(m));
    remaining &= ~m;
  }
}

// Exclusive prefixes of candidates and of wavefront pairs per key (a key of S segments needs ceil(n / floor(64 / S))
// pairs); the counts become the scatter's cursors.  One workgroup: thread j sums a contiguous run of keys, then a scan.
__global__ __launch_bounds__(1024) void sets_prefix_kernel(int n_keys, int fixed_S, int *meta) {
  int *cand = meta, *wave = meta + (n_keys + 1), *hist = meta + 2 * ((size_t)n_keys + 1);
  __shared__ int sc[1024], sw[1024];
  const int tid = threadIdx.x, per = (n_keys + 1023) / 1024;
  const int j0 = tid * per < n_keys ? tid * per : n_keys, j1 = j0 + per < n_keys ? j0 + per : n_keys;
  auto waves_of = [&](int j, int n) { const int gpw = 64 / (fixed_S > 0 ? fixed_S : 64 - (j & 63)); return (n + gpw - 1) / gpw; };
  int c = 0, w = 0;
  for (int j = j0; j < j1; j++) { const int n = hist[j]; c += n; w += waves_of(j, n); }
  sc[tid] = c; sw[tid] = w;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int ac = tid >= off ? sc[tid - off] : 0, aw = tid >= off ? sw[tid - off] : 0;
    __syncthreads();
    sc[tid] += ac; sw[tid] += aw;
    __syncthreads();
  }
  int pc = sc[tid] - c, pw = sw[tid] - w;
  for (int j = j0; j < j1; j++) {
    const int n = hist[j];
    cand[j] = pc; wave[j] = pw;
    pc += n; pw += waves_of(j, n);
    hist[j] = 0;   // becomes the scatter cursor
  }
  if (tid == 1023) { cand[n_keys] = sc[1023]; wave[n_keys] = sw[1023]; }
}

// order[cand_prefix[key] + ...] = b.  Inside a key: lane order within a wavefront, wavefronts in the order their atomics
// land -- which candidates share a wavefront; every group is solved on its own, so results do not depend on it.
// Candidates without a key get their records here: BTRAPZ_NO_CORRIDOR, iters 0 (cost +inf from finalize_kernel).
__global__ __launch_bounds__(256) void sets_scatter_kernel(int B, int seg_stride, const int *seg_count, const int *set_index,
                                                           int n_sets, int n_keys, int *meta, int *order, double *axis_obj,
                                                           int *axis_status, int *axis_iters) {
  const int *cand = meta;
  int *cursor = meta + 2 * ((size_t)n_keys + 1);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int key = i < B ? sets_key(i, seg_stride, seg_count, set_index, n_sets) : -1;
  if (i < B && key < 0 && axis_status) {   // (no records: the lists of the rescue pass, whose keyless problems have theirs)
    axis_obj[2 * (size_t)i] = 0.0; axis_obj[2 * (size_t)i + 1] = 0.0;
    axis_status[2 * (size_t)i] = BTRAPZ_NO_CORRIDOR; axis_status[2 * (size_t)i + 1] = BTRAPZ_NO_CORRIDOR;
    axis_iters[2 * (size_t)i] = 0; axis_iters[2 * (size_t)i + 1] = 0;
  }
  int pos = 0;
  unsigned long long remaining = __ballot(key >= 0);
  while (remaining) {
    const int leader = __ffsll((long long)remaining) - 1;
    const int k = __builtin_amdgcn_readlane(key, leader);
    const unsigned long long m = __ballot(key == k);
    int base = 0;
    if (lane == leader) base = atomicAdd(&cursor[k], __popcll(m));
    base = __builtin_amdgcn_readlane(base, leader);
    if (key == k) pos = cand[k] + base + __popcll(m & ((1ull << lane) - 1ull));
    remaining &= ~m;
  }
  if (key >= 0) order[pos] = i;
}

// Rescue pass of a sets batch (btrapz_solve_long_sets_device): the three kernels above list the stalled problems of one
// axis when they are given masked[axis] in place of set_index -- the candidate's set where that axis problem ended
// BTRAPZ_MAX_ITER_REACHED, -1 (no key) elsewhere.  A candidate whose set index is out of range is BTRAPZ_NO_CORRIDOR
// by then, not stalled.
__global__ __launch_bounds__(256) void sets_rescue_index_kernel(int B, const int *set_index, const int *axis_status, int *masked) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int set = set_index[b];
  masked[b] = axis_status[2 * (size_t)b] == BTRAPZ_MAX_ITER_REACHED ? set : -1;
  masked[(size_t)B + b] = axis_status[2 * (size_t)b + 1] == BTRAPZ_MAX_ITER_REACHED ? set : -1;
}

}  // namespace btrapz
