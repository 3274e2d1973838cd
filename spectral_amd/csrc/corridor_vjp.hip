// corridor_vjp.hip -- the backward pass of the batched corridor stage (btrapz_corridor_batch_vjp_device).
//
// corridor_vjp_kernel: one wavefront per candidate, as the forward has (corridor_kernels.hip).  It makes the forward's
// decisions again with the serial statements of corridor_core.h -- the statements the forward's wave-wide phases are
// held to bit for bit -- and carries the provenance of every segment in Seg::count (corridor_vjp_core.h) through
// selection, de-dup, std::sort's order, reorder and overlap (the decision phases: corridor_decide.h, shared with the
// forward-mode kernel of corridor_jvp.hip):
//   slopes of every obstacle across the lanes into LDS (the expression of SlopesOnTheFly) -> extract_segments_core, lane o
//   owning obstacle o, with the note that records (i0, h) -> the selection, one lane per segment, the running counter as a
//   scan -> dedup_segments_core, std_sort_core, resolve_segments_core on ONE lane (the lists are in LDS; a dozen segments)
//   -> segment_adjoint, lane k owning output segment k, its terms staged in LDS -> the ordered pass: the first term that
//   names an entry owns it, adds every term naming it in ascending (segment, term) order and stores the sum.
// No atomics, no order left to the hardware: the same inputs give the same bits.  The outputs are zeroed by the host call
// (one hipMemsetAsync per wanted array, in front of the launch) and written sparsely: a candidate touches a few dozen entries.
// Two passes, the forward's pattern: lists sized for the usual case first, the candidates that overflow them again with the
// capacities the forward ends on (VJP_MAX_ALL, VJP_MAX_SEL); what overflows those has seg_count = -1 and gets zeros.
// corridor_core.h switches FP contraction off for the rest of the translation unit: kept -- the host twin then computes
// the same terms in the same order.
#include <hip/hip_runtime.h>

#include "btrapz_device.h"
#include "corridor_decide.h"
#include "corridor_vjp_core.h"

namespace btrapz {

namespace {

__device__ __forceinline__ constexpr int term_base(int group) {
  return group == VJP_G_S ? 0 : group == VJP_G_L ? VJP_TERMS_S : group == VJP_G_DS ? VJP_TERMS_S + VJP_TERMS_L
         : group == VJP_G_SREF ? VJP_TERMS_S + VJP_TERMS_L + VJP_TERMS_DS : VJP_TERMS_S + VJP_TERMS_L + VJP_TERMS_DS + VJP_TERMS_REF;
}
static_assert(term_base(VJP_G_LREF) + VJP_TERMS_REF == kCorridorVjpTerms, "the staging rows of btrapz_device.h");

struct LdsSink {   // term t of row r at [t * rows + r]: neighbouring lanes, neighbouring words
  int *idx;
  double *val;
  int rows, row;
  __device__ __forceinline__ void add(int group, int p, int index, double value) {
    const int e = (term_base(group) + p) * rows + row;
    idx[e] = index; val[e] = value;
  }
};

// The ordered pass of one output array: P terms per row, R rows.  The first (row, term) that names an entry owns it.
template <int P>
__device__ __forceinline__ void ordered_sums(const int *idx, const double *val, int rows, int R, int lane, double *out) {
  if (!out) return;
  for (int me = lane; me < R; me += 64)   // (R <= 65: row 64, the terms behind 64 segments, is lane 0's second)
#pragma unroll
    for (int p = 0; p < P; p++) {
      const int mine = idx[p * rows + me];
      if (mine < 0) continue;
      bool owner = true;
      double sum = 0.0;
      for (int r = 0; r < R && owner; r++)
#pragma unroll
        for (int q = 0; q < P; q++)
          if (idx[q * rows + r] == mine) {
            if (r < me || (r == me && q < p)) owner = false;
            sum += val[q * rows + r];
          }
      if (owner) out[mine] = sum;
    }
}

__device__ __forceinline__ void corridor_vjp_candidate(const CorridorVjpArgs &a, int b, unsigned char *lds_raw) {
  const int lane = threadIdx.x;
  const int N = a.N, O = a.num_obs;
  const CorridorVjpLds L = corridor_vjp_lds(N, O, a.cap_o, a.cap_sel, a.seg_stride, a.staged);
  const int S = corridor_decide(a, b, lds_raw, L);
  if (S <= 0) return;
  SegF *sel = reinterpret_cast<SegF *>(lds_raw + L.sel);
  const double *dsb = reinterpret_cast<const double *>(lds_raw + L.dyn) + 2 * N;
  // ---- the terms of every output segment, then the ordered pass ----
  const int rows = L.rows;
  double *val = reinterpret_cast<double *>(lds_raw);
  int *idx = reinterpret_cast<int *>(val + (size_t)kCorridorVjpTerms * rows);
  for (int e = lane; e < kCorridorVjpTerms * rows; e += 64) idx[e] = -1;
  __syncthreads();
  if (lane < S) {
    LdsSink sink{idx, val, rows, lane};
    const Seg c = sel[lane];
    segment_adjoint(a.variant, N, a.delta, lane, c, dsb, a.seg_bar ? a.seg_bar + (size_t)b * a.seg_stride + lane : nullptr,
                    (size_t)a.B * a.seg_stride, sink);
  }
  if (lane == 0 && a.ref_end_bar) {   // ref_end = (s_ref[N-1], l_ref[N-1]): row S, behind every segment
    LdsSink sink{idx, val, rows, S};
    sink.add(VJP_G_SREF, 0, N - 1, a.ref_end_bar[(size_t)b * 2]);
    sink.add(VJP_G_LREF, 0, N - 1, a.ref_end_bar[(size_t)b * 2 + 1]);
  }
  __syncthreads();
  const size_t pairs = (size_t)O * N * 2;
  ordered_sums<VJP_TERMS_S>(idx + term_base(VJP_G_S) * rows, val + term_base(VJP_G_S) * rows, rows, S, lane, a.out.s_bounds ? a.out.s_bounds + b * pairs : nullptr);
  ordered_sums<VJP_TERMS_L>(idx + term_base(VJP_G_L) * rows, val + term_base(VJP_G_L) * rows, rows, S, lane, a.out.l_bounds ? a.out.l_bounds + b * pairs : nullptr);
  ordered_sums<VJP_TERMS_DS>(idx + term_base(VJP_G_DS) * rows, val + term_base(VJP_G_DS) * rows, rows, S, lane, a.out.ds_bounds ? a.out.ds_bounds + (size_t)b * N * 2 : nullptr);
  ordered_sums<VJP_TERMS_REF>(idx + term_base(VJP_G_SREF) * rows, val + term_base(VJP_G_SREF) * rows, rows, S + 1, lane, a.out.s_ref ? a.out.s_ref + (size_t)b * N : nullptr);
  ordered_sums<VJP_TERMS_REF>(idx + term_base(VJP_G_LREF) * rows, val + term_base(VJP_G_LREF) * rows, rows, S + 1, lane, a.out.l_ref ? a.out.l_ref + (size_t)b * N : nullptr);
  // dl_bounds[2 i + j] = dl_bounds_knots[min(i, N-1)][j], i = 0..4: lane 2 ii + j owns knot ii
  if (a.dl10_bar && a.out.dl_bounds_knots && lane < 10) {
    const int ii = lane >> 1;
    if (ii <= N - 1) {
      double sum = 0.0;
      for (int i = 0; i < 5; i++)
        if ((i > N - 1 ? N - 1 : i) == ii) sum += a.dl10_bar[(size_t)b * 10 + 2 * i + (lane & 1)];
      a.out.dl_bounds_knots[((size_t)b * N + ii) * 2 + (lane & 1)] = sum;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64) void corridor_vjp_kernel(const CorridorVjpArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  if (a.pass == 0) {
    corridor_vjp_candidate(a, (int)blockIdx.x, lds_raw);
  } else {   // retry pass: the candidates the first pass could not hold
    const int n = *a.retry_count;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
      corridor_vjp_candidate(a, __builtin_amdgcn_readfirstlane(a.retry_list[i]), lds_raw);
      __syncthreads();
    }
  }
}

}  // namespace btrapz
