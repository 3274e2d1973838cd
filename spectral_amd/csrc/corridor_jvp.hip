// corridor_jvp.hip -- the forward-mode derivative of the batched corridor stage (btrapz_corridor_batch_jvp_device).
//
// corridor_jvp_kernel: one wavefront per candidate.  The decision phases are the backward pass's (corridor_decide.h: slopes
// -> extract_segments_core with the provenance note -> selection scan -> de-dup / sort / resolve on one lane), with the same
// two-pass capacities.  After them lane k owns output segment k: it finds where the segment reads once (segment_reads), then
// loops over the T directions, evaluates segment_tangent -- the whole arithmetic, shared with btrapz_corridor_jvp_host -- and
// stores field f of direction t at seg_dot[t][f][b][k]: neighbouring lanes write neighbouring words.  The tangents are read
// sparsely from global memory (about 16 entries per segment and direction) and are not staged.  Lanes >= seg_count write
// zeros, and so does every lane of a candidate without a corridor: each output entry is written exactly once per call, by the
// pass that settles the candidate.  No sums, no order left to the hardware: the same inputs give the same bits, and the host
// twin's.  corridor_core.h switches FP contraction off for the translation unit.
#include <hip/hip_runtime.h>

#include "btrapz_device.h"
#include "corridor_decide.h"
#include "corridor_jvp.h"
#include "corridor_vjp_core.h"

namespace btrapz {

namespace {

__device__ __forceinline__ void corridor_jvp_candidate(const CorridorJvpArgs &a, int b, unsigned char *lds_raw) {
  const int lane = threadIdx.x;
  const int N = a.N, O = a.num_obs, B = a.B, T = a.T, stride = a.seg_stride;
  const CorridorVjpLds L = corridor_vjp_lds(N, O, a.cap_o, a.cap_sel, stride, a.staged);
  const int S = corridor_decide(a, b, lds_raw, L);
  if (S == kCorridorDeferred) return;   // the retry pass writes this candidate
  const SegF *sel = reinterpret_cast<const SegF *>(lds_raw + L.sel);
  const double *dsb = reinterpret_cast<const double *>(lds_raw + L.dyn) + 2 * N;
  const size_t pairs = (size_t)O * N * 2;
  if (a.seg_dot && lane < stride) {
    const bool mine = lane < S;
    SegmentReads r = {0, 0, 0, 1, -1, -1, 0, 0};
    if (mine) { const Seg c = sel[lane]; r = segment_reads(N, lane, c, dsb); }
    for (int t = 0; t < T; t++) {
      const size_t cand = (size_t)t * B + b;
      double out[BTRAPZ_NUM_SEG_FIELDS];
      if (mine) {
        const KnotTangentSource src{a.s_dot ? a.s_dot + cand * pairs : nullptr, a.l_dot ? a.l_dot + cand * pairs : nullptr,
                                    a.ds_dot ? a.ds_dot + cand * N * 2 : nullptr, a.sref_dot ? a.sref_dot + cand * N : nullptr,
                                    a.lref_dot ? a.lref_dot + cand * N : nullptr, N};
        segment_tangent(a.variant, a.delta, r, src, out);
      } else {
#pragma unroll
        for (int f = 0; f < BTRAPZ_NUM_SEG_FIELDS; f++) out[f] = 0.0;
      }
      double *dst = a.seg_dot + ((size_t)t * BTRAPZ_NUM_SEG_FIELDS * B + b) * stride + lane;
#pragma unroll
      for (int f = 0; f < BTRAPZ_NUM_SEG_FIELDS; f++) dst[(size_t)f * B * stride] = out[f];
    }
  }
  const bool has = S > 0;
  // ref_end = (s_ref[N-1], l_ref[N-1]);  dl_bounds[2 i + j] = dl_bounds_knots[min(i, N-1)][j], i = 0..4
  if (a.ref_end_dot && lane < 2)
    for (int t = 0; t < T; t++) {
      const size_t cand = (size_t)t * B + b;
      const double *ref = lane == 0 ? a.sref_dot : a.lref_dot;
      a.ref_end_dot[cand * 2 + lane] = has && ref ? ref[cand * N + (N - 1)] : 0.0;
    }
  if (a.dl10_dot && lane < 10) {
    const int i = lane >> 1, ii = i > N - 1 ? N - 1 : i;
    for (int t = 0; t < T; t++) {
      const size_t cand = (size_t)t * B + b;
      a.dl10_dot[cand * 10 + lane] = has && a.dl_knots_dot ? a.dl_knots_dot[(cand * N + ii) * 2 + (lane & 1)] : 0.0;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64) void corridor_jvp_kernel(const CorridorJvpArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  if (a.pass == 0) {
    corridor_jvp_candidate(a, (int)blockIdx.x, lds_raw);
  } else {   // retry pass: the candidates the first pass could not hold
    const int n = *a.retry_count;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
      corridor_jvp_candidate(a, __builtin_amdgcn_readfirstlane(a.retry_list[i]), lds_raw);
      __syncthreads();
    }
  }
}

}  // namespace btrapz
