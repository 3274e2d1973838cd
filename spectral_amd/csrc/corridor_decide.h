// corridor_decide.h -- the decision phases of the wave-wide corridor stage made again with provenance, one wavefront per
// candidate: what corridor_vjp_kernel (corridor_vjp.hip) and corridor_jvp_kernel (corridor_jvp.hip) share.  Device only.
//   slopes of every obstacle across the lanes into LDS (the expression of SlopesOnTheFly) -> extract_segments_core, lane o
//   owning obstacle o, with the note that records (i0, h) -> the selection, one lane per segment, the running counter as a
//   scan -> dedup_segments_core, std_sort_core, resolve_segments_core on ONE lane (the lists are in LDS; a dozen segments).
// Args: CorridorVjpArgs or CorridorJvpArgs (btrapz_device.h) -- the fields read here carry the same names in both.
#ifndef BTRAPZ_CORRIDOR_DECIDE_H
#define BTRAPZ_CORRIDOR_DECIDE_H

#include <hip/hip_runtime.h>

#include "btrapz_device.h"
#include "corridor_vjp_core.h"

namespace btrapz {

namespace {

// A Seg that copies itself field by field: the compiler moves a plain Seg through a 104-byte stack slot (scratch) wherever
// the serial statements of corridor_core.h copy a whole one inside LDS.  Same layout, same fields, same statements.
struct SegF : Seg {
  __device__ __forceinline__ SegF() {}
  __device__ __forceinline__ SegF(const Seg &o) { *this = o; }
  __device__ __forceinline__ SegF(const SegF &o) { *this = static_cast<const Seg &>(o); }
  __device__ __forceinline__ SegF &operator=(const SegF &o) { return *this = static_cast<const Seg &>(o); }
  __device__ __forceinline__ SegF &operator=(const Seg &o) {
    beg_t = o.beg_t; end_t = o.end_t; t = o.t; beg_l = o.beg_l; end_l = o.end_l;
    upp_skew = o.upp_skew; upp_bias = o.upp_bias; down_skew = o.down_skew; down_bias = o.down_bias;
    l_upp_skew = o.l_upp_skew; l_upp_bias = o.l_upp_bias; l_down_skew = o.l_down_skew; l_down_bias = o.l_down_bias;
    count = o.count;
    return *this;
  }
};
static_assert(sizeof(SegF) == sizeof(Seg), "SegF is a Seg");

__device__ __forceinline__ int scan_inclusive(int v, int lane) {   // integers: any order of the additions is exact
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// Returns the candidate's segment count S >= 1 with the segments in sel[0..S) (provenance in Seg::count) and s_ref | l_ref
// | ds_bounds staged in LDS behind L.dyn; 0 when the candidate has no corridor (the forward's seg_count 0 or -1);
// kCorridorDeferred when its lists overflowed in pass 0 and the retry pass takes it.  Every lane returns the same value.
enum { kCorridorDeferred = -2 };
template <class Args>
__device__ __forceinline__ int corridor_decide(const Args &a, int b, unsigned char *lds_raw, const CorridorVjpLds &L) {
  const int lane = threadIdx.x;
  const int N = a.N, O = a.num_obs, cap_o = a.cap_o, cap_all = cap_o * O, cap_sel = a.cap_sel;
  Seg *all = reinterpret_cast<Seg *>(lds_raw);                       // later: the staged terms
  SegF *sel = reinterpret_cast<SegF *>(lds_raw + L.sel);
  double *dyn = reinterpret_cast<double *>(lds_raw + L.dyn);          // slope table; later s_ref | l_ref | ds_bounds
  int *ocount = reinterpret_cast<int *>(lds_raw + L.ints);            // [64]; later std_sort_core's frames
  int *word = ocount + 64;                                            // [4]
  short *slot_of = reinterpret_cast<short *>(word + 4);               // [cap_all]
  short *pick = slot_of + cap_all;                                    // [cap_sel]
  const double *gs = a.s_bounds + (size_t)b * O * N * 2, *gl = a.l_bounds + (size_t)b * O * N * 2;

  // ---- slopes, all lanes: (b(i) - b(i-1)) / delta, the expression of SlopesOnTheFly ----
  if (a.staged) {
    const double2 *gs2 = reinterpret_cast<const double2 *>(gs);
    double2 *sk2 = reinterpret_cast<double2 *>(dyn);
    const int n2 = O * N;
    for (int i = lane; i < n2; i += 64) {
      const double2 c2 = gs2[i], p2 = gs2[i > 0 ? i - 1 : 0];
      if (i % N > 0) sk2[i] = make_double2((c2.x - p2.x) / a.delta, (c2.y - p2.y) / a.delta);
    }
  }
  __syncthreads();
  // ---- CorridorGeneration + CorridorSplit: lane o owns obstacle o, the serial statement, provenance noted ----
  if (lane < O) {
    const BoundsView sb{gs + (size_t)lane * N * 2}, lb{gl + (size_t)lane * N * 2};
    Seg *list = all + lane * cap_o;
    if (a.staged)
      ocount[lane] = extract_segments_core(a.variant, N, a.delta, sb, lb, SlopeTable{dyn + (size_t)lane * N * 2}, list, cap_o, ProvenanceNote{list});
    else
      ocount[lane] = extract_segments_core(a.variant, N, a.delta, sb, lb, SlopesOnTheFly{sb, a.delta}, list, cap_o, ProvenanceNote{list});
  }
  __syncthreads();                                                    // the slope table has been read for the last time
  double *sref = dyn, *lref = dyn + N, *dsb = dyn + 2 * N;
  bool refs_finite = true;
  {
    const double *gsr = a.s_ref + (size_t)b * N, *glr = a.l_ref + (size_t)b * N;
    const double2 *gds = reinterpret_cast<const double2 *>(a.ds_bounds + (size_t)b * N * 2);
    double2 *d2 = reinterpret_cast<double2 *>(dsb);
    for (int i = lane; i < N; i += 64) {
      const double s = gsr[i], l = glr[i];
      sref[i] = s; lref[i] = l; d2[i] = gds[i];
      refs_finite = refs_finite && fabs(s) < 1e300 && fabs(l) < 1e300;
    }
  }
  refs_finite = __all(refs_finite);
  // ---- selection along the reference (solve_3d.cc:534-596): one lane per segment, the running counter as a scan ----
  int total = 0;
  bool overflow = false;
  for (int o = 0; o < O; o++) {
    const int n = ocount[o];
    if (n < 0) { overflow = true; break; }
    for (int j = lane; j < n; j += 64) slot_of[total + j] = (short)(o * cap_o + j);
    total += n;
  }
  __syncthreads();
  int nsel = 0;
  if (!overflow) {
    int carry = 0;
    for (int q0 = 0; q0 < total; q0 += 64) {
      const int q = q0 + lane;
      int h = 0;
      bool equals_itself = true;
      if (q < total) {
        const Seg c = all[slot_of[q]];
        equals_itself = same_segment(c, c);
        // a knot outside the segment's own span cannot be inside it when these hold (corridor_kernels.hip, the selection)
        const double gap0 = c.upp_bias - c.down_bias, gap1 = c.down_skew * a.delta + c.down_bias - c.upp_skew * a.delta - c.upp_bias;
        const bool own_range = refs_finite && gap0 > 0.0 && gap0 < 1e300 && gap1 < 0.0 && gap1 > -1e300 && c.beg_t <= c.end_t;
        const int i_lo = own_range ? (c.beg_t > 0 ? c.beg_t : 0) : 0;
        const int i_hi = own_range ? (c.end_t < N - 1 ? c.end_t : N - 1) : N - 1;
        for (int i = i_lo; i <= i_hi; i++) h += knot_inside(c, sref[i], lref[i], (double)i, a.delta) ? 1 : 0;
      }
      const int upto = scan_inclusive(h, lane);
      int counter = (carry + upto - h) % 3;
      const int copies = q < total ? selection_copies(selection_pushes(h, counter), equals_itself) : 0;
      const int placed = scan_inclusive(copies, lane);
      for (int j = 0, r = nsel + placed - copies; j < copies && r < cap_sel; j++, r++) pick[r] = slot_of[q];
      nsel += __builtin_amdgcn_readlane(placed, 63);
      carry = (carry + __builtin_amdgcn_readlane(upto, 63)) % 3;
    }
    if (nsel > cap_sel) overflow = true;
  }
  __syncthreads();
  if (overflow) {   // second chance with the full lists; beyond those: seg_count = -1, the zeros stay
    if (a.pass == 0 && a.retry_list) {
      if (lane == 0) a.retry_list[atomicAdd(a.retry_count, 1)] = b;
      return kCorridorDeferred;
    }
    return 0;
  }
  if (nsel == 0) return 0;
  // ---- de-dup (keep first), std::sort's order, reorder, overlap: the serial statements, on one lane ----
  if (lane < nsel) {
    const int slot = pick[lane];
    SegF mine = all[slot];
    mine.count = provenance_pack(slot / cap_o, mine.count);
    sel[lane] = mine;
  }
  __syncthreads();
  if (lane == 0) {
    int n = dedup_segments_core(sel, nsel);
    if (a.variant == 0) sort_segments_core(sel, n, ocount);   // (frames: 36 ints for n <= 64)
    resolve_segments_core(a.variant, a.delta, sel, n);
    word[0] = n;
  }
  __syncthreads();
  const int S = word[0];
  bool bad = S > a.seg_stride;
  if (!bad && lane < S && !(sel[lane].t > 0.0)) bad = true;
  return __any(bad) ? 0 : S;
}

}  // namespace

}  // namespace btrapz
#endif
