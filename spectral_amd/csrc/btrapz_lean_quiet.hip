// btrapz_lean_quiet.hip -- the lean two-launch solve when one axis hands nothing over ("the quiet axis").
// Axis a spreads and goes through the cap as before (btrapz_lean_pipe.hip: its capped launch, the bucketing of its
// lists); axis b is quiet -- every problem of it takes about the same number of iterations -- and is solved by the plain
// one-launch body, in memory order, in the grid that also carries a's resume wavefronts.  b has no cap bookkeeping, no
// lists and no resume launch; its results are the one-launch solve's because its code is.
// One KernelArgs at kernarg offset 0 serves both parts, as in btrapz_lean_pipe.hip: the plain memory-order body reads
// none of cap_* / susp_* / order / cand_prefix / wave_prefix / bucket_S.
#include "btrapz_lean_body.h"

namespace btrapz {

// wavefront blk: axis `axis` of candidates blk gpw + [0, gpw), memory order, to the end (the body of ipm_solve_lean_kernel
// for one axis: A/B runs and schedules that give the quiet axis a launch of its own)
LEAN_KERNEL void ipm_solve_lean_quiet_plain_kernel(const KernelArgs a, const double *__restrict__ mqm, int axis) {
  __shared__ double lds[LN_ROWS][64];
  lean_solve_body<false, false, false>(a, mqm, lds, 2 * (int)blockIdx.x + axis, (int)threadIdx.x);
}

// The first n_resume blocks: the resume wavefronts of axis `resume_axis` (dispatched first, far-from-convergence first);
// the others: axis `plain_axis` of the batch.  No wavefront waits for another: what the resume part reads was written by
// earlier kernels on the stream, and the two parts write the records and control points of different axes.
// (Each part reads the arguments through its own laundered copy of the kernarg pointer, as ipm_solve_lean_pipe_kernel
//  does and for its reason.  104 B of scratch per lane against the 132 B of that kernel.)
LEAN_KERNEL void ipm_solve_lean_quiet_kernel(const KernelArgs, const double *__restrict__ mqm, int n_resume, int resume_axis,
                                             int plain_axis) {
  __shared__ double lds[LN_ROWS][64];
  typedef const KernelArgs __attribute__((address_space(4))) kargs_t;
  kargs_t *kp = (kargs_t *)__builtin_amdgcn_kernarg_segment_ptr();   // (KernelArgs is the first parameter: offset 0)
  const int blk = (int)blockIdx.x;
  KernelArgs a;
  if (blk < n_resume) {   // (wave-uniform: a block is one wavefront)
    asm volatile("; resume part" : "+s"(kp));
    __builtin_memcpy(&a, kp, sizeof(KernelArgs));
    lean_solve_body<true, false, true>(a, mqm, lds, 2 * blk + resume_axis, (int)threadIdx.x);
  } else {
    asm volatile("; plain part" : "+s"(kp));
    __builtin_memcpy(&a, kp, sizeof(KernelArgs));
    lean_solve_body<false, false, false>(a, mqm, lds, 2 * (blk - n_resume) + plain_axis, (int)threadIdx.x);
  }
}

// What the next solve chooses its schedule by, after a solve whose quiet axis went uncapped and so handed nothing over:
// the first axis's count is the length of its resume list as in pipe_counts_kernel; the quiet axis's is an ESTIMATE of
// what the capped launch would have handed over, from the iteration counts the solve left in axis_iters.
// The model.  A group's count n is the pass in which it finished: it is still iterating in pass e exactly when e < n.
// In the capped body a group hands over in pass e when it is the only one of its wavefront still iterating and
// e >= cap_iter (e >= 1 for a group that was alone from pass 0 on), or when e >= cap_hi.  With m the largest count among
// the OTHER groups of the memory-order wavefront (gpw consecutive candidates), the first rule fires for some e iff
// n > max(m, cap_iter) -- cap_iter becomes 1 when m == 0: no other group, or none that could start -- and the second is
// counted from n >= cap_hi ("reaches": one pass early, it over-counts the groups that finish in pass cap_hi itself).
// Two groups that tie for the largest count never hand over under the first rule, here as there.  Left out: hand-over
// slots running out, and a group's neighbours having handed over earlier under the second rule (then counted from
// their full counts, so the group that outlasts them may be missed).  A full wavefront of equal counts below cap_hi
// gives 0; the estimate only moves time.
// One thread per wavefront of the batch; acc[0] the sum, acc[1] the blocks that have added theirs (both zeroed on the
// stream before the solve): the last block writes the two counts into host memory the device can write.
__global__ __launch_bounds__(256) void quiet_counts_kernel(const int *__restrict__ axis_iters, int B, int gpw, int quiet_axis,
                                                           int cap_iter, int cap_hi, const int *tables, int *acc,
                                                           volatile int *host_counts) {
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long c0 = w * gpw;
  int n_over = 0;
  if (c0 < B) {
    const int ng = (int)(B - c0 < gpw ? B - c0 : gpw);
    int top = 0, second = 0, n_top = 0;   // the largest count, the largest below it, how many groups hold the largest
    for (int g = 0; g < ng; g++) {
      const int n = axis_iters[2 * (c0 + g) + quiet_axis];
      if (n > top) { second = top; top = n; n_top = 1; }
      else if (n == top) n_top++;
      else if (n > second) second = n;
      n_over += n >= cap_hi;
    }
    // only a single holder of the largest count can be alone; m: the largest count among the others
    if (n_top == 1 && top < cap_hi && top > (second > 0 ? (second > cap_iter ? second : cap_iter) : 1)) n_over++;
  }
  for (int d = 32; d > 0; d >>= 1) n_over += __shfl_xor(n_over, d);
  if ((threadIdx.x & 63) == 0) {
    if (n_over) atomicAdd(&acc[0], n_over);
    __threadfence();   // (the sum's share is out before the block is counted)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(&acc[1], 1) == (int)gridDim.x - 1) {
      host_counts[quiet_axis] = atomicAdd(&acc[0], 0);
      host_counts[1 - quiet_axis] = tables[(1 - quiet_axis) * 198 + 65];
    }
  }
}

}  // namespace btrapz
