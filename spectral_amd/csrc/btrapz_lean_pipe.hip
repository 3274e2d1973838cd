// btrapz_lean_pipe.hip -- the lean two-launch solve with the resume launch of one axis inside the capped launch of the
// other ("three launches").  One grid of n_resume + n_capped wavefronts: the first n_resume blocks are
// the resume wavefronts of axis `resume_axis` (they read that axis's lists and tables, far-from-convergence first), the
// others the capped launch of axis `capped_axis` in memory order.  The resume wavefronts are dispatched first: their
// long dependent chains run beside full-width work instead of on an empty device.  No wavefront waits for another and
// nothing depends on the order in which blocks are dispatched: what the resume part reads was written by an EARLIER
// kernel on the stream (the capped launch of its axis, the bucketing of its lists), the slots the capped part takes
// from the shared counter lie behind those the resume part reads, and the two parts write the records, keys, slots and
// control points of different axes.
// One KernelArgs at kernarg offset 0 serves both parts (btrapz_lean_body.h reads its arguments through the kernarg
// segment pointer): the memory-order capped body reads none of order / cand_prefix / wave_prefix / bucket_S, the resume
// body none of cap_iter / cap_alone / cap_hi / cap_score / S.
// Launches 1 and 3 of the schedule -- one axis's capped launch, one axis's resume launch -- are single-body kernels: fused,
// the two loop bodies share one register allocation and come out at 132 B of scratch per lane instead of 112 and 92.
#include "btrapz_lean_body.h"

namespace btrapz {

// wavefront blk: axis `axis` of candidates blk gpw + [0, gpw), memory order
LEAN_KERNEL void ipm_solve_lean_pipe_capped_kernel(const KernelArgs a, const double *__restrict__ mqm, int axis) {
  __shared__ double lds[LN_ROWS][64];
  lean_solve_body<false, true, false>(a, mqm, lds, 2 * (int)blockIdx.x + axis, (int)threadIdx.x);
}

// wavefront blk: wavefront blk of axis `axis`'s resume lists
LEAN_KERNEL void ipm_solve_lean_pipe_resume_kernel(const KernelArgs a, const double *__restrict__ mqm, int axis) {
  __shared__ double lds[LN_ROWS][64];
  lean_solve_body<true, false, true>(a, mqm, lds, 2 * (int)blockIdx.x + axis, (int)threadIdx.x);
}

// (Each part reads the arguments through its own laundered copy of the kernarg pointer: left to itself the optimiser
//  loads the union of what the two bodies read at the top of the kernel and carries it into both -- 152 spilled SGPRs,
//  a third VGPR for their lanes, 144 B of scratch per lane instead of 132.)
LEAN_KERNEL void ipm_solve_lean_pipe_kernel(const KernelArgs, const double *__restrict__ mqm, int n_resume, int resume_axis,
                                            int capped_axis) {
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
    asm volatile("; capped part" : "+s"(kp));
    __builtin_memcpy(&a, kp, sizeof(KernelArgs));
    lean_solve_body<false, true, false>(a, mqm, lds, 2 * (blk - n_resume) + capped_axis, (int)threadIdx.x);
  }
}

// The lengths of the two axes' resume lists (cand_prefix[65] of each table) into host memory the device can write: what
// the next solve of the context chooses its schedule by (btrapz_host.hip).  Stream-ordered behind the bucketing.
__global__ void pipe_counts_kernel(const int *tables, volatile int *host_counts) {
  if (threadIdx.x < 2) host_counts[threadIdx.x] = tables[threadIdx.x * 198 + 65];
}

}  // namespace btrapz
