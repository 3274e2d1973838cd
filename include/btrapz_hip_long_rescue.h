/* btrapz_hip_long_rescue.h -- the rescue pass (btrapz_options.elastic = 1) for candidates of 65..256 segments, uniform and
 * ragged, cold or warm-started: a header beside btrapz_hip_long.h (which it includes), plain C99.
 *
 * The entry points that were there stop short of it: btrapz_solve_batch_device refuses elastic = 1 beyond
 * BTRAPZ_MAX_SEGMENTS_LONG_RESCUE (192) segments, btrapz_solve_ragged_device / btrapz_solve_warm_device with elastic = 1
 * leave a candidate of more than 64 segments at BTRAPZ_NO_CORRIDOR, btrapz_solve_long_warm_device refuses elastic != 0.
 * They keep every answer and every refusal.  This call has the arguments, array layouts and btrapz_warm of
 * btrapz_solve_long_warm_device (warm may be NULL) and accepts opt->elastic 0 or 1:
 *
 *   opt NULL or opt->elastic == 0: the call IS btrapz_solve_long_warm_device -- results bit for bit its own.
 *   seg_stride <= 64 (uniform or ragged, any opt->elastic): the call IS btrapz_solve_warm_device.
 *   seg_count NULL, 65 <= seg_stride <= 192, warm NULL or x0 == lam0 == lam_out == NULL: the call IS
 *     btrapz_solve_batch_device with elastic = 1 (btrapz_last_solve_form 2).
 *   seg_count NULL otherwise (193..256 segments, or 65..192 with a start or lam_out): the launch of
 *     btrapz_solve_long_warm_device, then one rescue launch -- a workgroup per axis problem again, and only those whose
 *     problem ended BTRAPZ_MAX_ITER_REACHED do work: they solve it again with elastic rows (btrapz_options.elastic in
 *     btrapz_hip.h), cold, patiently (at least 120 iterations, conservative steps).  Asynchronous, stream-ordered, no host
 *     round trip.  btrapz_last_solve_form 16.  warm->hint is not read.
 *   seg_count given, 65 <= seg_stride <= 256: the candidates of at most 64 segments are solved exactly as
 *     btrapz_solve_warm_device with elastic = 1 solves them, its rescue pass included; then those of 65..256 segments, one
 *     plain launch and one rescue launch per segment count over the listed candidates of that count -- ONE host
 *     synchronisation for the counts, + 16 in btrapz_last_solve_form.  A long candidate gets the bits the uniform call
 *     of its own width and start gives it.  A candidate whose count is outside 1..seg_stride: BTRAPZ_NO_CORRIDOR.
 *
 * A rescued candidate -- no feasible point, least violation (in control-point units, see btrapz_options.elastic_tol)
 * within the tolerance -- has status BTRAPZ_SOLVED_INACCURATE (2), a finite cost and the control points of the relaxed
 * problem's solution; beyond the tolerance it is BTRAPZ_PRIMAL_INFEASIBLE, cost +inf.  Candidates the plain solve answered
 * keep its status, cost, iteration count and control points to the last bit.  The rescue launch writes no multipliers: lam_out
 * of a rescued candidate holds those of the stalled plain solve, as after btrapz_solve_warm_device's rescue pass -- a poor
 * start, never a wrong one.  btrapz_rescue_violations_device works after the call.
 *
 * BTRAPZ_EINVAL (btrapz_last_error names the argument) for opt->elastic outside {0, 1} with seg_stride > 64 (elastic
 * rows for every candidate, 2, are not served beyond 64 segments), for seg_stride > BTRAPZ_MAX_SEGMENTS_LONG, for shared,
 * seg, init, ref_end, dl_bounds, ctrl, cost or status NULL, B < 1, seg_stride < 1, another layout of btrapz_options.
 * iters may be NULL.  Parameter sets are not served. */
#ifndef BTRAPZ_HIP_LONG_RESCUE_H
#define BTRAPZ_HIP_LONG_RESCUE_H
#include "btrapz_hip_long.h"
#ifdef __cplusplus
extern "C" {
#endif

int btrapz_solve_long_rescue_device(btrapz_ctx *ctx, const btrapz_shared *shared, const btrapz_options *opt,
                                    const btrapz_warm *warm, int B, int seg_stride, const double *seg,
                                    const int *seg_count, const double *init, const double *ref_end,
                                    const double *dl_bounds, double *ctrl, double *cost, int *status,
                                    int *iters, void *stream);

#ifdef __cplusplus
}
#endif
#endif
