/* btrapz_hip_long.h -- warm starts and kept multipliers for candidates of 65..256 segments: a sixth
 * header beside btrapz_hip.h (which it includes), plain C99.
 *
 * btrapz_solve_warm_device stops at BTRAPZ_MAX_SEGMENTS: a uniform batch of more segments is refused, and in a ragged
 * batch a candidate of more than 64 segments comes back as BTRAPZ_NO_CORRIDOR.  This call is the same solve -- same
 * arguments, same array layouts, same btrapz_warm -- with seg_stride up to BTRAPZ_MAX_SEGMENTS_LONG: a candidate of
 * 65..256 segments is solved by the long form (one axis problem per workgroup of up to four wavefronts) in its
 * warm-start instantiation, which reads x0 / lam0, restarts a guess that does not pay off from the cold start once, and
 * writes lam_out.  The optimum does not depend on the start; the iteration count does.
 *
 *   seg_count NULL, 65 <= seg_stride <= 256: one launch, asynchronous, stream-ordered, no host round trip.  warm NULL,
 *     or x0 == lam0 == NULL: the cold start, and lam_out (if given) is still written.  warm->hint is not read.
 *     btrapz_last_solve_form reports 16.
 *   seg_stride <= 64 (uniform or ragged): the call IS btrapz_solve_warm_device -- results bit for bit its own.
 *   seg_count given, 65 <= seg_stride <= 256: the candidates of at most 64 segments are solved by
 *     btrapz_solve_warm_device's own launch (bit for bit what it returns for them), then those of 65..256 segments by
 *     the long form, one launch per segment count with the candidates of that count listed -- as the cold ragged solve
 *     serves them: ONE host synchronisation for the counts, and + 16 in btrapz_last_solve_form.  warm->hint is not
 *     read.  x0, lam0 and lam_out have seg_stride slots per candidate; a slot beyond a candidate's count is neither read
 *     nor written.  A candidate whose count is outside 1..seg_stride: BTRAPZ_NO_CORRIDOR.
 *
 * lam_out of a long candidate has the layout and meaning of btrapz_warm.lam_out: rows 0, 6 and 11 of every segment (the
 * bounds a joint's two segments state twice live in the previous segment's last rows) are written as 0.
 *
 * No rescue pass and no parameter sets: BTRAPZ_EINVAL (btrapz_last_error says why) for opt->elastic != 0, for
 * seg_stride > BTRAPZ_MAX_SEGMENTS_LONG, and for what btrapz_solve_warm_device refuses -- ctx, shared, seg, init,
 * ref_end, dl_bounds, ctrl, cost or status NULL, B < 1, seg_stride < 1, another layout of btrapz_options.  iters may be
 * NULL. */
#ifndef BTRAPZ_HIP_LONG_H
#define BTRAPZ_HIP_LONG_H
#include "btrapz_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int btrapz_solve_long_warm_device(btrapz_ctx *ctx, const btrapz_shared *shared, const btrapz_options *opt,
                                  const btrapz_warm *warm, int B, int seg_stride, const double *seg,
                                  const int *seg_count, const double *init, const double *ref_end,
                                  const double *dl_bounds, double *ctrl, double *cost, int *status,
                                  int *iters, void *stream);

#ifdef __cplusplus
}
#endif
#endif
