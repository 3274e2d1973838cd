/* btrapz_hip_long_sets.h -- a parameter set per candidate (btrapz_solve_sets_device in btrapz_hip.h) with what the one-set
 * entry points have and that call refuses: warm starts and kept multipliers for candidates of 65..256 segments, and the
 * rescue pass (btrapz_options.elastic = 1) at every width.  A header beside btrapz_hip_long_rescue.h (which
 * it includes), plain C99.
 *
 * btrapz_solve_sets_device keeps every answer and every refusal.  This call has its arguments and array layouts: sets
 * [n_sets], set_index [B] (device), btrapz_warm as in btrapz_solve_long_warm_device (warm may be NULL; warm->hint is not read).
 *
 * The contract: candidate b's slots of ctrl, cost, status, iters and warm->lam_out hold, bit for bit, what
 * btrapz_solve_long_rescue_device writes there for a batch of the same shape with sets[set_index[b]] as its btrapz_shared,
 * the same warm and the same options (btrapz_options.lean pinned to 1 or -1 and cap_iter = -1, so that the one-set call has
 * no choice of form left that this one does not make alike).
 *
 *   opt NULL or opt->elastic == 0, and seg_stride <= 64 or x0 == lam0 == lam_out == NULL: the call IS
 *     btrapz_solve_sets_device (same btrapz_last_solve_form).
 *   seg_count NULL, 65 <= seg_stride <= 256, x0, lam0 or lam_out given: ONE launch of the warm long form, a workgroup per
 *     axis problem that reads its candidate's set; it starts from x0 / lam0, restarts cold once when that does not pay,
 *     and writes lam_out.  Asynchronous, stream-ordered, no host round trip.  btrapz_last_solve_form 16.
 *   seg_count given, 65 <= seg_stride <= 256, x0, lam0 or lam_out given: the candidates of at most 64 segments exactly as
 *     btrapz_solve_sets_device solves them warm; then those of 65..256 segments, one launch of the warm long form per
 *     segment count over the listed candidates of that count -- ONE host synchronisation for the counts, + 16 in
 *     btrapz_last_solve_form.
 *   opt->elastic == 1, any width: the plain solve as above, then the rescue pass over the axis problems that ended
 *     BTRAPZ_MAX_ITER_REACHED: cold, patient (at least 120 iterations, conservative steps), with elastic rows
 *     (btrapz_options.elastic in btrapz_hip.h), each problem with the weights, limits and M'QM table of its candidate's set.
 *     Up to 64 segments the stalled problems are listed per axis on the device, bucketed by (set, segment count); beyond,
 *     one rescue launch follows every plain launch -- three wavefronts per workgroup up to 192 segments, four beyond -- and
 *     a uniform batch beyond 192 segments takes the warm long form for its plain launch whatever the start
 *     (btrapz_last_solve_form 16; 2 for 65..192 segments without a start).  The rescue launch writes no multipliers.
 *     Statuses and costs of a rescued candidate: btrapz_hip_long_rescue.h.  btrapz_rescue_violations_device works after
 *     the call.
 *
 * A candidate whose set index is outside [0, n_sets): BTRAPZ_NO_CORRIDOR, cost +inf, its slots of ctrl and lam_out
 * untouched; the rescue pass does not look at it.
 *
 * BTRAPZ_EINVAL (btrapz_last_error names the argument) for opt->elastic outside {0, 1}; opt->cap_iter > 0, compact = 1,
 * queue, start; seg_stride > BTRAPZ_MAX_SEGMENTS_LONG; sets of different variant or delta; n_sets outside
 * 1..BTRAPZ_MAX_SETS; sets, set_index, seg, init, ref_end, dl_bounds, ctrl, cost or status NULL; B < 1, seg_stride < 1;
 * another layout of btrapz_options.  iters may be NULL. */
#ifndef BTRAPZ_HIP_LONG_SETS_H
#define BTRAPZ_HIP_LONG_SETS_H
#include "btrapz_hip_long_rescue.h"
#ifdef __cplusplus
extern "C" {
#endif

int btrapz_solve_long_sets_device(btrapz_ctx *ctx, const btrapz_shared *sets, int n_sets, const int *set_index,
                                  const btrapz_options *opt, const btrapz_warm *warm, int B, int seg_stride,
                                  const double *seg, const int *seg_count, const double *init, const double *ref_end,
                                  const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                  void *stream);

#ifdef __cplusplus
}
#endif
#endif
