/* btrapz_hip_long_grad.h -- gradients and directional derivatives of solves whose candidates have 65..256 segments
 * (DESIGN.md 3.16): a seventh header beside btrapz_hip.h (which it includes), plain C99.
 *
 * btrapz_solve_vjp_device and btrapz_solve_jvp_device stop at BTRAPZ_MAX_SEGMENTS slots per candidate.  The two calls
 * here are the same derivatives -- same arguments, same array layouts, same defined cases, same method (the KKT system
 * restricted to the active rows, the equalities eliminated, the active rows by the method of multipliers with relative
 * penalty 1e6 and three passes on one block LDL' factorisation) -- with seg_stride up to BTRAPZ_MAX_SEGMENTS_LONG.  They
 * read what btrapz_solve_long_warm_device (btrapz_hip_long.h) returns: ctrl, status and lam = btrapz_warm.lam_out
 * [2][36][B][seg_stride], of a solve with btrapz_options.elastic = 0.
 *
 *   seg_stride <= 64 (seg_count NULL or given): the call IS btrapz_solve_vjp_device / btrapz_solve_jvp_device -- results
 *     bit for bit their own, refusals included.
 *   65 <= seg_stride <= 256, seg_count NULL (uniform) or given (ragged): one axis problem per workgroup of
 *     ceil(seg_stride / 64) wavefronts, 2 B workgroups.  The VJP is one launch.  The JVP is one launch, and a second,
 *     tiny one behind it on the same stream when cost_dot is wanted: the two axes of a candidate are two workgroups,
 *     each leaves its share of cost_dot in a [2][T][B] workspace of the context, and the second launch adds them in the
 *     fixed order s + l.  Asynchronous and stream-ordered, no host round trip, no atomics.
 *     In a ragged record EVERY candidate is handled by these kernels, one of at most 64 segments included: its rows agree
 *     with btrapz_solve_vjp_device / _jvp_device at seg_stride = count to rounding (the per-candidate sums are added in
 *     segment order here, pairwise there), not bit for bit.  A candidate of n > 64 segments gets bit for bit what the
 *     uniform call at seg_stride = n gives it: nothing depends on the stride or on the number of wavefronts.
 *     A count outside 1..seg_stride: exact zeros in every output row of that candidate.  Slots beyond a count are written
 *     as 0 in grads.seg and ctrl_dot (the layout of btrapz_solve_jvp_device: s axis at [0, 6 S_b), l axis at
 *     [6 S_b, 12 S_b), zeros beyond) and are not read in seg, ctrl, lam, ctrl_bar or the tangents.
 *   Parameter sets (sets, n_sets, set_index) as in the siblings: a set per candidate, one variant and delta.
 *
 * Defined cases: the siblings' -- status not 1 or 2, a set index outside [0, n_sets) or a bad count: zeros; field 0 of
 * seg: 0 / ignored; bounds that are no bounds: 0 / ignored; a joint's bound stated twice: the tighter side's, on an exact
 * tie segment k's; a kept multiplier that is no number: the row is classified by its slack alone.
 *
 * Refused (BTRAPZ_EINVAL, btrapz_last_error says why): seg_stride > BTRAPZ_MAX_SEGMENTS_LONG, and what the siblings
 * refuse -- ctx, sets, seg, ref_end, dl_bounds, ctrl, lam or status NULL, n_sets outside 1..BTRAPZ_MAX_SETS, B < 1,
 * seg_stride < 1, sets of different variant or delta; VJP: out NULL, ctrl_bar and cost_bar both NULL; JVP: both outputs
 * NULL, every tangent NULL, T < 1 or T > BTRAPZ_MAX_TANGENTS. */
#ifndef BTRAPZ_HIP_LONG_GRAD_H
#define BTRAPZ_HIP_LONG_GRAD_H
#include "btrapz_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int btrapz_solve_long_vjp_device(btrapz_ctx *ctx, const btrapz_shared *sets, int n_sets, const int *set_index,
                                 int B, int seg_stride, const double *seg, const int *seg_count,
                                 const double *init, const double *ref_end, const double *dl_bounds,
                                 const double *ctrl, const double *lam, const int *status,
                                 const double *ctrl_bar, const double *cost_bar,
                                 const btrapz_grads *out, void *stream);

int btrapz_solve_long_jvp_device(btrapz_ctx *ctx, const btrapz_shared *sets, int n_sets, const int *set_index,
                                 int B, int seg_stride, const double *seg, const int *seg_count,
                                 const double *init, const double *ref_end, const double *dl_bounds,
                                 const double *ctrl, const double *lam, const int *status,
                                 int T, const btrapz_tangents *tangents, double *ctrl_dot, double *cost_dot, void *stream);

#ifdef __cplusplus
}
#endif
#endif
