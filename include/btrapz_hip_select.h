/* btrapz_hip_select.h -- deterministic K-best selection beside the arg-min: a fourth header beside
 * btrapz_hip.h (which it includes), plain C99.
 *
 * The order is btrapz_argmin_device's, a total one: cost ascending, equal costs -> lowest global index.  "Nobody" is
 * (-1, +inf), as there.  Every result is exact (cost bits, int64 indices) and does not depend on how the work is split
 * over wavefronts, blocks or ranks. */
#ifndef BTRAPZ_HIP_SELECT_H
#define BTRAPZ_HIP_SELECT_H
#include "btrapz_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define BTRAPZ_MAX_TOPK 64

/* The K best candidates of every contiguous group of `group` costs (B % group == 0), in the total order of
 * btrapz_argmin_device: cost ascending, equal costs -> lowest global index.  A candidate takes part iff cost < +inf
 * (NaN and +inf never do).  best_idx / best_cost [B/group][K]; slots beyond the number of candidates that take part
 * (K > group included) hold -1 / +inf.  K == 1 gives btrapz_argmin_device's output bit for bit.  Device pointers,
 * asynchronous, stream-ordered; the result does not depend on how the work is split over blocks.
 * BTRAPZ_EINVAL: K < 1 or K > BTRAPZ_MAX_TOPK; B < 1, group < 1 or B % group != 0; a null pointer. */
int btrapz_topk_device(btrapz_ctx *ctx, int B, int group, int K, long long index_base, const double *cost,
                       long long *best_idx, double *best_cost, void *stream);

/* Merge of per-rank lists after an all-gather: pairs [world][n][K][2] int64 = (bit pattern of the cost, global index or
 * -1), in any order within a list; entries with index -1 or a cost that is NaN / +inf are skipped.  Output as above,
 * [n][K].  (K == 1: btrapz_argmin_pairs_device's result.)  BTRAPZ_EINVAL: world < 1, n < 1, K out of range, a null
 * pointer. */
int btrapz_topk_pairs_device(btrapz_ctx *ctx, int world, int n, int K, const long long *pairs, double *best_cost,
                             long long *best_idx, void *stream);

/* rows[j] = src[idx[j] - index_base] (row_doubles doubles each) for j < n; a row whose idx is -1 or outside
 * [index_base, index_base + B) is filled with NaN.  For hosts without torch: the K winners' control points.
 * BTRAPZ_EINVAL: n < 1, B < 1, row_doubles < 1, a null pointer. */
int btrapz_gather_rows_device(btrapz_ctx *ctx, int n, const long long *idx, long long index_base, int B, int row_doubles,
                              const double *src, double *rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
