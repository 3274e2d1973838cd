/* btrapz_hip_check.h -- a batched audit of given control points against every row of their QP: a fifth
 * header beside btrapz_hip.h (which it includes), plain C99.
 *
 * The solve returns control points; this call says whether ANY control points -- a first-order update ctrl + J dtheta, the
 * previous step's winner under the new record, a plan from elsewhere -- satisfy the rows of the problem a batch record
 * states, without solving it.
 *
 * The rows are the reference's own, row by row (solve_3d.cc:779-1129, cuboid_3d.cc:632-988): per axis and segment k the 18
 * inequality rows
 *     r = 0..5    position       t c_i                                   i = r
 *     r = 6..10   velocity       5 (c_i+1 - c_i)                         i = r - 6
 *     r = 11..14  acceleration   20 (c_i - 2 c_i+1 + c_i+2)              i = r - 11
 *     r = 15..17  jerk           60 (c_i+3 - 3 c_i+2 + 3 c_i+1 - c_i)    i = r - 15
 * numbered 18 k + r (the numbering of btrapz_warm.lam0), then the 3 initial-state rows and the 3 continuity rows of every
 * joint.  This is NOT the merged form the solve iterates on:
 *   - the rows at a joint are not intersected with the next segment's;
 *   - no bound is moved: a side of a row is dropped where ITS OWN bound is at least 1e9 in size, and nowhere else (a
 *     position line with one end at 1e10 keeps the rows of its other end); a header limit (ddl, ddds, dddl) of at least
 *     1e9 in size is no limit, whatever the segment's duration;
 *   - the s axis' velocity interval is cut into [0, 1000] and its acceleration limits into [-1000, 1000], as the
 *     reference does; on the l axis the velocity bounds are dl_bounds, indexed by control point;
 *   - the cuboid variant takes the inscribed s interval within [0, 100], and beg_l / end_l. */
#ifndef BTRAPZ_HIP_CHECK_H
#define BTRAPZ_HIP_CHECK_H
#include <stddef.h>
#include "btrapz_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct btrapz_row_check {
  size_t struct_size; /* sizeof(btrapz_row_check): another layout is rejected (BTRAPZ_EINVAL) */
  int    unit;        /* 0: each row in its own unit (t c_i, 5 (c_i+1 - c_i), 20 (c_i - 2 c_i+1 + c_i+2), 60 (...): the
                         units of btrapz_rescue_violations_device); 1: divided by the row's norm |g|
                         (t, sqrt(50), sqrt(2400), sqrt(72000): the unit of btrapz_options.elastic_tol) */
  double *margin;     /* [B][2][4]  s axis then l axis; position, velocity, acceleration, jerk rows: the smallest
                         min(g.x - l, u - g.x) over the class's rows; negative = violated */
  int    *worst;      /* [B][2][4]  the row that attains it: 18 k + r, k = segment, r = 0..5 position, 6..10 velocity,
                         11..14 acceleration, 15..17 jerk (the numbering of btrapz_warm.lam0); lowest on a tie; -1 none */
  double *eq_res;     /* [B][2][2]  largest |g.x - b| of the three initial-state rows, and of the 3 (n - 1) continuity rows
                         (0 for one segment), in the rows' own units whatever `unit` says */
  double *obj;        /* [B]        0.5 x'Px + q'x, the quantity the solve returns as cost */
} btrapz_row_check;   /* any output pointer may be NULL (not wanted); all NULL -> BTRAPZ_EINVAL */

/* Audits ctrl [B][12 * seg_stride] (the solve's layout: a candidate of n segments holds its s axis in the first 6 n
 * doubles, its l axis in the next 6 n) against the rows of the batch record.  sets, n_sets, set_index: as in
 * btrapz_solve_sets_device, set_index NULL = every candidate with sets[0]; seg_count NULL = a uniform batch of
 * seg_stride segments, else seg_count[b] of the seg_stride slots are used.  Device pointers; ctrl 16-byte aligned.
 * One launch, asynchronous, stream-ordered, no host round trip; nothing is allocated beyond what the context keeps for
 * the sets (their device view and M'QM tables).  An output that is not wanted does not change the bits of the others,
 * and a candidate's figures do not depend on the batch around it.
 *
 * Defined cases:
 *   - a class none of whose rows has a side left: margin +inf, worst -1;
 *   - a candidate with a control point among its 12 n that is no finite number, with a duration t <= 0 (or none) in a
 *     used segment, with seg_count outside 1..seg_stride or with set_index outside [0, n_sets): every margin -inf, every
 *     worst -1, eq_res +inf, obj +inf -- it fails every `margin >= -tol`, `eq_res <= tol` a caller writes; the other
 *     candidates are not touched by it;
 *   - a bound, limit or initial state that is NaN: the margin of its class is -inf (worst: its lowest such row), its
 *     residual +inf.
 * BTRAPZ_EINVAL (btrapz_last_error says why): ctx or out NULL; out->struct_size another; every output NULL; unit other
 * than 0 or 1; seg_stride outside 1..BTRAPZ_MAX_SEGMENTS_LONG; B < 0; n_sets outside 1..BTRAPZ_MAX_SETS; sets of mixed
 * variant; with B > 0 a NULL batch array or ctrl, or a ctrl that is not 16-byte aligned.  B == 0 succeeds and launches
 * nothing. */
int btrapz_check_rows_device(btrapz_ctx *ctx, const btrapz_shared *sets, int n_sets, const int *set_index,
                             int B, int seg_stride, const double *seg, const int *seg_count, const double *init,
                             const double *ref_end, const double *dl_bounds, const double *ctrl,
                             const btrapz_row_check *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
