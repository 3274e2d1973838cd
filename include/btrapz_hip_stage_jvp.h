/* btrapz_hip_stage_jvp.h -- forward-mode derivatives (Jacobian-vector products) of the two stages in front of the solve:
 * obstacle prisms -> per-knot bounds (btrapz_prism_bounds_device) and per-knot bounds -> batch record
 * (btrapz_corridor_batch_device).  Chained with btrapz_solve_jvp_device they carry T <= BTRAPZ_MAX_TANGENTS input
 * directions per scene from the obstacle prisms to the control points: one launch per stage, one factorisation per axis
 * problem.  Plain C99; the structs, limits and error codes are those of btrapz_hip.h.
 *
 * Common to the four calls: the stage's discrete decisions are FROZEN and made again from the stage's inputs with the
 * statements of the backward passes (btrapz_prism_bounds_vjp_device, btrapz_corridor_batch_vjp_device): these are the
 * transposes of those maps, read forwards.  The device calls are asynchronous and stream-ordered, take DEVICE pointers and
 * make one launch sequence without a host round trip; every output is OVERWRITTEN completely (entries nothing reaches: 0),
 * no atomics, the same inputs give the same bits on every run, and the `_host` twin (host pointers, no GPU, no context)
 * gives the device call's bits.  Tangents and outputs carry a leading axis T.
 * MEMORY: the prism stage's outputs are dense, 2 x 16 T B O N bytes (T = 12, B = 65 536, O = 5, N = 71: 8.9 GB); chunk T or
 * B when that does not fit. */
#ifndef BTRAPZ_HIP_STAGE_JVP_H
#define BTRAPZ_HIP_STAGE_JVP_H

#include "btrapz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prism stage ---------------------------------------------------------------------------------------------------
 * prisms_dot [T][B][P][8]: tangents of s0, l0, t0, vel_s, vel_l, T; entries 6 and 7 (`active`, `reserved`) are never
 * read, and neither is the tangent of an inactive slot.  Outputs s_bounds_dot, l_bounds_dot [T][B][O][N][2]; either may be
 * NULL (not wanted), not both.
 *   edges: edge_dot[j] is the tangent of the candidate that supplied edge j: l0_dot for the stationary end of a car,
 *       (l0_dot + T vel_l_dot) + vel_l T_dot for the end that is l0 + vel_l T -+ w_safe, 0 for a road edge.
 *       l_bounds_dot[j][i] = (edge_dot[j], edge_dot[j+1]) at every knot i.
 *   faces: the two-decimal rounding is the identity (straight-through).  Where car q's face is the lower / upper s bound of
 *       strip j at knot i, the tangent is (s0_dot + vel_s_dot (i / rate - t0)) - vel_s t0_dot of car q; where the bound is
 *       the road's limit, 0.
 *   padding strips (j >= n_strips) get 0; a scene with more strips than O (the forward's n_strips = -1) gets 0 everywhere.
 * Refused with BTRAPZ_EINVAL (btrapz_last_error says why on the device call): what btrapz_prism_bounds_vjp_device refuses
 * (prisms or road NULL; B, P, N or O < 1; P > 16; knots_per_second not > 0), T < 1 or T > BTRAPZ_MAX_TANGENTS, prisms_dot
 * NULL, both outputs NULL. */
int btrapz_prism_bounds_jvp_device(btrapz_ctx *ctx, int B, int P, int N, const btrapz_road *road, const double *prisms,
                                   int O, int T, const double *prisms_dot, double *s_bounds_dot, double *l_bounds_dot,
                                   void *stream);
int btrapz_prism_bounds_jvp_host(int B, int P, int N, const btrapz_road *road, const double *prisms, int O, int T,
                                 const double *prisms_dot, double *s_bounds_dot, double *l_bounds_dot);

/* ---- corridor stage --------------------------------------------------------------------------------------------------
 * Tangents of the stage's six input arrays; any may be NULL (zero), not all. */
typedef struct btrapz_knot_tangents {
  const double *s_bounds;         /* [T][B][num_obs][N][2] */
  const double *l_bounds;         /* [T][B][num_obs][N][2] */
  const double *ds_bounds;        /* [T][B][N][2] */
  const double *dl_bounds_knots;  /* [T][B][N][2] */
  const double *s_ref, *l_ref;    /* [T][B][N] */
} btrapz_knot_tangents;

/* Outputs, in the shapes btrapz_solve_jvp_device takes as btrapz_tangents: seg_dot [T][NUM_SEG_FIELDS][B][seg_stride],
 * ref_end_dot [T][B][2], dl_bounds_dot [T][B][10]; any may be NULL (not wanted), not all three.
 * Output segment k of a candidate has the provenance (o, i0, h) of btrapz_corridor_batch_vjp_device (obstacle, opening
 * knot, one-second pieces in front of it); lo / hi the obstacle's s bounds, llo / lhi its l bounds, d = delta:
 *   down_skew_dot = (lo_dot(i0+1) - lo_dot(i0)) / d,  down_bias_dot = lo_dot(i0) + h down_skew_dot;  upp_* with hi.
 *   beg_l_dot = llo_dot(i0), end_l_dot = lhi_dot(i0).  Trapezoid: l_down_bias_dot = llo_dot(i0), l_down_skew_dot the forward
 *       difference of llo_dot at knot 0 for i0 = 0, else the backward difference at i0, over d; l_upp_* with lhi.  Cuboid: 0.
 *   ds_lo_dot / ds_hi_dot = ds_bounds_dot at the earliest knot of the final span that attains the max / min; 0 where the
 *       default (0 / 1000) attains it.
 *   x_bias_dot = s_ref_dot(r0), x_skew_dot = (s_ref_dot(r1) - s_ref_dot(r0)) / d, r0 = min(10 k, N-1), r1 = min(10 k + 1,
 *       N-1); y_* with l_ref.
 *   field 0 (T) gets 0; slots >= seg_count get 0; every entry of a candidate whose forward seg_count is 0 or -1 gets 0.
 *   ref_end_dot = (s_ref_dot[N-1], l_ref_dot[N-1]);  dl_bounds_dot[2 i + j] = dl_bounds_knots_dot[min(i, N-1)][j], i = 0..4.
 * Limits and refusals are those of btrapz_corridor_batch_vjp_device (N <= 512, num_obs <= 64, seg_stride <=
 * BTRAPZ_MAX_SEGMENTS, the six inputs non-NULL), and T must be in 1..BTRAPZ_MAX_TANGENTS. */
int btrapz_corridor_batch_jvp_device(btrapz_ctx *ctx, int variant, int B, int N, int num_obs, double delta,
                                     const double *s_bounds, const double *l_bounds, const double *ds_bounds,
                                     const double *dl_bounds_knots, const double *s_ref, const double *l_ref,
                                     int seg_stride, int T, const btrapz_knot_tangents *tangents, double *seg_dot,
                                     double *ref_end_dot, double *dl_bounds_dot, void *stream);
/* ONE candidate on the host (B = 1); *seg_count (may be NULL) receives the forward's count. */
int btrapz_corridor_jvp_host(int variant, int N, int num_obs, double delta, const double *s_bounds,
                             const double *l_bounds, const double *ds_bounds, const double *dl_bounds_knots,
                             const double *s_ref, const double *l_ref, int seg_stride, int T,
                             const btrapz_knot_tangents *tangents, double *seg_dot, double *ref_end_dot,
                             double *dl_bounds_dot, int *seg_count);

#ifdef __cplusplus
}
#endif
#endif
