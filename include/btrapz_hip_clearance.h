/* btrapz_hip_clearance.h -- batched clearance of the ego's rectangle against moving obstacles' rectangles in the plane,
 * an audit of it per row, and its derivatives: a twelfth header beside btrapz_hip_cartesian.h (which it
 * includes), plain C99.
 *
 * The prisms the QP is built from are axis-aligned in (s, l) and padded; this stage checks what they approximate: whether
 * the car's rectangle, at the pose btrapz_cartesian_device gives a sample, stays clear of every obstacle's rectangle at
 * the same instant.
 *
 * The ego rectangle A at sample j of row r: pose (x, y, theta) = rows BTRAPZ_CART_X / _Y / _THETA of cart [R][6][n];
 *   centre c_A = (x + off cos theta, y + off sin theta);  axes u_A = (cos theta, sin theta), n_A = (-sin theta, cos theta);
 *   half extents (half_length, half_width) along (u_A, n_A).  One footprint serves the whole call.
 * The obstacle rectangle B: obstacle o of the row's scene at sample j has centre c_B = (ox, oy), heading otheta (axes
 *   u_B, n_B alike) and its own half extents.  COLUMN j OF pose IS THE OBSTACLE AT THE TIME OF SAMPLE j OF THE ROW:
 *   aligning the two in time is the caller's responsibility, nothing here knows a time.
 *
 * The signed clearance of the pair, with d = c_B - c_A, c = u_A . u_B, s = n_A . u_B:
 *   over the four face normals e_0 .. e_3 = u_A, n_A, u_B, n_B:  g_k = |e_k . d| - r_A(e_k) - r_B(e_k), r a rectangle's
 *   projected half extent (r_A(u_A) = half_length, r_B(u_A) = hl_B |c| + hw_B |s|, ...);  g = max_k g_k.
 *   - touching or overlapping (g <= 0): the clearance is g, minus the penetration depth exactly; the feature is k, the
 *     lowest k on a tie.  g = 0 is this branch.
 *   - disjoint (g > 0): the clearance is the Euclidean distance of the two rectangles, the smallest of eight
 *     vertex-to-box distances: features 4 .. 7 the vertices of A against B, 8 .. 11 the vertices of B against A, the
 *     vertices in the order (+,+), (-,+), (-,-), (+,-) of the owner's frame.  With p the vertex in the box's frame,
 *     q = (|p_u| - h_l, |p_n| - h_w) and the distance is sqrt(max(q_0, 0)^2 + max(q_1, 0)^2); the lowest feature wins a tie.
 * The clearance of a sample is the minimum over the obstacles present, the lowest obstacle index on a tie, and
 *   which [R][n] = obstacle * 16 + feature, or -1 when there is none.  `which` is the frozen decision of both derivatives.
 *
 * Derivatives: with n the unit direction from B's witness point to A's and the witness points carried rigidly by their
 * rectangles, the rate of the clearance is n . (p_A' - p_B').  In the overlap branch n = -sign(e_k . d) e_k, the witness
 * is the other rectangle's support vertex, and the sign of e_k . d and the signs inside the projected radii are frozen
 * (a sign of exactly 0 counts as +).  At an exact tie between features or obstacles -- edges of cars parallel in their
 * lanes make them -- the derivative is the winner's: a one-sided derivative.  A disjoint feature whose distance is
 * exactly 0 has derivative 0.  A `which` that names no obstacle of the scene or no feature has derivative 0.
 * Such a 0 is written, not formed as 0 times the caller's cotangent or tangent: a NaN or an infinity there does not come through.
 *
 * Defined cases:
 *   - an ego sample whose pose holds a NaN (an OUTSIDE sample of the Cartesian stage): clearance NaN, which -1, counted
 *     in n_invalid, in no extreme, derivative 0;
 *   - an obstacle whose pose holds a NaN at a sample is ABSENT at that sample (its prediction ended);
 *   - no obstacle present (obs_count 0, or all absent): clearance +inf, which -1, derivative 0; +inf enters no extreme;
 *   - a scene_index outside [0, n_scenes): the whole row is invalid (every sample read counts in n_invalid);
 *   - entries at and beyond a row's count keep what the caller put there (clear, which, clear_dot) or are 0 (cart_bar). */
#ifndef BTRAPZ_HIP_CLEARANCE_H
#define BTRAPZ_HIP_CLEARANCE_H
#include "btrapz_hip_cartesian.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the ego's rectangle: half extents > 0 and finite; centre_offset (finite) moves the centre along the heading from the
 * pose's point (a rear-axle pose has centre_offset = wheelbase / 2 or so) */
typedef struct btrapz_footprint {
  double half_length, half_width, centre_offset;
} btrapz_footprint;

/* n_scenes scenes of up to O obstacles, n samples each.  DEVICE pointers in the *_device calls, HOST pointers in the
 * *_host calls.  pose [n_scenes][O][3][n]: rows (x, y, theta), contiguous along the samples; half [n_scenes][O][2]:
 * (half_length, half_width), > 0 and finite -- a precondition the DEVICE calls cannot check without a round trip (the
 * host calls refuse it; on the device a pair with such an extent gives a meaningless value, never an access outside the
 * arrays).  obs_count [n_scenes] may be NULL (every scene has O obstacles), else scene k has min(max(obs_count[k], 0), O). */
typedef struct btrapz_obstacles {
  int n_scenes;
  int O;
  int n;
  const double *pose;
  const double *half;
  const int *obs_count;
} btrapz_obstacles;

#define BTRAPZ_CLEAR_FEATURES 12 /* 0..3 face normals (overlap), 4..7 vertices of A, 8..11 vertices of B (disjoint) */

/* The audit of a row, from the same launch.  Pointers of the kind the call takes; any may be NULL, all NULL ->
 * BTRAPZ_EINVAL.  Over the samples read that are valid: a row without a finite clearance gets clear_min = +inf and
 * worst = (-1, -1) (the "nobody" convention of btrapz_kin_audit).  Order of the reduction: lane q of the row's wavefront
 * takes the samples q, q + 64, ... in rising order, then a butterfly over the lanes (xor 32 ... 1) under the total order
 * "smaller value, then lower sample": no atomics, the same inputs give the same bits on every run. */
typedef struct btrapz_clear_audit {
  double *clear_min; /* [R]    the smallest clearance of the row */
  int    *worst;     /* [R][2] the sample that attains it (lowest on a tie) and that sample's obstacle */
  int    *n_below;   /* [R]    samples with clearance < d_safe */
  int    *n_invalid; /* [R]    samples with a NaN ego pose among those read */
} btrapz_clear_audit;

/* clear [R][n], which [R][n] and / or the audit.  scene_index [R] may be NULL (every row uses scene 0); count [R] may be
 * NULL (every row has n samples), else only samples j < min(count[r], n) are read and written, a count <= 0 is an empty
 * row.  clear, which and audit are each optional, not all three NULL; the audit's bits do not depend on the others.
 * One launch, asynchronous, stream-ordered, no host round trip, no workspace.
 * BTRAPZ_EINVAL (btrapz_last_error says why): ctx, footprint, obstacles, its pose or half, or cart NULL; R, n, O or
 * n_scenes < 1; obstacles.n != n; a footprint half extent that is not > 0 and finite, or a centre_offset that is not
 * finite; nothing asked for; audit with every field NULL. */
int btrapz_clearance_device(btrapz_ctx *ctx, const btrapz_footprint *footprint, const btrapz_obstacles *obstacles,
                            const int *scene_index, int R, int n, const double *cart, const int *count, double d_safe,
                            double *clear, int *which, const btrapz_clear_audit *audit, void *stream);

/* cart_bar [R][6][n], overwritten as a whole = the transpose of the clearance's derivative in (x, y, theta) under the
 * frozen `which` [R][n], applied to clear_bar [R][n]: rows kappa, v, a are 0, and samples not read, with a NaN pose or
 * with which = -1 are 0; whatever clear_bar holds at samples that were not read is ignored.  cart_bar feeds
 * btrapz_cartesian_vjp_device unchanged.  No obstacle loop: O(1) per sample.  The gradient with respect to the obstacles
 * is not formed in reverse mode.
 * BTRAPZ_EINVAL: as above, and which, clear_bar or cart_bar NULL. */
int btrapz_clearance_vjp_device(btrapz_ctx *ctx, const btrapz_footprint *footprint, const btrapz_obstacles *obstacles,
                                const int *scene_index, int R, int n, const double *cart, const int *count, const int *which,
                                const double *clear_bar, double *cart_bar, void *stream);

/* clear_dot [T][R][n] = the derivative under the frozen `which`, formed once per sample, applied to the T tangents
 * cart_dot [T][R][6][n] (rows x, y, theta are read) and, when obs_dot [T][n_scenes][O][3][n] is not NULL, to the
 * obstacles' tangents (NULL: the obstacles do not move).  Samples at and beyond a row's count keep what the caller put
 * there; samples with a NaN pose or which = -1 get 0.
 * BTRAPZ_EINVAL: as above, which, cart_dot or clear_dot NULL, T < 1 or T > BTRAPZ_MAX_TANGENTS. */
int btrapz_clearance_jvp_device(btrapz_ctx *ctx, const btrapz_footprint *footprint, const btrapz_obstacles *obstacles,
                                const int *scene_index, int R, int n, const double *cart, const int *count, const int *which,
                                int T, const double *cart_dot, const double *obs_dot, double *clear_dot, void *stream);

/* The same three on the host: HOST pointers throughout, no GPU, no context (a refusal returns BTRAPZ_EINVAL and nothing
 * else); they also refuse an obstacle half extent that is not > 0 and finite.  They share the per-pair statements with
 * the kernels but not sin and cos: the two are held to the same tolerance, not to each other's bits. */
int btrapz_clearance_host(const btrapz_footprint *footprint, const btrapz_obstacles *obstacles, const int *scene_index, int R,
                          int n, const double *cart, const int *count, double d_safe, double *clear, int *which,
                          const btrapz_clear_audit *audit);
int btrapz_clearance_vjp_host(const btrapz_footprint *footprint, const btrapz_obstacles *obstacles, const int *scene_index,
                              int R, int n, const double *cart, const int *count, const int *which, const double *clear_bar,
                              double *cart_bar);
int btrapz_clearance_jvp_host(const btrapz_footprint *footprint, const btrapz_obstacles *obstacles, const int *scene_index,
                              int R, int n, const double *cart, const int *count, const int *which, int T,
                              const double *cart_dot, const double *obs_dot, double *clear_dot);

#ifdef __cplusplus
}
#endif
#endif
