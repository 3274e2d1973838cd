/* btrapz_hip_cartesian.h -- batched Cartesian states of Frenet trajectories, a kinematic audit of them, and the
 * derivatives of the map: a tenth header beside btrapz_hip.h (which it includes), plain C99.
 *
 * Everything else the library returns -- control points, samples, evaluated states, scores -- is in the Frenet
 * coordinates (s, l) of a reference line.  This stage places samples in the plane: per sample the pose (x, y, theta),
 * the path curvature kappa, the speed v and the acceleration a along the path; per row the extremes a Frenet QP cannot
 * state because they are nonlinear -- |kappa|, the lateral acceleration v^2 |kappa|, and the validity of the frame
 * itself, 1 - kappa_r l > 0.
 *
 * The reference line is a table; the lookup at arc length s:
 *   i = the largest index with rs[i] <= s, clamped to M - 2;   w = (s - rs[i]) / (rs[i+1] - rs[i]);
 *   rx, ry, rkappa, rdkappa = q[i] + w (q[i+1] - q[i]);   rtheta = theta[i] + w wrap(theta[i+1] - theta[i]);
 *   wrap(a) = fmod(a + pi, 2 pi), plus 2 pi if negative, minus pi (the reference's NormalizeAngle, cart_frenet.py:193).
 * A sample is OUTSIDE when its s is below rs[0], above rs[M-1] or NaN: nothing is extrapolated.  The choice of i is a
 * decision: it is frozen in every derivative.  THE TABLE ITSELF IS NOT DIFFERENTIATED.
 *
 * The map, per sample (s, ds, dds, l, dl, ddl), in TIME derivatives -- nothing is divided by ds:
 *   c, sg = cos, sin(rtheta);   w = 1 - rkappa l;   vt = ds w;   vn = dl;
 *   at = dds w - ds^2 rdkappa l - 2 rkappa ds dl;       an = ddl + rkappa ds^2 w;
 *   x = rx - sg l;   y = ry + c l;   v = sqrt(vt^2 + vn^2);   theta = wrap(rtheta + atan2(vn, vt));
 *   a = (vt at + vn an) / v;   kappa = (vt an - vn at) / v^3.
 * For ds > 0 this is the reference's frenet_to_cartesian3D (cart_frenet.py:347-381) with d' = dl / ds and
 * d'' = (ddl - d' dds) / ds^2.
 *
 * Defined cases:
 *   - an OUTSIDE sample: NaN in all six rows of cart, 0 in f_bar and in cart_dot; counted in n_outside, it enters no
 *     extreme;
 *   - v == 0 exactly: theta = wrap(rtheta), kappa = 0, a = at; theta, kappa, v and a have zero derivative there, x and
 *     y keep theirs;
 *   - w <= 0 (beyond the centre of curvature): the formulas are regular there and are evaluated; frame_min reports it;
 *   - entries at and beyond a row's count keep what the caller put there (cart, cart_dot) or are 0 (f_bar);
 *   - a line_index outside [0, n_lines): the whole row is OUTSIDE. */
#ifndef BTRAPZ_HIP_CARTESIAN_H
#define BTRAPZ_HIP_CARTESIAN_H
#include "btrapz_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* n_lines tables of M >= 2 points each; every array is [n_lines][M].  DEVICE pointers in the *_device calls, HOST
 * pointers in the *_host calls.  rs is strictly increasing within a line: a precondition the calls do not check (a
 * table that breaks it gives meaningless values, never an access outside the table). */
typedef struct btrapz_refline {
  int n_lines;
  int M;
  const double *rs, *rx, *ry, *rtheta, *rkappa, *rdkappa;
} btrapz_refline;

/* input layouts */
#define BTRAPZ_FRENET_SAMPLES 0 /* f [R][6][n], rows (s, ds, dds, l, dl, ddl): btrapz_sample_device's out, n = max_points */
#define BTRAPZ_FRENET_STATES 1  /* f [R][2][n][3]: the x of btrapz_eval_states_device */

/* rows of cart [R][6][n] */
#define BTRAPZ_CART_X 0
#define BTRAPZ_CART_Y 1
#define BTRAPZ_CART_THETA 2
#define BTRAPZ_CART_KAPPA 3
#define BTRAPZ_CART_V 4
#define BTRAPZ_CART_A 5

/* The audit of a row, from the same launch as cart.  Pointers of the kind the call takes (device / host); any may be
 * NULL (not wanted), all NULL -> BTRAPZ_EINVAL.  The extremes are taken over the values as written to cart, over the
 * samples that are read and not OUTSIDE; a row without such a sample gets -inf for a maximum, +inf for a minimum and
 * index -1 (the "nobody" convention of btrapz_topk_device).  A value that is no number enters no extreme.
 * Order of the reduction: lane q of the row's wavefront takes the samples q, q + 64, ... in rising order, then a
 * butterfly over the lanes (xor 32 ... 1) under the total order "better value, then lower sample": no atomics, the same
 * inputs give the same bits on every run. */
typedef struct btrapz_kin_audit {
  double *kappa_abs_max; /* [R]    max |kappa| */
  double *alat_abs_max;  /* [R]    max v^2 |kappa| */
  double *a_min;         /* [R] */
  double *a_max;         /* [R] */
  double *v_max;         /* [R] */
  double *frame_min;     /* [R]    min (1 - rkappa l) */
  int    *n_outside;     /* [R]    OUTSIDE samples among those read */
  int    *worst;         /* [R][6] the sample that attains each extreme, in the order of the fields above; lowest on a tie */
} btrapz_kin_audit;

/* cart [R][6][n] (rows x, y, theta, kappa, v, a) and / or the audit of f under `layout`.  line_index [R] may be NULL
 * (every row uses line 0; used like set_index); count [R] may be NULL (every row has n samples), else only samples
 * j < min(count[r], n) are read and written, a count <= 0 is an empty row (the sampler's npoints goes here).  cart may
 * be NULL when only the audit is wanted (half the traffic); the audit's bits do not depend on it.
 * One launch, asynchronous, stream-ordered, no host round trip, no workspace.
 * BTRAPZ_EINVAL (btrapz_last_error says why): ctx, refline, one of its six arrays or f NULL; R, n or n_lines < 1; M < 2;
 * an unknown layout; cart NULL and audit NULL; audit with every field NULL. */
int btrapz_cartesian_device(btrapz_ctx *ctx, const btrapz_refline *refline, const int *line_index, int R, int n, int layout,
                            const double *f, const int *count, double *cart, const btrapz_kin_audit *audit, void *stream);

/* f_bar (the layout of f, overwritten) = the transpose of the map's 6 x 6 Jacobian per sample applied to
 * cart_bar [R][6][n]; the derivative through s goes through the interpolation, interval frozen.  Samples that were not
 * read and OUTSIDE samples get 0; whatever cart_bar holds at samples that were not read (NaN included) is ignored.
 * f_bar feeds btrapz_sample_vjp_device / btrapz_eval_states_vjp_device unchanged.
 * BTRAPZ_EINVAL: as above, and cart_bar or f_bar NULL. */
int btrapz_cartesian_vjp_device(btrapz_ctx *ctx, const btrapz_refline *refline, const int *line_index, int R, int n, int layout,
                                const double *f, const int *count, const double *cart_bar, double *f_bar, void *stream);

/* cart_dot [T][R][6][n] = the Jacobian per sample, formed once, applied to the T tangents f_dot ([T] x the layout of f).
 * Samples at and beyond a row's count keep what the caller put there; OUTSIDE samples get 0.
 * BTRAPZ_EINVAL: as above, f_dot or cart_dot NULL, T < 1 or T > BTRAPZ_MAX_TANGENTS. */
int btrapz_cartesian_jvp_device(btrapz_ctx *ctx, const btrapz_refline *refline, const int *line_index, int R, int n, int layout,
                                const double *f, const int *count, int T, const double *f_dot, double *cart_dot, void *stream);

/* The same three on the host: HOST pointers throughout, no GPU, no context (a refusal returns BTRAPZ_EINVAL and nothing
 * else).  They share the per-sample statements with the kernels but not sin, cos and atan2: the two are held to the
 * same tolerance, not to each other's bits. */
int btrapz_cartesian_host(const btrapz_refline *refline, const int *line_index, int R, int n, int layout, const double *f,
                          const int *count, double *cart, const btrapz_kin_audit *audit);
int btrapz_cartesian_vjp_host(const btrapz_refline *refline, const int *line_index, int R, int n, int layout, const double *f,
                              const int *count, const double *cart_bar, double *f_bar);
int btrapz_cartesian_jvp_host(const btrapz_refline *refline, const int *line_index, int R, int n, int layout, const double *f,
                              const int *count, int T, const double *f_dot, double *cart_dot);

#ifdef __cplusplus
}
#endif
#endif
