/* btrapz_hip_frenet.h -- batched Cartesian states projected onto the reference line, and the derivatives of that map
 * (DESIGN.md 3.20): an eleventh header beside btrapz_hip_cartesian.h (which it includes for btrapz_refline, the layouts
 * and the row names), plain C99.
 *
 * It is the inverse of btrapz_cartesian_device on the same table: a pose in the plane (x, y, theta, kappa, v, a) goes to
 * the Frenet state (s, ds, dds, l, dl, ddl) that every entry point which starts a plan takes.  The matched point on the
 * line -- which the reference's cartesian_to_frenet1D / 2D / 3D (cart_frenet.py:205-344) leave to the caller -- is found
 * here, per query p = (x, y):
 *
 * 1. Coarse pass.  At every table point g_i = (x - rx_i) cos rtheta_i + (y - ry_i) sin rtheta_i.  Interval i
 *    (0 <= i <= M - 2) is a CANDIDATE when g_i >= 0 and g_{i+1} < 0; interval M - 2 also when g_i >= 0 and g_{i+1} == 0
 *    (the half-open rule of the forward's lookup, "the largest i with rs[i] <= s, clamped to M - 2").  With a window
 *    s_window[r] = (lo, hi) only intervals with rs[i+1] >= lo and rs[i] <= hi count.  The winner is the candidate with
 *    the smallest squared chord distance |p - r_i - t e_i|^2, e_i = r_{i+1} - r_i, t = clamp((p - r_i) . e_i / |e_i|^2,
 *    0, 1); a tie goes to the lowest i.  The query is OUTSIDE when there is no candidate, x or y is NaN, a window entry
 *    is NaN or lo > hi, or line_index is outside [0, n_lines): nothing is extrapolated.  A - -> + change (a point beyond
 *    the centre of curvature) is deliberately no candidate.
 * 2. Refinement.  The root w in [0, 1] of g(w) = (p - r(w)) . (cos theta(w), sin theta(w)), r and theta interpolated
 *    exactly as the forward's lookup does (theta(w) = theta_i + w wrap(theta_{i+1} - theta_i)): safeguarded Newton on the
 *    bracket [0, 1] from the secant point g_i / (g_i - g_{i+1}); a step that leaves the bracket, or a zero slope, is
 *    replaced by a bisection step; at most 64 steps.  The contract is the tolerance of DESIGN 3.20, not the iteration.
 *    s = rs_i + w (rs_{i+1} - rs_i);  l = (y - r_y) cos theta - (x - r_x) sin theta.
 *    btrapz_cartesian_device of the result returns p up to rounding (a chord-foot projection would miss by O(l kappa h)).
 * 3. Map, in TIME derivatives, regular for every heading difference -- nothing is divided by a cosine:
 *      D = theta - theta(w);  om = 1 - rkappa l;  vt = v cos D;  vn = v sin D;  ds = vt / om;  dl = vn;
 *      at = a cos D - v^2 kappa sin D;  an = a sin D + v^2 kappa cos D;
 *      dds = (at + ds^2 rdkappa l + 2 rkappa ds dl) / om;   ddl = an - rkappa ds^2 om.
 *    For cos D > 0 this is the reference's cartesian_to_frenet3D with d' = dl / ds, d'' = (ddl - d' dds) / ds^2.
 *    A departure: the reference sets l = 0 when the distance is below 0.01.  That snap is NOT kept: it breaks the round
 *    trip and the derivative.
 *
 * order = 0, 1 or 2 follows the reference's 1D / 2D / 3D trio: rows of cart above the order are not read and the outputs
 * above the order are 0.  Order 0 reads x and y and gives s and l; order 1 also reads theta and v and gives ds and dl
 * (what an obstacle needs); order 2 reads and gives everything.
 *
 * Defined cases:
 *   - an OUTSIDE sample: NaN in all six outputs, interval = -1, counted in n_outside, 0 in every derivative;
 *   - om == 0: IEEE results as they fall;
 *   - om <= 0 cannot be the winner of a + -> - change unless rkappa disagrees with the slope of rtheta; it is evaluated,
 *     not refused;
 *   - entries at and beyond a row's count keep the caller's contents (frenet, interval, frenet_dot) or are 0 (cart_bar);
 *   - v == 0 is regular here, unlike the forward. */
#ifndef BTRAPZ_HIP_FRENET_H
#define BTRAPZ_HIP_FRENET_H
#include "btrapz_hip_cartesian.h"
#ifdef __cplusplus
extern "C" {
#endif

/* cart [R][6][n] (rows x, y, theta, kappa, v, a: btrapz_cartesian_device's output) -> frenet under `layout`
 * (BTRAPZ_FRENET_SAMPLES [R][6][n] or BTRAPZ_FRENET_STATES [R][2][n][3]).  line_index [R] and count [R] as in
 * btrapz_cartesian_device (NULL: line 0 / n samples).  s_window [R][2] = (lo, hi) per row, or NULL (the whole line).
 * interval [R][n] (int: the winner's i, -1 OUTSIDE) and n_outside [R] (int: OUTSIDE samples among those read) are
 * optional (NULL: not wanted); the derivatives below need interval.
 * One launch, asynchronous, stream-ordered, no workspace, no host round trip, no atomics: the same inputs give the
 * same bits on every run.
 * BTRAPZ_EINVAL (btrapz_last_error says why): ctx, refline, one of its six arrays, cart or frenet NULL; R, n or n_lines
 * < 1; M < 2; an unknown layout; order outside 0 .. 2. */
int btrapz_frenet_device(btrapz_ctx *ctx, const btrapz_refline *refline, const int *line_index, int R, int n, int layout,
                         int order, const double *cart, const int *count, const double *s_window, double *frenet,
                         int *interval, int *n_outside, void *stream);

/* cart_bar [R][6][n] (overwritten) = the transpose of the map's 6 x 6 Jacobian per sample applied to frenet_bar (the
 * layout of frenet).  cart, frenet and interval are the forward's: nothing is searched or refined again.  The interval
 * is frozen and THE TABLE IS NOT DIFFERENTIATED.  Samples that were not read and OUTSIDE samples (interval outside
 * [0, M - 2]) get 0; whatever frenet_bar holds there is ignored.  Rows of cart_bar above the order are 0.
 * BTRAPZ_EINVAL: as above, and interval, frenet_bar or cart_bar NULL. */
int btrapz_frenet_vjp_device(btrapz_ctx *ctx, const btrapz_refline *refline, const int *line_index, int R, int n, int layout,
                             int order, const double *cart, const double *frenet, const int *interval, const int *count,
                             const double *frenet_bar, double *cart_bar, void *stream);

/* frenet_dot ([T] x the layout of frenet) = the Jacobian per sample, formed once, applied to the T tangents
 * cart_dot [T][R][6][n].  Samples at and beyond a row's count keep what the caller put there; OUTSIDE samples get 0.
 * BTRAPZ_EINVAL: as above, cart_dot or frenet_dot NULL, T < 1 or T > BTRAPZ_MAX_TANGENTS. */
int btrapz_frenet_jvp_device(btrapz_ctx *ctx, const btrapz_refline *refline, const int *line_index, int R, int n, int layout,
                             int order, const double *cart, const double *frenet, const int *interval, const int *count,
                             int T, const double *cart_dot, double *frenet_dot, void *stream);

/* The same three on the host: HOST pointers throughout, no GPU, no context (a refusal returns BTRAPZ_EINVAL and nothing
 * else).  They share the per-sample statements with the kernels but not sin and cos: the two are held to the same
 * tolerance, not to each other's bits. */
int btrapz_frenet_host(const btrapz_refline *refline, const int *line_index, int R, int n, int layout, int order,
                       const double *cart, const int *count, const double *s_window, double *frenet, int *interval,
                       int *n_outside);
int btrapz_frenet_vjp_host(const btrapz_refline *refline, const int *line_index, int R, int n, int layout, int order,
                           const double *cart, const double *frenet, const int *interval, const int *count,
                           const double *frenet_bar, double *cart_bar);
int btrapz_frenet_jvp_host(const btrapz_refline *refline, const int *line_index, int R, int n, int layout, int order,
                           const double *cart, const double *frenet, const int *interval, const int *count, int T,
                           const double *cart_dot, double *frenet_dot);

#ifdef __cplusplus
}
#endif
#endif
