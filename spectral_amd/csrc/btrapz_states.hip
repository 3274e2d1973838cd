// btrapz_states.hip -- vector-Jacobian products of the two maps from control points to what a caller looks at:
// the sampled trajectory (btrapz_sample_vjp_device: transpose of sample_candidate, btrapz_kernels.hip) and the state at
// given times (btrapz_eval_states_vjp_device: transpose of eval_states_kernel, and its derivative along the trajectory).
// Both maps are linear in the control points; the Bezier conventions are the forward's: position is the Bernstein sum
// TIMES the segment duration, velocity is unscaled, acceleration is DIVIDED by the duration.
//
// Mapping: one wavefront per selection / candidate, kWaves wavefronts per workgroup, each with its own slice of LDS.
// Gather form: the pair of entries ctrl_bar[.][s axis | l axis][k][i] is owned by ONE lane, which sums the
// contributions of the samples (times) of segment k in increasing sample (time) index.  No atomics, no cross-lane
// reduction: repeated calls are bit-identical.  Lanes loop over the 6 S (segment, control point) pairs, so 256 segments
// (3 072 entries) are covered by 24 passes.
//
// Sampling: the samples of segment k are the contiguous rows base_k .. base_k + linter_k - 1 (base_k = 1 + the sum of
// the earlier segments' (int)(t / delta)), so the owner needs no search: the durations go to LDS once, with the
// exclusive prefix of the counts built by a wave scan, and the Bernstein powers of a sample live in registers.
//
// States: the times are arbitrary and unsorted.  In chunks of 64, lane j walks the durations as the forward does
// (rem > tt[k]) for time j, and leaves in LDS its segment and the 12 coefficients G[j][axis][i] = p_bar d p / d c_i +
// v_bar d v / d c_i + a_bar d a / d c_i; then the owners sum the rows whose segment is theirs.  The same lane j
// writes times_bar[j].  A later chunk adds to what its own lane wrote for the chunk before.
//
// Every wavefront of a workgroup passes the same barriers: an invalid or surplus wavefront runs the loops with S = 0.
#include <hip/hip_runtime.h>

#include <climits>

#include "btrapz_device.h"

#define UNROLL _Pragma("unroll")

namespace btrapz {

namespace {

constexpr int kWaves = kStatesWaves;
constexpr int kGStride = 13;   // 12 coefficients per time, padded: the lanes' rows fall on different banks

// d x / d c_i (before the factor t), d dx / d c_i, d ddx / d c_i (before the factor 1 / t) at parameter tau, for
// every control point: the expressions of sample_candidate / eval_states_kernel, term by term.
struct Basis {
  double d0[6], d1[6], d2[6];
};
__device__ __forceinline__ void powers(double tau, double pw[6], double qw[6]) {
  const double om = 1.0 - tau;
  pw[0] = 1.0; qw[0] = 1.0;
  UNROLL for (int q = 1; q < 6; q++) { pw[q] = pw[q - 1] * tau; qw[q] = qw[q - 1] * om; }
}
__device__ __forceinline__ Basis basis_at(double tau) {
  const double bc0[6] = {1, 5, 10, 10, 5, 1}, bc1[5] = {1, 4, 6, 4, 1}, bc2[4] = {1, 3, 3, 1};
  double pw[6], qw[6];
  powers(tau, pw, qw);
  Basis r;
  UNROLL for (int q = 0; q < 6; q++) { r.d0[q] = bc0[q] * pw[q] * qw[5 - q]; r.d1[q] = 0.0; r.d2[q] = 0.0; }
  UNROLL for (int q = 0; q < 5; q++) {
    const double b1 = 5.0 * (bc1[q] * pw[q] * qw[4 - q]);
    r.d1[q + 1] += b1; r.d1[q] -= b1;
  }
  UNROLL for (int q = 0; q < 4; q++) {
    const double b2 = 20.0 * (bc2[q] * pw[q] * qw[3 - q]);
    r.d2[q + 2] += b2; r.d2[q + 1] -= 2.0 * b2; r.d2[q] += b2;
  }
  return r;
}
// ... and of one control point jc (a lane's own), without indexing a register array by a variable
__device__ __forceinline__ void basis_of(double tau, int jc, double &d0, double &d1, double &d2) {
  const double bc0[6] = {1, 5, 10, 10, 5, 1}, bc1[5] = {1, 4, 6, 4, 1}, bc2[4] = {1, 3, 3, 1};
  double pw[6], qw[6];
  powers(tau, pw, qw);
  d0 = 0.0; d1 = 0.0; d2 = 0.0;
  UNROLL for (int q = 0; q < 6; q++) if (q == jc) d0 = bc0[q] * pw[q] * qw[5 - q];
  UNROLL for (int q = 0; q < 5; q++) {
    const double b1 = 5.0 * (bc1[q] * pw[q] * qw[4 - q]);
    if (q + 1 == jc) d1 += b1;
    if (q == jc) d1 -= b1;
  }
  UNROLL for (int q = 0; q < 4; q++) {
    const double b2 = 20.0 * (bc2[q] * pw[q] * qw[3 - q]);
    if (q + 2 == jc) d2 += b2;
    if (q + 1 == jc) d2 -= 2.0 * b2;
    if (q == jc) d2 += b2;
  }
}

// (int)(t / delta) as the forward takes it, for the durations the forward is defined on; a duration that is not > 0
// (find_traj refuses such a corridor) has no samples, and a quotient beyond int saturates.
__device__ __forceinline__ int count_of(double t, double delta) {
  if (!(t > 0.0)) return 0;
  const double x = t / delta;
  return x < 2147483647.0 ? (int)x : INT_MAX;
}

}  // namespace

__global__ __launch_bounds__(64 * kStatesWaves) void sample_vjp_kernel(const SampleVjpArgs a) {
  __shared__ double tseg_[kWaves][BTRAPZ_MAX_SEGMENTS_LONG];
  __shared__ int pre_[kWaves][BTRAPZ_MAX_SEGMENTS_LONG + 1];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  double *tseg = tseg_[wave];
  int *pre = pre_[wave];   // pre[k]: samples before segment k, saturated at max_points (rows beyond are not written)
  const long long j = (long long)blockIdx.x * kWaves + wave;
  const bool active = j < a.nsel;
  const long long b = active ? a.sel[j] : -1;
  int S = 0;
  if (b >= 0 && b < a.B) {
    S = a.seg_count ? a.seg_count[b] : a.seg_stride;
    if (S < 1 || S > a.seg_stride) S = 0;   // the forward answers npoints = 0
  }
  const int lim = a.max_points;
  {
    const double *tt = a.seg + (size_t)BTRAPZ_F_T * a.B * a.seg_stride + (size_t)(S ? b : 0) * a.seg_stride;
    long long carry = 0;
    for (int k0 = 0; k0 < S; k0 += 64) {
      const int k = k0 + lane;
      long long inc = 0;
      if (k < S) {
        const double t = tt[k];
        tseg[k] = t;
        inc = count_of(t, a.delta);
      }
      UNROLL for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
      }
      if (k < S) { const long long p = carry + inc; pre[k + 1] = p < lim ? (int)p : lim; }
      carry += __shfl(inc, 63);
    }
    if (lane == 0) pre[0] = 0;
  }
  __syncthreads();
  if (!active) return;
  const double *ob = a.out_bar + (size_t)j * 6 * lim;
  // sample 0 is init: its cotangent goes to init_bar and nowhere else
  if (a.init_bar && lane < 6) a.init_bar[j * 6 + lane] = S ? ob[(size_t)lane * lim] : 0.0;
  if (!a.ctrl_bar) return;
  double *cb = a.ctrl_bar + (size_t)j * 12 * a.seg_stride;
  // The forward's npoints never cuts a written row off: it accumulates 1 + sum t_k / delta in double with a truncation
  // per step, and rounding is monotone, so it is at least 1 + sum (int)(t_k / delta), the last row the forward writes.
  // Rows at and beyond max_points were not written: pre saturates there.
  for (int e = lane; e < 6 * S; e += 64) {
    const int k = e / 6, jc = e - 6 * k;
    const double t = tseg[k];
    const int linter = count_of(t, a.delta);
    const int base = 1 + pre[k];                    // row of the segment's first sample
    const int n = linter < lim - base ? linter : lim - base;
    double acc0 = 0.0, acc1 = 0.0;
    for (int l = 1; l <= n; l++) {
      const int vi = base + l - 1;
      double d0, d1, d2;
      basis_of((double)l / (double)linter, jc, d0, d1, d2);
      d0 *= t; d2 /= t;
      acc0 += ob[vi] * d0 + ob[(size_t)lim + vi] * d1 + ob[(size_t)2 * lim + vi] * d2;
      acc1 += ob[(size_t)3 * lim + vi] * d0 + ob[(size_t)4 * lim + vi] * d1 + ob[(size_t)5 * lim + vi] * d2;
    }
    cb[e] = acc0;
    cb[(size_t)6 * S + e] = acc1;
  }
  for (int q = 12 * S + lane; q < 12 * a.seg_stride; q += 64) cb[q] = 0.0;
}

__global__ __launch_bounds__(64 * kStatesWaves) void eval_states_vjp_kernel(const StatesVjpArgs a) {
  __shared__ double tseg_[kWaves][BTRAPZ_MAX_SEGMENTS_LONG];
  __shared__ double g_[kWaves][64 * kGStride];
  __shared__ int kk_[kWaves][64];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  double *tseg = tseg_[wave];
  double *G = g_[wave];
  int *kk = kk_[wave];
  const long long b = (long long)blockIdx.x * kWaves + wave;
  const bool active = b < a.B;
  int S = 0;
  if (active) {
    S = a.seg_count ? a.seg_count[b] : a.seg_stride;
    if (S < 1 || S > a.seg_stride) S = 0;   // the forward writes NaN
  }
  const int nt = a.n_times;
  double *cb = active && a.ctrl_bar ? a.ctrl_bar + (size_t)b * 12 * a.seg_stride : nullptr;
  double *tb = active && a.times_bar ? a.times_bar + (size_t)b * nt : nullptr;
  if (S == 0) {
    if (cb) for (int q = lane; q < 12 * a.seg_stride; q += 64) cb[q] = 0.0;
    if (tb) for (int q = lane; q < nt; q += 64) tb[q] = 0.0;
  } else {
    const double *tt = a.seg + (size_t)BTRAPZ_F_T * a.B * a.seg_stride + (size_t)b * a.seg_stride;
    for (int k = lane; k < S; k += 64) tseg[k] = tt[k];
  }
  __syncthreads();
  for (int c0 = 0; c0 < nt; c0 += 64) {
    const int j = c0 + lane;
    if (S > 0 && j < nt) {
      // the forward's branches, statement by statement
      double rem = a.times[(size_t)b * nt + j];
      const bool clamped = !(rem > 0.0);
      if (clamped) rem = 0.0;
      int k = 0;
      while (k < S - 1 && rem > tseg[k]) { rem -= tseg[k]; ++k; }
      const double t = tseg[k];
      const double over = rem > t ? rem - t : 0.0;     // beyond the horizon
      const bool beyond = over > 0.0;
      const double tau = beyond ? 1.0 : rem / t;
      const Basis h = basis_at(tau);
      const double *xb = a.x_bar + ((size_t)b * 2 * nt + j) * 3;
      double tbar = 0.0;
      UNROLL for (int ax = 0; ax < 2; ax++) {
        const double pb = xb[(size_t)ax * nt * 3], vb = xb[(size_t)ax * nt * 3 + 1], ab = xb[(size_t)ax * nt * 3 + 2];
        // p = t sum c d0 + over sum c d1, v = sum c d1, a = beyond ? 0 : sum c d2 / t
        UNROLL for (int i = 0; i < 6; i++) {
          double g = pb * (t * h.d0[i] + over * h.d1[i]) + vb * h.d1[i];
          if (!beyond) g += ab * (h.d2[i] / t);
          G[lane * kGStride + 6 * ax + i] = g;
        }
        if (tb && !clamped) {
          // along the trajectory: dp/dt = v, dv/dt = a, da/dt = the jerk (third derivative / t^2); beyond the horizon
          // p moves with the end velocity and v, a stand still
          const double *c = a.ctrl + (size_t)b * 12 * a.seg_stride + (size_t)ax * 6 * S + (size_t)k * 6;
          double cc[6];
          UNROLL for (int i = 0; i < 6; i++) cc[i] = c[i];
          double v = 0.0, acc = 0.0;
          UNROLL for (int i = 0; i < 6; i++) { v += cc[i] * h.d1[i]; acc += cc[i] * h.d2[i]; }
          if (beyond) {
            tbar += pb * v;
          } else {
            const double om = 1.0 - tau;
            const double b2[3] = {om * om, 2.0 * tau * om, tau * tau};
            double jerk = 0.0;
            UNROLL for (int i = 0; i < 3; i++) jerk += 60.0 * (cc[i + 3] - 3.0 * cc[i + 2] + 3.0 * cc[i + 1] - cc[i]) * b2[i];
            tbar += pb * v + vb * (acc / t) + ab * (jerk / (t * t));
          }
        }
      }
      kk[lane] = k;
      if (tb) tb[j] = tbar;
    }
    __syncthreads();
    if (cb) {
      const int m = nt - c0 < 64 ? nt - c0 : 64;
      for (int e = lane; e < 6 * S; e += 64) {
        const int k = e / 6, jc = e - 6 * k;
        double acc0 = c0 ? cb[e] : 0.0, acc1 = c0 ? cb[(size_t)6 * S + e] : 0.0;
        for (int q = 0; q < m; q++)
          if (kk[q] == k) { acc0 += G[q * kGStride + jc]; acc1 += G[q * kGStride + 6 + jc]; }
        cb[e] = acc0;
        cb[(size_t)6 * S + e] = acc1;
      }
    }
    __syncthreads();
  }
  if (cb && S > 0)
    for (int q = 12 * S + lane; q < 12 * a.seg_stride; q += 64) cb[q] = 0.0;
}

}  // namespace btrapz
