// btrapz_acost.hip -- a_cost of sampled trajectories (btrapz_traj_cost_device) and its vector-Jacobian product
// (btrapz_traj_cost_vjp_device): trajectory_cost() of traj_cost.h on the samples sample_candidate() (btrapz_kernels.hip)
// produces, for a batch of candidates.
//
// Mapping: one wavefront (workgroup of 64) per candidate.  The segment durations go to LDS, with the exclusive prefix of
// the per-segment sample counts (int)(t_k / delta) built by a wave scan; a sample finds its segment there by binary
// search.  The samples are walked in chunks: lane l of the chunk that starts at c0 evaluates sample i = c0 + l - 1, lanes
// 1..62 OWN their sample and lanes 0 and 63 are halos, so an owner reads its neighbours' dds / ddl (the jerk terms, and
// their derivatives) by a shuffle.  Reference reads s_ref[i] / l_ref[i] are consecutive over the lanes.  Sums and maxima
// are per lane in sample order, then reduced by a fixed butterfly: repeated calls are bit-identical.
//
// The VJP walks the same chunks: every owner turns d a_cost / d(its sample) into the cotangents of the sample's
// (x, dx, ddx) per axis and leaves them in LDS; then lanes (segment, control point) -- six per segment, both axes --
// sum the samples of their segment (in sample order) into ctrl_bar.  A segment that continues into the next chunk carries
// its partial sums in LDS.  No atomics.  The cuboid's max terms are differentiated at the first index that attains the
// maximum, found by a first pass over the samples.
#include <hip/hip_runtime.h>

#include <climits>

#include "btrapz_device.h"

#define UNROLL _Pragma("unroll")

namespace btrapz {

namespace {

constexpr int kOwn = 62;   // samples owned per chunk (64 lanes less the two halos)

__device__ __forceinline__ double wave_sum(double v) {
  UNROLL for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// (value, index) of the largest value, the smallest index on a tie
__device__ __forceinline__ void wave_argmax(double &v, int &i) {
  UNROLL for (int m = 32; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(v, m);
    const int oi = __shfl_xor(i, m);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// What every candidate needs before its samples: its layout, its set, and whether it is scored.
struct Cand {
  int S, np, set;
  bool ok;
};

// Loads the candidate's durations into tseg[0..S), the exclusive prefix of the per-segment sample counts into
// pre[0..S] (pre[S] = total), the quotients t_k / delta into xq, and checks what makes the candidate scored.  Every lane returns the same.
__device__ Cand setup(const AcostArgs &a, long long b, int lane, double *tseg, double *xq, int *pre, int *flag) {
  Cand c;
  c.S = a.seg_count ? a.seg_count[b] : a.seg_stride;
  c.np = 0;
  c.set = a.set_index ? a.set_index[b] : 0;
  c.ok = c.S >= 1 && c.S <= a.seg_stride && c.set >= 0 && c.set < a.n_sets;
  if (c.ok && a.status) { const int st = a.status[b]; c.ok = st == 1 || st == 2; }
  if (!c.ok) return c;
  const double *tt = a.seg + (size_t)BTRAPZ_F_T * a.B * a.seg_stride + (size_t)b * a.seg_stride;
  const double delta = a.delta;
  int carry = 0;
  bool bad = false;
  for (int k0 = 0; k0 < c.S; k0 += 64) {
    const int k = k0 + lane;
    int lin = 0;
    if (k < c.S) {
      const double t = tt[k];
      const double x = t / delta;
      tseg[k] = t;
      xq[k] = x;
      bad |= !(t > 0.0);   // (find_traj refuses such a corridor)
      lin = (int)x;
    }
    int inc = lin;   // inclusive scan over the wave
    UNROLL for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (k < c.S) pre[k + 1] = carry + inc;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) pre[0] = 0;
  bad = __any(bad);
  __syncthreads();
  // num_of_points_: int accumulated with += double (solve_3d.cc:1279-1282), against the int sum (:1407)
  if (lane == 0) {
    int np = 1;
    for (int k = 0; k < c.S; k++) np = (int)((double)np + xq[k]);   // (xq[k] = tseg[k] / delta, staged above)
    *flag = np;
  }
  __syncthreads();
  const int np = *flag;
  c.ok = !bad && np == 1 + pre[c.S] && np >= 1;
  c.np = np;
  return c;
}

// Segment of sample idx (0-based, after the initial state): the last k with pre[k] <= idx.
__device__ __forceinline__ int segment_of(const int *pre, int S, int idx) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Sample i of candidate b: s, ds, dds, l, dl, ddl -- the expressions of sample_candidate, in its order.
__device__ __forceinline__ void sample_at(const AcostArgs &a, long long b, int S, const double *tseg, const int *pre, int i,
                                          double v[6]) {
  if (i == 0) {
    UNROLL for (int q = 0; q < 6; q++) v[q] = a.init[b * 6 + q];
    return;
  }
  const int idx = i - 1;
  const int k = segment_of(pre, S, idx);
  const int linter = pre[k + 1] - pre[k];
  const double t = tseg[k];
  const int l = idx - pre[k] + 1;
  const double tau = (double)l / (double)linter, om = 1.0 - tau;
  const double bc0[6] = {1, 5, 10, 10, 5, 1}, bc1[5] = {1, 4, 6, 4, 1}, bc2[4] = {1, 3, 3, 1};
  double pw[6], qw[6];
  pw[0] = 1.0; qw[0] = 1.0;
  UNROLL for (int q = 1; q < 6; q++) { pw[q] = pw[q - 1] * tau; qw[q] = qw[q - 1] * om; }
  UNROLL for (int ax = 0; ax < 2; ax++) {
    const double *c = a.ctrl + (size_t)b * 12 * a.seg_stride + (size_t)ax * 6 * S + (size_t)k * 6;
    double x = 0, dx = 0, ddx = 0;
    UNROLL for (int q = 0; q < 6; q++) x += c[q] * bc0[q] * pw[q] * qw[5 - q];
    UNROLL for (int q = 0; q < 5; q++) dx += 5.0 * (c[q + 1] - c[q]) * bc1[q] * pw[q] * qw[4 - q];
    UNROLL for (int q = 0; q < 4; q++) ddx += 20.0 * (c[q + 2] - 2.0 * c[q + 1] + c[q]) * bc2[q] * pw[q] * qw[3 - q];
    v[3 * ax + 0] = x * t;
    v[3 * ax + 1] = dx;
    v[3 * ax + 2] = ddx / t;
  }
}

// One chunk's sample at lane `lane` and the dds / ddl of its neighbours.
struct Chunk {
  int i;
  bool own;
  double v[6];
  double prev[2], next[2];   // dds, ddl of samples i - 1 and i + 1 (valid where those exist)
};
__device__ __forceinline__ Chunk chunk_at(const AcostArgs &a, long long b, const Cand &c, const double *tseg, const int *pre,
                                          int c0, int lane) {
  Chunk h;
  h.i = c0 + lane - 1;
  const bool have = h.i >= 0 && h.i < c.np;
  h.own = have && lane >= 1 && lane <= kOwn;
  UNROLL for (int q = 0; q < 6; q++) h.v[q] = 0.0;
  if (have) sample_at(a, b, c.S, tseg, pre, h.i, h.v);
  UNROLL for (int ax = 0; ax < 2; ax++) {
    h.prev[ax] = __shfl_up(h.v[3 * ax + 2], 1);
    h.next[ax] = __shfl_down(h.v[3 * ax + 2], 1);
  }
  return h;
}

// The jerk of sample i (trajectory_cost: (dd[1] - dd[0]) / dt at i = 0, (dd[i] - dd[i - 1]) / dt after)
__device__ __forceinline__ double jerk_of(int i, int np, double dd, double prev, double next, double dt) {
  return i == 0 ? ((np > 1 ? next : dd) - dd) / dt : (dd - prev) / dt;
}

// Per-candidate sums: T[0..3] s axis (reference error, speed, acceleration, jerk), T[4..7] l axis, T[8] the end term;
// the cuboid's acceleration and jerk sums of the s axis are of fourth powers.  mx / mi: max |dds|, |ddl| and where.
struct Sums {
  double T[9];
  double mx[2];
  int mi[2];
};

__device__ __forceinline__ void add_terms(const AcostArgs &a, long long b, const Cand &c, const Chunk &h, Sums &s) {
  const double dt = a.delta;
  const int N = a.N;
  const int ri = h.i < N - 1 ? h.i : N - 1;
  const size_t rb = (size_t)b * a.ref_stride;
  UNROLL for (int ax = 0; ax < 2; ax++) {
    const double x = h.v[3 * ax], dx = h.v[3 * ax + 1], ddx = h.v[3 * ax + 2];
    const double e = x - (ax == 0 ? a.s_ref : a.l_ref)[rb + ri];
    const double j = jerk_of(h.i, c.np, ddx, h.prev[ax], h.next[ax], dt);
    s.T[4 * ax + 0] += e * e * dt;
    s.T[4 * ax + 1] += dx * dx * dt;
    if (a.variant == BTRAPZ_CUBOID && ax == 0) {
      s.T[2] += ddx * ddx * ddx * ddx * dt;
      s.T[3] += j * j * j * j * dt;
    } else {
      s.T[4 * ax + 2] += ddx * ddx * dt;
      s.T[4 * ax + 3] += j * j * dt;
    }
    const double m = fabs(ddx);
    if (m > s.mx[ax]) { s.mx[ax] = m; s.mi[ax] = h.i; }
  }
  if (a.variant == BTRAPZ_TRAPEZOID && h.i == (N - 1 < c.np - 1 ? N - 1 : c.np - 1)) {
    const double e = h.v[3] - a.l_ref[rb + N - 1];
    s.T[8] += e * e * dt;
  }
}

__device__ __forceinline__ void init_sums(Sums &s) {
  UNROLL for (int q = 0; q < 9; q++) s.T[q] = 0.0;
  s.mx[0] = s.mx[1] = 0.0;
  s.mi[0] = s.mi[1] = INT_MAX;
}
__device__ __forceinline__ void reduce_sums(Sums &s) {
  UNROLL for (int q = 0; q < 9; q++) s.T[q] = wave_sum(s.T[q]);
  wave_argmax(s.mx[0], s.mi[0]);
  wave_argmax(s.mx[1], s.mi[1]);
}

__device__ __forceinline__ double cost_of(const AcostArgs &a, const Shared &p, const Sums &s) {
  if (a.variant == BTRAPZ_TRAPEZOID) {
    const double sc = p.w_s[0] * s.T[0] + p.w_s[1] * s.T[1] + p.w_s[2] * s.T[2] + p.w_s[3] * s.T[3];
    const double lc = p.w_l[0] * s.T[4] + p.w_l[1] * s.T[5] + p.w_l[2] * s.T[6] + p.w_l[3] * s.T[7] + p.weight_end_l * s.T[8];
    return sc + lc;
  }
  const double m2 = s.mx[0] * s.mx[0];
  const double sc = s.T[0] + s.T[1] + s.T[2] + s.T[3] + m2 * m2;
  const double lc = s.T[4] + s.T[5] + s.T[6] + s.T[7] + s.mx[1] * s.mx[1];
  return sc + lc;
}

__device__ __forceinline__ double sgn(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

}  // namespace

__global__ __launch_bounds__(64) void acost_kernel(const AcostArgs a) {
  __shared__ double tseg[BTRAPZ_MAX_SEGMENTS_LONG], xq[BTRAPZ_MAX_SEGMENTS_LONG];
  __shared__ int pre[BTRAPZ_MAX_SEGMENTS_LONG + 1];
  __shared__ int flag;
  const long long b = blockIdx.x;
  const int lane = (int)threadIdx.x;
  const Cand c = setup(a, b, lane, tseg, xq, pre, &flag);
  if (!c.ok) {
    if (lane == 0) { a.a_cost[b] = __builtin_huge_val(); if (a.n_points) a.n_points[b] = 0; }
    return;
  }
  Sums s;
  init_sums(s);
  for (int c0 = 0; c0 < c.np; c0 += kOwn) {
    const Chunk h = chunk_at(a, b, c, tseg, pre, c0, lane);
    if (h.own) add_terms(a, b, c, h, s);
  }
  reduce_sums(s);
  if (lane == 0) {
    a.a_cost[b] = cost_of(a, a.sets[c.set], s);
    if (a.n_points) a.n_points[b] = c.np;
  }
}

__global__ __launch_bounds__(64) void acost_vjp_kernel(const AcostArgs a) {
  __shared__ double tseg[BTRAPZ_MAX_SEGMENTS_LONG], xq[BTRAPZ_MAX_SEGMENTS_LONG];
  __shared__ int pre[BTRAPZ_MAX_SEGMENTS_LONG + 1];
  __shared__ int flag;
  __shared__ double gbuf[64][6];     // cotangents of the chunk's samples: x, dx, ddx of the s axis, then the l axis
  __shared__ double carry[6][2];     // partial ctrl_bar of a segment that continues into the next chunk
  const long long b = blockIdx.x;
  const int lane = (int)threadIdx.x;
  const Cand c = setup(a, b, lane, tseg, xq, pre, &flag);
  const int N = a.N, S = c.S;
  double *cb = a.ctrl_bar ? a.ctrl_bar + (size_t)b * 12 * a.seg_stride : nullptr;
  double *gs = a.s_ref_bar ? a.s_ref_bar + (size_t)b * N : nullptr;
  double *gl = a.l_ref_bar ? a.l_ref_bar + (size_t)b * N : nullptr;
  if (!c.ok) {
    if (cb) for (int q = lane; q < 12 * a.seg_stride; q += 64) cb[q] = 0.0;
    if (gs) for (int q = lane; q < N; q += 64) gs[q] = 0.0;
    if (gl) for (int q = lane; q < N; q += 64) gl[q] = 0.0;
    if (a.init_bar && lane < 6) a.init_bar[b * 6 + lane] = 0.0;
    if (a.params_bar && lane < 20) a.params_bar[b * 20 + lane] = 0.0;
    return;
  }
  const Shared &p = a.sets[c.set];
  const bool cub = a.variant == BTRAPZ_CUBOID;
  const double dt = a.delta, abar = a.a_cost_bar[b];
  // the cuboid's max terms: where the maxima are, before any cotangent
  Sums m;
  init_sums(m);
  if (cub) {
    for (int c0 = 0; c0 < c.np; c0 += kOwn) {
      const Chunk h = chunk_at(a, b, c, tseg, pre, c0, lane);
      if (h.own)
        UNROLL for (int ax = 0; ax < 2; ax++) {
          const double v = fabs(h.v[3 * ax + 2]);
          if (v > m.mx[ax]) { m.mx[ax] = v; m.mi[ax] = h.i; }
        }
    }
    wave_argmax(m.mx[0], m.mi[0]);
    wave_argmax(m.mx[1], m.mi[1]);
  }
  // weights of the terms: w[ax][term]; the cuboid scores without weights
  double w[2][4];
  UNROLL for (int q = 0; q < 4; q++) { w[0][q] = cub ? 1.0 : p.w_s[q]; w[1][q] = cub ? 1.0 : p.w_l[q]; }
  const double w_end = cub ? 0.0 : p.weight_end_l;
  const int i_end = N - 1 < c.np - 1 ? N - 1 : c.np - 1;
  const size_t rb = (size_t)b * a.ref_stride;
  Sums s;
  init_sums(s);
  double clamp_bar[2] = {0.0, 0.0};   // what the clamped reads put on s_ref[N-1] / l_ref[N-1]
  int k_next = 0;                     // first segment whose ctrl_bar is not written yet
  bool has_carry = false;
  const int o = lane / 6, jc = lane - 6 * (lane / 6);   // (segment in the pass, control point) of this lane
  for (int c0 = 0; c0 < c.np; c0 += kOwn) {
    const Chunk h = chunk_at(a, b, c, tseg, pre, c0, lane);
    if (h.own) {
      add_terms(a, b, c, h, s);
      const int ri = h.i < N - 1 ? h.i : N - 1;
      double g[6];
      UNROLL for (int ax = 0; ax < 2; ax++) {
        const double x = h.v[3 * ax], dx = h.v[3 * ax + 1], dd = h.v[3 * ax + 2];
        const double e = x - (ax == 0 ? a.s_ref : a.l_ref)[rb + ri];
        double ge = abar * w[ax][0] * 2.0 * e * dt;
        g[3 * ax + 1] = abar * w[ax][1] * 2.0 * dx * dt;
        const bool quartic = cub && ax == 0;
        double gdd = abar * w[ax][2] * (quartic ? 4.0 * dd * dd * dd : 2.0 * dd) * dt;
        // jerk terms: q(J) = d(w J^2 dt)/dJ * (1 / dt), J_0 = J_1 (both (dd[1] - dd[0]) / dt)
        auto qj = [&](double J) { return abar * w[ax][3] * (quartic ? 4.0 * J * J * J : 2.0 * J) * dt / dt; };
        const int i = h.i;
        if (i == 0) {
          if (c.np > 1) { const double q1 = qj((h.next[ax] - dd) / dt); gdd -= q1 + q1; }
        } else {
          const double qi = qj((dd - h.prev[ax]) / dt);
          gdd += qi;
          if (i == 1) gdd += qi;
          if (i + 1 < c.np) gdd -= qj((h.next[ax] - dd) / dt);
        }
        if (cub && i == m.mi[ax]) {
          const double M = m.mx[ax];
          gdd += abar * (ax == 0 ? 4.0 * M * M * M : 2.0 * M) * sgn(dd);
        }
        double *gref = ax == 0 ? gs : gl;
        if (ax == 1 && i == i_end) {
          const double ee = x - a.l_ref[rb + N - 1];
          const double gend = abar * w_end * 2.0 * ee * dt;
          ge += gend;
          clamp_bar[1] -= gend;
        }
        // the reference line: its own sample's term (the end term went to clamp_bar above)
        const double gr = -(abar * w[ax][0] * 2.0 * e * dt);
        if (i < N - 1) { if (gref) gref[i] = gr; } else clamp_bar[ax] += gr;
        g[3 * ax + 0] = ge;
        g[3 * ax + 2] = gdd;
      }
      if (h.i == 0) {
        if (a.init_bar) UNROLL for (int q = 0; q < 6; q++) a.init_bar[b * 6 + q] = g[q];
      } else {
        UNROLL for (int q = 0; q < 6; q++) gbuf[lane][q] = g[q];
      }
    }
    __syncthreads();
    // ctrl_bar of the segments whose samples this chunk owns (samples idx = i - 1 of i in [max(c0, 1), hi])
    const int ilo = c0 > 1 ? c0 : 1;
    const int ihi = (c0 + kOwn < c.np ? c0 + kOwn : c.np) - 1;
    if (cb && ilo <= ihi) {
      const int idx_lo = ilo - 1, idx_hi = ihi - 1;
      const int k_hi = segment_of(pre, S, idx_hi);
      const bool hi_done = pre[k_hi + 1] <= idx_hi + 1;
      for (int kb = k_next; kb <= k_hi; kb += 10) {
        const int k = kb + o;
        if (o < 10 && k <= k_hi) {
          double acc[2] = {0.0, 0.0};
          if (has_carry && k == k_next) { acc[0] = carry[jc][0]; acc[1] = carry[jc][1]; }
          const int linter = pre[k + 1] - pre[k];
          const double t = tseg[k];
          const int s_lo = pre[k] > idx_lo ? pre[k] : idx_lo;
          const int s_hi = pre[k + 1] < idx_hi + 1 ? pre[k + 1] : idx_hi + 1;
          const double bc0[6] = {1, 5, 10, 10, 5, 1}, bc1[5] = {1, 4, 6, 4, 1}, bc2[4] = {1, 3, 3, 1};
          for (int idx = s_lo; idx < s_hi; idx++) {
            const int l = idx - pre[k] + 1;
            const double tau = (double)l / (double)linter, om = 1.0 - tau;
            double pw[6], qw[6];
            pw[0] = 1.0; qw[0] = 1.0;
            UNROLL for (int q = 1; q < 6; q++) { pw[q] = pw[q - 1] * tau; qw[q] = qw[q - 1] * om; }
            double d0 = 0.0, d1 = 0.0, d2 = 0.0;   // d x / d c_j, d dx / d c_j, d ddx / d c_j
            UNROLL for (int q = 0; q < 6; q++) if (q == jc) d0 = t * (bc0[q] * pw[q] * qw[5 - q]);
            UNROLL for (int q = 0; q < 5; q++) {
              const double b1 = bc1[q] * pw[q] * qw[4 - q];
              if (q + 1 == jc) d1 += 5.0 * b1;
              if (q == jc) d1 -= 5.0 * b1;
            }
            UNROLL for (int q = 0; q < 4; q++) {
              const double b2 = bc2[q] * pw[q] * qw[3 - q];
              if (q + 2 == jc) d2 += 20.0 * b2;
              if (q + 1 == jc) d2 -= 40.0 * b2;
              if (q == jc) d2 += 20.0 * b2;
            }
            d2 /= t;
            const double *gq = gbuf[idx + 2 - c0];
            acc[0] += gq[0] * d0 + gq[1] * d1 + gq[2] * d2;
            acc[1] += gq[3] * d0 + gq[4] * d1 + gq[5] * d2;
          }
          if (k < k_hi || hi_done) {
            cb[(size_t)k * 6 + jc] = acc[0];
            cb[(size_t)6 * S + (size_t)k * 6 + jc] = acc[1];
          } else {
            carry[jc][0] = acc[0]; carry[jc][1] = acc[1];
          }
        }
      }
      has_carry = !hi_done;
      k_next = hi_done ? k_hi + 1 : k_hi;
    }
    __syncthreads();
  }
  // segments without samples, and the slots beyond the candidate's count
  if (cb) {
    for (int q = 6 * k_next + lane; q < 6 * S; q += 64) { cb[q] = 0.0; cb[6 * S + q] = 0.0; }
    for (int q = 12 * S + lane; q < 12 * a.seg_stride; q += 64) cb[q] = 0.0;
  }
  // the reference line beyond the samples, and its clamped last entry
  for (int q = c.np + lane; q < N - 1; q += 64) {
    if (gs) gs[q] = 0.0;
    if (gl) gl[q] = 0.0;
  }
  clamp_bar[0] = wave_sum(clamp_bar[0]);
  clamp_bar[1] = wave_sum(clamp_bar[1]);
  reduce_sums(s);
  if (lane == 0) {
    if (gs) gs[N - 1] = clamp_bar[0];
    if (gl) gl[N - 1] = clamp_bar[1];
  }
  if (a.params_bar && lane < 20) {
    double v = 0.0;
    if (!cub) {
      UNROLL for (int q = 0; q < 8; q++) if (lane == q) v = abar * s.T[q];
      if (lane == 9) v = abar * s.T[8];
    }
    a.params_bar[b * 20 + lane] = v;
  }
}

}  // namespace btrapz
