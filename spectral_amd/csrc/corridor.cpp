// corridor.cpp -- see corridor.hpp.
#include "corridor.hpp"

#include "corridor_core.h"
#include "corridor_vjp_core.h"
#include "../../include/btrapz_hip_stage_jvp.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace btrapz {

// ---- input file ---------------------------------------------------------------------------
// The reference reads with `ifs >> v` and never checks the stream: after the first failed
// extraction every later one is a no-op that leaves its target untouched
// (src/c_road_s1_2.txt has a short last row and relies on this).  TokenReader mirrors it.
// strtod for the numbers corridor files hold.  Plain decimals ([+-]digits[.digits][e[+-]digits]) of at most 15
// significant digits and a decimal exponent within +-22 are converted exactly as strtod does it, by ONE correctly
// rounded operation on two exactly representable values (Clinger's fast path); everything else -- longer digit
// strings, inf / nan / hex, no number at all -- goes to strtod itself.  Three times faster on the ~3 000 tokens of a
// 20-second scene (the scan was a third of a file-based find_traj call).
double parse_double(const char *p, const char **end) {
  static const double P10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  const char *q = p;
  while (*q == ' ' || *q == '\n' || *q == '\t' || *q == '\r' || *q == '\f' || *q == '\v') ++q;
  bool neg = false;
  if (*q == '+' || *q == '-') { neg = *q == '-'; ++q; }
  unsigned long long mant = 0;
  int digits = 0, scale = 0;
  bool any = false, slow = false;
  while (*q >= '0' && *q <= '9') {
    any = true;
    if (mant || *q != '0') { if (++digits > 15) slow = true; else mant = mant * 10 + (unsigned)(*q - '0'); }
    ++q;
  }
  if (*q == '.') {
    ++q;
    while (*q >= '0' && *q <= '9') {
      any = true;
      if (mant || *q != '0') { if (++digits > 15) slow = true; else mant = mant * 10 + (unsigned)(*q - '0'); }
      --scale; ++q;
    }
  }
  if (any && !slow && (*q == 'e' || *q == 'E')) {
    const char *r = q + 1;
    bool eneg = false;
    if (*r == '+' || *r == '-') { eneg = *r == '-'; ++r; }
    if (*r >= '0' && *r <= '9') {
      int ex = 0;
      while (*r >= '0' && *r <= '9') { if (ex < 10000) ex = ex * 10 + (*r - '0'); ++r; }
      scale += eneg ? -ex : ex;
      q = r;
    }
  }
  if (!any || slow || scale < -22 || scale > 22 || *q == 'x' || *q == 'X' || *q == 'p' || *q == 'P') {
    char *e = nullptr;
    const double v = strtod(p, &e);
    *end = e;
    return v;
  }
  double v = (double)mant;                       // exact: below 1e15
  v = scale < 0 ? v / P10[-scale] : v * P10[scale];
  *end = q;
  return neg ? -v : v;
}

// printf("%.3f") for the numbers a trajectory file holds: v * 1000 is rounded once, to within 1e-4 of the true
// product, and unless its fraction is within 1e-3 of a tie (the residual is below 1e-4 for |v| < 1e9) the nearest integer is the correctly
// rounded decimal -- what printf computes from the exact binary expansion.  Near a tie, for |v| >= 1e9 and for inf / nan, snprintf decides.  Returns the length.
int format_3(char *out, double v) {
  const double a = fabs(v);
  if (!(a < 1e9)) return snprintf(out, FORMAT_3_MAX, "%.3f", v);
  const double y = a * 1000.0;                   // a * 1000 = y + e exactly, |e| <= ulp(y) / 2
  const double r = floor(y), frac = y - r;       // exact: y < 2^53
  if (fabs(frac - 0.5) < 1e-3) return snprintf(out, FORMAT_3_MAX, "%.3f", v);
  unsigned long long R = (unsigned long long)r + (frac > 0.5 ? 1u : 0u);
  char tmp[24];
  int n = 0;
  const unsigned f3 = (unsigned)(R % 1000u);
  unsigned long long ip = R / 1000u;
  do { tmp[n++] = (char)('0' + ip % 10u); ip /= 10u; } while (ip);
  char *o = out;
  if (signbit(v)) *o++ = '-';
  while (n) *o++ = tmp[--n];
  *o++ = '.';
  *o++ = (char)('0' + f3 / 100u); *o++ = (char)('0' + f3 / 10u % 10u); *o++ = (char)('0' + f3 % 10u);
  *o = 0;
  return (int)(o - out);
}

namespace {
// The whole file is read at once and scanned with strtod / strtol (the stream extraction it replaces spent 0.1 ms on
// the ~1000 tokens of a corridor file -- as long as the solve).
class TokenReader {
 public:
  explicit TokenReader(const std::string &path) {
    if (FILE *f = fopen(path.c_str(), "rb")) {
      open_ = true;
      char chunk[1 << 14];
      size_t n;
      while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) buf_.append(chunk, n);
      fclose(f);
    }
    p_ = buf_.c_str();
  }
  bool open() const { return open_; }
  void get(double &v) {
    if (failed_) return;
    const char *end = nullptr;
    const double t = parse_double(p_, &end);
    if (end == p_) failed_ = true; else { v = t; p_ = end; }
  }
  void get(int &v) {
    if (failed_) return;
    char *end = nullptr;
    const long t = strtol(p_, &end, 10);
    if (end == p_) failed_ = true; else { v = (int)t; p_ = end; }
  }
  bool failed() const { return failed_; }
 private:
  std::string buf_;
  const char *p_ = nullptr;
  bool open_ = false, failed_ = false;
};
}  // namespace

bool read_traj_input(const std::string &path, TrajInput &in) {
  TokenReader r(path);
  if (!r.open()) return false;
  r.get(in.N); r.get(in.delta);
  for (double &v : in.init_s) r.get(v);
  for (double &v : in.init_l) r.get(v);
  r.get(in.num_obs);
  r.get(in.ds_ref); r.get(in.dl_ref);
  r.get(in.dds[0]); r.get(in.dds[1]);
  r.get(in.ddds[0]); r.get(in.ddds[1]);
  r.get(in.ddl[0]); r.get(in.ddl[1]);
  r.get(in.dddl[0]); r.get(in.dddl[1]);
  if (r.failed() || in.N < 3 || in.N > 100000 || in.num_obs < 0 || in.num_obs > 1000 || !(in.delta > 0)) return false;
  double lo = 0, hi = 0;
  auto read_pairs = [&](Bounds &b) {
    b.clear(); b.reserve(in.N);
    for (int i = 0; i < in.N; i++) { r.get(lo); r.get(hi); b.emplace_back(lo, hi); }
  };
  auto read_vals = [&](std::vector<double> &v) {
    v.clear(); v.reserve(in.N);
    for (int i = 0; i < in.N; i++) { r.get(lo); v.push_back(lo); }
  };
  in.s_bounds.resize(in.num_obs); in.l_bounds.resize(in.num_obs);
  for (int o = 0; o < in.num_obs; o++) { read_pairs(in.s_bounds[o]); read_pairs(in.l_bounds[o]); }
  read_pairs(in.ds_bounds); read_pairs(in.dl_bounds);
  read_vals(in.s_ref); read_vals(in.l_ref); read_vals(in.s_kappa); read_vals(in.l_kappa);
  return true;
}

bool write_trajectory_file(const std::string &path, int np, double delta, const double *s, const double *l, const double *ds,
                           const double *dl, const double *dds, const double *ddl) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) return false;
  std::string text;
  text.reserve((size_t)(np > 0 ? np : 0) * 64);
  char num[FORMAT_3_MAX + 1];
  for (int i = 0; i < np; i++) {
    const double row[7] = {i * delta, s[i], l[i], ds[i], dl[i], dds[i], ddl[i]};
    for (int c = 0; c < 7; c++) { int n = format_3(num, row[c]); num[n++] = c < 6 ? ' ' : '\n'; text.append(num, (size_t)n); }
  }
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  return fclose(f) == 0 && ok;
}

// ---- per-obstacle extraction and selection: thin std::vector wrappers over corridor_core.h ----------
static Segment to_segment(const Seg &c) {
  Segment s;
  s.beg_t = c.beg_t; s.end_t = c.end_t; s.t = c.t; s.beg_l = c.beg_l; s.end_l = c.end_l;
  s.upp_skew = c.upp_skew; s.upp_bias = c.upp_bias; s.down_skew = c.down_skew; s.down_bias = c.down_bias;
  s.l_upp_skew = c.l_upp_skew; s.l_upp_bias = c.l_upp_bias; s.l_down_skew = c.l_down_skew; s.l_down_bias = c.l_down_bias;
  s.count = c.count;
  return s;
}
static Seg to_seg(const Segment &c) {
  Seg s;
  s.beg_t = c.beg_t; s.end_t = c.end_t; s.t = c.t; s.beg_l = c.beg_l; s.end_l = c.end_l;
  s.upp_skew = c.upp_skew; s.upp_bias = c.upp_bias; s.down_skew = c.down_skew; s.down_bias = c.down_bias;
  s.l_upp_skew = c.l_upp_skew; s.l_upp_bias = c.l_upp_bias; s.l_down_skew = c.l_down_skew; s.l_down_bias = c.l_down_bias;
  s.count = c.count;
  return s;
}
static_assert(sizeof(std::pair<double, double>) == 2 * sizeof(double), "Bounds must be interleaved (lower, upper) pairs");

std::vector<Segment> extract_segments(int variant, int N, double delta, const Bounds &sb, const Bounds &lb) {
  std::vector<Seg> buf(2 * (size_t)N + 16);
  const BoundsView s{reinterpret_cast<const double *>(sb.data())}, l{reinterpret_cast<const double *>(lb.data())};
  const int n = extract_segments_core(variant, N, delta, s, l, SlopesOnTheFly{s, delta}, buf.data(), (int)buf.size());
  std::vector<Segment> out;
  for (int i = 0; i < n; i++) out.push_back(to_segment(buf[i]));
  return out;
}

bool select_segments(int variant, double delta, const std::vector<std::vector<Segment>> &lists,
                     const std::vector<double> &s_ref, const std::vector<double> &l_ref, std::vector<Segment> &out) {
  out.clear();
  std::vector<Seg> sel;
  int carry = 0;
  for (const auto &list : lists)
    for (const Segment &c0 : list) {
      const Seg c = to_seg(c0);
      int hits = 0;
      for (size_t i = 0; i < s_ref.size(); i++) hits += knot_inside(c, s_ref[i], l_ref[i], double(i), delta) ? 1 : 0;
      for (int copies = selection_copies(selection_pushes(hits, carry), c); copies > 0; copies--) { Seg t = c; t.count = 3; sel.push_back(t); }
    }
  if (sel.empty()) return false;
  const int n = order_segments_core(variant, delta, sel.data(), (int)sel.size());
  for (int i = 0; i < n; i++) out.push_back(to_segment(sel[i]));
  return true;
}

// ---- backward pass of the corridor stage, one candidate on the host (the twin of corridor_vjp_kernel) --------------------
// The decisions are those of the device stage within the wave-wide kernels' limits: the serial statements of
// corridor_core.h on lists of the capacities the forward's retry pass has, provenance noted in Seg::count.
// Returns the forward's seg_count (0: nothing selected, -1: overflow or a segment with t <= 0).
static int decide_with_provenance(int variant, int N, int O, double delta, const double *gs, const double *gl, const double *sref,
                                  const double *lref, int seg_stride, std::vector<Seg> &sel) {
  const int cap_o = VJP_MAX_ALL / O, cap_sel = VJP_MAX_SEL;
  std::vector<Seg> list((size_t)cap_o);
  sel.clear();
  int carry = 0;
  for (int o = 0; o < O; o++) {
    const BoundsView sb{gs + (size_t)o * N * 2}, lb{gl + (size_t)o * N * 2};
    const int n = extract_segments_core(variant, N, delta, sb, lb, SlopesOnTheFly{sb, delta}, list.data(), cap_o, ProvenanceNote{list.data()});
    if (n < 0) return -1;
    for (int j = 0; j < n; j++) {   // CollisionCheck's selection, solve_3d.cc:534-596
      const Seg c = list[j];
      int hits = 0;
      for (int i = 0; i < N; i++) hits += knot_inside(c, sref[i], lref[i], (double)i, delta) ? 1 : 0;
      for (int copies = selection_copies(selection_pushes(hits, carry), c); copies > 0; copies--) {
        if ((int)sel.size() >= cap_sel) return -1;
        Seg t = c; t.count = provenance_pack(o, c.count); sel.push_back(t);
      }
    }
  }
  if (sel.empty()) return 0;
  const int S = order_segments_core(variant, delta, sel.data(), (int)sel.size());
  if (S > seg_stride) return -1;
  for (int k = 0; k < S; k++) if (!(sel[k].t > 0.0)) return -1;
  return S;
}

namespace {
struct HostSink {   // adds every term where it belongs, in the order it comes: segments ascending
  double *g[VJP_GROUPS];
  void add(int group, int /*p*/, int index, double value) { if (g[group] && index >= 0) g[group][index] += value; }
};
}  // namespace

}  // namespace btrapz

extern "C" __attribute__((visibility("default"))) int btrapz_corridor_vjp_host(
    int variant, int N, int num_obs, double delta, const double *s_bounds, const double *l_bounds, const double *ds_bounds,
    const double *dl_bounds_knots, const double *s_ref, const double *l_ref, int seg_stride, const double *seg_bar,
    const double *ref_end_bar, const double *dl_bounds_bar, const btrapz_knot_grads *out, int *seg_count) {
  using namespace btrapz;
  if (variant < 0 || variant > 1 || N < 3 || N > VJP_MAX_KNOTS || num_obs < 1 || num_obs > VJP_MAX_OBS || !(delta > 0) || seg_stride < 1 ||
      seg_stride > BTRAPZ_MAX_SEGMENTS || !s_bounds || !l_bounds || !ds_bounds || !dl_bounds_knots || !s_ref || !l_ref ||
      (!seg_bar && !ref_end_bar && !dl_bounds_bar) || !out ||
      (!out->s_bounds && !out->l_bounds && !out->ds_bounds && !out->dl_bounds_knots && !out->s_ref && !out->l_ref))
    return BTRAPZ_EINVAL;
  const size_t n_pairs = (size_t)num_obs * N * 2;
  auto zero = [](double *p, size_t n) { if (p) for (size_t i = 0; i < n; i++) p[i] = 0.0; };
  zero(out->s_bounds, n_pairs); zero(out->l_bounds, n_pairs); zero(out->ds_bounds, (size_t)N * 2);
  zero(out->dl_bounds_knots, (size_t)N * 2); zero(out->s_ref, (size_t)N); zero(out->l_ref, (size_t)N);
  std::vector<Seg> sel;
  const int S = decide_with_provenance(variant, N, num_obs, delta, s_bounds, l_bounds, s_ref, l_ref, seg_stride, sel);
  if (seg_count) *seg_count = S;
  if (S < 1) return BTRAPZ_OK;
  HostSink sink{{out->s_bounds, out->l_bounds, out->ds_bounds, out->s_ref, out->l_ref}};
  for (int k = 0; k < S; k++)
    segment_adjoint(variant, N, delta, k, sel[k], ds_bounds, seg_bar ? seg_bar + k : nullptr, (size_t)seg_stride, sink);
  if (ref_end_bar) {
    if (out->s_ref) out->s_ref[N - 1] += ref_end_bar[0];
    if (out->l_ref) out->l_ref[N - 1] += ref_end_bar[1];
  }
  if (dl_bounds_bar && out->dl_bounds_knots)
    for (int j = 0; j < 10; j++) {
      const int i = j >> 1, ii = i > N - 1 ? N - 1 : i;
      out->dl_bounds_knots[2 * ii + (j & 1)] += dl_bounds_bar[j];
    }
  return BTRAPZ_OK;
}

// ---- forward-mode derivative of the corridor stage, one candidate on the host (the twin of corridor_jvp_kernel) ----------
// decide_with_provenance, then segment_tangent on every segment and direction: the kernel's statements, the kernel's bits.
extern "C" __attribute__((visibility("default"))) int btrapz_corridor_jvp_host(
    int variant, int N, int num_obs, double delta, const double *s_bounds, const double *l_bounds, const double *ds_bounds,
    const double *dl_bounds_knots, const double *s_ref, const double *l_ref, int seg_stride, int T,
    const btrapz_knot_tangents *tangents, double *seg_dot, double *ref_end_dot, double *dl_bounds_dot, int *seg_count) {
  using namespace btrapz;
  if (variant < 0 || variant > 1 || N < 3 || N > VJP_MAX_KNOTS || num_obs < 1 || num_obs > VJP_MAX_OBS || !(delta > 0) || seg_stride < 1 ||
      seg_stride > BTRAPZ_MAX_SEGMENTS || T < 1 || T > BTRAPZ_MAX_TANGENTS || !s_bounds || !l_bounds || !ds_bounds || !dl_bounds_knots ||
      !s_ref || !l_ref || !tangents ||
      (!tangents->s_bounds && !tangents->l_bounds && !tangents->ds_bounds && !tangents->dl_bounds_knots && !tangents->s_ref && !tangents->l_ref) ||
      (!seg_dot && !ref_end_dot && !dl_bounds_dot))
    return BTRAPZ_EINVAL;
  std::vector<Seg> sel;
  const int S = decide_with_provenance(variant, N, num_obs, delta, s_bounds, l_bounds, s_ref, l_ref, seg_stride, sel);
  if (seg_count) *seg_count = S;
  const bool has = S > 0;
  const size_t pairs = (size_t)num_obs * N * 2;
  std::vector<SegmentReads> reads;
  for (int k = 0; k < (has ? S : 0); k++) reads.push_back(segment_reads(N, k, sel[k], ds_bounds));
  for (int t = 0; t < T; t++) {
    const KnotTangentSource src{tangents->s_bounds ? tangents->s_bounds + t * pairs : nullptr,
                                tangents->l_bounds ? tangents->l_bounds + t * pairs : nullptr,
                                tangents->ds_bounds ? tangents->ds_bounds + (size_t)t * N * 2 : nullptr,
                                tangents->s_ref ? tangents->s_ref + (size_t)t * N : nullptr,
                                tangents->l_ref ? tangents->l_ref + (size_t)t * N : nullptr, N};
    if (seg_dot)
      for (int k = 0; k < seg_stride; k++) {
        double out[BTRAPZ_NUM_SEG_FIELDS];
        if (has && k < S) segment_tangent(variant, delta, reads[k], src, out);
        else for (int f = 0; f < BTRAPZ_NUM_SEG_FIELDS; f++) out[f] = 0.0;
        for (int f = 0; f < BTRAPZ_NUM_SEG_FIELDS; f++) seg_dot[((size_t)t * BTRAPZ_NUM_SEG_FIELDS + f) * seg_stride + k] = out[f];
      }
    if (ref_end_dot) {
      ref_end_dot[2 * t] = has ? src.sr(N - 1) : 0.0;
      ref_end_dot[2 * t + 1] = has ? src.lr(N - 1) : 0.0;
    }
    if (dl_bounds_dot)
      for (int j = 0; j < 10; j++) {
        const int i = j >> 1, ii = i > N - 1 ? N - 1 : i;
        dl_bounds_dot[10 * t + j] = has && tangents->dl_bounds_knots ? tangents->dl_bounds_knots[((size_t)t * N + ii) * 2 + (j & 1)] : 0.0;
      }
  }
  return BTRAPZ_OK;
}
