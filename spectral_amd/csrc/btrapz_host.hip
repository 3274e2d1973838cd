// btrapz_host.hip -- host side of the batched C-ABI (include/btrapz_hip.h): context,
// workspace, kernel launches.  No CPU fallback: without a HIP device every entry point
// fails with BTRAPZ_ENODEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <cstddef>
#include <type_traits>
#include "btrapz_device.h"
#include "btrapz_select.h"
#include "corridor_jvp.h"
#include "../../include/btrapz_hip_stage_jvp.h"
#include "../../include/btrapz_hip_schedule.h"
#include "../../include/btrapz_hip_check.h"
#include "../../include/btrapz_hip_long.h"
#include "../../include/btrapz_hip_long_rescue.h"
#include "../../include/btrapz_hip_long_sets.h"
#include "../../include/btrapz_hip_long_grad.h"
#include "btrapz_long_grad.h"
#include "prism_core.h"

using namespace btrapz;

// Environment overrides of btrapz_options for experiments (BTRAPZ_CAP, _QUEUE, _LEAN, _SPLIT, _START, _STALL_FACTOR: A/B
// runs of tools/ without touching the caller).  Only in a -DBTRAPZ_EXPERIMENTS build: in the shipped library this file
// reads no environment variable at all -- the batched entry points and btrapz_launch_single take every choice from
// btrapz_options.  (find_traj, whose only configuration channel IS the environment, translates its documented
// variables -- BTRAPZ_EPS, _ELASTIC, _ELASTIC_TOL, _WARM, _SPLIT, _SPIN, _DEVICE, _INPUT, _OUTPUT_PREFIX, _VERBOSE --
// into options in find_traj.hip; btrapz_multi.hip reads BTRAPZ_RCCL_LIB, a path.)
static inline const char *experiment_env(const char *name) {
#ifdef BTRAPZ_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// Step-length rule of the interior-point iterations (btrapz_options).  Measured on MI355X, 65 536 x 20 synthetic
// candidates (mean iterations / kernel ms) and 65 536 jittered copies of c_road_s1_3.txt, a quarter of them infeasible
// and many close to it (candidates the 0.995 rule solves and the setting loses):
//   fraction 0.995 everywhere                     9.47 / 8.06    lost  0   (the classic conservative choice)
//   fraction 0.9999 everywhere                    7.81 / 6.85    lost 91   (blocked steps end too close to the
//                                                                           boundary, centrality is lost, mu stalls)
//   0.9999 when the step to the boundary >= 0.9,
//   0.995 otherwise and after 12 iterations       8.24 / 7.11    lost  0   <- default
// and over 262 144 jittered candidates of all bundled scenarios, both variants: lost 0 (1 lost / 17 gained with the
// jitter raised to 1.5 m).  tests/test_gpu_properties.py keeps that comparison as a regression test.
#define BTRAPZ_DEFAULT_STEP_FRACTION 0.9999
#define BTRAPZ_DEFAULT_STEP_THRESHOLD 0.9
#define BTRAPZ_AGGRESSIVE_ITERATIONS 12
// Divergence / infeasibility test: after BTRAPZ_STALL_START iterations, BTRAPZ_STALL_LENGTH iterations without a better
// score end the solve.  On the same 2 x 262 144 jittered candidates: (12, 8) 0 lost, infeasible candidates end after
// 21.5 iterations on average; (10, 6) 0 lost, 19.5; (8, 5) 3 lost; (8, 4) 18 lost; (6, 3) 87 lost.
#define BTRAPZ_STALL_START 10
#define BTRAPZ_STALL_LENGTH 6
// "Without progress" = no better score AND no residual (the score without its complementarity part) below
// BTRAPZ_STALL_FACTOR times the smallest one so far.  The score alone lost solvable candidates on corridors with runs
// of short segments, where mu climbs for ten iterations while the residuals fall 40-fold (found by a fuzz of find_traj
// against the oracle): 49 of the 48 821 solvable ones of the cuboid bench batch, 1 of 16 384 jittered c6.txt.  Lost
// with factor 0.3 / 0.5 / 0.7..1.0: 17 / 5 / 0; infeasible candidates of the jittered c_road_s1_3.txt end after
// 19.4 / 20.1 / 22.2-24.1 iterations (18.4 with the score alone).
#define BTRAPZ_STALL_FACTOR 0.8f
// An infeasible solve does not just stall: a few iterations after its residuals stop falling mu explodes (1 -> 45 ->
// 500 -> 1e5 -> ... on the jittered c_road_s1_3.txt).  mu above BTRAPZ_DIVERGE_FACTOR times the best score so far ends
// the solve at once.  The largest climb seen on a candidate that then converged is 10x; with 1e4 / 1e3 / 1e2 / 30 no
// solvable candidate of the sets above is lost and the infeasible ones of c_road_s1_3.txt end after 17.2 / 16.9 / 16.0 /
// 15.5 iterations (22.7 without the test).
#define BTRAPZ_DIVERGE_FACTOR 1e3f
// Rescue pass (btrapz_options.elastic): penalty parameter of the relaxed rows and the violation still accepted.
// delta: the relaxed solution is within delta * |multipliers| (1e2..1e4 here) of the least-violation limit; 1e-8 keeps
// that below 1e-4 and the interior-point method still converges in 25-40 iterations (1e-10: 40+, scores near 1e-7).
// tol, in the unit of the penalty (violation / |g_r|): the iterate the reference accepted on src/c7.txt (oracle OSQP
// port, status 2) violates acceleration rows by 0.492 = 0.01004 |g|, velocity rows by 0.013, position rows by 1e-4 m;
// the least-squares solution of that input in the same norm violates them by 0.477 / 0.027 / 3e-4 m (0.0097 |g|; cuboid:
// 0.0019 |g|); a grossly infeasible input such as src/c_road_s1_2.txt is at 4.9 |g|.  Default 0.0125: a quarter above
// what the reference is seen accepting; at most 0.0125 t metres outside a position row.  (Round 2 penalised every row in
// its own unit and accepted 0.5 of it: the least-squares solution then leaves c7's lateral corridor by 0.09 m.)
#define BTRAPZ_DEFAULT_ELASTIC_DELTA 1e-8
#define BTRAPZ_DEFAULT_ELASTIC_TOL 0.0125
// Two-launch solve (btrapz_options.cap_iter): who hands over -- a group that is the only one of its wavefront still
// iterating after cap_iter iterations, and any group still iterating BTRAPZ_CAP_HI iterations later; hand-over slots for
// BTRAPZ_SUSP_PERCENT of the axis problems, at most BTRAPZ_SUSP_BYTES_MAX of workspace.  (Tuned on the bench batches,
// cap_alone 1 / 2 / 3: 6.39 / 6.47 / 6.58 ms; cap_hi 2 / 4 / 8: 6.44 / 6.39 / 6.41; 12-21 % of the problems
// hand over.)  Compile-time constants: a stray environment variable must not change what a drop-in library does.
#ifndef BTRAPZ_CAP_ALONE
#define BTRAPZ_CAP_ALONE 1
#endif
#ifndef BTRAPZ_CAP_HI
#define BTRAPZ_CAP_HI 4
#endif
// BTRAPZ_CAP_SCORE > 0: a lone group whose score is already below it is NOT handed over (quadratic convergence: one or
// two iterations left; half of what scenario_1 hands over and three quarters of the generic batch is below 1e-5).
// Measured, round 4 (65 536 x 20, lean form): it halves the hand-over traffic and costs time -- scenario_1 4.85 ms without,
// 4.94 / 4.99 / 5.01 / 5.05 with 1e-6 / 1e-5 / 1e-4 / 1e-3; generic 3.78 -> 3.90 ... 4.01: a group alone in its wavefront
// runs its last iteration at a third of the machine's width, and that costs more than 74 doubles per segment out and
// back.  Off.
#ifndef BTRAPZ_CAP_SCORE
#define BTRAPZ_CAP_SCORE 0.0
#endif
// (round 5: 25 -> 15 % -- 8.5-12 % of the axis problems of the bench batches hand over; a group that finds no slot goes on
//  to the end where it is, which costs time, never a result)
#ifndef BTRAPZ_SUSP_PERCENT
#define BTRAPZ_SUSP_PERCENT 15
#endif
#define BTRAPZ_SUSP_BYTES_MAX (1ull << 30)
// The lean two-launch solve of a uniform batch in memory order may run as THREE launches, one axis's resume wavefronts
// inside the other axis's capped launch (launch_pipelined below).  0: the schedule never runs and nothing
// is remembered -- the two launches as they were (A/B builds: tools/build_variant.sh X -DBTRAPZ_PIPELINE=0).
#ifndef BTRAPZ_PIPELINE
#define BTRAPZ_PIPELINE 1
#endif
// ... chosen when the last finished solve of the same shape handed over at least this many times more problems of one
// axis than of the other (a condition, not a tuned number: the bench families sit at 1 : 1 and at 10 000 : 1)
#define BTRAPZ_PIPELINE_RATIO 4
// ... and with the other axis QUIET -- solved uncapped, in the grid of the first axis's resume wavefronts
// (launch_quiet_axis below) -- when it handed over at least this many times more (again a condition: the families whose
// lateral axis is quiet sit at 1 000 : 1 and beyond -- 11 149 : 1, 1 067 : 0, 5 073 : 0, 15 410 : 1)
#define BTRAPZ_QUIET_RATIO 256

// Layout the lean kernels rely on (btrapz_lean_body.h reads the row limits of its axis as (&sh.acc_s[0])[2 axis + i],
// (&sh.acc_s[0])[4 + 2 axis + i], and its arguments through the kernarg segment pointer: KernelArgs is the first parameter).
static_assert(offsetof(btrapz::Shared, acc_l) == offsetof(btrapz::Shared, acc_s) + 2 * sizeof(double) &&
              offsetof(btrapz::Shared, jerk_s) == offsetof(btrapz::Shared, acc_s) + 4 * sizeof(double) &&
              offsetof(btrapz::Shared, jerk_l) == offsetof(btrapz::Shared, acc_s) + 6 * sizeof(double), "Shared: acc_s, acc_l, jerk_s, jerk_l contiguous");
static_assert(std::is_trivially_copyable<btrapz::KernelArgs>::value && alignof(btrapz::KernelArgs) <= 8, "KernelArgs is passed by value at kernarg offset 0");

// One device allocation of a context.  Every buffer enters its context's list when it is constructed: btrapz_destroy and
// btrapz_workspace_bytes walk that list.  grow() is what every workspace here does when a launch needs more than the
// buffer holds: free it and allocate exactly the bytes asked for (no rounding; the contents are not kept).
// Fatal use: GROW(c, buffer, bytes) below.  Non-fatal use (the two-launch solve's workspace, the corridor stage's lists):
// test grow()'s result and clear HIP's error with hipGetLastError().
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  explicit DevBuf(std::vector<DevBuf *> &owner) { owner.push_back(this); }
  DevBuf(const DevBuf &) = delete;
  void release() { (void)hipFree(p); p = nullptr; bytes = 0; }
  __attribute__((always_inline)) hipError_t grow(size_t need) { return need <= bytes ? hipSuccess : regrow(need); }   // (the usual case: a compare)
  __attribute__((noinline)) hipError_t regrow(size_t need) {
    release();
    const hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need; else p = nullptr;
    return e;
  }
};
template <class T> struct Buf : DevBuf {   // ... that holds elements of T
  using DevBuf::DevBuf;
  T *ptr() const { return static_cast<T *>(p); }
  operator T *() const { return ptr(); }
  size_t cap() const { return bytes / sizeof(T); }
};
// Arrays that move together under one capacity (read off the one allocated LAST): all are released before any is
// allocated, so an allocation that fails half-way leaves the last one empty and the next call starts over.
template <class... B> static void release_all(B &...b) { (b.release(), ...); }

struct btrapz_ctx {
  int device = 0;
  std::string err;
  std::vector<DevBuf *> bufs;       // every device buffer below (declared first: the buffers register here)
  // workspace (grown on demand): per-axis records of the last solve; one capacity, d_axis_iters is allocated last
  Buf<double> d_axis_obj{bufs};
  Buf<double> d_axis_viol{bufs};    // [2B][4] rescue pass: row violations per class
  Buf<int> d_axis_status{bufs}, d_axis_iters{bufs};
  size_t viol_valid = 0;            // candidates of the last solve with a rescue pass (0: none)
  Buf<double> d_mqm{bufs};          // [2][4][21]
  double h_mqm_w[8] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};  // weights the table was built for
  // ragged batches: candidate order by segment count + bucket tables
  Buf<int> d_order{bufs};
  Buf<int> d_meta{bufs};            // [198] histogram/cand_prefix, wave_prefix, cursors
  Buf<int> d_retry{bufs};           // corridor stage: [0] count, [1..] candidates of the retry pass
  Buf<char> d_strips{bufs};         // btrapz_prism_corridor_batch_device's two-launch path: the strips
  Buf<char> d_corr_ws{bufs};        // corridor_serial_kernel's segment lists (horizons beyond the wave-wide kernels)
  Buf<int> d_vjp_retry{bufs};       // the corridor stage's backward pass: [0] count, [1..] candidates of its retry pass
  Buf<int> d_long_list{bufs};       // ragged batches: the candidates of more than 64 segments, by count
  // The workspaces serve one launch sequence at a time.  Launches of one context issued on DIFFERENT streams are
  // ordered behind each other with this event (recorded after every sequence, waited for when the stream changes: ws_open).
  hipEvent_t ws_free = nullptr; hipStream_t ws_stream = nullptr; bool ws_used = false;
  Buf<double> d_argmin_cost{bufs}; Buf<long long> d_argmin_idx{bufs};   // partial arg-mins (one capacity, idx allocated last)
  Buf<double> d_topk_cost{bufs}; Buf<long long> d_topk_idx{bufs};       // partial K-best lists (btrapz_select.hip), the same way
  // rescue pass (btrapz_options.elastic): keys [2][B], per-axis candidate lists [2][B], bucket tables [2][198]
  // (with parameter sets, sets_rescue_pass: masked set indices [2][B], lists [2][B], tables [2][3 n_keys + 2])
  Buf<int> d_rescue{bufs};
  Buf<int> d_rescue_meta{bufs};
  // staging for the host-pointer wrapper
  Buf<double> d_stage{bufs};
  Buf<int> d_istage{bufs};
  Buf<double> d_single{bufs};       // control points of the single-candidate launch (find_traj)
  // what a warm single-candidate launch leaves for the next one: joint states [2][64][3], multipliers [2][36][64] (two
  // sets, read / written alternately), and the problem shape they belong to
  Buf<double> d_single_warm{bufs}; int single_S = 0, single_variant = -1, single_flip = 0;
  Buf<int> d_queue{bufs};           // [2] candidate counters of the persistent launch (ipm_solve_queue_kernel)
  // capped solve (btrapz_options.cap_iter): iterates of the suspended axis problems, their slots and list keys
  Buf<double> d_susp_state{bufs};
  Buf<int> d_susp_ints{bufs};       // [count, 3 pad] [bucket tables 2 x 198] [2B keys] [2B slots]
  int resident_waves = 1024;        // wavefronts the device holds at one per SIMD
  int last_form = -1;               // btrapz_last_solve_form
  int last_launches = 0;            // btrapz_debug_solve_launches: solve-kernel launches of the last solve's main step
  // Schedule of the lean two-launch solve (launch_pipelined): what the last FINISHED solve handed over per axis.  Every such
  // solve leaves its two list lengths in h_pipe_counts (pinned host memory the device writes, stream-ordered) and records
  // pipe_landed behind them; a later call takes them in only when a non-blocking query says they have landed.
  int *h_pipe_counts = nullptr; hipEvent_t pipe_landed = nullptr; bool pipe_pending = false;
  int pipe_pending_S = 0, pipe_pending_variant = -1;              // shape of the solve whose counts are on their way
  int pipe_S = 0, pipe_variant = -1, pipe_count[2] = {0, 0};      // the counts that landed last, and their shape (pipe_S 0: none)
  int schedule_mode = 0;            // btrapz_debug_set_schedule: 0 automatic, -1 never, 1 / 2 pipelined with s / l first, 3 / 4 s / l first and the other axis quiet
  // btrapz_solve_sets_device: the device view of every set and its M'QM table, cached by content (h_sets: what the tables
  // were built from); uploads go through two pinned staging buffers used in turn, the copy out of each marked by its event
  Buf<Shared> d_sets{bufs}; Buf<double> d_mqm_sets{bufs}; size_t sets_cap = 0;
  std::vector<Shared> h_sets;
  Shared *h_sets_stage[2] = {nullptr, nullptr}; hipEvent_t sets_copied[2] = {nullptr, nullptr};
  bool sets_copy_pending[2] = {false, false}; int sets_stage_next = 0;
  Buf<int> d_sets_meta{bufs};       // bucket tables of a sets batch: [n_keys + 1] x 2 + [n_keys]
  Buf<double> d_mqm_unit{bufs};     // the M'QM table with every weight 1 ([2][4][21]): the solve's VJP and JVP
  Buf<double> d_long_cost{bufs};    // btrapz_solve_long_jvp_device: the axes' shares of cost_dot, [2][T][B]
};

#define HIPCHK_AS(ctx, what, call)                                                            \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (ctx)->err = std::string(what) + ": " + hipGetErrorString(e_);                          \
      return BTRAPZ_EHIP;                                                                     \
    }                                                                                         \
  } while (0)
#define HIPCHK(ctx, call) HIPCHK_AS(ctx, #call, call)
// (a fatal grow(): its message reads as the hipMalloc call it stands for)
#define GROW(ctx, buf, nbytes) HIPCHK_AS(ctx, "hipMalloc(&c->" #buf ", " #nbytes ")", (ctx)->buf.grow(nbytes))
#define TRY(call) do { const int rc_ = (call); if (rc_ != BTRAPZ_OK) return rc_; } while (0)   // (a step of this file that failed)

// A launch sequence on the context's workspaces: opened by waiting for the sequence before it when that ran on another
// stream, closed by recording the event the next one waits for.  Entry points that touch no workspace do neither.
static int ws_wait(btrapz_ctx *c, hipStream_t stream) {
  if (c->ws_used && stream != c->ws_stream) HIPCHK(c, hipStreamWaitEvent(stream, c->ws_free, 0));
  return BTRAPZ_OK;
}
static int ws_open(btrapz_ctx *c, hipStream_t stream) { HIPCHK(c, hipSetDevice(c->device)); return ws_wait(c, stream); }
static int ws_close(btrapz_ctx *c, hipStream_t stream) {
  c->ws_stream = stream; c->ws_used = true;
  HIPCHK(c, hipEventRecord(c->ws_free, stream));
  return BTRAPZ_OK;
}

int btrapz_ctx_device(const btrapz_ctx *c) { return c ? c->device : 0; }
void btrapz_ctx_set_error(btrapz_ctx *c, const char *what) { if (c) c->err = what; }
// btrapz_select.h: the workspace of the K-best selection's two-launch path (btrapz_select.hip)
int btrapz_ctx_select_workspace(btrapz_ctx *c, size_t entries, void *stream_, double **cost, long long **idx) {
  if (entries > c->d_topk_idx.cap()) {
    release_all(c->d_topk_cost, c->d_topk_idx);
    GROW(c, d_topk_cost, sizeof(double) * entries);
    GROW(c, d_topk_idx, sizeof(long long) * entries);
  }
  TRY(ws_wait(c, (hipStream_t)stream_));
  *cost = c->d_topk_cost.ptr(); *idx = c->d_topk_idx.ptr();
  return BTRAPZ_OK;
}
int btrapz_ctx_workspace_close(btrapz_ctx *c, void *stream_) { return ws_close(c, (hipStream_t)stream_); }

BTRAPZ_EXPORT int btrapz_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

BTRAPZ_EXPORT int btrapz_build_has_experiments(void) {
#ifdef BTRAPZ_EXPERIMENTS
  return 1;
#else
  return 0;
#endif
}

static void free_buffers(btrapz_ctx *c) { for (DevBuf *b : c->bufs) b->release(); }

BTRAPZ_EXPORT int btrapz_create(btrapz_ctx **out, int device) {
  if (!out) return BTRAPZ_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return BTRAPZ_ENODEVICE;
  if (hipSetDevice(device) != hipSuccess) return BTRAPZ_ENODEVICE;
  btrapz_ctx *c = new btrapz_ctx();
  c->device = device;
  if (c->d_mqm.grow(sizeof(double) * 168) != hipSuccess) { delete c; return BTRAPZ_ENOMEM; }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->resident_waves = 4 * cus;
  }
  if (c->d_queue.grow(sizeof(int) * 2) != hipSuccess) { free_buffers(c); delete c; return BTRAPZ_ENOMEM; }
  if (hipEventCreateWithFlags(&c->ws_free, hipEventDisableTiming) != hipSuccess) { free_buffers(c); delete c; return BTRAPZ_ENOMEM; }
  *out = c;
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_destroy(btrapz_ctx *c) {
  if (!c) return BTRAPZ_EINVAL;
  (void)hipSetDevice(c->device);
  free_buffers(c);
  for (int i = 0; i < 2; i++) {
    if (c->sets_copy_pending[i]) (void)hipEventSynchronize(c->sets_copied[i]);
    if (c->h_sets_stage[i]) (void)hipHostFree(c->h_sets_stage[i]);
    if (c->sets_copied[i]) (void)hipEventDestroy(c->sets_copied[i]);
  }
  if (c->ws_free) (void)hipEventDestroy(c->ws_free);
  if (c->pipe_pending) (void)hipEventSynchronize(c->pipe_landed);   // (the device may still be writing h_pipe_counts)
  if (c->pipe_landed) (void)hipEventDestroy(c->pipe_landed);
  if (c->h_pipe_counts) (void)hipHostFree(c->h_pipe_counts);
  delete c;
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT const char *btrapz_last_error(const btrapz_ctx *c) { return c ? c->err.c_str() : "null context"; }
// Device memory the context holds for its launches right now (it grows on demand and is kept): every device buffer of
// the context -- per-axis records, bucket tables and lists, the hand-over workspace of the two-launch solve, the corridor
// stage's lists, the sets' tables, staging of the host-pointer wrapper.
BTRAPZ_EXPORT long long btrapz_workspace_bytes(const btrapz_ctx *c) {
  if (!c) return 0;
  size_t n = 0;
  for (const DevBuf *b : c->bufs) n += b->bytes;
  return (long long)n;
}
BTRAPZ_EXPORT int btrapz_last_solve_form(const btrapz_ctx *c) { return c ? c->last_form : -1; }

static int ensure_axis_ws(btrapz_ctx *c, size_t nprob) {
  if (nprob <= c->d_axis_iters.cap()) return BTRAPZ_OK;
  release_all(c->d_axis_obj, c->d_axis_status, c->d_axis_iters, c->d_axis_viol);
  c->viol_valid = 0;
  GROW(c, d_axis_obj, sizeof(double) * nprob);
  GROW(c, d_axis_viol, sizeof(double) * 4 * nprob);
  GROW(c, d_axis_status, sizeof(int) * nprob);
  GROW(c, d_axis_iters, sizeof(int) * nprob);
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT void btrapz_options_init(btrapz_options *opt) {
  if (!opt) return;
  memset(opt, 0, sizeof(*opt));
  opt->struct_size = (int)sizeof(btrapz_options);
}
// A caller built against another layout of btrapz_options would make the library read fields that are not there.
static bool options_ok(btrapz_ctx *c, const btrapz_options *opt) {
  if (!opt || opt->struct_size == (int)sizeof(btrapz_options)) return true;
  if (c) c->err = "invalid argument: btrapz_options.struct_size (call btrapz_options_init first)";
  return false;
}

// Weights, limits and iteration parameters of a launch (everything of KernelArgs that is not a pointer or a size).
static void fill_parameters(KernelArgs &a, const btrapz_shared *sh, const btrapz_options *opt, const btrapz_warm *warm) {
  memcpy(a.sh.w_s, sh->w_s, sizeof(a.sh.w_s)); memcpy(a.sh.w_l, sh->w_l, sizeof(a.sh.w_l));
  a.sh.weight_end_s = sh->weight_end_s; a.sh.weight_end_l = sh->weight_end_l;
  a.sh.ds_ref = sh->ds_ref; a.sh.dl_ref = sh->dl_ref;
  // a header limit left at the reference's default of +-1e10 (piecewise_jerk_problem.cc:9,25-35) is no limit: moved to
  // +-BTRAPZ_FAR_LIMIT, where the kernels know it for one (an infinite or NaN limit stays a defect of the input)
  auto limit = [](double v) { const double m = fabs(v); return (m >= BTRAPZ_FAR && m <= 1.7e308) ? copysign(BTRAPZ_FAR_LIMIT, v) : v; };
  a.sh.acc_s[0] = fmax(sh->dds[0], -1000.0); a.sh.acc_s[1] = fmin(sh->dds[1], 1000.0);  // solve_3d.cc:836,843-844
  a.sh.acc_l[0] = limit(sh->ddl[0]); a.sh.acc_l[1] = limit(sh->ddl[1]);
  a.sh.jerk_s[0] = limit(sh->ddds[0]); a.sh.jerk_s[1] = limit(sh->ddds[1]);
  a.sh.jerk_l[0] = limit(sh->dddl[0]); a.sh.jerk_l[1] = limit(sh->dddl[1]);
  a.sh.variant = sh->variant;
  a.eps = (opt && opt->eps > 0) ? opt->eps : 1e-9;
  a.max_iter = (opt && opt->max_iter > 0) ? opt->max_iter : 60;
  a.tau = (opt && opt->step_fraction > 0 && opt->step_fraction < 1) ? opt->step_fraction : BTRAPZ_DEFAULT_STEP_FRACTION;
  a.tau_iters = BTRAPZ_AGGRESSIVE_ITERATIONS;
  a.stall_start = BTRAPZ_STALL_START; a.stall_len = BTRAPZ_STALL_LENGTH;
  static const float stall_factor_env = [] { const char *v = experiment_env("BTRAPZ_STALL_FACTOR"); return v ? (float)atof(v) : 0.0f; }();   // (experiments)
  a.stall_factor = stall_factor_env > 0.0f ? stall_factor_env : BTRAPZ_STALL_FACTOR;
  a.diverge_factor = BTRAPZ_DIVERGE_FACTOR;
  a.tau_thr = (opt && opt->step_threshold > 0) ? opt->step_threshold : BTRAPZ_DEFAULT_STEP_THRESHOLD;
  a.x0 = warm ? warm->x0 : nullptr; a.lam0 = warm ? warm->lam0 : nullptr; a.lam_out = warm ? warm->lam_out : nullptr;
  a.mu0 = (warm && warm->mu0 > 0) ? warm->mu0 : 1e-4;
  a.smin = (warm && warm->smin > 0) ? warm->smin : 1e-2;
  a.elastic_delta = (opt && opt->elastic_delta > 0) ? opt->elastic_delta : BTRAPZ_DEFAULT_ELASTIC_DELTA;
  a.elastic_tol = (opt && opt->elastic_tol > 0) ? opt->elastic_tol : BTRAPZ_DEFAULT_ELASTIC_TOL;
  a.bucket_S = 0;
  a.cap_iter = 0; a.cap_alone = 0; a.cap_hi = 0; a.cap_score = 0.0; a.susp_cap = 0; a.susp_state = nullptr; a.susp_count = nullptr; a.susp_slot = nullptr; a.susp_key = nullptr;
#ifdef BTRAPZ_EXPERIMENTS
  static const int start_env = [] { const char *e = experiment_env("BTRAPZ_START"); return e ? atoi(e) : -1; }();
  a.unc_start = start_env >= 0 ? start_env : (opt ? opt->start : 0);
#else
  a.unc_start = 0;   // (btrapz_options.start: the optimum does not depend on it, the iteration count does -- for the worse; experiment builds only)
#endif
}

// M' pQp_d M on the host (solve_3d.cc:87-143): the single-candidate path hands the table over with its inputs.
void btrapz_mqm_table_host(const btrapz_shared *sh, double *table) {
#pragma clang fp contract(off)   // the device builder (mqm_table_kernel) evaluates the same expressions: same bits
  static const double M[6][6] = {{1, 0, 0, 0, 0, 0},      {-5, 5, 0, 0, 0, 0},      {10, -20, 10, 0, 0, 0},
                                 {-10, 30, -30, 10, 0, 0}, {5, -20, 30, -20, 5, 0}, {-1, 5, -10, 10, -5, 1}};
  for (int axis = 0; axis < 2; axis++) {
    const double *w = axis == 0 ? sh->w_s : sh->w_l;
    for (int d = 0; d < 4; d++)
      for (int j = 0; j < 6; j++)
        for (int i = 0; i <= j; i++) {
          double acc = 0.0;
          for (int a = d; a < 6; a++) {
            double t = 0.0;
            for (int b = d; b < 6; b++) {
              double num = w[d];
              for (int r = 0; r < d; r++) num *= double((a - r) * (b - r));
              t += num / double(a + b - 2 * d + 1) * M[b][j];
            }
            acc += M[a][i] * t;
          }
          table[(axis * 4 + d) * 21 + j * (j + 1) / 2 + i] = acc;
        }
  }
}

// The M'QM table of the weights (w_s, w_l), built on the device in stream order.
static void launch_mqm_table(hipStream_t stream, const double *w_s, const double *w_l, double *table) {
  MqmWeights mw;
  memcpy(mw.w[0], w_s, sizeof(double) * 4); memcpy(mw.w[1], w_l, sizeof(double) * 4);
  hipLaunchKernelGGL(mqm_table_kernel, dim3(1), dim3(192), 0, stream, mw, table);
}

void btrapz_single_forget(btrapz_ctx *c) { if (c) c->single_S = 0; }

// Test hook: the M'QM table as find_traj's single launch receives it (host builder) and as the batched entry points
// use it (device builder), [2][4][21] each -- the two must agree bit for bit (tests/test_gpu_properties.py).
BTRAPZ_EXPORT int btrapz_debug_mqm_tables(btrapz_ctx *c, const btrapz_shared *sh, double *host_table, double *device_table) {
  if (!c || !sh || !host_table || !device_table) return BTRAPZ_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  btrapz_mqm_table_host(sh, host_table);
  double *d = nullptr;
  HIPCHK(c, hipMalloc(&d, sizeof(double) * 168));
  launch_mqm_table(nullptr, sh->w_s, sh->w_l, d);
  hipError_t e = hipMemcpy(device_table, d, sizeof(double) * 168, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIPCHK(c, e);
  return BTRAPZ_OK;
}

// Test / analysis hook: iterations and status of the 2 B axis problems of the context's last batched solve
// ([b][axis], host arrays; synchronises the device).  tools/resume_model.py reads them.
BTRAPZ_EXPORT int btrapz_debug_axis_records(btrapz_ctx *c, int B, int *iters, int *status) {
  if (!c || B < 1 || (size_t)2 * B > c->d_axis_iters.cap() || !iters || !status) return BTRAPZ_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(iters, c->d_axis_iters, sizeof(int) * 2 * B, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(status, c->d_axis_status, sizeof(int) * 2 * B, hipMemcpyDeviceToHost));
  return BTRAPZ_OK;
}
// ... and the keys [2][B] the last capped solve's resume launch was bucketed by (0: the axis problem was not handed over)
BTRAPZ_EXPORT int btrapz_debug_resume_keys(btrapz_ctx *c, int B, int *keys) {
  if (!c || B < 1 || !keys || c->d_susp_ints.cap() < 400 + 4 * (size_t)B) return BTRAPZ_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(keys, c->d_susp_ints + 400, sizeof(int) * 2 * B, hipMemcpyDeviceToHost));
  return BTRAPZ_OK;
}
// ... the schedule of the lean two-launch solves of uniform batches in memory order that follow (0: chosen from what
// the last finished solve of the same shape handed over; -1: never three launches; 1 / 2: three launches with the s / l
// axis first; 3 / 4: the s / l axis first and the other one quiet, uncapped), and the number of solve-kernel launches the
// main step of the last solve made (1, 2 or 3)
BTRAPZ_EXPORT int btrapz_debug_set_schedule(btrapz_ctx *c, int mode) {
  if (!c || mode < -1 || mode > 4) return BTRAPZ_EINVAL;
  c->schedule_mode = mode;
  return BTRAPZ_OK;
}
BTRAPZ_EXPORT int btrapz_debug_solve_launches(const btrapz_ctx *c) { return c ? c->last_launches : -1; }

int btrapz_launch_single(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt, int S, const double *in,
                         double *out, int max_points, int warm, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!c || !sh || S < 1 || S > BTRAPZ_MAX_SEGMENTS || !in || !out || max_points < 1 || !options_ok(c, opt)) return BTRAPZ_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  KernelArgs a;
  fill_parameters(a, sh, opt, nullptr);
  a.B = 1; a.S = S; a.seg_stride = S; a.order = nullptr; a.seg_count = nullptr; a.cand_prefix = nullptr; a.wave_prefix = nullptr;
  const double *mqm = in + (size_t)BTRAPZ_NUM_SEG_FIELDS * S + 18;
  a.seg = in; a.init = in + (size_t)BTRAPZ_NUM_SEG_FIELDS * S; a.ref_end = a.init + 6; a.dl_bounds = a.ref_end + 2; a.mqm = mqm;
  // what the kernel reads back stays in device memory: the context's per-axis records and a control-point block
  TRY(ensure_axis_ws(c, 2));
  GROW(c, d_single, sizeof(double) * 12 * BTRAPZ_MAX_SEGMENTS);
  TRY(ws_wait(c, stream));
  a.axis_obj = c->d_axis_obj; a.axis_status = c->d_axis_status; a.axis_iters = c->d_axis_iters;
  a.ctrl = c->d_single; a.queue = nullptr; a.x_out = nullptr; a.axis_viol = nullptr;
  // at most 21 segments: the split form (rows of a segment over three lanes), ~0.8 of the time per iteration
  const bool split_form = S <= 21 && !(opt && opt->split < 0);   // (find_traj maps BTRAPZ_SPLIT onto opt->split)
  if (warm) {
    const size_t nx = 2 * 64 * 3, nl = 2 * 36 * 64, set = nx + nl;
    GROW(c, d_single_warm, sizeof(double) * 2 * set);
    double *rd = c->d_single_warm + (size_t)c->single_flip * set, *wr = c->d_single_warm + (size_t)(1 - c->single_flip) * set;
    const bool have = c->single_S == S && c->single_variant == sh->variant;
    // layouts for B = 1, seg_stride = S: x [2][S][3], lam [2][36][1][S]
    a.x0 = have ? rd : nullptr; a.lam0 = have ? rd + nx : nullptr;
    a.x_out = wr; a.lam_out = wr + nx;
    c->single_flip = 1 - c->single_flip; c->single_S = S; c->single_variant = sh->variant;
  }
  auto kernel = warm ? (split_form ? single_candidate_warm_split_kernel : single_candidate_warm_kernel)
                     : (split_form ? single_candidate_split_kernel : single_candidate_kernel);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(128), 0, stream, a, mqm, sh->delta, max_points, out);
  TRY(ws_close(c, stream));
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

// ---- the batched solve: what solve_common and btrapz_solve_sets_device share, then solve_common's steps -----------------

// Histogram -> prefix -> scatter: the candidates whose key is listed, bucket by bucket (btrapz_kernels.hip).  ny is the
// grid's y extent: 2 builds the lists of both axes in one launch each (keys [2][B], tables [2][198], lists [2][B]).
static void launch_bucket_lists(hipStream_t stream, unsigned ny, int B, int S, const int *keys, int *tables, int *lists,
                                double *obj, int *status, int *iters, int fixed_S) {
  const unsigned nb = (unsigned)((B + 255) / 256);
  hipLaunchKernelGGL(bucket_hist_kernel, dim3(nb, ny), dim3(256), 0, stream, B, S, keys, tables, fixed_S);
  hipLaunchKernelGGL(bucket_prefix_kernel, dim3(1, ny), dim3(64), 0, stream, tables, fixed_S);
  hipLaunchKernelGGL(bucket_scatter_kernel, dim3(nb, ny), dim3(256), 0, stream, B, S, keys, tables, lists, obj, status, iters, fixed_S);
}

// What the choice of form depends on.  split, lean, cap_iter and queue are REQUESTS (0 automatic, > 0 on, < 0 off) that
// the caller has resolved: solve_common from btrapz_options and, in experiment builds, the environment (solve_requests);
// btrapz_solve_sets_device from btrapz_options alone, and with cap_iter = -1 (it never runs the two launches).
struct FormQuery {
  int B, S, elastic, max_iter, unc_start, resident_waves;
  bool ragged, warm_kernel, ordered, compact;   // ordered: the launch goes through a candidate list (a.order)
  int split, lean, cap_iter; bool queue;        // the requests
  unsigned blocks;                              // wavefronts of the one-launch packed form
};
struct Form { bool long_form, split_on, lean_on, capped, queue_on; int cap_iter; };   // cap_iter: iterations of the first of two launches

static Form choose_form(const FormQuery &q) {
  Form f;
  f.long_form = !q.ragged && q.S > BTRAPZ_MAX_SEGMENTS;   // one axis problem per workgroup (ipm_solve_long_kernel)
  f.queue_on = q.queue;
  // Few candidates: one per wavefront, rows over three lanes (btrapz_options.split; ipm_solve_split_kernel)
  f.split_on = !q.ordered && !q.warm_kernel && q.S <= 21 &&
               (q.split > 0 || (q.split == 0 && 2u * (unsigned)q.B <= (unsigned)q.resident_waves));
  // Two wavefronts per SIMD (btrapz_options.lean / BTRAPZ_LEAN; btrapz_lean.hip): cold solves of at most 64 segments
  const bool lean_ok = !f.long_form && !f.split_on && !f.queue_on && (q.S >= 3 || q.ragged) && q.S <= BTRAPZ_MAX_SEGMENTS && q.unc_start == 0;   // (uniform batches of one or two segments: the packed form -- only the lean kernels of ragged batches carry the end-lane fix-up)
  // Automatic: batches that give every SIMD its two wavefronts several times over.  Measured (tools/lean_bench.py,
  // scenario_1 x 20, packed -> lean, one launch): 512 candidates 0.375 -> 0.435 ms, 2 048 0.447 -> 0.517, 8 192 1.117 ->
  // 1.032, 16 384 1.964 -> 1.733, 65 536 7.05 -> 5.61: a lone wavefront per SIMD runs the packed form's shorter
  // instruction stream faster; from about three wavefronts per SIMD on the second resident one pays.
  const unsigned est_waves = 2u * (unsigned)((size_t)q.B / (size_t)(64 / (q.S < 64 ? q.S : 64)) + 1);
  // (round 5, re-measured with the final kernels, packed -> lean in one launch, ms: scenario_1 x 20 -- 512 candidates
  //  0.30 -> 0.34, 2 048 0.40 -> 0.38, 4 096 0.63 -> 0.52, 8 192 0.91 -> 0.78; generic x 10 -- 2 048 0.14 -> 0.17, 4 096
  //  0.22 -> 0.19, 8 192 0.33 -> 0.29: the crossover sits at about 1.25 wavefronts per SIMD, not at 3)
  f.lean_on = lean_ok && (q.lean > 0 || (q.lean == 0 && 4u * est_waves >= 5u * (unsigned)q.resident_waves));
  // Two launches for uniform cold batches much larger than the machine (btrapz_options.cap_iter / BTRAPZ_CAP): every
  // group stops at cap_iter iterations, the unfinished ones are carried on by a second launch, like with like, the
  // far-from-converged first (CAPPED / RESUME in btrapz_kernels.hip).  Same iterates, same results.
  // Measured (tools/cap_bench.py, 65 536 candidates, one launch -> two): scenario_1 x 20 7.00 -> 6.39 ms, its cuboid
  // variant 6.70 -> 6.35, generic x 20 5.21 -> 5.18, scenario_1 x 10 2.24 -> 2.46 (six groups per wavefront: what a
  // lone straggler wastes is less than what the second launch costs).  Automatic (cap_iter = 0): 6 for uniform cold
  // batches of 16 to 64 segments that fill the device at least eight times over; -1: never.
  // Ragged batches (round 3, late): the same two launches on request (cap_iter > 0), the resume lists bucketed by
  // segment count instead of by convergence class.  Not automatic: measured on 65 536 candidates, knots -> control
  // points (tools/pipeline_bench.py, one launch -> cap 8): jittered c_road_s1_3.txt, 8 segments, a quarter of the
  // candidates infeasible (16-19 iterations against 9-12) 3.20 -> 2.90 ms; scenario_1 at knot level, 18-24 segments
  // 9.56 -> 9.79; two-car scenes, 7-9 segments, all feasible 3.21 -> 3.54 -- it pays where iteration counts spread
  // widely, which the library does not know.
  f.cap_iter = q.cap_iter;
  // (S <= 32: a wavefront that holds ONE group has nobody to wait for -- with 33..64 segments every group would be
  //  "alone" at once and a quarter of the batch be written out and read back for nothing: ADVICE r4)
  if (f.cap_iter == 0 && !q.ragged && q.S >= 16 && q.S <= 32 && q.blocks >= 8u * (unsigned)q.resident_waves) f.cap_iter = 6;
  f.capped = f.cap_iter > 0 && !f.long_form && !f.split_on && (!q.ordered || q.ragged || q.compact) && !q.warm_kernel && !f.queue_on && q.S <= BTRAPZ_MAX_SEGMENTS &&
             f.cap_iter < q.max_iter && f.cap_iter + BTRAPZ_CAP_HI < 4000 && q.elastic != 2;   // (4000: the lean record's 12-bit counters)
  return f;
}

// Ragged batch with slots for more than 64 segments: the candidates that HAVE more than 64 (the bucket kernels have
// marked them "no usable corridor") are solved by the long form, one launch per segment count with the candidates of
// that count listed.  The counts come to the host for this (one synchronisation: horizons beyond 64 s are not the
// throughput path); cold solves without a rescue pass -- what the long form serves.  The reference has no limit on the
// segment count (std::vector, src/solve_3d.cc:323-486,729-772).  launch(args, n, s): the long-form kernel of the caller
// over the n listed candidates of s segments.
template <class Launch>
static int solve_long_candidates(btrapz_ctx *c, hipStream_t stream, const KernelArgs &a, const int *seg_count, Launch launch) {
  const int B = a.B, S = a.S;
  std::vector<int> counts((size_t)B);
  HIPCHK(c, hipMemcpyAsync(counts.data(), seg_count, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  const int smax = S < BTRAPZ_MAX_SEGMENTS_LONG ? S : BTRAPZ_MAX_SEGMENTS_LONG;
  std::vector<std::vector<int>> by_count((size_t)smax + 1);
  size_t n_long = 0;
  for (int b = 0; b < B; b++)
    if (counts[b] > BTRAPZ_MAX_SEGMENTS && counts[b] <= smax) { by_count[(size_t)counts[b]].push_back(b); ++n_long; }
  if (!n_long) return BTRAPZ_OK;
  GROW(c, d_long_list, sizeof(int) * n_long);
  std::vector<int> flat; flat.reserve(n_long);
  for (const auto &l : by_count) flat.insert(flat.end(), l.begin(), l.end());
  HIPCHK(c, hipMemcpyAsync(c->d_long_list, flat.data(), sizeof(int) * n_long, hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipStreamSynchronize(stream));   // (flat goes out of scope)
  size_t off = 0;
  for (int s = BTRAPZ_MAX_SEGMENTS + 1; s <= smax; s++) {
    const size_t n = by_count[(size_t)s].size();
    if (!n) continue;
    KernelArgs l = a;
    l.S = s; l.order = c->d_long_list + off; l.bucket_S = (int)n; l.seg_count = nullptr; l.cand_prefix = nullptr; l.wave_prefix = nullptr;
    launch(l, (unsigned)n, s);
    HIPCHK(c, hipGetLastError());
    off += n;
  }
  c->last_form |= 16;   // (+ 16: the long form served part of a ragged batch)
  return BTRAPZ_OK;
}

// Last step of a solve: per-candidate cost, status and iterations from the per-axis records; closes the launch sequence.
static int finalize_and_close(btrapz_ctx *c, hipStream_t stream, int B, double *cost, int *status, int *iters) {
  hipLaunchKernelGGL(finalize_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, c->d_axis_obj, c->d_axis_status,
                     c->d_axis_iters, cost, status, iters);
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

// The kernel arguments of a batched solve that are the same in every form: shapes, the batch, the context's per-axis records.
static void batch_arguments(btrapz_ctx *c, KernelArgs &a, int B, int S, const double *seg, const double *init, const double *ref_end,
                            const double *dl_bounds, double *ctrl, const double *mqm) {
  a.B = B; a.S = S; a.seg_stride = S; a.order = nullptr; a.seg_count = nullptr; a.cand_prefix = nullptr; a.wave_prefix = nullptr;
  a.seg = seg; a.init = init; a.ref_end = ref_end; a.dl_bounds = dl_bounds; a.mqm = mqm;
  a.ctrl = ctrl; a.axis_obj = c->d_axis_obj; a.axis_status = c->d_axis_status; a.axis_iters = c->d_axis_iters;
  a.axis_viol = c->d_axis_viol; c->viol_valid = 0;
  a.x_out = nullptr; a.queue = c->d_queue;
}

// State of one solve_common call, handed from step to step.
struct Solve {
  btrapz_ctx *c; hipStream_t stream; const btrapz_options *opt;
  int B, S; const int *seg_count;   // S: segments of a uniform batch (seg_count == nullptr), slot stride of a ragged one
  KernelArgs a;
  int elastic; bool compact, warm_kernel;
  bool long_warm;                   // btrapz_solve_long_warm_device: candidates of 65..256 segments take ipm_solve_long_warm_kernel
  bool long_rescue;                 // btrapz_solve_long_rescue_device: ... and have their rescue pass up to 256 segments, listed ones too
  unsigned blocks;                  // wavefronts of the one-launch packed / lean form
};

// Step: the batch-invariant M'QM table, rebuilt only when the weights change.
static int solve_weights_table(btrapz_ctx *c, const btrapz_shared *sh, hipStream_t stream) {
  double wkey[8];
  memcpy(wkey, sh->w_s, sizeof(double) * 4); memcpy(wkey + 4, sh->w_l, sizeof(double) * 4);
  if (memcmp(wkey, c->h_mqm_w, sizeof(wkey)) == 0) return BTRAPZ_OK;
  // built on the device, in stream order: no host buffer to keep alive, no synchronisation, and a launch that is
  // still reading the previous table (same stream, or ordered by the event of ws_open) finishes first
  launch_mqm_table(stream, sh->w_s, sh->w_l, c->d_mqm);
  HIPCHK(c, hipGetLastError());
  memcpy(c->h_mqm_w, wkey, sizeof(wkey));
  return BTRAPZ_OK;
}

// Step: pre-pass and ordering.  Sets a.order and the bucket tables where the launches go through a list, and s.blocks.
static int solve_order_candidates(Solve &s, const btrapz_shared *sh, const int *hint) {
  btrapz_ctx *c = s.c; KernelArgs &a = s.a;
  const int B = s.B, S = s.S, *seg_count = s.seg_count;
  // Candidates that cannot start (btrapz_options.compact): a pre-pass lists the live ones, the launches below take them
  // through a.order.  Cold solves without a rescue pass only (the rescue pass solves what stalled, axis by axis: it needs
  // every axis's record); automatic for large ragged batches and large batches of the cuboid variant.
  const bool warm_args = a.x0 || a.lam0 || a.lam_out;
  const int compact_opt = s.opt ? s.opt->compact : 0;
  const unsigned waves_needed = 2u * (unsigned)((size_t)B / (size_t)(64 / (S < 64 ? S : 64)) + 1);
  s.compact = s.elastic == 0 && !warm_args && !hint && S <= BTRAPZ_MAX_SEGMENTS && a.unc_start == 0 &&
              (compact_opt > 0 || (compact_opt == 0 && (seg_count || sh->variant == BTRAPZ_CUBOID) && waves_needed >= 3u * (unsigned)c->resident_waves));
  int *compact_keys = nullptr;
  if (s.compact) {
    GROW(c, d_rescue, sizeof(int) * 4 * (size_t)B);   // (keys [B] at the front of the rescue pass's lists: no rescue pass in this solve)
    compact_keys = c->d_rescue;
    KernelArgs pa = a;
    pa.seg_stride = S;
    const int pre_gpw = 64 / S;   // (S: the slot stride, at most 64 here)
    hipLaunchKernelGGL(prestart_kernel, dim3((unsigned)((B + pre_gpw - 1) / pre_gpw)), dim3(64), 0, s.stream, pa, seg_count ? 0 : S, seg_count, compact_keys);
    HIPCHK(c, hipGetLastError());
  }
  if (seg_count || hint || s.compact) {
    GROW(c, d_order, sizeof(int) * (size_t)B);
    GROW(c, d_meta, sizeof(int) * 198);
    HIPCHK(c, hipMemsetAsync(c->d_meta, 0, sizeof(int) * 198, s.stream));
    // keys: segment counts (ragged), hint classes (uniform, fixed_S > 0), or -- compact -- the pre-pass's list keys: the
    // count / 1 of a live candidate, 0 for one that is not listed (uniform: fixed_S < 0, "a key <= 0 is not listed"); the
    // pre-pass has written the records of what it dropped, so the scatter kernel writes none
    const int fixed_S = seg_count ? 0 : (s.compact ? -S : S);
    const int *keys = s.compact ? compact_keys : seg_count ? seg_count : hint;
    launch_bucket_lists(s.stream, 1, B, S, keys, c->d_meta, c->d_order, s.compact ? (double *)nullptr : c->d_axis_obj.ptr(),
                        s.compact ? (int *)nullptr : c->d_axis_status.ptr(), s.compact ? (int *)nullptr : c->d_axis_iters.ptr(), fixed_S);
    HIPCHK(c, hipGetLastError());
    a.order = c->d_order; a.seg_count = seg_count; a.cand_prefix = c->d_meta; a.wave_prefix = c->d_meta + 66;
    a.bucket_S = seg_count ? 0 : S;
    // upper bound on wavefront pairs without a host round trip: every bucket wastes less than one pair
    const int gpw_min = seg_count ? 1 : 64 / S;
    s.blocks = 2u * (unsigned)(B / gpw_min + 65);
  } else {
    const int gpw = S <= 64 ? 64 / S : 1;  // axis problems per wavefront; wave w: axis w&1 of candidates (w>>1)*gpw + [0,gpw)
    s.blocks = 2u * (unsigned)((B + gpw - 1) / gpw);
  }
  s.warm_kernel = a.x0 || a.lam0 || a.lam_out;   // (a hint alone only reorders the candidates)
  return BTRAPZ_OK;
}

// The requests of btrapz_options for the choice of form, with the environment's word in experiment builds
// (experiment_env: BTRAPZ_SPLIT is read at every call, the others once).
static void solve_requests(const btrapz_options *opt, FormQuery &q) {
  // Uniform cold batches with several candidates per resident wavefront slot may run on persistent wavefronts that
  // draw candidates from a queue (btrapz_options.queue / BTRAPZ_QUEUE=1): a wavefront's groups then do not wait for
  // its slowest one, at the price of ~half an iteration per hand-over for all of its groups.  Measured (65 536
  // candidates, kernel ms off -> on): scenario_1 x 20 6.93 -> 6.59, its cuboid variant (16 % stalling) 6.57 -> 5.71,
  // generic x 20 5.12 -> 5.33, scenario_1 x 10 2.13 -> 2.34: it pays where iteration counts spread widely, so it is
  // the caller's choice and off by default.
#ifdef BTRAPZ_EXPERIMENTS
  static const int queue_env = [] { const char *q = experiment_env("BTRAPZ_QUEUE"); return q ? (*q == '0' ? -1 : 1) : 0; }();
  q.queue = queue_env ? queue_env > 0 : (opt && opt->queue > 0);
#else
  q.queue = false;   // (btrapz_options.queue: scheduling only, a measured loss -- honoured by experiment builds, ignored here)
#endif
  const char *split_q = experiment_env("BTRAPZ_SPLIT");
  const int split_env = split_q ? (*split_q == '0' ? -1 : 1) : 0;
  q.split = split_env ? split_env : (opt ? opt->split : 0);
  static const int cap_env = [] { const char *q = experiment_env("BTRAPZ_CAP"); return q ? atoi(q) : -1; }();
  q.cap_iter = cap_env > 0 ? cap_env : cap_env == 0 ? -1 : (opt ? opt->cap_iter : 0);   // BTRAPZ_CAP=0: never
  static const int lean_env = [] { const char *q = experiment_env("BTRAPZ_LEAN"); return q ? (*q == '0' ? -1 : 1) : 0; }();
  q.lean = lean_env ? lean_env : (opt ? opt->lean : 0);
}

// Workspace of the two launches: hand-over slots for BTRAPZ_SUSP_PERCENT of the axis problems (a group that finds none simply
// goes on), 74 doubles per segment each -- 19 KB per slot at 64 segments, 388 MB for 65 536 candidates of 20 -- but
// never more than BTRAPZ_SUSP_BYTES_MAX.  When the device cannot give it, a solve that chose the two launches by
// itself (cap_iter = 0) runs as one launch (*slots_out = 0); one that was asked for them (requested) fails with BTRAPZ_ENOMEM.
static int capped_workspace(Solve &s, bool requested, size_t *slots_out) {
  btrapz_ctx *c = s.c; const size_t B = (size_t)s.B, S = (size_t)s.S;
  size_t slots = 2 * B * (size_t)BTRAPZ_SUSP_PERCENT / 100;
  if (slots < 1024) slots = 1024;
  const size_t slots_max = (size_t)BTRAPZ_SUSP_BYTES_MAX / (sizeof(double) * 74 * S);
  if (slots > slots_max) slots = slots_max;
  if (slots > (size_t)0x7fffffff) slots = (size_t)0x7fffffff;   // (susp_cap is an int)
  bool ok = slots >= 64;
  ok = ok && c->d_susp_state.grow(sizeof(double) * slots * 74 * S) == hipSuccess;
  ok = ok && c->d_susp_ints.grow(sizeof(int) * (400 + 4 * B)) == hipSuccess;   // count[4] tables[2][198] keys[2][B] slots[2B]
  ok = ok && c->d_rescue.grow(sizeof(int) * 4 * B) == hipSuccess;
  ok = ok && c->d_rescue_meta.grow(sizeof(int) * 2 * 198) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();   // (the failed allocation's error is handled here)
    if (requested) { c->err = "btrapz_options.cap_iter: no memory for the hand-over workspace"; return BTRAPZ_ENOMEM; }
  }
  *slots_out = ok ? slots : 0;
  return BTRAPZ_OK;
}

// The two-launch solve: capped launch, the lists of what it handed over, resume launch.
static int launch_capped_and_resume(Solve &s, const Form &f, size_t slots) {
  btrapz_ctx *c = s.c; const int B = s.B, S = s.S;
  const bool ragged = s.seg_count != nullptr;
  // (one workspace, one memset: the counter, the bucket tables of both axes and the keys are zeroed together)
  int *count = c->d_susp_ints, *tables = count + 4, *keys = tables + 2 * 198, *slot_of = keys + 2 * (size_t)B;
  HIPCHK(c, hipMemsetAsync(count, 0, sizeof(int) * (400 + 2 * (size_t)B), s.stream));
  KernelArgs p1 = s.a;
  p1.cap_iter = f.cap_iter; p1.cap_alone = BTRAPZ_CAP_ALONE; p1.cap_hi = f.cap_iter + BTRAPZ_CAP_HI; p1.cap_score = BTRAPZ_CAP_SCORE; p1.susp_cap = (int)slots; p1.susp_state = c->d_susp_state; p1.susp_count = count;
  p1.susp_slot = slot_of; p1.susp_key = keys;
  // (the ordered instantiation serves ragged batches and uniform ones that go through a.order -- the pre-pass -- and
  //  gives a uniform batch the bits of the memory-order one: btrapz_lean_body.h)
  auto first = f.lean_on ? (p1.order ? ipm_solve_lean_capped_ordered_kernel : ipm_solve_lean_capped_kernel)
                         : (p1.order ? ipm_solve_capped_ordered_kernel : ipm_solve_capped_kernel);
  hipLaunchKernelGGL(first, dim3(s.blocks), dim3(64), 0, s.stream, p1, (const double *)c->d_mqm);
  int *lists = c->d_rescue + 2 * (size_t)B;
  const int list_S = ragged ? 0 : -S;   // ragged: keys are segment counts; uniform: convergence classes, 0 = not listed
  // both axes in one launch each (gridDim.y = 2: keys [2][B], tables [2][198], lists [2][B])
  launch_bucket_lists(s.stream, 2, B, S, keys, tables, lists, nullptr, nullptr, nullptr, list_S);
  KernelArgs p2 = p1;
  p2.cap_iter = 0; p2.order = lists; p2.seg_count = nullptr; p2.cand_prefix = tables; p2.wave_prefix = tables + 66;
  p2.bucket_S = ragged ? 0 : S;
  // (ragged: no candidate has more than min(S, 64) segments, so no wavefront holds fewer groups than that allows)
  const unsigned rblocks = 2u * (unsigned)(slots / (size_t)(64 / (S < 64 ? S : 64)) + 65);
  hipLaunchKernelGGL(f.lean_on ? ipm_solve_lean_resume_kernel : ipm_solve_resume_kernel, dim3(rblocks), dim3(64), 0, s.stream, p2, (const double *)c->d_mqm);
  c->last_form = f.lean_on ? 11 : 3;
  c->last_launches = 2;
  return BTRAPZ_OK;
}

// The schedule of a lean two-launch solve of a uniform batch in memory order.  -1: the two launches; 0 / 1: three
// launches with the s / l axis first (launch_pipelined); 2 / 3: the s / l axis first and the other one quiet
// (launch_quiet_axis).  Automatic: from what the last finished solve of this shape (S, variant) handed over per axis -- at
// least BTRAPZ_QUIET_RATIO times more problems of one axis than of the other: that axis first, the other quiet; at least
// BTRAPZ_PIPELINE_RATIO times more: that axis first -- the library cannot know the spread axis before it solves, and
// consecutive batches of a planner are of one family.  Every schedule returns the one-launch solve's bits: what is
// remembered only moves time.
static int pipeline_schedule(btrapz_ctx *c, int S, int variant) {
#if BTRAPZ_PIPELINE
  if (c->schedule_mode != 0) return c->schedule_mode < 0 ? -1 : c->schedule_mode - 1;
  if (c->pipe_pending) {   // never waited for: counts that have not landed leave the ones before them in place
    if (hipEventQuery(c->pipe_landed) == hipSuccess) {
      c->pipe_pending = false;
      c->pipe_S = c->pipe_pending_S; c->pipe_variant = c->pipe_pending_variant;
      c->pipe_count[0] = c->h_pipe_counts[0]; c->pipe_count[1] = c->h_pipe_counts[1];
    } else {
      (void)hipGetLastError();   // (hipErrorNotReady is an answer, not an error of this solve)
    }
  }
  if (c->pipe_S != S || c->pipe_variant != variant) return -1;
  const long long n0 = c->pipe_count[0], n1 = c->pipe_count[1];
  if (n0 > 0 && n0 >= BTRAPZ_QUIET_RATIO * n1) return 2;
  if (n1 > 0 && n1 >= BTRAPZ_QUIET_RATIO * n0) return 3;
  if (n0 > 0 && n0 >= BTRAPZ_PIPELINE_RATIO * n1) return 0;
  if (n1 > 0 && n1 >= BTRAPZ_PIPELINE_RATIO * n0) return 1;
#endif
  return -1;
}

// ... and what this solve handed over, for the next one: the two list lengths (cand_prefix[65] of each axis's table),
// copied by the device behind the bucketing, and the event that says they have landed.  An axis that ran quiet
// (quiet_axis 0 / 1; -1: none) has no list: its entry is the estimate of quiet_counts_kernel (btrapz_lean_quiet.hip) of
// what the cap would have made it hand over -- or the library would never learn that the axis has started to talk.
// Failing to get the pinned memory or the event only means that the schedule is never chosen automatically.
static void pipeline_remember(Solve &s, int *count, int variant, int quiet_axis, int cap_iter) {
#if BTRAPZ_PIPELINE
  btrapz_ctx *c = s.c;
  const int *tables = count + 4;
  if (!c->h_pipe_counts) {
    if (hipHostMalloc((void **)&c->h_pipe_counts, sizeof(int) * 2, hipHostMallocDefault) != hipSuccess) { c->h_pipe_counts = nullptr; (void)hipGetLastError(); return; }
    c->h_pipe_counts[0] = 0; c->h_pipe_counts[1] = 0;
  }
  if (!c->pipe_landed && hipEventCreateWithFlags(&c->pipe_landed, hipEventDisableTiming) != hipSuccess) { c->pipe_landed = nullptr; (void)hipGetLastError(); return; }
  if (quiet_axis < 0) {
    hipLaunchKernelGGL(pipe_counts_kernel, dim3(1), dim3(64), 0, s.stream, tables, c->h_pipe_counts);
  } else {
    // (one thread per memory-order wavefront; count[1], count[2]: the pad behind the slot counter, zeroed with it)
    const int gpw = 64 / s.S;
    const unsigned waves = (unsigned)((s.B + gpw - 1) / gpw);
    hipLaunchKernelGGL(quiet_counts_kernel, dim3((waves + 255u) / 256u), dim3(256), 0, s.stream, (const int *)s.a.axis_iters, s.B, gpw, quiet_axis,
                       cap_iter, cap_iter + BTRAPZ_CAP_HI, tables, count + 1, c->h_pipe_counts);
  }
  if (hipEventRecord(c->pipe_landed, s.stream) != hipSuccess) { (void)hipGetLastError(); c->pipe_pending = false; c->pipe_S = 0; return; }
  c->pipe_pending = true; c->pipe_pending_S = s.S; c->pipe_pending_variant = variant;
#else
  (void)s; (void)count; (void)variant; (void)quiet_axis; (void)cap_iter;
#endif
}

// The lean two-launch solve of a uniform batch in memory order as three launches on the one stream:
//   1. the capped launch of axis a0 alone, then the bucketing of ITS hand-over lists;
//   2. one grid: the resume wavefronts of a0 (dispatched first: their long dependent chains run beside full-width work)
//      and, behind them, the capped launch of the other axis a1;
//   3. the bucketing of a1's lists and a1's resume launch.
// Every dependency is a kernel boundary; inside launch 2 no wavefront waits for another (btrapz_lean_pipe.hip).  One
// KernelArgs serves all three; one memset, one slot counter: the slots a1 takes lie behind those a0's resume part reads.
static int launch_pipelined(Solve &s, const Form &f, size_t slots, int a0) {
  btrapz_ctx *c = s.c; const int B = s.B, S = s.S, a1 = 1 - a0;
  int *count = c->d_susp_ints, *tables = count + 4, *keys = tables + 2 * 198, *slot_of = keys + 2 * (size_t)B;
  HIPCHK(c, hipMemsetAsync(count, 0, sizeof(int) * (400 + 2 * (size_t)B), s.stream));
  int *lists = c->d_rescue + 2 * (size_t)B;
  KernelArgs p = s.a;
  p.cap_iter = f.cap_iter; p.cap_alone = BTRAPZ_CAP_ALONE; p.cap_hi = f.cap_iter + BTRAPZ_CAP_HI; p.cap_score = BTRAPZ_CAP_SCORE; p.susp_cap = (int)slots; p.susp_state = c->d_susp_state; p.susp_count = count;
  p.susp_slot = slot_of; p.susp_key = keys;
  // (what the resume parts read and the memory-order capped parts do not: the lists and their tables, [2][..] by axis)
  p.order = lists; p.seg_count = nullptr; p.cand_prefix = tables; p.wave_prefix = tables + 66; p.bucket_S = S;
  const int gpw = 64 / S;
  const unsigned cblocks = (unsigned)((B + gpw - 1) / gpw);            // one axis of the batch
  const unsigned rblocks = (unsigned)(slots / (size_t)gpw + 65);       // one axis's lists at most: every class wastes less than one wavefront
  auto bucket = [&](int ax) {
    launch_bucket_lists(s.stream, 1, B, S, keys + (size_t)ax * B, tables + ax * 198, lists + (size_t)ax * B, nullptr, nullptr, nullptr, -S);
  };
  hipLaunchKernelGGL(ipm_solve_lean_pipe_capped_kernel, dim3(cblocks), dim3(64), 0, s.stream, p, (const double *)c->d_mqm, a0);
  bucket(a0);
  hipLaunchKernelGGL(ipm_solve_lean_pipe_kernel, dim3(rblocks + cblocks), dim3(64), 0, s.stream, p, (const double *)c->d_mqm, (int)rblocks, a0, a1);
  bucket(a1);
  hipLaunchKernelGGL(ipm_solve_lean_pipe_resume_kernel, dim3(rblocks), dim3(64), 0, s.stream, p, (const double *)c->d_mqm, a1);
  c->last_form = 11;
  c->last_launches = 3;
  return BTRAPZ_OK;
}

// ... and with axis a1 quiet (btrapz_lean_quiet.hip): a1 hands nothing over, so it needs no cap, no lists
// and no resume launch -- it goes through the plain one-launch body, behind a0's resume wavefronts:
//   1. the capped launch of axis a0 alone, then the bucketing of its hand-over lists (as in launch_pipelined);
//   2. one grid: the resume wavefronts of a0 and, behind them, axis a1 of the batch in memory order, to the end.
// Two solve kernels and one bucketing triple; a1's keys stay as the memset left them.  btrapz_debug_solve_launches
// answers 3 as for launch_pipelined: it is what tells an axis-first schedule from the two launches of both axes.
static int launch_quiet_axis(Solve &s, const Form &f, size_t slots, int a0) {
  btrapz_ctx *c = s.c; const int B = s.B, S = s.S, a1 = 1 - a0;
  int *count = c->d_susp_ints, *tables = count + 4, *keys = tables + 2 * 198, *slot_of = keys + 2 * (size_t)B;
  HIPCHK(c, hipMemsetAsync(count, 0, sizeof(int) * (400 + 2 * (size_t)B), s.stream));
  int *lists = c->d_rescue + 2 * (size_t)B;
  KernelArgs p = s.a;
  p.cap_iter = f.cap_iter; p.cap_alone = BTRAPZ_CAP_ALONE; p.cap_hi = f.cap_iter + BTRAPZ_CAP_HI; p.cap_score = BTRAPZ_CAP_SCORE; p.susp_cap = (int)slots; p.susp_state = c->d_susp_state; p.susp_count = count;
  p.susp_slot = slot_of; p.susp_key = keys;
  p.order = lists; p.seg_count = nullptr; p.cand_prefix = tables; p.wave_prefix = tables + 66; p.bucket_S = S;
  const int gpw = 64 / S;
  const unsigned cblocks = (unsigned)((B + gpw - 1) / gpw);
  const unsigned rblocks = (unsigned)(slots / (size_t)gpw + 65);
  hipLaunchKernelGGL(ipm_solve_lean_pipe_capped_kernel, dim3(cblocks), dim3(64), 0, s.stream, p, (const double *)c->d_mqm, a0);
  launch_bucket_lists(s.stream, 1, B, S, keys + (size_t)a0 * B, tables + a0 * 198, lists + (size_t)a0 * B, nullptr, nullptr, nullptr, -S);
  hipLaunchKernelGGL(ipm_solve_lean_quiet_kernel, dim3(rblocks + cblocks), dim3(64), 0, s.stream, p, (const double *)c->d_mqm, (int)rblocks, a0, a1);
  c->last_form = 11;
  c->last_launches = 3;
  return BTRAPZ_OK;
}

// Step: the main launch -- the form is chosen, the two-launch solve gets its workspace, the kernels go out.
static int solve_main_launch(Solve &s, Form &f) {
  btrapz_ctx *c = s.c; KernelArgs &a = s.a;
  const int B = s.B, S = s.S;
  c->last_launches = 1;
  FormQuery q{};
  q.B = B; q.S = S; q.ragged = s.seg_count != nullptr; q.warm_kernel = s.warm_kernel; q.ordered = a.order != nullptr; q.compact = s.compact;
  q.elastic = s.elastic; q.max_iter = a.max_iter; q.unc_start = a.unc_start; q.resident_waves = c->resident_waves; q.blocks = s.blocks;
  solve_requests(s.opt, q);
  f = choose_form(q);
  if (f.long_form && (a.order || (s.warm_kernel && !s.long_warm) || s.elastic == 2 || (s.elastic == 1 && S > BTRAPZ_MAX_SEGMENTS_LONG_RESCUE && !s.long_rescue))) {
    c->err = "more than 64 segments: uniform cold solve only, rescue pass (elastic = 1) up to 192 segments";
    return BTRAPZ_EINVAL;
  }
  if (s.elastic == 2) return BTRAPZ_OK;   // (elastic rows for every candidate: the rescue pass is the solve)
  size_t slots = 0;   // (q.cap_iter > 0: asked for by the caller; the automatic choice falls back to one launch without the workspace)
  if (f.capped) TRY(capped_workspace(s, q.cap_iter > 0, &slots));
  if (slots) {
    // (three launches: the lean form on uniform batches in memory order; not the ordered path -- ragged batches, the
    //  pre-pass -- whose capped part needs a.order and the prefix tables for its own lists, nor the packed form)
    const bool pipe_ok = f.lean_on && !s.seg_count && !a.order;
    const int schedule = pipe_ok ? pipeline_schedule(c, S, a.sh.variant) : -1;
    if (schedule >= 2) TRY(launch_quiet_axis(s, f, slots, schedule - 2));
    else if (schedule >= 0) TRY(launch_pipelined(s, f, slots, schedule));
    else TRY(launch_capped_and_resume(s, f, slots));
    if (pipe_ok) pipeline_remember(s, c->d_susp_ints, a.sh.variant, schedule >= 2 ? 3 - schedule : -1, f.cap_iter);
  } else if (f.long_form && s.long_warm) {
    c->last_form = 16;   // (the warm instantiation, whatever the start: it is the one that writes lam_out)
    hipLaunchKernelGGL(ipm_solve_long_warm_kernel, dim3(2u * (unsigned)B), dim3(64u * (unsigned)((S + 63) / 64)), 0, s.stream, a, (const double *)c->d_mqm);
  } else if (f.long_form) {
    c->last_form = 2;
    hipLaunchKernelGGL(ipm_solve_long_kernel, dim3(2u * (unsigned)B), dim3(64u * (unsigned)((S + 63) / 64)), 0, s.stream, a, (const double *)c->d_mqm);
  } else if (f.split_on) {
    c->last_form = 1;
    hipLaunchKernelGGL(ipm_solve_split_kernel, dim3(2u * (unsigned)B), dim3(64), 0, s.stream, a, (const double *)c->d_mqm);
#ifdef BTRAPZ_EXPERIMENTS
  } else if (f.queue_on && !a.order && !s.warm_kernel && s.blocks >= 3u * (unsigned)c->resident_waves) {
    HIPCHK(c, hipMemsetAsync(c->d_queue, 0, sizeof(int) * 2, s.stream));
    c->last_form = 4;
    hipLaunchKernelGGL(ipm_solve_queue_kernel, dim3((unsigned)c->resident_waves & ~1u), dim3(64), 0, s.stream, a, (const double *)c->d_mqm);
#endif
  } else if (f.lean_on) {
    c->last_form = 8;
    // (a.order: the buckets of a ragged batch, or the hint classes / the pre-pass's list of a uniform one)
    auto lean_kernel = s.warm_kernel ? (a.order ? ipm_solve_lean_warm_ordered_kernel : ipm_solve_lean_warm_kernel)
                                     : (a.order ? ipm_solve_lean_ordered_kernel : ipm_solve_lean_kernel);
    hipLaunchKernelGGL(lean_kernel, dim3(s.blocks), dim3(64), 0, s.stream, a, (const double *)c->d_mqm);
  } else {
    c->last_form = 0;
    auto kernel = s.warm_kernel ? (a.order ? ipm_solve_warm_ordered_kernel : ipm_solve_warm_kernel)
                                : (a.order ? ipm_solve_ordered_kernel : ipm_solve_kernel);
    hipLaunchKernelGGL(kernel, dim3(s.blocks), dim3(64), 0, s.stream, a, (const double *)c->d_mqm);
  }
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

// The arguments of both rescue passes: cold, and patient.
// Least-violation problems take 25-40 iterations, and up to 60 where a row's violation is fixed by the data (an
// initial state outside segment 0's rows): its multiplier has to grow to violation / delta before the score moves.
// The pass is rare and not on the throughput path: be patient (the oracle's relaxed solve is; with these limits every
// one of 6 000 fuzzed find_traj calls decides as it does, with 80 / 2x / 2x six of 4 800 did not).
static KernelArgs rescue_arguments(const KernelArgs &a) {
  KernelArgs e = a;
  e.x0 = nullptr; e.lam0 = nullptr; e.lam_out = nullptr;
  e.max_iter = a.max_iter < 120 ? 120 : a.max_iter;
  e.tau_iters = 0;                                  // conservative step rule throughout
  e.stall_start = 4 * BTRAPZ_STALL_START; e.stall_len = 4 * BTRAPZ_STALL_LENGTH;
  return e;
}

// Rescue launch of the long form over n candidates of `segs` segments -- a (with a.order == nullptr: the uniform batch in
// memory order; else the list of solve_long_candidates) are the arguments of the plain launch it follows.  One workgroup
// per axis problem again; those whose problem did not stall leave at once.  Up to 192 segments three wavefronts, beyond
// (btrapz_solve_long_rescue_device) the four-wavefront kernel: a width is served by ONE kernel, whichever path leads to it.
// set_index (btrapz_solve_long_sets_device): the same two kernels with SETS, every workgroup reading its candidate's set.
static void launch_long_rescue(btrapz_ctx *c, hipStream_t stream, const KernelArgs &a, unsigned n, int segs,
                               const int *set_index = nullptr, int n_sets = 0) {
  const KernelArgs e = rescue_arguments(a);
  const dim3 grid(2u * n), block(64u * (unsigned)((segs + 63) / 64));
  if (set_index) {
    auto kernel = segs > BTRAPZ_MAX_SEGMENTS_LONG_RESCUE ? ipm_solve_long_rescue_sets_kernel : ipm_solve_long_elastic_sets_kernel;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, e, (const double *)c->d_mqm_sets, (const Shared *)c->d_sets, set_index, n_sets);
    return;
  }
  auto kernel = segs > BTRAPZ_MAX_SEGMENTS_LONG_RESCUE ? ipm_solve_long_rescue_kernel : ipm_solve_long_elastic_kernel;
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, e, (const double *)c->d_mqm);
}

// Step: the rescue pass (btrapz_options.elastic) of the long form and of the packed form.
static int solve_rescue_pass(Solve &s, bool long_form) {
  btrapz_ctx *c = s.c; const int B = s.B, S = s.S;
  if (long_form) {
    HIPCHK(c, hipMemsetAsync(c->d_axis_viol, 0, sizeof(double) * 8 * (size_t)B, s.stream));
    c->viol_valid = (size_t)B;
    KernelArgs e = s.a;
    e.order = nullptr;
    launch_long_rescue(c, s.stream, e, (unsigned)B, S);
    HIPCHK(c, hipGetLastError());
    return BTRAPZ_OK;
  }
  // Rescue pass: the axis problems that stalled (elastic == 2: all of them) are listed per axis, bucketed by
  // segment count with the machinery of the ragged batches, and solved again with elastic rows.  The lists are
  // built on the device; the launch is sized for the worst case and its unused wavefronts leave at once.
  GROW(c, d_rescue, sizeof(int) * 4 * (size_t)B);
  GROW(c, d_rescue_meta, sizeof(int) * 2 * 198);
  HIPCHK(c, hipMemsetAsync(c->d_axis_viol, 0, sizeof(double) * 8 * (size_t)B, s.stream));
  c->viol_valid = (size_t)B;
  int *keys = c->d_rescue, *lists = c->d_rescue + 2 * (size_t)B;
  const unsigned nb = (unsigned)((B + 255) / 256);
  if (s.elastic == 2)
    hipLaunchKernelGGL(rescue_init_kernel, dim3(nb), dim3(256), 0, s.stream, B, S, s.seg_count, c->d_axis_obj,
                       c->d_axis_status, c->d_axis_iters);
  hipLaunchKernelGGL(rescue_keys_kernel, dim3(nb), dim3(256), 0, s.stream, B, S, s.seg_count, (const int *)c->d_axis_status,
                     keys, s.elastic == 2 ? 1 : 0);
  HIPCHK(c, hipMemsetAsync(c->d_rescue_meta, 0, sizeof(int) * 2 * 198, s.stream));
  for (int ax = 0; ax < 2; ax++)   // (an axis at a time: three launches each)
    launch_bucket_lists(s.stream, 1, B, S, keys + (size_t)ax * B, c->d_rescue_meta + ax * 198, lists + (size_t)ax * B, nullptr, nullptr, nullptr, 0);
  HIPCHK(c, hipGetLastError());
  KernelArgs e = rescue_arguments(s.a);
  e.order = lists; e.seg_count = s.seg_count; e.cand_prefix = c->d_rescue_meta; e.wave_prefix = c->d_rescue_meta + 66;
  e.bucket_S = 0;
  const int smax = s.seg_count ? (S < 64 ? S : 64) : S;
  const unsigned eblocks = 2u * (unsigned)(B / (64 / smax) + 65);
  hipLaunchKernelGGL(ipm_solve_elastic_kernel, dim3(eblocks), dim3(64), 0, s.stream, e, (const double *)c->d_mqm);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

// Uniform batches: seg_count == nullptr, S segments each.  Ragged: S is the slot stride, seg_count[b] the use.
// The steps: validate -> open the launch sequence, per-axis records -> M'QM table -> kernel arguments and options ->
// pre-pass and ordering -> main launch -> rescue pass -> long candidates of a ragged batch -> finalise and close.
static int solve_common(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt, const btrapz_warm *warm,
                        int B, int S, const int *seg_count, const double *seg, const double *init, const double *ref_end,
                        const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters, void *stream_,
                        bool long_warm = false, bool long_rescue = false) {
  if (!c) return BTRAPZ_EINVAL;
  if (!sh || B < 1 || S < 1 || (!seg_count && S > BTRAPZ_MAX_SEGMENTS_LONG) || !seg || !init || !ref_end || !dl_bounds ||
      !ctrl || !cost || !status) {
    c->err = "invalid argument";
    return BTRAPZ_EINVAL;
  }
  if (!options_ok(c, opt)) return BTRAPZ_EINVAL;
  Solve s;
  s.c = c; s.stream = (hipStream_t)stream_; s.opt = opt; s.B = B; s.S = S; s.seg_count = seg_count; s.long_warm = long_warm; s.long_rescue = long_rescue;
  TRY(ws_open(c, s.stream));
  TRY(ensure_axis_ws(c, 2 * (size_t)B));
  TRY(solve_weights_table(c, sh, s.stream));
  KernelArgs &a = s.a; fill_parameters(a, sh, opt, warm);
  batch_arguments(c, a, B, S, seg, init, ref_end, dl_bounds, ctrl, c->d_mqm);
  s.elastic = opt ? opt->elastic : 0;
  if (s.elastic < 0 || s.elastic > 2) { c->err = "invalid argument: btrapz_options.elastic"; return BTRAPZ_EINVAL; }
#ifndef BTRAPZ_EXPERIMENTS
  // the two experimental schedules exist in -DBTRAPZ_EXPERIMENTS builds only: asking this build for one is an error, not a
  // silent default (btrapz_build_has_experiments() tells a caller which build it holds)
  if (opt && (opt->queue > 0 || opt->start != 0)) {
    c->err = "invalid argument: btrapz_options.queue / .start are honoured by -DBTRAPZ_EXPERIMENTS builds only (this build has neither kernel)";
    return BTRAPZ_EINVAL;
  }
#endif
  TRY(solve_order_candidates(s, sh, (warm && !seg_count) ? warm->hint : nullptr));   // (a hint: uniform batches only)
  Form f;
  TRY(solve_main_launch(s, f));
  if (s.elastic) TRY(solve_rescue_pass(s, f.long_form));
  if (seg_count && S > BTRAPZ_MAX_SEGMENTS && (!s.warm_kernel || long_warm) && (s.elastic == 0 || (long_rescue && s.elastic == 1))) {
    // (a warm ragged solve leaves its long candidates at BTRAPZ_NO_CORRIDOR; btrapz_solve_long_warm_device solves them warm.
    //  With a rescue pass -- btrapz_solve_long_rescue_device -- a count's plain launch is followed by its rescue launch over
    //  the same list (the packed rescue pass above has zeroed d_axis_viol), and a count beyond 192 takes the kernel the
    //  uniform call of that width takes: the warm instantiation, whatever the start.)
    auto launch = [&](const KernelArgs &l, unsigned n, int segs) {
      const bool warm_k = s.warm_kernel || (long_rescue && segs > BTRAPZ_MAX_SEGMENTS_LONG_RESCUE);
      hipLaunchKernelGGL(warm_k ? ipm_solve_long_warm_kernel : ipm_solve_long_kernel, dim3(2u * n), dim3(64u * (unsigned)((segs + 63) / 64)), 0, s.stream, l, (const double *)c->d_mqm);
      if (s.elastic) launch_long_rescue(c, s.stream, l, n, segs);
    };
    TRY(solve_long_candidates(c, s.stream, a, seg_count, launch));
  }
  return finalize_and_close(c, s.stream, B, cost, status, iters);
}

BTRAPZ_EXPORT int btrapz_solve_batch_device(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt, int B,
                                         int S, const double *seg, const double *init, const double *ref_end,
                                         const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                         void *stream) {
  return solve_common(c, sh, opt, nullptr, B, S, nullptr, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters, stream);
}

BTRAPZ_EXPORT int btrapz_solve_ragged_device(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt, int B,
                                          int seg_stride, const double *seg, const int *seg_count, const double *init,
                                          const double *ref_end, const double *dl_bounds, double *ctrl, double *cost,
                                          int *status, int *iters, void *stream) {
  if (c && !seg_count) { c->err = "seg_count is null"; return BTRAPZ_EINVAL; }
  return solve_common(c, sh, opt, nullptr, B, seg_stride, seg_count, seg, init, ref_end, dl_bounds, ctrl, cost, status,
                      iters, stream);
}

BTRAPZ_EXPORT int btrapz_solve_warm_device(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt,
                                        const btrapz_warm *warm, int B, int seg_stride, const double *seg,
                                        const int *seg_count, const double *init, const double *ref_end,
                                        const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                        void *stream) {
  return solve_common(c, sh, opt, warm, B, seg_stride, seg_count, seg, init, ref_end, dl_bounds, ctrl, cost, status,
                      iters, stream);
}

// btrapz_solve_warm_device for candidates of up to BTRAPZ_MAX_SEGMENTS_LONG segments (include/btrapz_hip_long.h): at most
// 64 slots per candidate -- the call is btrapz_solve_warm_device; beyond, solve_common with the long form's warm
// instantiation for the uniform batch or, after the launch of the short candidates, for the long ones of a ragged batch.
BTRAPZ_EXPORT int btrapz_solve_long_warm_device(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt,
                                             const btrapz_warm *warm, int B, int seg_stride, const double *seg,
                                             const int *seg_count, const double *init, const double *ref_end,
                                             const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                             void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  if (!options_ok(c, opt)) return BTRAPZ_EINVAL;
  if (seg_stride > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: seg_stride > BTRAPZ_MAX_SEGMENTS_LONG";
    return BTRAPZ_EINVAL;
  }
  if (opt && opt->elastic != 0) {
    c->err = "invalid argument: btrapz_solve_long_warm_device has no rescue pass (btrapz_options.elastic must be 0)";
    return BTRAPZ_EINVAL;
  }
  if (seg_stride <= BTRAPZ_MAX_SEGMENTS)
    return solve_common(c, sh, opt, warm, B, seg_stride, seg_count, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters, stream);
  btrapz_warm w;   // (the hint orders the packed forms' wavefronts: it says nothing to one problem per workgroup)
  if (warm) { w = *warm; w.hint = nullptr; }
  return solve_common(c, sh, opt, warm ? &w : nullptr, B, seg_stride, seg_count, seg, init, ref_end, dl_bounds, ctrl, cost,
                      status, iters, stream, true);
}

// btrapz_solve_long_warm_device with the rescue pass (include/btrapz_hip_long_rescue.h).  Each case is handed to the path
// that serves it already wherever there is one -- the answer is then that path's, bit for bit: without a rescue pass the call
// above; up to 64 slots btrapz_solve_warm_device; a uniform batch of 65..192 segments without a start btrapz_solve_batch_device.
// What is left -- a uniform batch beyond 192 segments or with a start, a ragged record with slots beyond 64 -- is
// solve_common with long_rescue.
BTRAPZ_EXPORT int btrapz_solve_long_rescue_device(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt,
                                               const btrapz_warm *warm, int B, int seg_stride, const double *seg,
                                               const int *seg_count, const double *init, const double *ref_end,
                                               const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                               void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  const char *missing = !sh ? "shared" : !seg ? "seg" : !init ? "init" : !ref_end ? "ref_end" : !dl_bounds ? "dl_bounds" : !ctrl ? "ctrl" :
                        !cost ? "cost" : !status ? "status" : B < 1 ? "B" : seg_stride < 1 ? "seg_stride" : nullptr;
  if (missing) {
    c->err = std::string("invalid argument: btrapz_solve_long_rescue_device: ") + missing + (B < 1 || seg_stride < 1 ? " < 1" : " is NULL");
    return BTRAPZ_EINVAL;
  }
  if (!options_ok(c, opt)) return BTRAPZ_EINVAL;
  if (!opt || opt->elastic == 0)
    return btrapz_solve_long_warm_device(c, sh, opt, warm, B, seg_stride, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost,
                                         status, iters, stream);
  if (seg_stride > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: seg_stride > BTRAPZ_MAX_SEGMENTS_LONG";
    return BTRAPZ_EINVAL;
  }
  if (seg_stride <= BTRAPZ_MAX_SEGMENTS)
    return solve_common(c, sh, opt, warm, B, seg_stride, seg_count, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters, stream);
  if (opt->elastic != 1) {
    c->err = "invalid argument: btrapz_options.elastic beyond 64 segments: 0 or 1 (elastic rows for every candidate, 2, are not served)";
    return BTRAPZ_EINVAL;
  }
  const bool start = warm && (warm->x0 || warm->lam0 || warm->lam_out);
  if (!seg_count && seg_stride <= BTRAPZ_MAX_SEGMENTS_LONG_RESCUE && !start)
    return solve_common(c, sh, opt, nullptr, B, seg_stride, nullptr, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters, stream);
  btrapz_warm w;   // (the hint orders the packed forms' wavefronts: it says nothing to one problem per workgroup)
  if (warm) { w = *warm; w.hint = nullptr; }
  return solve_common(c, sh, opt, warm ? &w : nullptr, B, seg_stride, seg_count, seg, init, ref_end, dl_bounds, ctrl, cost,
                      status, iters, stream, true, true);
}

// ---- entry points that take parameter sets: the sets solve, its VJP and JVP, traj_cost ---------------------------------

static bool sets_in_range(const btrapz_shared *sets, int n_sets) { return sets && n_sets >= 1 && n_sets <= BTRAPZ_MAX_SETS; }

// One launch reads variant and delta from set 0 for every candidate.
static bool sets_alike(btrapz_ctx *c, const btrapz_shared *sets, int n_sets) {
  for (int g = 1; g < n_sets; g++)
    if (sets[g].variant != sets[0].variant || !(sets[g].delta == sets[0].delta)) {
      c->err = "invalid argument: every parameter set must have the same variant and delta";
      return false;
    }
  return true;
}

// The M'QM table with every weight 1 (the derivative of a table with respect to its weight): built at first use.
static int unit_mqm_table(btrapz_ctx *c, hipStream_t stream) {
  if (c->d_mqm_unit.bytes) return BTRAPZ_OK;
  GROW(c, d_mqm_unit, sizeof(double) * 168);
  const double ones[4] = {1.0, 1.0, 1.0, 1.0};
  launch_mqm_table(stream, ones, ones, c->d_mqm_unit);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

// The device view of the sets and their M'QM tables, kept by the context and rebuilt, stream-ordered, only when the sets change.
static int sets_tables(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, hipStream_t stream) {
  // the sets as the kernels read them (fill_parameters' limits), padding zeroed so that the cache can compare bytes
  std::vector<Shared> h((size_t)n_sets);
  for (int g = 0; g < n_sets; g++) {
    KernelArgs t;
    memset(&t, 0, sizeof(t));
    fill_parameters(t, &sets[g], nullptr, nullptr);
    memcpy(&h[(size_t)g], &t.sh, sizeof(Shared));
  }
  if (h.size() != c->h_sets.size() || memcmp(h.data(), c->h_sets.data(), sizeof(Shared) * h.size()) != 0) {
    c->h_sets.clear();   // (until the new tables are enqueued)
    if ((size_t)n_sets > c->sets_cap) {
      for (int i = 0; i < 2; i++) {
        if (c->sets_copy_pending[i]) { HIPCHK(c, hipEventSynchronize(c->sets_copied[i])); c->sets_copy_pending[i] = false; }
        (void)hipHostFree(c->h_sets_stage[i]); c->h_sets_stage[i] = nullptr;
      }
      release_all(c->d_sets, c->d_mqm_sets);
      c->sets_cap = 0;   // (set again once the device tables AND the pinned staging buffers stand)
      const size_t cap = (size_t)BTRAPZ_MAX_SETS < 64 * (((size_t)n_sets + 63) / 64) ? (size_t)BTRAPZ_MAX_SETS : 64 * (((size_t)n_sets + 63) / 64);
      GROW(c, d_sets, sizeof(Shared) * cap);
      GROW(c, d_mqm_sets, sizeof(double) * 168 * cap);
      for (int i = 0; i < 2; i++) HIPCHK(c, hipHostMalloc((void **)&c->h_sets_stage[i], sizeof(Shared) * cap, hipHostMallocDefault));
      c->sets_cap = cap;
    }
    // Two staging buffers in turn: a buffer is rewritten once ITS copy -- that of the change before the previous one -- has
    // left it.  The copy itself is stream-ordered behind the launches that still read the device tables (same stream, or
    // the event of ws_open), so a loop whose sets change at every step waits for the device only when it is two
    // changes ahead of it.
    const int si = c->sets_stage_next;
    c->sets_stage_next = 1 - si;
    if (!c->sets_copied[si]) HIPCHK(c, hipEventCreateWithFlags(&c->sets_copied[si], hipEventDisableTiming));
    if (c->sets_copy_pending[si]) HIPCHK(c, hipEventSynchronize(c->sets_copied[si]));
    memcpy(c->h_sets_stage[si], h.data(), sizeof(Shared) * h.size());
    HIPCHK(c, hipMemcpyAsync(c->d_sets, c->h_sets_stage[si], sizeof(Shared) * h.size(), hipMemcpyHostToDevice, stream));
    HIPCHK(c, hipEventRecord(c->sets_copied[si], stream));
    c->sets_copy_pending[si] = true;
    hipLaunchKernelGGL(mqm_sets_kernel, dim3((unsigned)n_sets), dim3(192), 0, stream, (const Shared *)c->d_sets, c->d_mqm_sets);
    HIPCHK(c, hipGetLastError());
    c->h_sets.swap(h);
  }
  return BTRAPZ_OK;
}

// A parameter set per candidate (btrapz_solve_sets_device).  The sets' device view and M'QM tables live in the context,
// cached by content: a loop that passes the same sets every step copies and builds nothing.  The candidates are bucketed
// on the device by (set, segment count) -- btrapz_sets.hip -- and solved in ONE launch of an ordered instantiation whose
// wavefronts each hold one set (ipm_solve_*sets*_kernel).  The split form (few candidates) and the long form (65..256
// segments; the long candidates of a cold ragged batch) hold one candidate per wavefront / workgroup and read its set
// themselves.  The form comes from choose_form, as for solve_common; the two-launch solve and the pre-pass are not served
// here, the rescue pass and warm starts beyond 64 segments through btrapz_solve_long_sets_device only, and the requests are
// those of btrapz_options (no environment).

// The packed / lean launch of a sets batch: candidates bucketed by key -- set (uniform) or 64 set + 64 - segment count
// (ragged) -- then one launch over the buckets.
static int launch_sets_buckets(btrapz_ctx *c, hipStream_t stream, KernelArgs &a, const int *seg_count, const int *set_index,
                               int n_sets, bool lean_on, bool warm_kernel) {
  const int B = a.B, S = a.S;
  const int n_keys = (seg_count ? 64 : 1) * n_sets;
  const size_t meta_need = 3 * (size_t)n_keys + 2;
  GROW(c, d_sets_meta, sizeof(int) * meta_need);
  GROW(c, d_order, sizeof(int) * (size_t)B);
  int *meta = c->d_sets_meta;
  HIPCHK(c, hipMemsetAsync(meta + 2 * ((size_t)n_keys + 1), 0, sizeof(int) * (size_t)n_keys, stream));
  const unsigned nb = (unsigned)((B + 255) / 256);
  hipLaunchKernelGGL(sets_hist_kernel, dim3(nb), dim3(256), 0, stream, B, S, seg_count, set_index, n_sets, n_keys, meta);
  hipLaunchKernelGGL(sets_prefix_kernel, dim3(1), dim3(1024), 0, stream, n_keys, seg_count ? 0 : S, meta);
  hipLaunchKernelGGL(sets_scatter_kernel, dim3(nb), dim3(256), 0, stream, B, S, seg_count, set_index, n_sets, n_keys, meta,
                     c->d_order, c->d_axis_obj, c->d_axis_status, c->d_axis_iters);
  HIPCHK(c, hipGetLastError());
  a.order = c->d_order; a.seg_count = seg_count; a.cand_prefix = meta; a.wave_prefix = meta + n_keys + 1;
  a.bucket_S = seg_count ? 0 : S;
  // Upper bound on the wavefront pairs without a host round trip: a key of n candidates needs ceil(n / gpw) pairs, less
  // than n / gpw + 1, and at most min(n_keys, B) keys are non-empty.  Ragged batches (gpw >= 1): at most 2 B + 2 pairs
  // against the ragged path's B + 65 -- the surplus wavefronts find no bucket in their binary search and leave.
  const int gpw_min = seg_count ? 1 : 64 / S;
  const unsigned blocks = 2u * (unsigned)((size_t)B / (size_t)gpw_min + (size_t)(n_keys < B ? n_keys : B) + 1);
  auto kernel = lean_on ? (warm_kernel ? ipm_solve_lean_sets_warm_ordered_kernel : ipm_solve_lean_sets_ordered_kernel)
                        : (warm_kernel ? ipm_solve_sets_warm_ordered_kernel : ipm_solve_sets_ordered_kernel);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, stream, a, (const double *)c->d_mqm_sets, (const Shared *)c->d_sets, n_keys);
  HIPCHK(c, hipGetLastError());
  c->last_form = lean_on ? 8 : 0;
  return BTRAPZ_OK;
}

// The rescue pass of a sets solve (btrapz_solve_long_sets_device, opt->elastic == 1), after its plain launch with arguments a.
// Long form: solve_rescue_pass's launch with SETS.  Up to 64 segments: the stalled axis problems are listed per axis and
// bucketed by (set, segment count) with the bucket kernels of the plain launch -- given, in place of set_index, the set of
// the candidates whose axis problem stalled and -1 for the others -- so that a wavefront of the elastic instantiation holds
// one set.  Tables: [2][3 n_keys + 2] in d_rescue_meta (n_keys = 64 n_sets for a ragged record: 1.5 MB at 1 024 sets);
// masked indices [2][B] and lists [2][B] in d_rescue.
static int sets_rescue_pass(btrapz_ctx *c, hipStream_t stream, const KernelArgs &a, const int *seg_count, const int *set_index,
                            int n_sets, bool long_form) {
  const int B = a.B, S = a.S;
  HIPCHK(c, hipMemsetAsync(c->d_axis_viol, 0, sizeof(double) * 8 * (size_t)B, stream));
  c->viol_valid = (size_t)B;
  if (long_form) {
    KernelArgs e = a;
    e.order = nullptr;
    launch_long_rescue(c, stream, e, (unsigned)B, S, set_index, n_sets);
    HIPCHK(c, hipGetLastError());
    return BTRAPZ_OK;
  }
  const int n_keys = (seg_count ? 64 : 1) * n_sets;
  const size_t per_axis = 3 * (size_t)n_keys + 2;
  GROW(c, d_rescue, sizeof(int) * 4 * (size_t)B);
  GROW(c, d_rescue_meta, sizeof(int) * 2 * per_axis);
  int *masked = c->d_rescue, *lists = c->d_rescue + 2 * (size_t)B, *meta = c->d_rescue_meta;
  const unsigned nb = (unsigned)((B + 255) / 256);
  hipLaunchKernelGGL(sets_rescue_index_kernel, dim3(nb), dim3(256), 0, stream, B, set_index, (const int *)c->d_axis_status, masked);
  HIPCHK(c, hipMemsetAsync(meta, 0, sizeof(int) * 2 * per_axis, stream));
  for (int ax = 0; ax < 2; ax++) {
    int *m = meta + (size_t)ax * per_axis;
    const int *idx = masked + (size_t)ax * B;
    hipLaunchKernelGGL(sets_hist_kernel, dim3(nb), dim3(256), 0, stream, B, S, seg_count, idx, n_sets, n_keys, m);
    hipLaunchKernelGGL(sets_prefix_kernel, dim3(1), dim3(1024), 0, stream, n_keys, seg_count ? 0 : S, m);
    hipLaunchKernelGGL(sets_scatter_kernel, dim3(nb), dim3(256), 0, stream, B, S, seg_count, idx, n_sets, n_keys, m,
                       lists + (size_t)ax * B, (double *)nullptr, (int *)nullptr, (int *)nullptr);
  }
  HIPCHK(c, hipGetLastError());
  KernelArgs e = rescue_arguments(a);
  e.order = lists; e.seg_count = seg_count; e.cand_prefix = meta; e.wave_prefix = meta + n_keys + 1;
  e.bucket_S = seg_count ? 0 : S;
  // (wavefront pairs per axis: launch_sets_buckets' bound)
  const int gpw_min = seg_count ? 1 : 64 / S;
  const unsigned eblocks = 2u * (unsigned)((size_t)B / (size_t)gpw_min + (size_t)(n_keys < B ? n_keys : B) + 1);
  hipLaunchKernelGGL(ipm_solve_elastic_sets_kernel, dim3(eblocks), dim3(64), 0, stream, e, (const double *)c->d_mqm_sets,
                     (const Shared *)c->d_sets, n_keys);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

// The steps of a sets solve behind the entry points' refusals.  extended (btrapz_solve_long_sets_device): the warm long sets
// kernel for candidates of 65..256 segments, and with opt->elastic == 1 the rescue pass -- every kernel choice is the one
// btrapz_solve_long_rescue_device makes for a one-set batch of the same shape, options and start.
static int solve_sets_steps(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index, const btrapz_options *opt,
                            const btrapz_warm *warm, int B, int S, const double *seg, const int *seg_count, const double *init,
                            const double *ref_end, const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                            void *stream_, bool extended) {
  hipStream_t stream = (hipStream_t)stream_;
  TRY(ws_open(c, stream));
  c->last_launches = 1;   // (the sets solve never runs the two launches)
  TRY(ensure_axis_ws(c, 2 * (size_t)B));
  TRY(sets_tables(c, sets, n_sets, stream));
  KernelArgs a;
  fill_parameters(a, &sets[0], opt, warm);   // (a.sh is not read: every wavefront reads its own set)
  batch_arguments(c, a, B, S, seg, init, ref_end, dl_bounds, ctrl, c->d_mqm_sets);
  const bool warm_kernel = a.x0 || a.lam0 || a.lam_out;
  const int elastic = (extended && opt) ? opt->elastic : 0;
  const double *mq = c->d_mqm_sets; const Shared *dsets = c->d_sets;
  // (ordered: a ragged batch always goes through the bucket list, a uniform one may take the split form; one launch:
  //  cap_iter = -1, and blocks -- which only the automatic two launches look at -- is not known yet)
  FormQuery q{};
  q.B = B; q.S = S; q.ragged = seg_count != nullptr; q.warm_kernel = warm_kernel; q.ordered = seg_count != nullptr; q.compact = false;
  q.elastic = 0; q.max_iter = a.max_iter; q.split = opt ? opt->split : 0; q.lean = opt ? opt->lean : 0; q.cap_iter = -1; q.queue = false;
  q.unc_start = a.unc_start; q.resident_waves = c->resident_waves; q.blocks = 0;
  const Form f = choose_form(q);
  // (long form: the warm instantiation with a start or lam_out, and -- with a rescue pass -- beyond 192 segments whatever the
  //  start, as solve_common picks it for btrapz_solve_long_rescue_device)
  auto long_warm_kernel = [&](int segs) { return warm_kernel || (elastic && segs > BTRAPZ_MAX_SEGMENTS_LONG_RESCUE); };
  if (f.long_form) {
    c->last_form = long_warm_kernel(S) ? 16 : 2;
    hipLaunchKernelGGL(long_warm_kernel(S) ? ipm_solve_long_warm_sets_kernel : ipm_solve_long_sets_kernel, dim3(2u * (unsigned)B),
                       dim3(64u * (unsigned)((S + 63) / 64)), 0, stream, a, mq, dsets, set_index, n_sets);
    HIPCHK(c, hipGetLastError());
  } else if (f.split_on) {
    c->last_form = 1;
    hipLaunchKernelGGL(ipm_solve_sets_split_kernel, dim3(2u * (unsigned)B), dim3(64), 0, stream, a, mq, dsets, set_index, n_sets);
    HIPCHK(c, hipGetLastError());
  } else {
    TRY(launch_sets_buckets(c, stream, a, seg_count, set_index, n_sets, f.lean_on, warm_kernel));
  }
  if (elastic) TRY(sets_rescue_pass(c, stream, a, seg_count, set_index, n_sets, f.long_form));
  // Ragged batch with slots for more than 64 segments: its long candidates, each workgroup reading its candidate's set
  // (btrapz_solve_sets_device: cold only -- warm starts keep them unsolved, as in solve_common; extended: warm-started too,
  // and a count's plain launch followed by its rescue launch over the same list).
  if (seg_count && S > BTRAPZ_MAX_SEGMENTS && (!warm_kernel || extended)) {
    auto launch = [&](const KernelArgs &l, unsigned n, int segs) {
      hipLaunchKernelGGL(long_warm_kernel(segs) ? ipm_solve_long_warm_sets_kernel : ipm_solve_long_sets_kernel, dim3(2u * n),
                         dim3(64u * (unsigned)((segs + 63) / 64)), 0, stream, l, mq, dsets, set_index, n_sets);
      if (elastic) launch_long_rescue(c, stream, l, n, segs, set_index, n_sets);
    };
    TRY(solve_long_candidates(c, stream, a, seg_count, launch));
  }
  return finalize_and_close(c, stream, B, cost, status, iters);
}

BTRAPZ_EXPORT int btrapz_solve_sets_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                        const btrapz_options *opt, const btrapz_warm *warm, int B, int seg_stride,
                                        const double *seg, const int *seg_count, const double *init, const double *ref_end,
                                        const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                        void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  const int S = seg_stride;
  if (!sets_in_range(sets, n_sets) || !set_index || B < 1 || S < 1 || !seg || !init || !ref_end ||
      !dl_bounds || !ctrl || !cost || !status) {
    c->err = "invalid argument (sets: 1 <= n_sets <= BTRAPZ_MAX_SETS, set_index and the batch arrays non-null, B >= 1)";
    return BTRAPZ_EINVAL;
  }
  if (!options_ok(c, opt)) return BTRAPZ_EINVAL;
  if (!seg_count && S > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: uniform batches of at most BTRAPZ_MAX_SEGMENTS_LONG segments";
    return BTRAPZ_EINVAL;
  }
  const bool warm_args = warm && (warm->x0 || warm->lam0 || warm->lam_out);
  if (!seg_count && S > BTRAPZ_MAX_SEGMENTS && warm_args) {
    c->err = "more than 64 segments: uniform cold solve only";
    return BTRAPZ_EINVAL;
  }
  if (!sets_alike(c, sets, n_sets)) return BTRAPZ_EINVAL;
  if (opt && (opt->elastic != 0 || opt->cap_iter > 0 || opt->compact > 0 || opt->queue > 0 || opt->start != 0)) {
    c->err = "invalid argument: with parameter sets, elastic, cap_iter > 0, compact = 1, queue and start are not served";
    return BTRAPZ_EINVAL;
  }
  return solve_sets_steps(c, sets, n_sets, set_index, opt, warm, B, S, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status,
                          iters, stream_, false);
}

// btrapz_solve_sets_device with warm starts and kept multipliers up to BTRAPZ_MAX_SEGMENTS_LONG segments and with the rescue
// pass at every width (include/btrapz_hip_long_sets.h).  What the older call serves is handed to it; the rest is
// solve_sets_steps, extended.
BTRAPZ_EXPORT int btrapz_solve_long_sets_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                             const btrapz_options *opt, const btrapz_warm *warm, int B, int seg_stride,
                                             const double *seg, const int *seg_count, const double *init, const double *ref_end,
                                             const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters,
                                             void *stream) {
  if (!c) return BTRAPZ_EINVAL;
  const char *missing = !sets ? "sets" : !set_index ? "set_index" : !seg ? "seg" : !init ? "init" : !ref_end ? "ref_end" :
                        !dl_bounds ? "dl_bounds" : !ctrl ? "ctrl" : !cost ? "cost" : !status ? "status" : nullptr;
  const char *bad = missing ? nullptr : B < 1 ? "B < 1" : seg_stride < 1 ? "seg_stride < 1" :
                    !sets_in_range(sets, n_sets) ? "n_sets outside 1..BTRAPZ_MAX_SETS" :
                    seg_stride > BTRAPZ_MAX_SEGMENTS_LONG ? "seg_stride > BTRAPZ_MAX_SEGMENTS_LONG" : nullptr;
  if (missing || bad) {
    c->err = std::string("invalid argument: btrapz_solve_long_sets_device: ") + (missing ? std::string(missing) + " is NULL" : std::string(bad));
    return BTRAPZ_EINVAL;
  }
  if (!options_ok(c, opt)) return BTRAPZ_EINVAL;
  if (opt) {
    const char *o = (opt->elastic < 0 || opt->elastic > 1) ? "btrapz_options.elastic: 0 or 1 (elastic rows for every candidate, 2, are not served with parameter sets)" :
                    opt->cap_iter > 0 ? "btrapz_options.cap_iter > 0 is not served with parameter sets" :
                    opt->compact > 0 ? "btrapz_options.compact = 1 is not served with parameter sets" :
                    opt->queue > 0 ? "btrapz_options.queue is not served with parameter sets" :
                    opt->start != 0 ? "btrapz_options.start is not served with parameter sets" : nullptr;
    if (o) { c->err = std::string("invalid argument: ") + o; return BTRAPZ_EINVAL; }
  }
  if (!sets_alike(c, sets, n_sets)) return BTRAPZ_EINVAL;
  const bool warm_args = warm && (warm->x0 || warm->lam0 || warm->lam_out);
  if ((!opt || opt->elastic == 0) && (seg_stride <= BTRAPZ_MAX_SEGMENTS || !warm_args))
    return btrapz_solve_sets_device(c, sets, n_sets, set_index, opt, warm, B, seg_stride, seg, seg_count, init, ref_end, dl_bounds,
                                    ctrl, cost, status, iters, stream);
  return solve_sets_steps(c, sets, n_sets, set_index, opt, warm, B, seg_stride, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost,
                          status, iters, stream, true);
}

// ---- gradients of a solve: btrapz_solve_vjp_device, btrapz_solve_jvp_device and their forms for 65..256 segments ----
// The refusals the four entry points share, in their order.  what: "vjp", "long jvp", ...; out_ok: the call's own output
// argument is there (backward: out); have_output: ctrl_bar or cost_bar, forward ctrl_dot or cost_dot; fwd: forward mode,
// whose tangents and T are checked too.
struct GradCall {
  const char *what;
  int max_segments;            // BTRAPZ_MAX_SEGMENTS or BTRAPZ_MAX_SEGMENTS_LONG
  bool fwd, out_ok, have_output;
  int T;
  const btrapz_tangents *tan;
};
static bool grad_args_ok(btrapz_ctx *c, const GradCall &g, const btrapz_shared *sets, int n_sets, int B, int seg_stride, const double *seg,
                         const double *ref_end, const double *dl_bounds, const double *ctrl, const double *lam, const int *status) {
  const std::string what = g.what;
  const bool packed = g.max_segments == BTRAPZ_MAX_SEGMENTS;
  if (!sets_in_range(sets, n_sets) || B < 1 || seg_stride < 1 || !seg || !ref_end || !dl_bounds || !g.out_ok)
    c->err = "invalid argument (" + what + ": 1 <= n_sets <= BTRAPZ_MAX_SETS, B >= 1, seg_stride >= 1, the batch arrays" +
             (g.fwd ? "" : " and out") + " non-null)";
  else if (seg_stride > g.max_segments)
    c->err = "invalid argument: " + what + " of candidates of at most " +
             (packed ? "BTRAPZ_MAX_SEGMENTS segments (the long form keeps no multipliers)" : "BTRAPZ_MAX_SEGMENTS_LONG segments");
  else if (!ctrl || !lam || !status)
    c->err = "invalid argument: " + what + " needs the solve's ctrl, lam (btrapz_warm.lam_out) and status";
  else if (!g.have_output)
    c->err = "invalid argument: " + what + (g.fwd ? " needs ctrl_dot or cost_dot (both NULL)" : " needs ctrl_bar or cost_bar (both NULL)");
  else if (g.fwd && (!g.tan || (!g.tan->seg && !g.tan->init && !g.tan->ref_end && !g.tan->dl_bounds && !g.tan->shared)))
    c->err = "invalid argument: " + what + " needs at least one tangent (all NULL)";
  else if (g.fwd && (g.T < 1 || g.T > BTRAPZ_MAX_TANGENTS))
    c->err = "invalid argument: " + what + " of 1 <= T <= BTRAPZ_MAX_TANGENTS tangents per call";
  else
    return sets_alike(c, sets, n_sets);
  return false;
}

// Opens the launch sequence, makes the tables the kernels read and fills what VjpArgs and JvpArgs have in common.
template <class Args>
static int fill_grad_args(btrapz_ctx *c, hipStream_t stream, Args &a, const btrapz_shared *sets, int n_sets, const int *set_index, int B,
                          int seg_stride, const double *seg, const int *seg_count, const double *ref_end, const double *dl_bounds,
                          const double *ctrl, const double *lam, const int *status) {
  TRY(ws_open(c, stream));
  TRY(sets_tables(c, sets, n_sets, stream));
  TRY(unit_mqm_table(c, stream));
  a.B = B; a.S = seg_stride; a.seg_stride = seg_stride; a.seg_count = seg_count;
  a.sets = c->d_sets; a.n_sets = n_sets; a.set_index = set_index; a.mqm = c->d_mqm_sets; a.mqm_unit = c->d_mqm_unit;
  a.seg = seg; a.ref_end = ref_end; a.dl_bounds = dl_bounds; a.ctrl = ctrl; a.lam = lam; a.status = status;
  return BTRAPZ_OK;
}

// Backward, both forms.  Up to 64 slots per candidate: one launch of vjp_kernel (btrapz_vjp.hip), groups of S lanes as the
// packed solve lays them out -- S = seg_stride for a ragged batch, whose lanes beyond a candidate's count stay idle.
// Beyond: one launch of long_vjp_kernel (btrapz_long_grad.hip), one axis problem per workgroup of ceil(seg_stride / 64)
// wavefronts.
static int solve_vjp(btrapz_ctx *c, const char *what, int max_segments, const btrapz_shared *sets, int n_sets, const int *set_index, int B,
                     int seg_stride, const double *seg, const int *seg_count, const double *ref_end, const double *dl_bounds,
                     const double *ctrl, const double *lam, const int *status, const double *ctrl_bar, const double *cost_bar,
                     const btrapz_grads *out, void *stream_) {
  const GradCall g = {what, max_segments, false, out != nullptr, ctrl_bar || cost_bar, 0, nullptr};
  if (!grad_args_ok(c, g, sets, n_sets, B, seg_stride, seg, ref_end, dl_bounds, ctrl, lam, status)) return BTRAPZ_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  VjpArgs a;
  TRY(fill_grad_args(c, stream, a, sets, n_sets, set_index, B, seg_stride, seg, seg_count, ref_end, dl_bounds, ctrl, lam, status));
  a.ctrl_bar = ctrl_bar; a.cost_bar = cost_bar;
  a.g_seg = out->seg; a.g_init = out->init; a.g_ref_end = out->ref_end; a.g_dl = out->dl_bounds; a.g_shared = out->shared;
  if (max_segments == BTRAPZ_MAX_SEGMENTS) {
    const unsigned gpw = 64u / (unsigned)seg_stride;
    const unsigned blocks = 2u * (unsigned)(((size_t)B + gpw - 1) / gpw);
    hipLaunchKernelGGL(vjp_kernel, dim3(blocks), dim3(64), 0, stream, a);
  } else {
    hipLaunchKernelGGL(long_vjp_kernel, dim3(2u * (unsigned)B), dim3(64u * (unsigned)((seg_stride + 63) / 64)), 0, stream, a);
  }
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

// Forward mode, both forms.  Up to 64 slots: one launch of jvp_kernel (btrapz_jvp.hip), vjp_kernel's groups of S lanes; a
// workgroup is the two wavefronts (s axis, l axis) of the same candidates.  Beyond: one launch of long_jvp_kernel, the
// backward kernel's mapping, and -- when cost_dot is wanted -- long_cost_dot_kernel behind it on the same stream, which
// adds the two axes' shares (the context's [2][T][B] workspace) in the order s + l.
static int solve_jvp(btrapz_ctx *c, const char *what, int max_segments, const btrapz_shared *sets, int n_sets, const int *set_index, int B,
                     int seg_stride, const double *seg, const int *seg_count, const double *ref_end, const double *dl_bounds,
                     const double *ctrl, const double *lam, const int *status, int T, const btrapz_tangents *tan, double *ctrl_dot,
                     double *cost_dot, void *stream_) {
  const GradCall g = {what, max_segments, true, true, ctrl_dot || cost_dot, T, tan};
  if (!grad_args_ok(c, g, sets, n_sets, B, seg_stride, seg, ref_end, dl_bounds, ctrl, lam, status)) return BTRAPZ_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  JvpArgs a;
  TRY(fill_grad_args(c, stream, a, sets, n_sets, set_index, B, seg_stride, seg, seg_count, ref_end, dl_bounds, ctrl, lam, status));
  a.T = T;
  a.seg_dot = tan->seg; a.init_dot = tan->init; a.ref_end_dot = tan->ref_end; a.dl_dot = tan->dl_bounds; a.shared_dot = tan->shared;
  a.ctrl_dot = ctrl_dot; a.cost_dot = cost_dot;
  if (max_segments == BTRAPZ_MAX_SEGMENTS) {
    const unsigned gpw = 64u / (unsigned)seg_stride;
    const unsigned blocks = (unsigned)(((size_t)B + gpw - 1) / gpw);
    hipLaunchKernelGGL(jvp_kernel, dim3(blocks), dim3(128), 0, stream, a);
    HIPCHK(c, hipGetLastError());
    return ws_close(c, stream);
  }
  const size_t n_cost = (size_t)T * (size_t)B;
  if (cost_dot) GROW(c, d_long_cost, sizeof(double) * 2 * n_cost);
  double *cost_ws = cost_dot ? c->d_long_cost.ptr() : nullptr;
  hipLaunchKernelGGL(long_jvp_kernel, dim3(2u * (unsigned)B), dim3(64u * (unsigned)((seg_stride + 63) / 64)), 0, stream, a, cost_ws);
  HIPCHK(c, hipGetLastError());
  if (cost_dot) {
    hipLaunchKernelGGL(long_cost_dot_kernel, dim3((unsigned)((n_cost + 255) / 256)), dim3(256), 0, stream, (const double *)cost_ws, cost_dot,
                       (unsigned)n_cost);
    HIPCHK(c, hipGetLastError());
  }
  return ws_close(c, stream);
}

// (init: the initial state enters the gradient through the returned control points of segment 0; forward, the tangent
//  system is stated at the returned control points and init_dot is what moves them)
BTRAPZ_EXPORT int btrapz_solve_vjp_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                       int B, int seg_stride, const double *seg, const int *seg_count, const double *init,
                                       const double *ref_end, const double *dl_bounds, const double *ctrl, const double *lam,
                                       const int *status, const double *ctrl_bar, const double *cost_bar,
                                       const btrapz_grads *out, void *stream_) {
  (void)init;
  if (!c) return BTRAPZ_EINVAL;
  return solve_vjp(c, "vjp", BTRAPZ_MAX_SEGMENTS, sets, n_sets, set_index, B, seg_stride, seg, seg_count, ref_end, dl_bounds, ctrl, lam,
                   status, ctrl_bar, cost_bar, out, stream_);
}

BTRAPZ_EXPORT int btrapz_solve_jvp_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                       int B, int seg_stride, const double *seg, const int *seg_count, const double *init,
                                       const double *ref_end, const double *dl_bounds, const double *ctrl, const double *lam,
                                       const int *status, int T, const btrapz_tangents *tan, double *ctrl_dot,
                                       double *cost_dot, void *stream_) {
  (void)init;
  if (!c) return BTRAPZ_EINVAL;
  return solve_jvp(c, "jvp", BTRAPZ_MAX_SEGMENTS, sets, n_sets, set_index, B, seg_stride, seg, seg_count, ref_end, dl_bounds, ctrl, lam,
                   status, T, tan, ctrl_dot, cost_dot, stream_);
}

// Solves of 65..256 segments (include/btrapz_hip_long_grad.h).  Up to 64 slots per candidate the calls ARE the two above.
BTRAPZ_EXPORT int btrapz_solve_long_vjp_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                            int B, int seg_stride, const double *seg, const int *seg_count, const double *init,
                                            const double *ref_end, const double *dl_bounds, const double *ctrl, const double *lam,
                                            const int *status, const double *ctrl_bar, const double *cost_bar,
                                            const btrapz_grads *out, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (seg_stride <= BTRAPZ_MAX_SEGMENTS)
    return btrapz_solve_vjp_device(c, sets, n_sets, set_index, B, seg_stride, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status,
                                   ctrl_bar, cost_bar, out, stream_);
  return solve_vjp(c, "long vjp", BTRAPZ_MAX_SEGMENTS_LONG, sets, n_sets, set_index, B, seg_stride, seg, seg_count, ref_end, dl_bounds, ctrl,
                   lam, status, ctrl_bar, cost_bar, out, stream_);
}

BTRAPZ_EXPORT int btrapz_solve_long_jvp_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                            int B, int seg_stride, const double *seg, const int *seg_count, const double *init,
                                            const double *ref_end, const double *dl_bounds, const double *ctrl, const double *lam,
                                            const int *status, int T, const btrapz_tangents *tan, double *ctrl_dot,
                                            double *cost_dot, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (seg_stride <= BTRAPZ_MAX_SEGMENTS)
    return btrapz_solve_jvp_device(c, sets, n_sets, set_index, B, seg_stride, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status,
                                   T, tan, ctrl_dot, cost_dot, stream_);
  return solve_jvp(c, "long jvp", BTRAPZ_MAX_SEGMENTS_LONG, sets, n_sets, set_index, B, seg_stride, seg, seg_count, ref_end, dl_bounds, ctrl,
                   lam, status, T, tan, ctrl_dot, cost_dot, stream_);
}

// The audit of given control points against every row of their QP (btrapz_check_rows_device, include/btrapz_hip_check.h):
// one launch of check_rows_kernel (btrapz_check.hip) -- groups of seg_stride lanes as vjp_kernel lays them out, one
// candidate per wavefront beyond 64 slots.  The sets' device view and M'QM tables are the context's; nothing else is kept.
BTRAPZ_EXPORT int btrapz_check_rows_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index,
                                        int B, int seg_stride, const double *seg, const int *seg_count, const double *init,
                                        const double *ref_end, const double *dl_bounds, const double *ctrl,
                                        const btrapz_row_check *out, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (!out || out->struct_size != sizeof(btrapz_row_check)) {
    c->err = "invalid argument: check_rows needs out, with out->struct_size = sizeof(btrapz_row_check)";
    return BTRAPZ_EINVAL;
  }
  if (!out->margin && !out->worst && !out->eq_res && !out->obj) {
    c->err = "invalid argument: check_rows needs at least one output (all NULL)";
    return BTRAPZ_EINVAL;
  }
  if (out->unit != 0 && out->unit != 1) {
    c->err = "invalid argument: check_rows: unit is 0 (the rows' own units) or 1 (divided by the rows' norms)";
    return BTRAPZ_EINVAL;
  }
  if (!sets_in_range(sets, n_sets)) {
    c->err = "invalid argument: 1 <= n_sets <= BTRAPZ_MAX_SETS and sets non-null";
    return BTRAPZ_EINVAL;
  }
  if (seg_stride < 1 || seg_stride > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: check_rows: 1 <= seg_stride <= BTRAPZ_MAX_SEGMENTS_LONG";
    return BTRAPZ_EINVAL;
  }
  if (B < 0) {
    c->err = "invalid argument: check_rows: B >= 0";
    return BTRAPZ_EINVAL;
  }
  for (int g = 1; g < n_sets; g++)
    if (sets[g].variant != sets[0].variant) {
      c->err = "invalid argument: check_rows: every parameter set must have the same variant";
      return BTRAPZ_EINVAL;
    }
  if (B == 0) return BTRAPZ_OK;
  if (!seg || !init || !ref_end || !dl_bounds || !ctrl) {
    c->err = "invalid argument: check_rows: the batch arrays and ctrl non-null";
    return BTRAPZ_EINVAL;
  }
  if (((size_t)ctrl & 15) != 0) {
    c->err = "invalid argument: check_rows: ctrl must be 16-byte aligned";
    return BTRAPZ_EINVAL;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRY(ws_open(c, stream));
  TRY(sets_tables(c, sets, n_sets, stream));
  CheckArgs a;
  a.B = B; a.seg_stride = seg_stride; a.unit = out->unit; a.seg_count = seg_count;
  a.sets = c->d_sets; a.n_sets = n_sets; a.set_index = set_index; a.mqm = c->d_mqm_sets;
  a.seg = seg; a.init = init; a.ref_end = ref_end; a.dl_bounds = dl_bounds; a.ctrl = ctrl;
  a.margin = out->margin; a.worst = out->worst; a.eq_res = out->eq_res; a.obj = out->obj;
  const unsigned gpw = seg_stride < 64 ? 64u / (unsigned)seg_stride : 1u;
  const unsigned blocks = (unsigned)(((size_t)B + gpw - 1) / gpw);
  hipLaunchKernelGGL(check_rows_kernel, dim3(blocks), dim3(64), 0, stream, a);
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

// a_cost of sampled trajectories and its VJP (btrapz_traj_cost_device, btrapz_traj_cost_vjp_device): one workgroup of 64
// per candidate (btrapz_acost.hip); the scoring sets come from the context's cache of btrapz_solve_sets_device.
static int traj_cost_common(btrapz_ctx *c, bool vjp, const btrapz_shared *sets, int n_sets, const int *set_index, int B,
                            int seg_stride, const double *seg, const int *seg_count, const double *init, const double *ctrl,
                            const int *status, int N, const double *s_ref, const double *l_ref, int ref_stride,
                            double *a_cost, int *n_points, const double *a_cost_bar, double *ctrl_bar, double *init_bar,
                            double *params_bar, double *s_ref_bar, double *l_ref_bar, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (!sets_in_range(sets, n_sets)) {
    c->err = "invalid argument: 1 <= n_sets <= BTRAPZ_MAX_SETS and sets non-null";
    return BTRAPZ_EINVAL;
  }
  if (!ctrl || !seg || !init || !s_ref || !l_ref) {
    c->err = "invalid argument: ctrl, seg, init, s_ref and l_ref must be non-null";
    return BTRAPZ_EINVAL;
  }
  if (B < 1 || N < 1 || seg_stride < 1) {
    c->err = "invalid argument: B >= 1, N >= 1 and seg_stride >= 1";
    return BTRAPZ_EINVAL;
  }
  if (seg_stride > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: seg_stride > BTRAPZ_MAX_SEGMENTS_LONG";
    return BTRAPZ_EINVAL;
  }
  if (!sets_alike(c, sets, n_sets)) return BTRAPZ_EINVAL;
  if (sets[0].variant != BTRAPZ_TRAPEZOID && sets[0].variant != BTRAPZ_CUBOID) {
    c->err = "invalid argument: variant";
    return BTRAPZ_EINVAL;
  }
  if (ref_stride != N && ref_stride != 0) {
    c->err = "invalid argument: ref_stride must be N (a reference line per candidate) or 0 (one line for all)";
    return BTRAPZ_EINVAL;
  }
  if (!vjp && !a_cost) {
    c->err = "invalid argument: a_cost is null";
    return BTRAPZ_EINVAL;
  }
  if (vjp && !a_cost_bar) {
    c->err = "invalid argument: a_cost_bar is null";
    return BTRAPZ_EINVAL;
  }
  hipStream_t stream = (hipStream_t)stream_;
  TRY(ws_open(c, stream));
  TRY(sets_tables(c, sets, n_sets, stream));
  AcostArgs a;
  a.B = B; a.seg_stride = seg_stride; a.seg_count = seg_count;
  a.sets = c->d_sets; a.n_sets = n_sets; a.set_index = set_index;
  a.seg = seg; a.init = init; a.ctrl = ctrl; a.status = status;
  a.N = N; a.ref_stride = ref_stride; a.s_ref = s_ref; a.l_ref = l_ref;
  a.delta = sets[0].delta; a.variant = sets[0].variant;
  a.a_cost = a_cost; a.n_points = n_points; a.a_cost_bar = a_cost_bar;
  a.ctrl_bar = ctrl_bar; a.init_bar = init_bar; a.params_bar = params_bar; a.s_ref_bar = s_ref_bar; a.l_ref_bar = l_ref_bar;
  if (vjp) hipLaunchKernelGGL(acost_vjp_kernel, dim3((unsigned)B), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(acost_kernel, dim3((unsigned)B), dim3(64), 0, stream, a);
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

BTRAPZ_EXPORT int btrapz_traj_cost_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index, int B,
                                       int seg_stride, const double *seg, const int *seg_count, const double *init,
                                       const double *ctrl, const int *status, int N, const double *s_ref, const double *l_ref,
                                       int ref_stride, double *a_cost, int *n_points, void *stream) {
  return traj_cost_common(c, false, sets, n_sets, set_index, B, seg_stride, seg, seg_count, init, ctrl, status, N, s_ref, l_ref,
                          ref_stride, a_cost, n_points, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

BTRAPZ_EXPORT int btrapz_traj_cost_vjp_device(btrapz_ctx *c, const btrapz_shared *sets, int n_sets, const int *set_index, int B,
                                           int seg_stride, const double *seg, const int *seg_count, const double *init,
                                           const double *ctrl, const int *status, int N, const double *s_ref,
                                           const double *l_ref, int ref_stride, const double *a_cost_bar, double *ctrl_bar,
                                           double *init_bar, double *params_bar, double *s_ref_bar, double *l_ref_bar,
                                           void *stream) {
  return traj_cost_common(c, true, sets, n_sets, set_index, B, seg_stride, seg, seg_count, init, ctrl, status, N, s_ref, l_ref,
                          ref_stride, nullptr, nullptr, a_cost_bar, ctrl_bar, init_bar, params_bar, s_ref_bar, l_ref_bar,
                          stream);
}

// Vector-Jacobian products of the sampling and of the state evaluation (btrapz_states.hip): one wavefront per selection /
// candidate, kStatesWaves of them per workgroup.  They read no workspace of the context.
BTRAPZ_EXPORT int btrapz_sample_vjp_device(btrapz_ctx *c, int B, int seg_stride, const int *seg_count, double delta,
                                        const double *seg, int nsel, const long long *sel, int max_points,
                                        const double *out_bar, double *ctrl_bar, double *init_bar, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (!seg || !sel || !out_bar) {
    c->err = "invalid argument: seg, sel and out_bar must be non-null";
    return BTRAPZ_EINVAL;
  }
  if (B < 1 || nsel < 1 || max_points < 1 || seg_stride < 1) {
    c->err = "invalid argument: B >= 1, nsel >= 1, max_points >= 1 and seg_stride >= 1";
    return BTRAPZ_EINVAL;
  }
  if (!(delta > 0)) {
    c->err = "invalid argument: delta must be > 0";
    return BTRAPZ_EINVAL;
  }
  if (seg_stride > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: seg_stride > BTRAPZ_MAX_SEGMENTS_LONG";
    return BTRAPZ_EINVAL;
  }
  if (!ctrl_bar && !init_bar) {
    c->err = "invalid argument: ctrl_bar and init_bar are both null";
    return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  SampleVjpArgs a;
  a.B = B; a.seg_stride = seg_stride; a.seg_count = seg_count; a.delta = delta; a.seg = seg;
  a.nsel = nsel; a.sel = sel; a.max_points = max_points; a.out_bar = out_bar; a.ctrl_bar = ctrl_bar; a.init_bar = init_bar;
  const unsigned blocks = (unsigned)(((size_t)nsel + kStatesWaves - 1) / kStatesWaves);
  hipLaunchKernelGGL(sample_vjp_kernel, dim3(blocks), dim3(64 * kStatesWaves), 0, (hipStream_t)stream_, a);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_eval_states_vjp_device(btrapz_ctx *c, int B, int seg_stride, const int *seg_count, const double *seg,
                                             const double *ctrl, int n_times, const double *times, const double *x_bar,
                                             double *ctrl_bar, double *times_bar, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (!seg || !times || !x_bar) {
    c->err = "invalid argument: seg, times and x_bar must be non-null";
    return BTRAPZ_EINVAL;
  }
  if (B < 1 || n_times < 1 || seg_stride < 1) {
    c->err = "invalid argument: B >= 1, n_times >= 1 and seg_stride >= 1";
    return BTRAPZ_EINVAL;
  }
  if (seg_stride > BTRAPZ_MAX_SEGMENTS_LONG) {
    c->err = "invalid argument: seg_stride > BTRAPZ_MAX_SEGMENTS_LONG";
    return BTRAPZ_EINVAL;
  }
  if (!ctrl_bar && !times_bar) {
    c->err = "invalid argument: ctrl_bar and times_bar are both null";
    return BTRAPZ_EINVAL;
  }
  if (times_bar && !ctrl) {
    c->err = "invalid argument: times_bar needs ctrl";
    return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  StatesVjpArgs a;
  a.B = B; a.seg_stride = seg_stride; a.seg_count = seg_count; a.seg = seg; a.ctrl = ctrl;
  a.n_times = n_times; a.times = times; a.x_bar = x_bar; a.ctrl_bar = ctrl_bar; a.times_bar = times_bar;
  const unsigned blocks = (unsigned)(((size_t)B + kStatesWaves - 1) / kStatesWaves);
  hipLaunchKernelGGL(eval_states_vjp_kernel, dim3(blocks), dim3(64 * kStatesWaves), 0, (hipStream_t)stream_, a);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_rescue_violations_device(btrapz_ctx *c, int B, double *viol, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (B < 1 || !viol) { c->err = "invalid argument"; return BTRAPZ_EINVAL; }
  if ((size_t)B != c->viol_valid) { c->err = "the context's last solve of B candidates had no rescue pass (btrapz_options.elastic)"; return BTRAPZ_EINVAL; }
  hipStream_t stream = (hipStream_t)stream_;
  // It writes no workspace, but it READS the last solve's records: closed like every sequence, so that the next solve on
  // another stream -- which clears and rewrites d_axis_viol -- waits for this read (ws_wait knows only the last closer).
  TRY(ws_open(c, stream));
  hipLaunchKernelGGL(rescue_violations_kernel, dim3((4 * B + 255) / 256), dim3(256), 0, stream, B, (const double *)c->d_axis_viol, viol);
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

BTRAPZ_EXPORT int btrapz_eval_states_device(btrapz_ctx *c, int B, int seg_stride, const int *seg_count, const double *seg,
                                         const double *ctrl, int n_times, const double *times, double *x,
                                         void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (B < 1 || seg_stride < 1 || n_times < 1 || !seg || !ctrl || !times || !x) { c->err = "invalid argument"; return BTRAPZ_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const long long n = (long long)B * n_times;
  hipLaunchKernelGGL(eval_states_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, B,
                     seg_stride, seg_count, seg, ctrl, n_times, times, x);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

// The launches of the corridor stage: `a` holds the shapes and every pointer but the retry list.  prisms: the fused
// prism + corridor kernels (the strips are evaluated from a.prisms instead of read from a.s_bounds / a.l_bounds).
// Beyond the wave-wide kernels' shapes (more than 512 knots or 64 obstacles): one lane per candidate on
// lists in a workspace (corridor_serial_kernel).  Capacities: what the host driver of find_traj allows itself (2 N + 16
// segments per obstacle) while the workspace stays below BTRAPZ_CORRIDOR_WS_MAX, else what a horizon of N knots needs when
// its bounds break at most 64 times per obstacle; as many selected segments (before the de-dup) as there are segments, under
// the same budget.
#ifndef BTRAPZ_CORRIDOR_WS_MAX
#define BTRAPZ_CORRIDOR_WS_MAX ((size_t)2 << 30)
#endif
static int launch_corridor_serial(btrapz_ctx *c, CorridorArgs a, hipStream_t stream) {
  const size_t seg_bytes = 104;   // sizeof(Seg): corridor_kernels.hip asserts it
  const size_t B = (size_t)a.B, O = (size_t)a.num_obs;
  size_t cap_o = 2 * (size_t)a.N + 16;
  const size_t cap_min = (size_t)(a.N - 1) / 10 + 1 + 64;
  if (B * O * cap_o * seg_bytes > BTRAPZ_CORRIDOR_WS_MAX) {
    cap_o = BTRAPZ_CORRIDOR_WS_MAX / (B * O * seg_bytes);
    if (cap_o < cap_min) cap_o = cap_min;
  }
  // selected segments before the de-dup: every segment of every obstacle can be one (its copies: only for NaN segments)
  size_t cap_sel = O * cap_o;
  if (B * cap_sel * seg_bytes > BTRAPZ_CORRIDOR_WS_MAX) {
    cap_sel = BTRAPZ_CORRIDOR_WS_MAX / (B * seg_bytes);
    if (cap_sel < 2 * (size_t)a.seg_stride + 16) cap_sel = 2 * (size_t)a.seg_stride + 16;
  }
  const size_t need = (B * O * cap_o + B * cap_sel) * seg_bytes;
  if (c->d_corr_ws.grow(need) != hipSuccess) { (void)hipGetLastError(); c->err = "corridor stage: no memory for the segment lists of this horizon"; return BTRAPZ_ENOMEM; }
  TRY(ws_wait(c, stream));
  a.cap_o = (int)cap_o; a.cap_sel = (int)cap_sel; a.pass = 0; a.retry_list = nullptr; a.retry_count = nullptr;
  Seg *all = reinterpret_cast<Seg *>(c->d_corr_ws.ptr());
  Seg *sel = reinterpret_cast<Seg *>(c->d_corr_ws.ptr() + B * O * cap_o * seg_bytes);
  hipLaunchKernelGGL(corridor_serial_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, a, all, sel);
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

static int launch_corridor_stage(btrapz_ctx *c, CorridorArgs a, bool prisms, hipStream_t stream) {
  const int B = a.B, N = a.N, num_obs = a.num_obs, seg_stride = a.seg_stride;
  if (!prisms && (N > 512 || num_obs > 64)) return launch_corridor_serial(c, a, stream);
  // Two passes (corridor_kernels.hip): lists sized for the usual case first -- LDS per workgroup is what limits the
  // wavefronts per CU -- then the candidates that overflowed them, with the full capacities.
  GROW(c, d_retry, sizeof(int) * ((size_t)B + 1));
  TRY(ws_wait(c, stream));   // (the retry counter and list are the context's: one launch sequence at a time)
  HIPCHK(c, hipMemsetAsync(c->d_retry, 0, sizeof(int), stream));
  a.retry_count = c->d_retry; a.retry_list = c->d_retry + 1;
  const int cap_o_big = 160 / num_obs, cap_sel_big = 64;        // MAX_ALL / O, MAX_SEL of corridor_kernels.hip
  // first-pass lists: one slot per second of horizon (CorridorSplit's pieces) plus a few for the slope breaks.  Every
  // slot is 104 bytes of LDS per obstacle and LDS bounds the wavefronts per CU; a candidate with more breaks only takes
  // the retry pass.  Measured on 65 536 candidates (+9 was round 2's margin): N = 71, 3 obstacles 0.305 -> 0.272 ms with
  // +3 and five wavefronts per SIMD; N = 201, 2 obstacles 0.686 -> 0.637 with +5 (0.663 with +3: more retries).
#ifndef CABL_CAPO_EXTRA
#define CABL_CAPO_EXTRA (N <= 128 ? 3 : 5)
#endif
  // (round 6, LDS once more: ocount[] cut to the obstacle count and 1.5 x seg_stride selected segments -- 7.4 -> 6.9 KB per
  //  wavefront -- N = 71 x 3 obstacles 0.240 -> 0.246 ms, N = 201 x 2 0.569 -> 0.542; with +2 instead of +3 slots per obstacle
  //  the retry pass takes over (0.84 ms at N = 201): LDS is not what holds this kernel any more)
  int cap_o_small = (N - 1) / 10 + CABL_CAPO_EXTRA, cap_sel_small = 2 * seg_stride < 16 ? 16 : 2 * seg_stride;
  if (cap_o_small > cap_o_big) cap_o_small = cap_o_big;
  if (cap_sel_small > cap_sel_big) cap_sel_small = cap_sel_big;
  const size_t slope_bytes = sizeof(double) * 2 * (size_t)N * num_obs;
  const int staged = slope_bytes <= 24 * 1024 ? 1 : 0;
  if (prisms && !staged) { c->err = "internal: fused corridor stage without a staged slope table"; return BTRAPZ_EINVAL; }
  auto lds_bytes = [&](int cap_o, int cap_sel) {
    const size_t cap_all = (size_t)cap_o * num_obs;
    return 104 * (cap_all > (size_t)cap_sel ? cap_all : (size_t)cap_sel) + (staged && slope_bytes > sizeof(double) * 4 * (size_t)N ? slope_bytes : sizeof(double) * 4 * (size_t)N) +
           sizeof(int) * (cap_all + 64 + cap_sel) + sizeof(short) * (cap_all + cap_sel) + 16 +
           (prisms ? prism_tab_bytes(a.P) + 8 : 0)
#ifdef CABL_PAD   // occupancy experiments: scratch/build_variant.sh X -DCABL_PAD=bytes
           + CABL_PAD
#endif
        ;
  };
  const bool two_pass = cap_o_small < cap_o_big || cap_sel_small < cap_sel_big;
  a.pass = 0; a.cap_o = cap_o_small; a.cap_sel = cap_sel_small;
  if (!two_pass) { a.retry_list = nullptr; a.retry_count = nullptr; }
  // (horizons of at most 128 knots: the instantiation that holds half the prefetch registers; the first pass of two
  //  runs without the serial statement of the extraction -- a candidate that needs it takes the retry pass)
  auto kernel = prisms ? (N <= 128 ? prism_corridor_batch_short_kernel : prism_corridor_batch_kernel)
                       : (N <= 128 ? corridor_batch_short_kernel : corridor_batch_kernel);
  auto first = !(two_pass && staged) ? kernel
               : prisms ? (N <= 128 ? prism_corridor_first_short_kernel : prism_corridor_first_kernel)
                        : (N <= 128 ? corridor_first_short_kernel : corridor_first_kernel);
  hipLaunchKernelGGL(first, dim3(B), dim3(64), lds_bytes(a.cap_o, a.cap_sel), stream, a, staged);
  HIPCHK(c, hipGetLastError());
  if (two_pass) {
    a.pass = 1; a.cap_o = cap_o_big; a.cap_sel = cap_sel_big;
    const unsigned blocks = B < 1024 ? (unsigned)B : 1024u;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds_bytes(a.cap_o, a.cap_sel), stream, a, staged);
  }
  HIPCHK(c, hipGetLastError());
  return ws_close(c, stream);
}

BTRAPZ_EXPORT int btrapz_corridor_batch_device(btrapz_ctx *c, int variant, int B, int N, int num_obs, double delta,
                                            const double *s_bounds, const double *l_bounds, const double *ds_bounds,
                                            const double *dl_bounds_knots, const double *s_ref, const double *l_ref,
                                            int seg_stride, double *seg, int *seg_count, double *ref_end,
                                            double *dl_bounds, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  // (N, num_obs: the reference has no limit -- std::vector --; the bounds here are those of find_traj's parser, corridor.cpp.
  //  More than 512 knots or 64 obstacles: the one-lane-per-candidate kernel instead of the wave-wide ones)
  if (variant < 0 || variant > 1 || B < 1 || N < 3 || N > 100000 || num_obs < 1 || num_obs > 1000 || !(delta > 0) ||
      seg_stride < 1 || seg_stride > BTRAPZ_MAX_SEGMENTS_LONG || !s_bounds || !l_bounds || !ds_bounds || !dl_bounds_knots || !s_ref || !l_ref || !seg ||
      !seg_count || !ref_end || !dl_bounds) {
    c->err = "invalid argument";
    return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  CorridorArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.N = N; a.num_obs = num_obs; a.variant = variant; a.seg_stride = seg_stride; a.delta = delta;
  a.s_bounds = s_bounds; a.l_bounds = l_bounds; a.ds_bounds = ds_bounds; a.dl_bounds = dl_bounds_knots;
  a.s_ref = s_ref; a.l_ref = l_ref; a.seg = seg; a.seg_count = seg_count; a.ref_end = ref_end; a.dl10 = dl_bounds;
  return launch_corridor_stage(c, a, false, (hipStream_t)stream_);
}

// The backward pass of the stage (corridor_vjp.hip): zero the wanted outputs, then the forward's two passes -- lists sized
// for the usual case, the candidates that overflow them again with the capacities the forward ends on.
BTRAPZ_EXPORT int btrapz_corridor_batch_vjp_device(btrapz_ctx *c, int variant, int B, int N, int num_obs, double delta,
                                                const double *s_bounds, const double *l_bounds, const double *ds_bounds,
                                                const double *dl_bounds_knots, const double *s_ref, const double *l_ref,
                                                int seg_stride, const double *seg_bar, const double *ref_end_bar,
                                                const double *dl_bounds_bar, const btrapz_knot_grads *out, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (variant < 0 || variant > 1 || B < 1 || N < 3 || num_obs < 1 || !(delta > 0) || seg_stride < 1) {
    c->err = "invalid argument: variant 0 or 1, B >= 1, N >= 3, num_obs >= 1, delta > 0 and seg_stride >= 1";
    return BTRAPZ_EINVAL;
  }
  if (N > 512 || num_obs > 64 || seg_stride > BTRAPZ_MAX_SEGMENTS) {
    c->err = "invalid argument: N > 512, num_obs > 64 or seg_stride > BTRAPZ_MAX_SEGMENTS -- beyond the wave-wide corridor kernels; "
             "the serial one-lane-per-candidate path of the stage is not differentiated";
    return BTRAPZ_EINVAL;
  }
  if (!s_bounds || !l_bounds || !ds_bounds || !dl_bounds_knots || !s_ref || !l_ref) {
    c->err = "invalid argument: s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref and l_ref must be non-null";
    return BTRAPZ_EINVAL;
  }
  if (!seg_bar && !ref_end_bar && !dl_bounds_bar) {
    c->err = "invalid argument: seg_bar, ref_end_bar and dl_bounds_bar are all null";
    return BTRAPZ_EINVAL;
  }
  if (!out || (!out->s_bounds && !out->l_bounds && !out->ds_bounds && !out->dl_bounds_knots && !out->s_ref && !out->l_ref)) {
    c->err = "invalid argument: no output wanted (out, or every pointer of it, is null)";
    return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_;
  GROW(c, d_vjp_retry, sizeof(int) * ((size_t)B + 1));
  TRY(ws_wait(c, stream));   // (as in launch_corridor_stage)
  HIPCHK(c, hipMemsetAsync(c->d_vjp_retry, 0, sizeof(int), stream));
  const size_t pairs = sizeof(double) * 2 * (size_t)B * num_obs * N, knots = sizeof(double) * (size_t)B * N;
  if (out->s_bounds) HIPCHK(c, hipMemsetAsync(out->s_bounds, 0, pairs, stream));
  if (out->l_bounds) HIPCHK(c, hipMemsetAsync(out->l_bounds, 0, pairs, stream));
  if (out->ds_bounds) HIPCHK(c, hipMemsetAsync(out->ds_bounds, 0, 2 * knots, stream));
  if (out->dl_bounds_knots) HIPCHK(c, hipMemsetAsync(out->dl_bounds_knots, 0, 2 * knots, stream));
  if (out->s_ref) HIPCHK(c, hipMemsetAsync(out->s_ref, 0, knots, stream));
  if (out->l_ref) HIPCHK(c, hipMemsetAsync(out->l_ref, 0, knots, stream));
  CorridorVjpArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.N = N; a.num_obs = num_obs; a.variant = variant; a.seg_stride = seg_stride; a.delta = delta;
  a.s_bounds = s_bounds; a.l_bounds = l_bounds; a.ds_bounds = ds_bounds; a.s_ref = s_ref; a.l_ref = l_ref;
  a.seg_bar = seg_bar; a.ref_end_bar = ref_end_bar; a.dl10_bar = dl_bounds_bar; a.out = *out;
  a.staged = sizeof(double) * 2 * (size_t)N * num_obs <= 24 * 1024 ? 1 : 0;
  a.retry_count = c->d_vjp_retry; a.retry_list = c->d_vjp_retry + 1;
  // (the forward's capacities: launch_corridor_stage)
  const int cap_o_big = 160 / num_obs, cap_sel_big = 64;
  int cap_o_small = (N - 1) / 10 + (N <= 128 ? 3 : 5), cap_sel_small = 2 * seg_stride < 16 ? 16 : 2 * seg_stride;
  if (cap_o_small > cap_o_big) cap_o_small = cap_o_big;
  if (cap_sel_small > cap_sel_big) cap_sel_small = cap_sel_big;
  const bool two_pass = cap_o_small < cap_o_big || cap_sel_small < cap_sel_big;
  a.pass = 0; a.cap_o = cap_o_small; a.cap_sel = cap_sel_small;
  if (!two_pass) { a.retry_list = nullptr; a.retry_count = nullptr; }
  hipLaunchKernelGGL(corridor_vjp_kernel, dim3(B), dim3(64), corridor_vjp_lds(N, num_obs, a.cap_o, a.cap_sel, seg_stride, a.staged).bytes, stream, a);
  HIPCHK(c, hipGetLastError());
  if (two_pass) {
    a.pass = 1; a.cap_o = cap_o_big; a.cap_sel = cap_sel_big;
    const unsigned blocks = B < 1024 ? (unsigned)B : 1024u;
    hipLaunchKernelGGL(corridor_vjp_kernel, dim3(blocks), dim3(64), corridor_vjp_lds(N, num_obs, a.cap_o, a.cap_sel, seg_stride, a.staged).bytes, stream, a);
    HIPCHK(c, hipGetLastError());
  }
  return ws_close(c, stream);
}

// The forward-mode derivative of the stage (corridor_jvp.hip, include/btrapz_hip_stage_jvp.h): the backward pass's two
// passes with the same capacities; every output entry is written by the pass that settles its candidate, nothing is zeroed.
BTRAPZ_EXPORT int btrapz_corridor_batch_jvp_device(btrapz_ctx *c, int variant, int B, int N, int num_obs, double delta,
                                                const double *s_bounds, const double *l_bounds, const double *ds_bounds,
                                                const double *dl_bounds_knots, const double *s_ref, const double *l_ref,
                                                int seg_stride, int T, const btrapz_knot_tangents *tan, double *seg_dot,
                                                double *ref_end_dot, double *dl_bounds_dot, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (variant < 0 || variant > 1 || B < 1 || N < 3 || num_obs < 1 || !(delta > 0) || seg_stride < 1) {
    c->err = "invalid argument: variant 0 or 1, B >= 1, N >= 3, num_obs >= 1, delta > 0 and seg_stride >= 1";
    return BTRAPZ_EINVAL;
  }
  if (N > 512 || num_obs > 64 || seg_stride > BTRAPZ_MAX_SEGMENTS) {
    c->err = "invalid argument: N > 512, num_obs > 64 or seg_stride > BTRAPZ_MAX_SEGMENTS -- beyond the wave-wide corridor kernels; "
             "the serial one-lane-per-candidate path of the stage is not differentiated";
    return BTRAPZ_EINVAL;
  }
  if (T < 1 || T > BTRAPZ_MAX_TANGENTS) { c->err = "invalid argument: T must be in 1..BTRAPZ_MAX_TANGENTS"; return BTRAPZ_EINVAL; }
  if (!s_bounds || !l_bounds || !ds_bounds || !dl_bounds_knots || !s_ref || !l_ref) {
    c->err = "invalid argument: s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref and l_ref must be non-null";
    return BTRAPZ_EINVAL;
  }
  if (!tan || (!tan->s_bounds && !tan->l_bounds && !tan->ds_bounds && !tan->dl_bounds_knots && !tan->s_ref && !tan->l_ref)) {
    c->err = "invalid argument: no tangent given (tangents, or every pointer of it, is null)";
    return BTRAPZ_EINVAL;
  }
  if (!seg_dot && !ref_end_dot && !dl_bounds_dot) {
    c->err = "invalid argument: seg_dot, ref_end_dot and dl_bounds_dot are all null";
    return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_;
  GROW(c, d_vjp_retry, sizeof(int) * ((size_t)B + 1));
  TRY(ws_wait(c, stream));   // (as in launch_corridor_stage)
  HIPCHK(c, hipMemsetAsync(c->d_vjp_retry, 0, sizeof(int), stream));
  CorridorJvpArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.N = N; a.num_obs = num_obs; a.variant = variant; a.seg_stride = seg_stride; a.T = T; a.delta = delta;
  a.s_bounds = s_bounds; a.l_bounds = l_bounds; a.ds_bounds = ds_bounds; a.s_ref = s_ref; a.l_ref = l_ref;
  a.s_dot = tan->s_bounds; a.l_dot = tan->l_bounds; a.ds_dot = tan->ds_bounds; a.dl_knots_dot = tan->dl_bounds_knots;
  a.sref_dot = tan->s_ref; a.lref_dot = tan->l_ref;
  a.seg_dot = seg_dot; a.ref_end_dot = ref_end_dot; a.dl10_dot = dl_bounds_dot;
  a.staged = sizeof(double) * 2 * (size_t)N * num_obs <= 24 * 1024 ? 1 : 0;
  a.retry_count = c->d_vjp_retry; a.retry_list = c->d_vjp_retry + 1;
  // (the forward's capacities: launch_corridor_stage)
  const int cap_o_big = 160 / num_obs, cap_sel_big = 64;
  int cap_o_small = (N - 1) / 10 + (N <= 128 ? 3 : 5), cap_sel_small = 2 * seg_stride < 16 ? 16 : 2 * seg_stride;
  if (cap_o_small > cap_o_big) cap_o_small = cap_o_big;
  if (cap_sel_small > cap_sel_big) cap_sel_small = cap_sel_big;
  const bool two_pass = cap_o_small < cap_o_big || cap_sel_small < cap_sel_big;
  a.pass = 0; a.cap_o = cap_o_small; a.cap_sel = cap_sel_small;
  if (!two_pass) { a.retry_list = nullptr; a.retry_count = nullptr; }
  hipLaunchKernelGGL(corridor_jvp_kernel, dim3(B), dim3(64), corridor_vjp_lds(N, num_obs, a.cap_o, a.cap_sel, seg_stride, a.staged).bytes, stream, a);
  HIPCHK(c, hipGetLastError());
  if (two_pass) {
    a.pass = 1; a.cap_o = cap_o_big; a.cap_sel = cap_sel_big;
    const unsigned blocks = B < 1024 ? (unsigned)B : 1024u;
    hipLaunchKernelGGL(corridor_jvp_kernel, dim3(blocks), dim3(64), corridor_vjp_lds(N, num_obs, a.cap_o, a.cap_sel, seg_stride, a.staged).bytes, stream, a);
    HIPCHK(c, hipGetLastError());
  }
  return ws_close(c, stream);
}

// Obstacle prisms -> strips -> corridors: btrapz_prism_bounds_device + btrapz_corridor_batch_device (num_obs = O) with
// the strips evaluated where the corridor stage reads them instead of written to memory and read back.  Scenes whose
// slope table does not fit the kernel's LDS (O * N * 16 bytes > 24 KB) take the two launches through a workspace of
// the context: the results are the same either way.
BTRAPZ_EXPORT int btrapz_prism_corridor_batch_device(btrapz_ctx *c, int variant, int B, int P, int N, const btrapz_road *road,
                                                  const double *prisms, int O, double delta, const double *ds_bounds,
                                                  const double *dl_bounds_knots, const double *s_ref, const double *l_ref,
                                                  int seg_stride, double *seg, int *seg_count, double *ref_end,
                                                  double *dl_bounds, int *n_strips, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (variant < 0 || variant > 1 || B < 1 || P < 1 || P > 16 || N < 3 || N > 512 || O < 1 || O > 64 || !(delta > 0) || !road ||
      !(road->knots_per_second > 0) || !prisms || seg_stride < 1 || !ds_bounds || !dl_bounds_knots || !s_ref || !l_ref ||
      !seg || !seg_count || !ref_end || !dl_bounds) {
    c->err = "invalid argument";
    return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_;
  CorridorArgs a;
  memset(&a, 0, sizeof a);
  a.B = B; a.N = N; a.num_obs = O; a.variant = variant; a.seg_stride = seg_stride; a.delta = delta;
  a.ds_bounds = ds_bounds; a.dl_bounds = dl_bounds_knots;
  a.s_ref = s_ref; a.l_ref = l_ref; a.seg = seg; a.seg_count = seg_count; a.ref_end = ref_end; a.dl10 = dl_bounds;
  if (sizeof(double) * 2 * (size_t)N * O <= 24 * 1024) {
    a.prisms = prisms; a.P = P; a.road = prism_road(road); a.n_strips = n_strips;
    return launch_corridor_stage(c, a, true, stream);
  }
  const size_t need = sizeof(double) * 4 * (size_t)B * O * N + sizeof(int) * (size_t)B;
  GROW(c, d_strips, need);
  TRY(ws_wait(c, stream));
  double *sb = reinterpret_cast<double *>(c->d_strips.ptr()), *lb = sb + 2 * (size_t)B * O * N;
  int *ns = n_strips ? n_strips : reinterpret_cast<int *>(lb + 2 * (size_t)B * O * N);
  TRY(btrapz_prism_bounds_device(c, B, P, N, road, prisms, O, sb, lb, ns, stream_));
  a.s_bounds = sb; a.l_bounds = lb;
  const int rc2 = launch_corridor_stage(c, a, false, stream);
  TRY(ws_close(c, stream));
  return rc2;
}

BTRAPZ_EXPORT int btrapz_argmin_device(btrapz_ctx *c, int B, int group, long long index_base, const double *cost,
                                    long long *best_idx, double *best_cost, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (B < 1 || group < 1 || B % group != 0 || !cost || !best_idx || !best_cost) { c->err = "invalid argument"; return BTRAPZ_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_;
  const int groups = B / group;
  // large groups are split over several blocks (a single block over 65 536 costs is latency-bound)
  int chunks = group >= 8192 ? (group + 1023) / 1024 : 1;
  if (chunks > 256) chunks = 256;
  if (chunks > 1) {
    const size_t need = (size_t)groups * chunks;
    if (need > c->d_argmin_idx.cap()) {
      release_all(c->d_argmin_cost, c->d_argmin_idx);
      GROW(c, d_argmin_cost, sizeof(double) * need);
      GROW(c, d_argmin_idx, sizeof(long long) * need);
    }
    TRY(ws_wait(c, stream));
  }
  hipLaunchKernelGGL(argmin_kernel, dim3(groups, chunks), dim3(256), 0, stream, group, index_base, cost, best_idx, best_cost,
                     c->d_argmin_cost.ptr(), c->d_argmin_idx.ptr());
  if (chunks > 1) {
    hipLaunchKernelGGL(argmin_final_kernel, dim3(groups), dim3(256), 0, stream, chunks, index_base,
                       (const double *)c->d_argmin_cost, (const long long *)c->d_argmin_idx, best_idx, best_cost);
    TRY(ws_close(c, stream));
  }
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_argmin_pairs_device(btrapz_ctx *c, int world, int n, const long long *pairs, double *best_cost,
                                          long long *best_idx, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (world < 1 || n < 1 || !pairs || !best_cost || !best_idx) { c->err = "invalid argument"; return BTRAPZ_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(argmin_pairs_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, world, n, pairs, best_cost,
                     best_idx);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_sample_device(btrapz_ctx *c, int B, int S, double delta, const double *seg, const double *init,
                                    const double *ctrl, int nsel, const long long *sel, int max_points, double *out,
                                    int *npoints, void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (B < 1 || S < 1 || nsel < 1 || !(delta > 0) || !seg || !init || !ctrl || !sel || !out || !npoints || max_points < 1) {
    c->err = "invalid argument"; return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(sample_kernel, dim3(nsel), dim3(64), 0, (hipStream_t)stream_, B, S, (const int *)nullptr, delta, seg,
                     init, ctrl, nsel, sel, max_points, out, npoints);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_sample_ragged_device(btrapz_ctx *c, int B, int seg_stride, const int *seg_count, double delta,
                                           const double *seg, const double *init, const double *ctrl, int nsel,
                                           const long long *sel, int max_points, double *out, int *npoints,
                                           void *stream_) {
  if (!c) return BTRAPZ_EINVAL;
  if (B < 1 || seg_stride < 1 || nsel < 1 || !(delta > 0) || !seg || !init || !ctrl || !sel || !out || !npoints ||
      max_points < 1) {
    c->err = "invalid argument"; return BTRAPZ_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(sample_kernel, dim3(nsel), dim3(64), 0, (hipStream_t)stream_, B, seg_stride, seg_count, delta, seg,
                     init, ctrl, nsel, sel, max_points, out, npoints);
  HIPCHK(c, hipGetLastError());
  return BTRAPZ_OK;
}

BTRAPZ_EXPORT int btrapz_solve_batch_host(btrapz_ctx *c, const btrapz_shared *sh, const btrapz_options *opt, int B, int S,
                                       const double *seg, const double *init, const double *ref_end,
                                       const double *dl_bounds, double *ctrl, double *cost, int *status, int *iters) {
  if (!c) return BTRAPZ_EINVAL;
  if (B < 1 || S < 1 || S > BTRAPZ_MAX_SEGMENTS_LONG) { c->err = "invalid argument"; return BTRAPZ_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n_seg = (size_t)BTRAPZ_NUM_SEG_FIELDS * B * S, n_init = (size_t)B * 6, n_re = (size_t)B * 2, n_dl = (size_t)B * 10;
  const size_t n_ctrl = (size_t)B * 12 * S, n_cost = B;
  const size_t need = n_seg + n_init + n_re + n_dl + n_ctrl + n_cost;
  GROW(c, d_stage, sizeof(double) * need);
  GROW(c, d_istage, sizeof(int) * 2 * (size_t)B);
  double *d_seg = c->d_stage, *d_init = d_seg + n_seg, *d_re = d_init + n_init, *d_dl = d_re + n_re;
  double *d_ctrl = d_dl + n_dl, *d_cost = d_ctrl + n_ctrl;
  int *d_status = c->d_istage, *d_iters = c->d_istage + B;
  HIPCHK(c, hipMemcpy(d_seg, seg, sizeof(double) * n_seg, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_init, init, sizeof(double) * n_init, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_re, ref_end, sizeof(double) * n_re, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_dl, dl_bounds, sizeof(double) * n_dl, hipMemcpyHostToDevice));
  TRY(btrapz_solve_batch_device(c, sh, opt, B, S, d_seg, d_init, d_re, d_dl, d_ctrl, d_cost, d_status, d_iters, nullptr));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(ctrl, d_ctrl, sizeof(double) * n_ctrl, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(cost, d_cost, sizeof(double) * n_cost, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(status, d_status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (iters) HIPCHK(c, hipMemcpy(iters, d_iters, sizeof(int) * B, hipMemcpyDeviceToHost));
  return BTRAPZ_OK;
}
