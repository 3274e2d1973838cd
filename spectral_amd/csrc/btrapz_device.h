// btrapz_device.h -- types shared by the kernels and the host side of libbtrapz_hip.so.
#ifndef BTRAPZ_DEVICE_H
#define BTRAPZ_DEVICE_H

#include "../../include/btrapz_hip.h"

// The library is built with -fvisibility=hidden: only the C-ABI of include/btrapz_hip.h is exported.
#define BTRAPZ_EXPORT extern "C" __attribute__((visibility("default")))

// Bounds that are no bounds (btrapz_ipm.h, "bounds that are no bounds"): a finite bound of at least BTRAPZ_FAR in
// magnitude can never be active; the kernels move such row bounds to BTRAPZ_FAR_FACTOR (1 + the lane's largest real
// bound), the host moves such header limits (acceleration, jerk) to +-BTRAPZ_FAR_LIMIT; neither enters |bounds|.
#define BTRAPZ_FAR 1e9
#define BTRAPZ_FAR_FACTOR 1048576.0
#define BTRAPZ_FAR_LIMIT 1e6
#define BTRAPZ_COLD_FAR 1e4

namespace btrapz {

// Device view of btrapz_shared: limits already in the form the rows use them.
struct Shared {
  double w_s[4], w_l[4];
  double weight_end_s, weight_end_l;
  double ds_ref, dl_ref;
  double acc_s[2];   // dds clamped to [-1000,1000] (solve_3d.cc:836,843-844; ddx_bounds_ is uniform)
  double acc_l[2];   // ddy_bounds_[i] (uniform, solve_3d.cc:1019-1020)
  double jerk_s[2], jerk_l[2];
  int variant;
};

struct KernelArgs {
  int B, S;                 // S: segments per candidate (uniform mode) / unused (ragged mode)
  int seg_stride;           // k-stride owner: seg[f][b][k] has seg_stride slots per candidate (== S when uniform)
  // ragged mode (order != nullptr): candidates bucketed by segment count s = 1..64
  const int *order;         // [B] candidate ids, stable counting sort by s
  const int *seg_count;     // [B] s of every candidate (<= 0 or > seg_stride: skipped, status set by the bucket kernel)
  const int *cand_prefix;   // [66] candidates with count < s
  const int *wave_prefix;   // [66] wavefront pairs needed by buckets < s
  const double *seg;        // [NUM_SEG_FIELDS][B][S]
  const double *init;       // [B][6]
  const double *ref_end;    // [B][2]
  const double *dl_bounds;  // [B][10]
  const double *mqm;        // [2][4][21]  M' pQp_d M, packed upper triangle (solve_3d.cc:87-143)
  double *ctrl;             // [B][12 S]
  double *axis_obj;         // [2B]
  int *axis_status;         // [2B]
  int *axis_iters;          // [2B]
  double *axis_viol;        // [2B][4] rescue pass: row violations per class (may be null)
  Shared sh;
  double eps;
  double tau;               // fraction of the step to the boundary ...
  double tau_thr;           // ... when that step is at least this long; 0.995 of it otherwise
  int max_iter;
  int tau_iters;            // iterations (since the start) during which tau may be used
  int stall_start, stall_len; // divergence test: after stall_start iterations, stall_len without a better score
  float stall_factor;         // ... and without residuals smaller by this factor
  float diverge_factor;       // mu above this multiple of the best score: the iterate has left for good
  // warm start (btrapz_warm): all optional
  const double *x0;         // [B][2][seg_stride][3] joint states at the end of every segment
  const double *lam0;       // [2][36][B][seg_stride] multipliers of an earlier solve
  double *lam_out;          // same layout, multipliers at the end of this solve
  double mu0, smin;         // lambda = lam0 + mu0 / s , s = max(gap, smin)
  // capped first launch + resume launch (btrapz_options.cap_iter): see CAPPED / RESUME in btrapz_kernels.hip
  int cap_iter;             // iterations after which a group of the capped launch may suspend (0: no cap) ...
  int cap_alone;            // ... when at most this many groups of its wavefront are still iterating,
  int cap_hi;               // and after which it suspends in any case
  double cap_score;         // a lone group whose KKT score is already below this stays: it is one or two iterations from done
  int susp_cap;             // slots of susp_state
  double *susp_state;       // [susp_cap][SUSP_FIELDS][seg_stride]
  int *susp_count;          // [1] slots handed out
  int *susp_slot;           // [2B] slot of a suspended axis problem
  int *susp_key;            // [2][B] convergence class of a suspended axis problem (key of the resume lists)
  int unc_start;            // btrapz_options.start: 1 = first one Newton step of the problem without its inequality rows
  int bucket_S;             // 0: the bucket id IS the segment count (ragged); else buckets are hint classes, S = bucket_S
  // rescue pass (btrapz_options.elastic): order = [2][B] per-axis lists, cand_prefix / wave_prefix = [2][198] tables
  double elastic_delta;     // penalty d^2 / (2 delta) on the relaxation d of every inequality row
  double elastic_tol;       // largest row violation still reported as BTRAPZ_SOLVED_INACCURATE
  int *queue;               // ipm_solve_queue_kernel: [2] next candidate per axis (zeroed before the launch)
  double *x_out;            // warm-start instantiations: joint states of the returned iterate, layout of x0 (may be null)
};

// btrapz_solve_vjp_device (btrapz_vjp.hip)
struct VjpArgs {
  int B, S, seg_stride;     // S: lanes per axis problem (the segment count of a uniform batch, seg_stride of a ragged one)
  const int *seg_count;     // [B] or null
  const Shared *sets;       // [n_sets] device view of the parameter sets
  int n_sets;
  const int *set_index;     // [B] or null (set 0)
  const double *mqm;        // [n_sets][168] M'QM tables of the sets
  const double *mqm_unit;   // [168] the same with every weight 1
  const double *seg, *ref_end, *dl_bounds, *ctrl, *lam;
  const int *status;
  const double *ctrl_bar, *cost_bar;   // either may be null
  double *g_seg, *g_init, *g_ref_end, *g_dl, *g_shared;   // any may be null
};
__global__ void vjp_kernel(const VjpArgs a);

// btrapz_solve_jvp_device (btrapz_jvp.hip)
struct JvpArgs {
  int B, S, seg_stride, T;  // S as in VjpArgs; T tangents per candidate (1..BTRAPZ_MAX_TANGENTS)
  const int *seg_count;     // [B] or null
  const Shared *sets;       // [n_sets] device view of the parameter sets
  int n_sets;
  const int *set_index;     // [B] or null (set 0)
  const double *mqm;        // [n_sets][168] M'QM tables of the sets
  const double *mqm_unit;   // [168] the same with every weight 1
  const double *seg, *ref_end, *dl_bounds, *ctrl, *lam;
  const int *status;
  const double *seg_dot, *init_dot, *ref_end_dot, *dl_dot, *shared_dot;   // tangents, leading axis T; any may be null (zero)
  double *ctrl_dot, *cost_dot;                                             // [T][B][12 seg_stride], [T][B]; either may be null
};
__global__ void jvp_kernel(const JvpArgs a);

// btrapz_check_rows_device (btrapz_check.hip)
struct CheckArgs {
  int B, seg_stride;        // groups of min(seg_stride, 64) lanes; beyond 64 slots one candidate per wavefront
  int unit;                 // btrapz_row_check.unit
  const int *seg_count;     // [B] or null
  const Shared *sets;       // [n_sets] device view of the parameter sets
  int n_sets;
  const int *set_index;     // [B] or null (set 0)
  const double *mqm;        // [n_sets][168] M'QM tables of the sets
  const double *seg, *init, *ref_end, *dl_bounds, *ctrl;
  double *margin; int *worst; double *eq_res, *obj;   // any may be null
};
__global__ void check_rows_kernel(const CheckArgs a);

// btrapz_traj_cost_device / btrapz_traj_cost_vjp_device (btrapz_acost.hip)
struct AcostArgs {
  int B, seg_stride;
  const int *seg_count;     // [B] or null (uniform)
  const Shared *sets;       // [n_sets] device view of the scoring sets
  int n_sets;
  const int *set_index;     // [B] or null (set 0)
  const double *seg, *init, *ctrl;
  const int *status;        // [B] or null (every candidate with a valid count)
  int N, ref_stride;        // ref_stride: N or 0
  const double *s_ref, *l_ref;
  double delta;
  int variant;
  double *a_cost;           // [B]
  int *n_points;            // [B] or null
  const double *a_cost_bar; // VJP: [B]
  double *ctrl_bar, *init_bar, *params_bar, *s_ref_bar, *l_ref_bar;   // VJP outputs, any may be null
};
__global__ void acost_kernel(const AcostArgs a);
__global__ void acost_vjp_kernel(const AcostArgs a);

// btrapz_sample_vjp_device / btrapz_eval_states_vjp_device (btrapz_states.hip): one wavefront per selection / candidate,
// kStatesWaves wavefronts per workgroup
constexpr int kStatesWaves = 4;
struct SampleVjpArgs {
  int B, seg_stride;
  const int *seg_count;     // [B] or null (uniform)
  double delta;
  const double *seg;
  int nsel;
  const long long *sel;     // [nsel]
  int max_points;
  const double *out_bar;    // [nsel][6][max_points]
  double *ctrl_bar;         // [nsel][12 seg_stride] or null
  double *init_bar;         // [nsel][6] or null
};
__global__ void sample_vjp_kernel(const SampleVjpArgs a);
struct StatesVjpArgs {
  int B, seg_stride;
  const int *seg_count;     // [B] or null (uniform)
  const double *seg;
  const double *ctrl;       // may be null when times_bar is
  int n_times;
  const double *times;      // [B][n_times]
  const double *x_bar;      // [B][2][n_times][3]
  double *ctrl_bar;         // [B][12 seg_stride] or null
  double *times_bar;        // [B][n_times] or null
};
__global__ void eval_states_vjp_kernel(const StatesVjpArgs a);

struct PrismRoad {              // btrapz_road in the form the prism stage uses it (prism_core.h)
  double rate;                  // knots per second (the reference hard-codes 10: `i/10`, `t0*10`)
  double s_lo, s_hi, l_lo, l_hi, l_safe, w_safe;
};

struct CorridorArgs {
  int B, N, num_obs, variant, seg_stride;
  double delta;
  const double *s_bounds, *l_bounds;   // [B][num_obs][N][2]; unused by the fused prism + corridor kernels
  // fused prism + corridor kernels (btrapz_prism_corridor_batch_device): the strips are evaluated from the prisms
  const double *prisms;                // [B][P][8]
  int P;
  PrismRoad road;
  int *n_strips;                       // [B]
  const double *ds_bounds, *dl_bounds; // [B][N][2]
  const double *s_ref, *l_ref;         // [B][N]
  double *seg;                         // [NUM_SEG_FIELDS][B][seg_stride]
  int *seg_count;                      // [B]
  double *ref_end;                     // [B][2]
  double *dl10;                        // [B][10]
  // segment-list capacities of this launch and the retry list (see corridor_kernels.hip)
  int cap_o, cap_sel;                  // segments per obstacle, selected segments
  int pass;                            // 0: one workgroup per candidate; 1: workgroups loop over retry_list
  int *retry_list, *retry_count;       // candidates whose lists overflowed in pass 0
};

__global__ void corridor_batch_kernel(const CorridorArgs a, int staged);
__global__ void corridor_batch_short_kernel(const CorridorArgs a, int staged);   // N <= 128
__global__ void corridor_first_kernel(const CorridorArgs a, int staged);         // first pass of a two-pass launch: no serial statement
__global__ void corridor_first_short_kernel(const CorridorArgs a, int staged);
__global__ void prism_corridor_batch_kernel(const CorridorArgs a, int staged);   // prisms -> strips -> corridors in one launch
__global__ void prism_corridor_batch_short_kernel(const CorridorArgs a, int staged);
__global__ void prism_corridor_first_kernel(const CorridorArgs a, int staged);
__global__ void prism_corridor_first_short_kernel(const CorridorArgs a, int staged);
struct Seg;
__global__ void corridor_serial_kernel(const CorridorArgs a, Seg *ws_all, Seg *ws_sel);   // beyond the wave-wide kernels' limits: one lane per candidate
// btrapz_corridor_batch_vjp_device (corridor_vjp.hip): the backward pass of the wave-wide corridor stage, one wavefront per
// candidate; the forward's two-pass pattern (pass, cap_o, cap_sel, retry list as in CorridorArgs)
struct CorridorVjpArgs {
  int B, N, num_obs, variant, seg_stride;
  double delta;
  const double *s_bounds, *l_bounds, *ds_bounds, *s_ref, *l_ref;
  const double *seg_bar, *ref_end_bar, *dl10_bar;   // cotangents, any may be null
  btrapz_knot_grads out;                            // zeroed in front of the launch; any may be null
  int cap_o, cap_sel, pass, staged;                 // staged: the slope table fits LDS
  int *retry_list, *retry_count;
};
constexpr int kCorridorVjpTerms = 16;               // terms an output segment stages (corridor_vjp_core.h: 4 + 6 + 2 + 2 + 2)
// Dynamic LDS of corridor_vjp_kernel, byte offsets (the host sizes the launch with `bytes`):
//   [0)    Seg all[O * cap_o]; later the staged terms, double val[16][rows] | int idx[16][rows]
//   [sel)  Seg sel[cap_sel]
//   [dyn)  slopes [O][N][2] when staged; later s_ref[N] | l_ref[N] | ds_bounds[N][2]
//   [ints) int ocount[64] | int word[4] | short slot_of[O * cap_o] | short pick[cap_sel]
struct CorridorVjpLds { int rows; size_t sel, dyn, ints, bytes; };
__host__ __device__ inline CorridorVjpLds corridor_vjp_lds(int N, int O, int cap_o, int cap_sel, int seg_stride, int staged) {
  CorridorVjpLds l;
  const size_t cap_all = (size_t)cap_o * O, seg_bytes = 104;   // sizeof(Seg)
  l.rows = (cap_sel < seg_stride ? cap_sel : seg_stride) + 1;   // output segments, and one row for ref_end
  const size_t terms = (size_t)kCorridorVjpTerms * l.rows * (sizeof(double) + sizeof(int));
  l.sel = ((seg_bytes * cap_all > terms ? seg_bytes * cap_all : terms) + 15) & ~(size_t)15;
  l.dyn = (l.sel + seg_bytes * cap_sel + 15) & ~(size_t)15;
  const size_t table = staged ? (size_t)O * N * 2 : 0, refs = (size_t)N * 4;
  l.ints = l.dyn + sizeof(double) * (table > refs ? table : refs);
  l.bytes = l.ints + sizeof(int) * (64 + 4) + sizeof(short) * (cap_all + cap_sel);
  return l;
}
__global__ void corridor_vjp_kernel(const CorridorVjpArgs a);
// fixed_S = 0: bucket by segment count (ragged batches); > 0: uniform batch of fixed_S segments, bucket by hint class
// candidates that cannot start: keys[b] = 0 and their records written here (btrapz_options.compact; btrapz_kernels.hip)
__global__ void prestart_kernel(const KernelArgs a, int S_uniform, const int *seg_count, int *keys);
__global__ void bucket_hist_kernel(int B, int seg_stride, const int *seg_count, int *meta, int fixed_S);
__global__ void bucket_prefix_kernel(int *meta, int fixed_S);
__global__ void bucket_scatter_kernel(int B, int seg_stride, const int *seg_count, int *meta, int *order,
                                      double *axis_obj, int *axis_status, int *axis_iters, int fixed_S);
__global__ void ipm_solve_kernel(const KernelArgs a, const double *__restrict__ mqm);
__global__ void ipm_solve_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm);       // through a.order
__global__ void ipm_solve_warm_kernel(const KernelArgs a, const double *__restrict__ mqm);          // + btrapz_warm
__global__ void ipm_solve_warm_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm);
#ifdef BTRAPZ_EXPERIMENTS
__global__ void ipm_solve_queue_kernel(const KernelArgs a, const double *__restrict__ mqm);         // persistent, candidate queue
#endif
__global__ void ipm_solve_elastic_kernel(const KernelArgs a, const double *__restrict__ mqm);       // rescue pass
__global__ void ipm_solve_split_kernel(const KernelArgs a, const double *__restrict__ mqm);         // one candidate per wavefront, rows over 3 lanes
__global__ void ipm_solve_capped_kernel(const KernelArgs a, const double *__restrict__ mqm);        // first launch of a capped solve
__global__ void ipm_solve_capped_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm);  // ... of a ragged batch
__global__ void ipm_solve_resume_kernel(const KernelArgs a, const double *__restrict__ mqm);        // ... and the launch that carries the suspended problems on
// the solve at two wavefronts per SIMD (btrapz_lean_body.h; instantiated in btrapz_lean.hip and btrapz_lean_warm.hip)
__global__ void ipm_solve_lean_kernel(const KernelArgs a, const double *__restrict__ mqm);
__global__ void ipm_solve_lean_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm);
__global__ void ipm_solve_lean_capped_kernel(const KernelArgs a, const double *__restrict__ mqm);
__global__ void ipm_solve_lean_capped_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm);
__global__ void ipm_solve_lean_resume_kernel(const KernelArgs a, const double *__restrict__ mqm);
// the lean two-launch solve as three launches (btrapz_lean_pipe.hip): one axis's capped launch, one grid of one axis's
// resume wavefronts + the other axis's capped launch, one axis's resume launch; the lengths of both resume lists to the host
__global__ void ipm_solve_lean_pipe_capped_kernel(const KernelArgs a, const double *__restrict__ mqm, int axis);
__global__ void ipm_solve_lean_pipe_resume_kernel(const KernelArgs a, const double *__restrict__ mqm, int axis);
__global__ void ipm_solve_lean_pipe_kernel(const KernelArgs a, const double *__restrict__ mqm, int n_resume, int resume_axis, int capped_axis);
__global__ void pipe_counts_kernel(const int *tables, volatile int *host_counts);
// ... and with one axis quiet (btrapz_lean_quiet.hip): that axis through the plain body -- in a launch of its own, or in one
// grid behind the other axis's resume wavefronts --, and the count it would have handed over, estimated from axis_iters
__global__ void ipm_solve_lean_quiet_plain_kernel(const KernelArgs a, const double *__restrict__ mqm, int axis);
__global__ void ipm_solve_lean_quiet_kernel(const KernelArgs a, const double *__restrict__ mqm, int n_resume, int resume_axis, int plain_axis);
__global__ void quiet_counts_kernel(const int *__restrict__ axis_iters, int B, int gpw, int quiet_axis, int cap_iter, int cap_hi,
                                    const int *tables, int *acc, volatile int *host_counts);
__global__ void ipm_solve_lean_warm_kernel(const KernelArgs a, const double *__restrict__ mqm);
__global__ void ipm_solve_lean_warm_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm);
// btrapz_solve_sets_device (btrapz_sets.hip, btrapz_kernels.hip): mqm = the per-set tables [n_sets][168]
__global__ void ipm_solve_sets_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, int n_keys);
__global__ void ipm_solve_sets_warm_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, int n_keys);
__global__ void ipm_solve_lean_sets_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, int n_keys);
__global__ void ipm_solve_lean_sets_warm_ordered_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, int n_keys);
__global__ void ipm_solve_sets_split_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, const int *set_index, int n_sets);
__global__ void ipm_solve_long_sets_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, const int *set_index, int n_sets);
// btrapz_solve_long_sets_device (btrapz_kernels.hip): warm starts beyond 64 segments and the rescue pass, with sets
__global__ void ipm_solve_long_warm_sets_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, const int *set_index, int n_sets);
__global__ void ipm_solve_elastic_sets_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, int n_keys);   // tables [2][3 n_keys + 2], lists [2][B]
__global__ void ipm_solve_long_elastic_sets_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, const int *set_index, int n_sets);
__global__ void ipm_solve_long_rescue_sets_kernel(const KernelArgs a, const double *__restrict__ mqm, const Shared *sets, const int *set_index, int n_sets);
// masked[axis][b] = set_index[b] where that axis problem stalled, else -1: the "set index" the bucket kernels list the rescue pass by
__global__ void sets_rescue_index_kernel(int B, const int *set_index, const int *axis_status, int *masked);
__global__ void sets_hist_kernel(int B, int seg_stride, const int *seg_count, const int *set_index, int n_sets, int n_keys, int *meta);
__global__ void sets_prefix_kernel(int n_keys, int fixed_S, int *meta);
__global__ void sets_scatter_kernel(int B, int seg_stride, const int *seg_count, const int *set_index, int n_sets, int n_keys,
                                    int *meta, int *order, double *axis_obj, int *axis_status, int *axis_iters);
#define BTRAPZ_SUSPENDED (-7)   // internal: an axis problem the capped launch handed over (never leaves the library)
__global__ void ipm_solve_long_kernel(const KernelArgs a, const double *__restrict__ mqm);          // 65..256 segments: one axis problem per workgroup
__global__ void ipm_solve_long_warm_kernel(const KernelArgs a, const double *__restrict__ mqm);     // + btrapz_warm (btrapz_solve_long_warm_device)
__global__ void ipm_solve_long_elastic_kernel(const KernelArgs a, const double *__restrict__ mqm);  // rescue pass of the long form (<= 192 segments)
__global__ void ipm_solve_long_rescue_kernel(const KernelArgs a, const double *__restrict__ mqm);   // ... of 193..256 segments (btrapz_solve_long_rescue_device)
__global__ void rescue_keys_kernel(int B, int S, const int *seg_count, const int *axis_status, int *keys, int all);
__global__ void rescue_init_kernel(int B, int S, const int *seg_count, double *axis_obj, int *axis_status, int *axis_iters);
struct MqmWeights { double w[2][4]; };   // [axis][ref, dref, acc, jerk]
__global__ void mqm_table_kernel(MqmWeights w, double *out);
__global__ void mqm_sets_kernel(const Shared *sets, double *out);   // one block per set: out [n_sets][2][4][21]
__global__ void rescue_violations_kernel(int B, const double *axis_viol, double *viol);
__global__ void finalize_kernel(int B, const double *axis_obj, const int *axis_status, const int *axis_iters,
                                double *cost, int *status, int *iters);
__global__ void argmin_kernel(int group, long long index_base, const double *cost, long long *best_idx,
                              double *best_cost, double *part_cost, long long *part_idx);
__global__ void argmin_final_kernel(int chunks, long long index_base, const double *part_cost, const long long *part_idx,
                                    long long *best_idx, double *best_cost);
__global__ void argmin_pairs_kernel(int world, int n, const long long *pairs, double *best_cost, long long *best_idx);
__global__ void eval_states_kernel(int B, int seg_stride, const int *seg_count, const double *seg, const double *ctrl,
                                   int n_times, const double *times, double *x);
__global__ void sample_kernel(int B, int seg_stride, const int *seg_count, double delta, const double *seg,
                              const double *init, const double *ctrl, int nsel, const long long *sel, int max_points,
                              double *out, int *npoints);

__global__ void single_candidate_kernel(const KernelArgs a, const double *__restrict__ mqm, double delta, int max_points,
                                        double *out);
__global__ void single_candidate_split_kernel(const KernelArgs a, const double *__restrict__ mqm, double delta, int max_points,
                                              double *out);
__global__ void single_candidate_warm_split_kernel(const KernelArgs a, const double *__restrict__ mqm, double delta, int max_points,
                                                   double *out);
__global__ void single_candidate_warm_kernel(const KernelArgs a, const double *__restrict__ mqm, double delta, int max_points,
                                             double *out);

}  // namespace btrapz

// library-internal: the HIP device a context lives on
int btrapz_ctx_device(const btrapz_ctx *ctx);
// library-internal: what btrapz_last_error returns next, for the entry points defined outside btrapz_host.hip
void btrapz_ctx_set_error(btrapz_ctx *ctx, const char *what);
// library-internal: find_traj's single-candidate path.  One launch; in and out may be host memory
// mapped into the device.  in: seg[17 S] init[6] ref_end[2] dl[10] mqm[168]; out: cost, status|iters, np, ctrl[12 S],
// traj[6 max_points].  The M'QM table comes from the caller (btrapz_mqm_table_host).
// warm: 0 cold; 1 start from what the previous warm call of this context left (same variant and segment count, else
// cold) and leave this call's joint states and multipliers for the next one.
int btrapz_launch_single(btrapz_ctx *ctx, const btrapz_shared *shared, const btrapz_options *opt, int S, const double *in,
                         double *out, int max_points, int warm, void *stream);
void btrapz_single_forget(btrapz_ctx *ctx);   // the next warm call starts cold
void btrapz_mqm_table_host(const btrapz_shared *shared, double *table /* [2][4][21] */);
#endif
