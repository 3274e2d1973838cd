"""The batched solve as a differentiable layer: spectral_amd.diff.solve(...) returns (ctrl, cost, status) with a
torch.autograd graph whose backward is one btrapz_solve_vjp_device launch (include/btrapz_hip.h).  The gradient math
is HIP; torch only sums the per-candidate parameter gradients of a set.  spectral_amd.diff.traj_cost(...) scores the
sampled trajectories as find_traj does (a_cost, btrapz_traj_cost_device) with a backward of one
btrapz_traj_cost_vjp_device launch: diff.solve followed by diff.traj_cost is the reference's tuning objective."""
import torch

from . import layout as L
from .solver import DeviceBatch

N_PARAMS = 20   # layout.Shared.as_array() without delta


def shared_from_params(row, variant=0, delta=0.1):
    """A [20] parameter row (w_s[4] w_l[4] weight_end_s weight_end_l ds_ref dl_ref dds[2] ddds[2] ddl[2] dddl[2]) ->
    layout.Shared."""
    v = [float(x) for x in row]
    return L.Shared(w_s=tuple(v[0:4]), w_l=tuple(v[4:8]), weight_end_s=v[8], weight_end_l=v[9], ds_ref=v[10],
                    dl_ref=v[11], dds=tuple(v[12:14]), ddds=tuple(v[14:16]), ddl=tuple(v[16:18]), dddl=tuple(v[18:20]),
                    delta=float(delta), variant=int(variant))


def params_from_shared(sh):
    """layout.Shared -> its [20] parameter row (numpy)."""
    return sh.as_array()[:N_PARAMS]


def _f64(t):
    return t if (t.dtype == torch.float64 and t.is_contiguous()) else t.to(torch.float64).contiguous()


def _on(solver, *tensors):
    """The tensors detached, as contiguous float64 on the solver's device."""
    return [_f64(t.detach()).to(solver.device) for t in tensors]


def _check_params(params, set_index):
    if set_index is None and params.dim() != 1:
        raise ValueError("params must be [20] without set_index, [n_sets, 20] with it")
    if params.shape[-1] != N_PARAMS:
        raise ValueError("params rows have %d entries (layout.Shared.as_array() without delta)" % N_PARAMS)


def _sets_of_params(params, variant, delta):
    """Parameter rows [20] or [n_sets, 20] -> list of layout.Shared."""
    return [shared_from_params(r, variant, delta) for r in params.detach().to("cpu", torch.float64).reshape(-1, N_PARAMS).tolist()]


def _sum_rows(g, set_index, n_sets):
    """Per-candidate parameter rows [B, 20] -> [n_sets, 20] (candidates outside [0, n_sets) carry zero rows)."""
    if set_index is None:
        return g.sum(0)
    idx = set_index.long().clamp(0, n_sets - 1)
    out = torch.zeros((n_sets, N_PARAMS), dtype=torch.float64, device=g.device)
    out.index_add_(0, idx, g)
    return out


def _solve_kept(solver, seg, init, ref_end, dl_bounds, params, seg_count, set_index, variant, delta):
    """(record, sets, result dict) of the solve with its multipliers kept and no rescue pass; ctrl starts zeroed."""
    rec = DeviceBatch.from_tensors(*_on(solver, seg, init, ref_end, dl_bounds), seg_count=seg_count)
    sets = _sets_of_params(params, variant, delta)
    o = solver.new_result(rec.B, rec.S, zero_ctrl=True)
    if set_index is not None:
        return rec, sets, solver.solve_sets(rec, sets, set_index, keep_multipliers=True, out=o)
    return rec, sets, solver.solve(rec, sets[0], keep_multipliers=True, out=o)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, init, ref_end, dl_bounds, params, solver, seg_count, set_index, variant, delta):
        ctx.rec, ctx.sets, o = _solve_kept(solver, seg, init, ref_end, dl_bounds, params, seg_count, set_index, variant, delta)
        ctx.solver, ctx.set_index, ctx.out = solver, set_index, o
        ctx.params_shape, ctx.params_device = params.shape, params.device
        ctx.mark_non_differentiable(o["status"])
        return o["ctrl"], o["cost"], o["status"]

    @staticmethod
    def backward(ctx, ctrl_bar, cost_bar, _status_bar):
        if ctrl_bar is None and cost_bar is None:
            return (None,) * 10
        g = ctx.solver.solve_vjp(ctx.rec, ctx.sets, ctx.out, ctrl_bar, cost_bar, set_index=ctx.set_index)
        need = ctx.needs_input_grad
        gp = None
        if need[4]:
            gp = _sum_rows(g["shared"], ctx.set_index, len(ctx.sets)).reshape(ctx.params_shape).to(ctx.params_device)
        return (g["seg"] if need[0] else None, g["init"] if need[1] else None, g["ref_end"] if need[2] else None,
                g["dl_bounds"] if need[3] else None, gp, None, None, None, None, None)


def solve(solver, seg, init, ref_end, dl_bounds, params, *, seg_count=None, set_index=None, variant=0, delta=0.1):
    """Differentiable batched solve.  seg [NUM_SEG_FIELDS, B, S], init [B, 6], ref_end [B, 2], dl_bounds [B, 10]: the
    batch (device tensors, float64); params: [20] (one set) or [n_sets, 20] with set_index (int32 [B]) -- the parameter
    rows of shared_from_params.  seg_count: int32 [B] for a ragged batch.  Returns (ctrl [B, 12 S], cost [B], status [B]);
    status is not differentiable.  The solve runs with its multipliers kept and no rescue pass (elastic = 0); gradients
    are defined for candidates of status 1 or 2 and are 0 elsewhere (btrapz_solve_vjp_device).  Field 0 of seg (the
    segment durations) gets no gradient."""
    _check_params(params, set_index)
    return _Solve.apply(seg, init, ref_end, dl_bounds, params, solver, seg_count, set_index, variant, delta)


def _solve_long_kept(solver, seg, init, ref_end, dl_bounds, params, seg_count, variant, delta, set_index=None):
    """_solve_kept through BatchSolver.solve_long: candidates of up to 256 segments; with set_index through
    BatchSolver.solve_long_sets, a parameter row per set."""
    rec = DeviceBatch.from_tensors(*_on(solver, seg, init, ref_end, dl_bounds), seg_count=seg_count)
    sets = _sets_of_params(params, variant, delta)
    o = solver.new_result(rec.B, rec.S, zero_ctrl=True)
    if set_index is not None:
        return rec, sets, solver.solve_long_sets(rec, sets, set_index, keep_multipliers=True, out=o)
    return rec, sets, solver.solve_long(rec, sets[0], keep_multipliers=True, out=o)


class _SolveLong(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, init, ref_end, dl_bounds, params, solver, seg_count, variant, delta, set_index):
        ctx.rec, ctx.sets, o = _solve_long_kept(solver, seg, init, ref_end, dl_bounds, params, seg_count, variant, delta, set_index)
        ctx.solver, ctx.set_index, ctx.out = solver, set_index, o
        ctx.params_shape, ctx.params_device = params.shape, params.device
        ctx.mark_non_differentiable(o["status"])
        return o["ctrl"], o["cost"], o["status"]

    @staticmethod
    def backward(ctx, ctrl_bar, cost_bar, _status_bar):
        if ctrl_bar is None and cost_bar is None:
            return (None,) * 10
        g = ctx.solver.solve_long_vjp(ctx.rec, ctx.sets, ctx.out, ctrl_bar, cost_bar, set_index=ctx.set_index)
        need = ctx.needs_input_grad
        gp = _sum_rows(g["shared"], ctx.set_index, len(ctx.sets)).reshape(ctx.params_shape).to(ctx.params_device) if need[4] else None
        return (g["seg"] if need[0] else None, g["init"] if need[1] else None, g["ref_end"] if need[2] else None,
                g["dl_bounds"] if need[3] else None, gp, None, None, None, None, None)


def solve_long(solver, seg, init, ref_end, dl_bounds, params, *, seg_count=None, variant=0, delta=0.1):
    """diff.solve for candidates of up to 256 segments: the forward is BatchSolver.solve_long with the multipliers kept
    (btrapz_solve_long_warm_device, cold start, no rescue pass), the backward one btrapz_solve_long_vjp_device launch.
    Arguments and results as diff.solve, with S up to 256 and params ONE row [20]; with a parameter row per set:
    solve_long_sets."""
    _check_params(params, None)
    return _SolveLong.apply(seg, init, ref_end, dl_bounds, params, solver, seg_count, variant, delta, None)


def solve_long_sets(solver, seg, init, ref_end, dl_bounds, params, *, set_index, seg_count=None, variant=0, delta=0.1):
    """solve_long with a parameter set per candidate: params [n_sets, 20], set_index int32 [B].  The forward is
    BatchSolver.solve_long_sets with the multipliers kept (btrapz_solve_long_sets_device, no rescue pass), the backward
    btrapz_solve_long_vjp_device with set_index; the gradient rows of params are summed per set as diff.solve sums them."""
    if set_index is None:
        raise ValueError("solve_long_sets: set_index (int32 [B]) is required; one parameter row: solve_long")
    _check_params(params, set_index)
    return _SolveLong.apply(seg, init, ref_end, dl_bounds, params, solver, seg_count, variant, delta, set_index)


class _TrajCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, init, params, s_ref, l_ref, seg, solver, seg_count, set_index, status, variant, delta):
        ctrl_d, init_d, seg_d, s_d, l_d = _on(solver, ctrl, init, seg, s_ref, l_ref)
        sets = _sets_of_params(params, variant, delta)
        rec = DeviceBatch.from_tensors(seg_d, init_d, seg_count=seg_count)
        cost, _ = solver.traj_cost(rec, sets, ctrl_d, s_d, l_d, status=status, set_index=set_index)
        ctx.solver, ctx.sets, ctx.rec, ctx.set_index, ctx.status = solver, sets, rec, set_index, status
        ctx.arrays = (ctrl_d, s_d, l_d)
        ctx.shapes = (params.shape, params.device, s_ref.shape, l_ref.shape)
        return cost

    @staticmethod
    def backward(ctx, cost_bar):
        if cost_bar is None:
            return (None,) * 12
        ctrl_d, s_d, l_d = ctx.arrays
        B = ctx.rec.B
        # a candidate that is not scored has cost +inf and a zero gradient: its cotangent must not turn that into NaN
        g = ctx.solver.traj_cost_vjp(ctx.rec, ctx.sets, ctrl_d, s_d, l_d, cost_bar.reshape(B), status=ctx.status,
                                     set_index=ctx.set_index)
        need = ctx.needs_input_grad
        p_shape, p_dev, s_shape, l_shape = ctx.shapes
        gp = _sum_rows(g["params"], ctx.set_index, len(ctx.sets)).reshape(p_shape).to(p_dev) if need[2] else None
        gs = (g["s_ref"].sum(0) if s_d.dim() == 1 else g["s_ref"]).reshape(s_shape) if need[3] else None
        gl = (g["l_ref"].sum(0) if l_d.dim() == 1 else g["l_ref"]).reshape(l_shape) if need[4] else None
        return (g["ctrl"] if need[0] else None, g["init"] if need[1] else None, gp, gs, gl,
                None, None, None, None, None, None, None)


def traj_cost(ctrl, seg, init, s_ref, l_ref, params, solver, seg_count=None, set_index=None, status=None, variant=0,
              delta=0.1):
    """Differentiable a_cost (btrapz_traj_cost_device): the score find_traj returns, of every candidate's sampled
    trajectory.  ctrl [B, 12 S], seg [NUM_SEG_FIELDS, B, S] (its durations place the samples), init [B, 6]; s_ref /
    l_ref: [B, N], or [N] for one line shared by every candidate; params: the SCORING parameter rows, [20] (one set) or
    [n_sets, 20] with set_index (int32 [B]) -- the cuboid variant uses no weights.  seg_count: int32 [B] for a ragged
    batch; status: int32 [B] (e.g. the solve's): candidates outside {1, 2} are not scored.  Returns a_cost [B] (+inf where
    not scored).  Gradients flow to ctrl, init, params (summed over a set's rows), s_ref and l_ref; the durations are not
    differentiated.  When the same params tensor also feeds diff.solve, autograd adds the explicit part and the part
    through the solve."""
    _check_params(params, set_index)
    return _TrajCost.apply(ctrl, init, params, s_ref, l_ref, seg, solver, seg_count, set_index, status, variant, delta)


def _sum_selections(rows, sel, B):
    """Per-selection rows [nsel, n] -> per-candidate rows [B, n] in a fixed order (sel may repeat a candidate, and
    index_add_ on the device adds with atomics): the r-th selection of every candidate is added in pass r, and within a
    pass no candidate appears twice.  Selections outside [0, B) carry zero rows."""
    out = torch.zeros((B, rows.shape[1]), dtype=rows.dtype, device=rows.device)
    idx = sel.long().clamp(0, B - 1)
    order = torch.sort(idx, stable=True).indices
    srt = idx[order]
    pos = torch.arange(srt.numel(), device=srt.device)
    heads = torch.ones_like(srt, dtype=torch.bool)
    heads[1:] = srt[1:] != srt[:-1]
    rank = torch.empty_like(pos)
    rank[order] = pos - torch.cummax(torch.where(heads, pos, torch.zeros_like(pos)), 0).values
    for r in range(int(rank.max().item()) + 1):
        m = rank == r
        out[idx[m]] += rows[m]
    return out


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, init, seg, solver, seg_count, sel, delta):
        d = solver.device
        ctrl_d, init_d, seg_d = _on(solver, ctrl, init, seg)
        rec = DeviceBatch.from_tensors(seg_d, init_d, seg_count=seg_count)
        sel = (torch.arange(rec.B, device=d) if sel is None else sel).to(d, dtype=torch.int64).contiguous()
        out, npts = solver.sample(rec, ctrl_d, sel, delta)
        ctx.solver, ctx.sel, ctx.delta, ctx.rec = solver, sel, delta, rec
        ctx.mark_non_differentiable(npts)
        return out, npts

    @staticmethod
    def backward(ctx, out_bar, _npts_bar):
        if out_bar is None:
            return (None,) * 7
        need = ctx.needs_input_grad
        g = ctx.solver.sample_vjp(ctx.rec, ctx.sel, ctx.delta, out_bar, want_ctrl=need[0], want_init=need[1])
        B = ctx.rec.B
        return (_sum_selections(g["ctrl"], ctx.sel, B) if need[0] else None,
                _sum_selections(g["init"], ctx.sel, B) if need[1] else None, None, None, None, None, None)


def sample(ctrl, seg, init, solver, seg_count=None, sel=None, delta=0.1):
    """Differentiable Bernstein sampling (btrapz_sample_device / btrapz_sample_ragged_device): the rows find_traj writes.
    ctrl [B, 12 S], seg [NUM_SEG_FIELDS, B, S] (its durations place the samples), init [B, 6] (sample 0); seg_count: int32
    [B] for a ragged batch; sel: the candidates to sample (int64, default every candidate in order; may repeat).  Returns
    (traj [nsel, 6, max_points] -- s, ds, dds, l, dl, ddl every delta seconds -- and npoints [nsel], not
    differentiable).  Gradients flow to ctrl and init through one btrapz_sample_vjp_device launch, whose per-selection
    rows are summed onto the candidates in a fixed order; the durations are not differentiated."""
    return _Sample.apply(ctrl, init, seg, solver, seg_count, sel, delta)


class _EvalStates(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctrl, times, seg, solver, seg_count):
        ctrl_d, times_d, seg_d = _on(solver, ctrl, times, seg)
        ctx.solver, ctx.rec = solver, DeviceBatch.from_tensors(seg_d, seg_count=seg_count)
        x = solver.eval_states(ctx.rec, ctrl_d, times_d)
        ctx.arrays = (ctrl_d, times_d)
        ctx.times_shape = times.shape
        return x

    @staticmethod
    def backward(ctx, x_bar):
        if x_bar is None:
            return (None,) * 5
        need = ctx.needs_input_grad
        ctrl_d, times_d = ctx.arrays
        g = ctx.solver.eval_states_vjp(ctx.rec, ctrl_d, times_d, x_bar, want_ctrl=need[0], want_times=need[1])
        return (g["ctrl"] if need[0] else None, g["times"].reshape(ctx.times_shape) if need[1] else None, None, None, None)


def eval_states(ctrl, seg, times, solver, seg_count=None):
    """Differentiable state evaluation (btrapz_eval_states_device): x [B, 2, n_times, 3] = (p, v, a) per axis of every
    candidate at times [B, n_times] seconds from the start of its horizon.  ctrl [B, 12 S], seg [NUM_SEG_FIELDS, B, S];
    seg_count: int32 [B] for a ragged batch.  Gradients flow to ctrl and to times (the derivative along the trajectory:
    0 for a time that is not > 0, the end velocity beyond the horizon) through one btrapz_eval_states_vjp_device launch;
    the durations are not differentiated."""
    return _EvalStates.apply(ctrl, times, seg, solver, seg_count)


# ---- forward mode: Jacobian-vector products (btrapz_solve_jvp_device) --------------------------------------------------

def solve_kept(solver, seg, init, ref_end, dl_bounds, params, *, seg_count=None, set_index=None, variant=0, delta=0.1):
    """The solve of diff.solve without a graph: multipliers kept, no rescue pass.  Returns the result dict ("ctrl", "cost",
    "status", "iters", "lam"): what solve_jacobian(out=...) and BatchSolver.solve_jvp / solve_vjp take."""
    return _solve_kept(solver, seg, init, ref_end, dl_bounds, params, seg_count, set_index, variant, delta)[2]


def solve_jacobian(solver, seg, init, ref_end, dl_bounds, params, columns, *, seg_count=None, set_index=None, variant=0,
                   delta=0.1, log=False, out=None):
    """Columns of the solve's Jacobian with respect to its parameters: one solve with the multipliers kept (solve_kept)
    and ONE btrapz_solve_jvp_device launch with
    T = len(columns) unit tangents on the named columns of the parameter row (shared_from_params' order), each
    candidate's on its own set's row.  log=True: the derivative with respect to the logarithm of the parameter (the unit
    tangent scaled by the parameter's value).  Arguments as diff.solve.  Returns a dict of device tensors: "ctrl"
    [B, 12 S], "cost" [B], "status" [B], "dctrl" [T, B, 12 S], "dcost" [T, B], and "out", the solve's result dict.

    out: the result dict of a solve_kept of a previous call, to skip the solve (the fit differentiates the point its last
    step accepted).  PRECONDITION: `out` is the solve of exactly these inputs, params, seg_count, set_index, variant and
    delta.  Nothing can check that: the derivative is stated at out["ctrl"] with the active set of out["lam"], and with
    another problem's arrays it is the derivative of nothing, returned without an error.  Only the shapes are checked."""
    _check_params(params, set_index)
    if out is not None:
        B_, S_ = seg.shape[1], seg.shape[2]
        if out.get("lam") is None or tuple(out["ctrl"].shape) != (B_, 12 * S_) or tuple(out["lam"].shape) != (2, 36, B_, S_) \
                or tuple(out["status"].shape) != (B_,):
            raise ValueError("out: the result dict of solve_kept for this batch (ctrl [B, 12 S], lam [2, 36, B, S], status [B])")
    columns = [int(c) for c in columns]
    if not columns or min(columns) < 0 or max(columns) >= N_PARAMS:
        raise ValueError("columns: at least one, each in [0, %d)" % N_PARAMS)
    d = solver.device
    rec = DeviceBatch.from_tensors(*_on(solver, seg, init, ref_end, dl_bounds), seg_count=seg_count)
    B = rec.B
    if out is None:
        out = solve_kept(solver, rec.seg, rec.init, rec.ref_end, rec.dl_bounds, params, seg_count=seg_count,
                         set_index=set_index, variant=variant, delta=delta)
    rows = params.detach().to(d, torch.float64).reshape(-1, N_PARAMS)
    sets = _sets_of_params(params, variant, delta)
    T = len(columns)
    tan = torch.zeros((T, B, N_PARAMS), dtype=torch.float64, device=d)
    per_cand = rows[set_index.long().clamp(0, rows.shape[0] - 1)] if set_index is not None else rows[:1].expand(B, N_PARAMS)
    for t, c in enumerate(columns):
        tan[t, :, c] = per_cand[:, c] if log else 1.0
    j = solver.solve_jvp(rec, sets, out, {"shared": tan}, set_index=set_index)
    return dict(ctrl=out["ctrl"], cost=out["cost"], status=out["status"], dctrl=j["ctrl"], dcost=j["cost"], out=out)


def solve_long_jacobian(solver, seg, init, ref_end, dl_bounds, params, columns, *, seg_count=None, variant=0, delta=0.1,
                        log=False, out=None):
    """diff.solve_jacobian for candidates of up to 256 segments: one BatchSolver.solve_long with the multipliers kept and
    ONE btrapz_solve_long_jvp_device call with T = len(columns) unit tangents on the named columns of the parameter row.
    params: one row [20] (a row per set: solve_long_sets_jacobian).  Arguments, `out` (with its precondition) and the returned
    dict as diff.solve_jacobian."""
    return _solve_long_jacobian(solver, seg, init, ref_end, dl_bounds, params, columns, seg_count, None, variant, delta, log, out)


def solve_long_sets_jacobian(solver, seg, init, ref_end, dl_bounds, params, columns, *, set_index, seg_count=None, variant=0,
                             delta=0.1, log=False, out=None):
    """solve_long_jacobian with a parameter set per candidate: params [n_sets, 20], set_index int32 [B]; the solve is
    BatchSolver.solve_long_sets with the multipliers kept, and each candidate's tangent sits on its own set's row."""
    if set_index is None:
        raise ValueError("solve_long_sets_jacobian: set_index (int32 [B]) is required; one parameter row: solve_long_jacobian")
    return _solve_long_jacobian(solver, seg, init, ref_end, dl_bounds, params, columns, seg_count, set_index, variant, delta, log, out)


def _solve_long_jacobian(solver, seg, init, ref_end, dl_bounds, params, columns, seg_count, set_index, variant, delta, log, out):
    _check_params(params, set_index)
    if out is not None:
        B_, S_ = seg.shape[1], seg.shape[2]
        if out.get("lam") is None or tuple(out["ctrl"].shape) != (B_, 12 * S_) or tuple(out["lam"].shape) != (2, 36, B_, S_) \
                or tuple(out["status"].shape) != (B_,):
            raise ValueError("out: the result dict of solve_long with the multipliers kept for this batch (ctrl [B, 12 S], lam [2, 36, B, S], status [B])")
    columns = [int(c) for c in columns]
    if not columns or min(columns) < 0 or max(columns) >= N_PARAMS:
        raise ValueError("columns: at least one, each in [0, %d)" % N_PARAMS)
    d = solver.device
    if out is None:
        rec, sets, out = _solve_long_kept(solver, seg, init, ref_end, dl_bounds, params, seg_count, variant, delta, set_index)
    else:
        rec = DeviceBatch.from_tensors(*_on(solver, seg, init, ref_end, dl_bounds), seg_count=seg_count)
        sets = _sets_of_params(params, variant, delta)
    rows = params.detach().to(d, torch.float64).reshape(-1, N_PARAMS)
    tan = torch.zeros((len(columns), rec.B, N_PARAMS), dtype=torch.float64, device=d)
    per_cand = rows[set_index.long().clamp(0, rows.shape[0] - 1)] if set_index is not None else rows[:1].expand(rec.B, N_PARAMS)
    for t, c in enumerate(columns):
        tan[t, :, c] = per_cand[:, c] if log else 1.0
    j = solver.solve_long_jvp(rec, sets, out, {"shared": tan}, set_index=set_index)
    return dict(ctrl=out["ctrl"], cost=out["cost"], status=out["status"], dctrl=j["ctrl"], dcost=j["cost"], out=out)


def sample_jvp(solver, dctrl, seg, dinit=None, seg_count=None, sel=None, delta=0.1):
    """Tangents of the sampled trajectories.  Sampling is linear in (ctrl, init), so its Jacobian-vector product is the
    forward kernel applied to the tangents: dctrl [T, B, 12 S] and dinit [T, B, 6] (None: zero) -> [T, nsel, 6, max_points],
    one launch over the T B tangent candidates (seg, seg_count and sel as diff.sample, repeated per tangent)."""
    d = solver.device
    dctrl, seg = _on(solver, dctrl, seg)
    T, B = dctrl.shape[0], dctrl.shape[1]
    di = torch.zeros((T * B, 6), dtype=torch.float64, device=d) if dinit is None else _on(solver, dinit)[0].reshape(T * B, 6)
    sel = (torch.arange(B, device=d) if sel is None else sel.to(d)).to(torch.int64)
    sel_rep = (sel[None, :] + B * torch.arange(T, device=d)[:, None]).reshape(-1)
    cnt = None if seg_count is None else seg_count.repeat(T).contiguous()
    with torch.no_grad():
        traj, _ = sample(dctrl.reshape(T * B, -1), seg.repeat(1, T, 1).contiguous(), di, solver, seg_count=cnt, sel=sel_rep, delta=delta)
    return traj.reshape(T, sel.numel(), 6, traj.shape[2])


def eval_states_jvp(solver, dctrl, seg, times, seg_count=None):
    """Tangents of the evaluated states.  State evaluation is linear in ctrl at fixed times, so its Jacobian-vector product
    is the forward kernel applied to the tangents: dctrl [T, B, 12 S], times [B, n_times] -> [T, B, 2, n_times, 3]."""
    dctrl, seg, times = _on(solver, dctrl, seg, times)
    T, B = dctrl.shape[0], dctrl.shape[1]
    cnt = None if seg_count is None else seg_count.repeat(T).contiguous()
    with torch.no_grad():
        x = eval_states(dctrl.reshape(T * B, -1), seg.repeat(1, T, 1).contiguous(), times.repeat(T, 1).contiguous(), solver, seg_count=cnt)
    return x.reshape(T, B, 2, times.shape[1], 3)


class _Corridor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref, solver, variant, delta, seg_stride):
        d = solver.device
        ins = _on(solver, s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref)
        B, N = ins[0].shape[0], ins[0].shape[2]
        init = torch.zeros((B, 6), dtype=torch.float64, device=d)   # (the stage does not read it)
        rec = solver.corridor_batch_tensors(variant, N, delta, *ins, init, seg_stride=seg_stride)
        ctx.solver, ctx.ins, ctx.variant, ctx.delta, ctx.seg_stride = solver, ins, variant, delta, seg_stride
        ctx.mark_non_differentiable(rec["seg_count"])
        return rec["seg"], rec["seg_count"], rec["ref_end"], rec["dl_bounds"]

    @staticmethod
    def backward(ctx, seg_bar, _count_bar, ref_end_bar, dl_bounds_bar):
        names = ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds_knots", "s_ref", "l_ref")
        want = tuple(n for n, need in zip(names, ctx.needs_input_grad[:6]) if need)
        if not want or (seg_bar is None and ref_end_bar is None and dl_bounds_bar is None):
            return (None,) * 10
        g = ctx.solver.corridor_batch_vjp(ctx.ins, ctx.variant, seg_bar, ref_end_bar, dl_bounds_bar, want=want, delta=ctx.delta,
                                          seg_stride=ctx.seg_stride)
        return tuple(g.get(n) for n in names) + (None, None, None, None)


def corridor(solver, s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref, *, variant=0, delta=0.1, seg_stride=16):
    """The device corridor stage as a differentiable layer (btrapz_corridor_batch_device; backward: one
    btrapz_corridor_batch_vjp_device launch).  s_bounds, l_bounds [B, O, N, 2]; ds_bounds, dl_bounds_knots [B, N, 2]; s_ref,
    l_ref [B, N].  Returns (seg [NUM_SEG_FIELDS, B, seg_stride], seg_count [B], ref_end [B, 2], dl_bounds [B, 10]) -- what
    diff.solve(...) takes, with seg_count for the ragged batch; seg_count is not differentiable.  The stage's discrete
    decisions are frozen: the gradient is that of the piecewise linear map around the inputs (include/btrapz_hip.h lists
    the rules); candidates without a corridor (seg_count 0 or -1) get zeros.  Up to 512 knots and 64 obstacles."""
    return _Corridor.apply(s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref, solver, int(variant), float(delta), int(seg_stride))


class _PrismBounds(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prisms, solver, N, O, road):
        p, = _on(solver, prisms)
        sb, lb, n = solver.prism_bounds(p, N, O, road=road)
        ctx.solver, ctx.prisms, ctx.N, ctx.O, ctx.road = solver, p, N, O, road
        ctx.shape, ctx.device_in = prisms.shape, prisms.device
        ctx.mark_non_differentiable(n)
        return sb, lb, n

    @staticmethod
    def backward(ctx, s_bar, l_bar, _n_bar):
        if not ctx.needs_input_grad[0] or (s_bar is None and l_bar is None):
            return (None,) * 5
        g = ctx.solver.prism_bounds_vjp(ctx.prisms, ctx.N, ctx.O, s_bar, l_bar, road=ctx.road)
        return (g.reshape(ctx.shape).to(ctx.device_in), None, None, None, None)


def prism_bounds(solver, prisms, N, O, road=None):
    """The prism stage as a differentiable layer (btrapz_prism_bounds_device; backward: one
    btrapz_prism_bounds_vjp_device launch).  prisms [B, P, 8]: s0, l0, t0, vel_s, vel_l, T, active, reserved.  Returns
    (s_bounds, l_bounds [B, O, N, 2], n_strips [B]) -- what diff.corridor(...) takes as its first two arguments; n_strips is
    not differentiable.  The stage's discrete decisions are frozen and the two-decimal rounding of the faces is
    differentiated as the identity (include/btrapz_hip.h lists the rules); `active` and `reserved` get 0, and so does every
    entry of a scene with more than O strips."""
    return _PrismBounds.apply(prisms, solver, int(N), int(O), road)


# ---- forward mode from the scene: prisms -> bounds -> record -> control points (include/btrapz_hip_stage_jvp.h) -----------

_KNOT_TANGENTS = ("ds_bounds", "dl_bounds_knots", "s_ref", "l_ref")
_RECORD_TANGENTS = ("init", "shared")
JVP_CHUNK = 32   # BTRAPZ_MAX_TANGENTS


def scene_jacobian(solver, prisms, prisms_dot, ds_bounds, dl_bounds_knots, s_ref, l_ref, init, params, *, O, variant=0,
                   delta=0.1, seg_stride=16, road=None, more=None):
    """Directional derivatives of the planned trajectories with respect to the scene.  One forward pipeline --
    prism_bounds -> corridor stage -> solve with its multipliers kept -- then, per chunk of at most 32 directions, one launch
    per stage on that one solve: prism_bounds_jvp -> corridor_batch_jvp -> solve_jvp.

    prisms [B, P, 8]; prisms_dot [T, B, P, 8]: T directions of the obstacle prisms (entries 6, 7 and inactive slots are not
    read; None: zero, with `more`); ds_bounds, dl_bounds_knots [B, N, 2]; s_ref, l_ref [B, N]; init [B, 6]; params [20].
    more: a dict of further tangents with the same leading axis T -- knot level "ds_bounds", "dl_bounds_knots" [T, B, N, 2],
    "s_ref", "l_ref" [T, B, N]; record level "init" [T, B, 6], "shared" [T, B, 20].
    Returns a dict: "ctrl" [B, 12 S], "cost", "status", "seg_count", "n_strips" [B], "dctrl" [T, B, 12 S], "dcost" [T, B], "rec"
    (the batch record that was solved) and "out" (the solve's result dict).  The decisions of both stages are frozen and the
    faces' rounding is straight-through; scenes without a corridor or a solution get zero tangents.
    MEMORY: a chunk holds the dense bounds tangents, 2 x 16 min(T, 32) B O N bytes, until its solve_jvp has been issued; a
    fused prisms -> record derivative would not need them."""
    _check_params(params, None)
    more = dict(more or {})
    unknown = set(more) - set(_KNOT_TANGENTS) - set(_RECORD_TANGENTS)
    if unknown:
        raise ValueError("unknown tangents: %s" % sorted(unknown))
    more = {k: v for k, v in more.items() if v is not None}
    if prisms_dot is None and not more:
        raise ValueError("no tangent given")
    p, ds, dl, sr, lr, ini = _on(solver, prisms, ds_bounds, dl_bounds_knots, s_ref, l_ref, init)
    B, N = p.shape[0], sr.shape[1]
    T = prisms_dot.shape[0] if prisms_dot is not None else next(iter(more.values())).shape[0]
    for k, v in more.items():
        if v.shape[0] != T:
            raise ValueError("tangent %r: %d directions, expected %d" % (k, v.shape[0], T))
    sb, lb, n_strips = solver.prism_bounds(p, N, O, road=road)
    staged = solver.corridor_batch_tensors(variant, N, delta, sb, lb, ds, dl, sr, lr, ini, seg_stride=seg_stride)
    rec, sets, out = _solve_kept(solver, staged["seg"], staged["init"], staged["ref_end"], staged["dl_bounds"], params,
                                 staged["seg_count"], None, variant, delta)
    knots = (sb, lb, ds, dl, sr, lr)
    dctrl, dcost = [], []
    for t0 in range(0, T, JVP_CHUNK):
        part = slice(t0, min(t0 + JVP_CHUNK, T))
        tan = {k: _on(solver, more[k][part])[0] for k in _KNOT_TANGENTS if k in more}
        if prisms_dot is not None:
            tan["s_bounds"], tan["l_bounds"] = solver.prism_bounds_jvp(p, N, O, _on(solver, prisms_dot[part])[0], road=road)
        rt = solver.corridor_batch_jvp(knots, variant, tan, delta=delta, seg_stride=seg_stride) if tan else {}
        for k in _RECORD_TANGENTS:
            if k in more:
                rt[k] = _on(solver, more[k][part])[0]
        j = solver.solve_jvp(rec, sets, out, rt)
        dctrl.append(j["ctrl"]); dcost.append(j["cost"])
    cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    return dict(ctrl=out["ctrl"], cost=out["cost"], status=out["status"], seg_count=rec.seg_count, n_strips=n_strips,
                dctrl=cat(dctrl), dcost=cat(dcost), rec=rec, out=out)


def trajectory_spread(solver, prisms, sigma, ds_bounds, dl_bounds_knots, s_ref, l_ref, init, params, *, O, variant=0,
                      delta=0.1, seg_stride=16, road=None, sel=None):
    """First-order spread of the sampled trajectories under independent uncertainties of the obstacle prisms.  sigma
    [B, P, 6]: standard deviations of s0, l0, t0, vel_s, vel_l, T of every car.  One unit direction per (car, parameter)
    column that has a non-zero sigma in any scene -> scene_jacobian -> sample_jvp; the spread of sample y is
    sqrt(sum_c (dy / dtheta_c sigma_c)^2), the columns added in ascending (car, parameter) order.  Other arguments as
    scene_jacobian; sel: the scenes to sample (int64, default every scene in order).
    Returns a dict: "traj" [nsel, 6, max_points] and "npoints" [nsel] (diff.sample's), "spread" [nsel, 6, max_points] (NaN
    for a scene that is not solved), "columns" (the list of (car, parameter) pairs) and "jac" (scene_jacobian's dict)."""
    d = solver.device
    p, sg = _on(solver, prisms, sigma)
    B, P = p.shape[0], p.shape[1]
    if tuple(sg.shape) != (B, P, 6):
        raise ValueError("sigma must be [B, P, 6] = %s, not %s" % ((B, P, 6), tuple(sg.shape)))
    columns = [(q, k) for q in range(P) for k in range(6) if bool((sg[:, q, k] != 0).any())]
    if not columns:
        raise ValueError("sigma is zero everywhere")
    pd = torch.zeros((len(columns), B, P, 8), dtype=torch.float64, device=d)
    for c, (q, k) in enumerate(columns):
        pd[c, :, q, k] = 1.0
    jac = scene_jacobian(solver, p, pd, ds_bounds, dl_bounds_knots, s_ref, l_ref, init, params, O=O, variant=variant, delta=delta,
                         seg_stride=seg_stride, road=road)
    rec = jac["rec"]
    sel = (torch.arange(B, device=d) if sel is None else sel.to(d)).to(torch.int64).contiguous()
    traj, npts = solver.sample(rec, jac["ctrl"], sel, delta)
    dy = sample_jvp(solver, jac["dctrl"], rec.seg, seg_count=rec.seg_count, sel=sel, delta=delta)
    var = torch.zeros_like(traj)
    for c, (q, k) in enumerate(columns):
        var += (dy[c, :, :, :traj.shape[2]] * sg[sel, q, k][:, None, None]) ** 2
    spread = torch.sqrt(var)
    status = jac["status"][sel]
    spread[(status != 1) & (status != 2)] = float("nan")
    return dict(traj=traj, npoints=npts, spread=spread, columns=columns, jac=jac)


# ---- Cartesian states of Frenet trajectories (include/btrapz_hip_cartesian.h) -----------------------------------------

class _Cartesian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frenet, refline, solver, layout, count, line_index):
        f, = _on(solver, frenet)
        ctx.solver, ctx.refline, ctx.layout, ctx.count, ctx.line_index, ctx.f = solver, refline, layout, count, line_index, f
        ctx.shape, ctx.device_in = frenet.shape, frenet.device
        return solver.cartesian(f, refline, layout=layout, count=count, line_index=line_index, want=("cart",))["cart"]

    @staticmethod
    def backward(ctx, cart_bar):
        if cart_bar is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        g = ctx.solver.cartesian_vjp(ctx.f, ctx.refline, cart_bar, layout=ctx.layout, count=ctx.count, line_index=ctx.line_index)
        return (g.reshape(ctx.shape).to(ctx.device_in), None, None, None, None, None)


def cartesian(frenet, refline, solver, layout=0, count=None, line_index=None):
    """Differentiable Cartesian states (btrapz_cartesian_device; backward: one btrapz_cartesian_vjp_device launch).
    frenet: [R, 6, n] -- diff.sample's traj, layout 0 (BTRAPZ_FRENET_SAMPLES) -- or [R, 2, n, 3] -- diff.eval_states' x,
    layout 1 (BTRAPZ_FRENET_STATES); refline: a layout.RefLine; count: int32 [R] (diff.sample's npoints), line_index: int32
    [R].  Returns cart [R, 6, n], rows (x, y, theta, kappa, v, a); samples outside the line and beyond a row's count are
    NaN and get a zero gradient -- reduce over the valid samples (torch.nansum, or a mask from count).  The interval of the
    lookup is frozen and the reference line is not differentiated.  Composes with diff.sample / diff.eval_states /
    diff.solve."""
    return _Cartesian.apply(frenet, refline, solver, int(layout), count, line_index)


def cartesian_jvp(solver, frenet, refline, frenet_dot, layout=0, count=None, line_index=None):
    """Tangents of the Cartesian states (btrapz_cartesian_jvp_device): frenet as diff.cartesian, frenet_dot [T] x its
    shape -- diff.sample_jvp's or diff.eval_states_jvp's result -> cart_dot [T, R, 6, n]."""
    f, fd = _on(solver, frenet, frenet_dot)
    return solver.cartesian_jvp(f, refline, fd, layout=int(layout), count=count, line_index=line_index)


def scene_jacobian_cartesian(solver, refline, prisms, prisms_dot, ds_bounds, dl_bounds_knots, s_ref, l_ref, init, params, *, O,
                             variant=0, delta=0.1, seg_stride=16, road=None, more=None, sel=None, line_index=None):
    """Directional derivatives of the planned trajectories IN THE PLANE with respect to the scene: scene_jacobian, then
    sample_jvp and cartesian_jvp on the sampled winners.  refline: a layout.RefLine; line_index: int32 [nsel]; sel: the
    scenes to sample (int64, default every scene in order); the other arguments are scene_jacobian's.  Returns its dict
    plus "traj" [nsel, 6, max_points] and "npoints" [nsel] (diff.sample's), "cart" [nsel, 6, max_points] and "dcart"
    [T, nsel, 6, max_points]; a tangent set in `more["init"]` moves sample 0 too."""
    jac = scene_jacobian(solver, prisms, prisms_dot, ds_bounds, dl_bounds_knots, s_ref, l_ref, init, params, O=O, variant=variant,
                         delta=delta, seg_stride=seg_stride, road=road, more=more)
    rec = jac["rec"]
    d = solver.device
    sel = (torch.arange(rec.B, device=d) if sel is None else sel.to(d)).to(torch.int64).contiguous()
    traj, npts = solver.sample(rec, jac["ctrl"], sel, delta)
    dinit = (more or {}).get("init")
    dtraj = sample_jvp(solver, jac["dctrl"], rec.seg, dinit=dinit, seg_count=rec.seg_count, sel=sel, delta=delta)[..., :traj.shape[2]]
    cart = solver.cartesian(traj, refline, count=npts, line_index=line_index, want=("cart",))["cart"]
    dcart = cartesian_jvp(solver, traj, refline, dtraj, count=npts, line_index=line_index)
    return dict(jac, traj=traj, npoints=npts, cart=cart, dcart=dcart)


# ---- Cartesian states projected onto the reference line (include/btrapz_hip_frenet.h) ---------------------------------

class _Frenet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cart, refline, solver, layout, order, count, line_index, s_window):
        c, = _on(solver, cart)
        o = solver.frenet(c, refline, layout=layout, order=order, count=count, line_index=line_index, s_window=s_window)
        ctx.solver, ctx.refline, ctx.layout, ctx.order, ctx.count, ctx.line_index = solver, refline, layout, order, count, line_index
        ctx.c, ctx.f, ctx.interval = c, o["frenet"], o["interval"]
        ctx.shape, ctx.device_in = cart.shape, cart.device
        ctx.mark_non_differentiable(o["interval"])
        return o["frenet"], o["interval"]

    @staticmethod
    def backward(ctx, frenet_bar, _interval_bar):
        if frenet_bar is None or not ctx.needs_input_grad[0]:
            return (None,) * 8
        g = ctx.solver.frenet_vjp(ctx.c, ctx.refline, ctx.f, ctx.interval, frenet_bar, layout=ctx.layout, order=ctx.order,
                                  count=ctx.count, line_index=ctx.line_index)
        return (g.reshape(ctx.shape).to(ctx.device_in),) + (None,) * 7


def frenet(cart, refline, solver, layout=0, order=2, count=None, line_index=None, s_window=None):
    """Differentiable projection onto the reference line (btrapz_frenet_device; backward: one btrapz_frenet_vjp_device
    launch).  cart: [R, 6, n], rows (x, y, theta, kappa, v, a) -- diff.cartesian's result, or measured poses; order 0, 1 or
    2: the rows that are read and the derivatives that are returned; s_window: [R, 2] or None.  Returns (frenet, interval):
    frenet [R, 6, n], rows (s, ds, dds, l, dl, ddl) under layout 0, or [R, 2, n, 3] under layout 1; interval [R, n] int32
    (-1: OUTSIDE), not differentiable.  OUTSIDE samples and samples beyond a row's count are NaN and get a zero gradient.
    The matched interval is frozen and the reference line is not differentiated; a query between two branches of the
    line jumps where their distances tie."""
    return _Frenet.apply(cart, refline, solver, int(layout), int(order), count, line_index, s_window)


def frenet_jvp(solver, cart, refline, frenet, interval, cart_dot, layout=0, order=2, count=None, line_index=None):
    """Tangents of the projection (btrapz_frenet_jvp_device): cart, frenet and interval as diff.frenet took and returned
    them, cart_dot [T, R, 6, n] -> frenet_dot [T] x the shape of frenet."""
    c, f, cd = _on(solver, cart, frenet, cart_dot)
    return solver.frenet_jvp(c, refline, f, interval, cd, layout=int(layout), order=int(order), count=count, line_index=line_index)


# ---- footprint clearance against moving obstacles (include/btrapz_hip_clearance.h) ------------------------------------

class _Clearance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cart, obstacles, footprint, solver, scene_index, count):
        c, = _on(solver, cart)
        o = solver.clearance(c, obstacles, footprint, scene_index=scene_index, count=count, want=("clear", "which"))
        ctx.solver, ctx.obstacles, ctx.footprint, ctx.scene_index, ctx.count = solver, obstacles, footprint, scene_index, count
        ctx.c, ctx.which = c, o["which"]
        ctx.shape, ctx.device_in = cart.shape, cart.device
        ctx.mark_non_differentiable(o["which"])
        return o["clear"], o["which"]

    @staticmethod
    def backward(ctx, clear_bar, _which_bar):
        if clear_bar is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        g = ctx.solver.clearance_vjp(ctx.c, ctx.obstacles, ctx.footprint, ctx.which, clear_bar, scene_index=ctx.scene_index,
                                     count=ctx.count)
        return (g.reshape(ctx.shape).to(ctx.device_in),) + (None,) * 5


def clearance(cart, obstacles, footprint, solver, scene_index=None, count=None):
    """Differentiable clearance of the ego's rectangle against moving obstacles (btrapz_clearance_device; backward: one
    btrapz_clearance_vjp_device launch).  cart: [R, 6, n] -- diff.cartesian's result; obstacles: a layout.Obstacles of the
    same n; footprint: (half_length, half_width, centre_offset); scene_index, count: int32 [R].  Returns (clear, which):
    clear [R, n] (NaN at invalid poses and beyond a row's count, +inf without an obstacle -- reduce over the finite ones),
    which [R, n] int32, not differentiable.  The winning obstacle and feature are frozen (a one-sided derivative at a tie)
    and the obstacles get no gradient.  Composes with diff.cartesian / diff.sample / diff.solve."""
    return _Clearance.apply(cart, obstacles, footprint, solver, scene_index, count)


def clearance_jvp(solver, cart, obstacles, footprint, which, cart_dot, obs_dot=None, scene_index=None, count=None):
    """Tangents of the clearance (btrapz_clearance_jvp_device): cart and which as diff.clearance took and returned them,
    cart_dot [T, R, 6, n] -- diff.cartesian_jvp's result -- and obs_dot [T, n_scenes, O, 3, n] or None -> clear_dot [T, R, n]."""
    c, cd = _on(solver, cart, cart_dot)
    od = _on(solver, obs_dot)[0] if obs_dot is not None else None
    return solver.clearance_jvp(c, obstacles, footprint, which, cd, obs_dot=od, scene_index=scene_index, count=count)
