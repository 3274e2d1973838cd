"""The batched solve as a differentiable layer: spectral_amd.diff.solve(...) returns (ctrl, cost, status) with a
torch.autograd graph whose backward is one btrapz_solve_vjp_device launch (include/btrapz_hip.h).  The gradient math
is HIP; torch only sums the per-candidate parameter gradients of a set."""
import types

import torch

from . import layout as L

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


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, init, ref_end, dl_bounds, params, solver, seg_count, set_index, variant, delta):
        d = solver.device
        seg, init, ref_end, dl_bounds = (_f64(t.detach()).to(d) for t in (seg, init, ref_end, dl_bounds))
        B, S = seg.shape[1], seg.shape[2]
        prm = params.detach().to("cpu", torch.float64)
        rows = prm.reshape(-1, N_PARAMS).tolist()
        sets = [shared_from_params(r, variant, delta) for r in rows]
        o = dict(ctrl=torch.zeros((B, 12 * S), dtype=torch.float64, device=d),
                 cost=torch.empty(B, dtype=torch.float64, device=d),
                 status=torch.empty(B, dtype=torch.int32, device=d), iters=torch.empty(B, dtype=torch.int32, device=d))
        if set_index is not None:
            if seg_count is None:
                rec = types.SimpleNamespace(B=B, S=S, seg=seg, init=init, ref_end=ref_end, dl_bounds=dl_bounds)
                o = solver.solve_sets(rec, sets, set_index, keep_multipliers=True, out=o)
            else:
                rec = dict(B=B, seg_stride=S, seg=seg, seg_count=seg_count, init=init, ref_end=ref_end, dl_bounds=dl_bounds)
                o = solver._sets_call(B, S, sets, set_index, rec, seg_count, o, None, True, {})
        else:
            o["lam"] = torch.empty((2, 36, B, S), dtype=torch.float64, device=d)
            stream = torch.cuda.current_stream(d).cuda_stream
            solver.ctx.solve_warm_device(B, S, sets[0], seg, seg_count, init, ref_end, dl_bounds, o["ctrl"], o["cost"],
                                         o["status"], o["iters"], lam_out=o["lam"], stream=stream)
        ctx.solver, ctx.sets, ctx.set_index, ctx.seg_count = solver, sets, set_index, seg_count
        ctx.params_shape, ctx.params_device = params.shape, params.device
        ctx.inputs = (seg, init, ref_end, dl_bounds)
        ctx.out = o
        ctx.mark_non_differentiable(o["status"])
        return o["ctrl"], o["cost"], o["status"]

    @staticmethod
    def backward(ctx, ctrl_bar, cost_bar, _status_bar):
        seg, init, ref_end, dl_bounds = ctx.inputs
        B, S = seg.shape[1], seg.shape[2]
        if ctrl_bar is None and cost_bar is None:
            return (None,) * 10
        if ctx.seg_count is None:
            rec = types.SimpleNamespace(B=B, S=S, seg=seg, init=init, ref_end=ref_end, dl_bounds=dl_bounds)
        else:
            rec = dict(B=B, seg_stride=S, seg=seg, seg_count=ctx.seg_count, init=init, ref_end=ref_end, dl_bounds=dl_bounds)
        g = ctx.solver.solve_vjp(rec, ctx.sets, ctx.out, ctrl_bar, cost_bar, set_index=ctx.set_index)
        need = ctx.needs_input_grad
        gp = None
        if need[4]:
            if ctx.set_index is None:
                gp = g["shared"].sum(0)
            else:
                n_sets = len(ctx.sets)
                idx = ctx.set_index.long().clamp(0, n_sets - 1)   # (unsolved candidates carry zero rows)
                gp = torch.zeros((n_sets, N_PARAMS), dtype=torch.float64, device=g["shared"].device)
                gp.index_add_(0, idx, g["shared"])
            gp = gp.reshape(ctx.params_shape).to(ctx.params_device)
        return (g["seg"] if need[0] else None, g["init"] if need[1] else None, g["ref_end"] if need[2] else None,
                g["dl_bounds"] if need[3] else None, gp, None, None, None, None, None)


def solve(solver, seg, init, ref_end, dl_bounds, params, *, seg_count=None, set_index=None, variant=0, delta=0.1):
    """Differentiable batched solve.  seg [NUM_SEG_FIELDS, B, S], init [B, 6], ref_end [B, 2], dl_bounds [B, 10]: the
    batch (device tensors, float64); params: [20] (one set) or [n_sets, 20] with set_index (int32 [B]) -- the parameter
    rows of shared_from_params.  seg_count: int32 [B] for a ragged batch.  Returns (ctrl [B, 12 S], cost [B], status [B]);
    status is not differentiable.  The solve runs with its multipliers kept and no rescue pass (elastic = 0); gradients
    are defined for candidates of status 1 or 2 and are 0 elsewhere (btrapz_solve_vjp_device).  Field 0 of seg (the
    segment durations) gets no gradient."""
    if set_index is None and params.dim() != 1:
        raise ValueError("params must be [20] without set_index, [n_sets, 20] with it")
    if params.shape[-1] != N_PARAMS:
        raise ValueError("params rows have %d entries (layout.Shared.as_array() without delta)" % N_PARAMS)
    return _Solve.apply(seg, init, ref_end, dl_bounds, params, solver, seg_count, set_index, variant, delta)
