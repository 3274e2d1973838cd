"""Device-resident batch solver: torch supplies HBM buffers and streams, the HIP library
(libbtrapz_hip.so) does all the work.  No torch ops on the data path."""
import numpy as np
import torch

from . import layout as L
from .native import Context


class DeviceBatch:
    """A candidate batch resident in HBM (field-major SoA, see layout.py)."""

    def __init__(self, batch, device):
        self.B, self.S = batch.B, batch.S
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.seg, self.init, self.ref_end, self.dl_bounds = f(batch.seg), f(batch.init), f(batch.ref_end), f(batch.dl_bounds)


class BatchSolver:
    """Solves DeviceBatches on one GPU; outputs stay on the device."""

    def __init__(self, device_index=0):
        if not torch.cuda.is_available():
            raise RuntimeError("spectral_amd.BatchSolver needs a HIP device (no CPU path)")
        self.device = torch.device("cuda", device_index)
        self.ctx = Context(device_index)
        self._out = {}

    def upload(self, batch):
        return DeviceBatch(batch, self.device)

    def _buffers(self, B, S):
        key = (B, S)
        if key not in self._out:
            d = self.device
            self._out[key] = dict(ctrl=torch.empty((B, 12 * S), dtype=torch.float64, device=d),
                                  cost=torch.empty(B, dtype=torch.float64, device=d),
                                  status=torch.empty(B, dtype=torch.int32, device=d),
                                  iters=torch.empty(B, dtype=torch.int32, device=d))
        return self._out[key]

    def solve(self, dbatch, shared, max_iter=0, eps=0.0, out=None, warm=None, keep_multipliers=False, elastic=0,
              elastic_tol=0.0, queue=0, split=0, start=0, cap_iter=0, lean=0, compact=0):
        """Launches the solve on torch's current stream; returns dict of device tensors.

        warm: dict with optional "x0" ([B,2,S,3] joint states, e.g. from eval_states) and "lam" ([2,36,B,S]
        multipliers kept by an earlier solve) plus optional "mu0", "smin" and "hint" ([B] int32 expected difficulty,
        e.g. the previous step's iters: scheduling only) -- btrapz_warm.  keep_multipliers
        adds this solve's multipliers to the result as "lam".  elastic: btrapz_options.elastic (0 off, 1 rescue pass
        over stalled candidates, 2 elastic rows for every candidate).  split: btrapz_options.split (0 automatic: the
        one-candidate-per-wavefront form for batches that leave SIMDs idle; 1 always where it applies; -1 never).  lean:
        btrapz_options.lean (the two-wavefronts-per-SIMD form of cold solves: 0 automatic, 1 where it applies, -1 never)."""
        o = out if out is not None else self._buffers(dbatch.B, dbatch.S)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if warm is None and not keep_multipliers:
            self.ctx.solve_device(dbatch.B, dbatch.S, shared, dbatch.seg, dbatch.init, dbatch.ref_end,
                                  dbatch.dl_bounds, o["ctrl"], o["cost"], o["status"], o["iters"], stream=stream,
                                  max_iter=max_iter, eps=eps, elastic=elastic, elastic_tol=elastic_tol, queue=queue,
                                  split=split, start=start, cap_iter=cap_iter, lean=lean, compact=compact)
            return o
        warm = warm or {}
        x0, lam0, hint = warm.get("x0"), warm.get("lam"), warm.get("hint")
        if hint is not None:
            assert hint.dtype == torch.int32 and hint.is_contiguous() and hint.numel() == dbatch.B
        if x0 is not None:
            assert x0.dtype == torch.float64 and x0.is_contiguous() and tuple(x0.shape) == (dbatch.B, 2, dbatch.S, 3)
        if lam0 is not None:
            assert lam0.dtype == torch.float64 and lam0.is_contiguous() and tuple(lam0.shape) == (2, 36, dbatch.B, dbatch.S)
        lam_out = None
        if keep_multipliers:
            # in place when a previous solve's array is passed in (allowed: include/btrapz_hip.h, btrapz_warm)
            lam_out = lam0 if lam0 is not None else torch.empty((2, 36, dbatch.B, dbatch.S), dtype=torch.float64,
                                                                device=self.device)
            o = dict(o); o["lam"] = lam_out
        self.ctx.solve_warm_device(dbatch.B, dbatch.S, shared, dbatch.seg, None, dbatch.init, dbatch.ref_end,
                                   dbatch.dl_bounds, o["ctrl"], o["cost"], o["status"], o["iters"], x0=x0, lam0=lam0,
                                   lam_out=lam_out, mu0=warm.get("mu0", 0.0), smin=warm.get("smin", 0.0),
                                   stream=stream, max_iter=max_iter, eps=eps, hint=hint, elastic=elastic,
                                   elastic_tol=elastic_tol, lean=lean)
        return o

    def prepare(self, dbatch, shared, out=None, **options):
        """solve(dbatch, shared, **options) prepared once: returns (call, out) where call() launches the solve on the
        stream that is current NOW and `out` is the dict of device tensors it fills (cold solves only)."""
        o = out if out is not None else self._buffers(dbatch.B, dbatch.S)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        call = self.ctx.prepared_solve(dbatch.B, dbatch.S, shared, dbatch.seg, dbatch.init, dbatch.ref_end, dbatch.dl_bounds,
                                       o["ctrl"], o["cost"], o["status"], o["iters"], stream=stream, **options)
        return call, o

    def eval_states(self, dbatch, ctrl, times):
        """(p, v, a) of every candidate's solved trajectory at times[b][j] (seconds from the start of its
        horizon) -> [B, 2, n_times, 3]; the x0 of a warm start."""
        times = times.to(self.device, dtype=torch.float64).contiguous()
        n = times.shape[1]
        x = torch.empty((dbatch.B, 2, n, 3), dtype=torch.float64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx.eval_states_device(dbatch.B, dbatch.S, None, dbatch.seg, ctrl, n, times, x, stream=stream)
        return x

    def corridor_batch(self, kb, variant, seg_stride=16):
        """Device corridor stage on a spectral_amd.knots.KnotBatch -> dict of device tensors forming a ragged
        batch record (seg, seg_count, init, ref_end, dl_bounds)."""
        d = self.device
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(d)
        B = kb.B
        rec = dict(B=B, seg_stride=seg_stride,
                   seg=torch.zeros((L.NUM_SEG_FIELDS, B, seg_stride), dtype=torch.float64, device=d),
                   seg_count=torch.zeros(B, dtype=torch.int32, device=d), init=f(kb.init),
                   ref_end=torch.zeros((B, 2), dtype=torch.float64, device=d),
                   dl_bounds=torch.zeros((B, 10), dtype=torch.float64, device=d))
        ins = [f(kb.s_bounds), f(kb.l_bounds), f(kb.ds_bounds), f(kb.dl_bounds), f(kb.s_ref), f(kb.l_ref)]
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.corridor_batch_device(variant, B, kb.N, kb.num_obs, kb.delta, *ins, seg_stride, rec["seg"],
                                       rec["seg_count"], rec["ref_end"], rec["dl_bounds"], stream=stream)
        rec["_inputs"] = ins  # keep the knot arrays alive until the launch has run
        return rec

    def corridor_batch_vjp(self, kb_or_tensors, variant, seg_bar, ref_end_bar=None, dl_bounds_bar=None,
                           want=("s_bounds", "l_bounds", "ds_bounds", "dl_bounds_knots", "s_ref", "l_ref"), delta=None,
                           seg_stride=None):
        """Gradients of the device corridor stage w.r.t. its per-knot inputs (btrapz_corridor_batch_vjp_device).
        kb_or_tensors: a spectral_amd.knots.KnotBatch, or the six arrays (s_bounds, l_bounds [B, O, N, 2]; ds_bounds,
        dl_bounds_knots [B, N, 2]; s_ref, l_ref [B, N]) as tensors with `delta` given.  seg_bar [NUM_SEG_FIELDS, B,
        seg_stride], ref_end_bar [B, 2], dl_bounds_bar [B, 10]: cotangents of the stage's outputs (any may be None, not
        all).  seg_stride: the forward call's (a corridor of more segments has seg_count -1 there and zeros here); it may be
        left out with a seg_bar, whose last extent it is, and is required without one.  Returns a dict of the arrays named
        in `want`, shaped like the inputs."""
        d = self.device
        if hasattr(kb_or_tensors, "s_bounds"):
            kb = kb_or_tensors
            f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(d)
            ins = [f(kb.s_bounds), f(kb.l_bounds), f(kb.ds_bounds), f(kb.dl_bounds), f(kb.s_ref), f(kb.l_ref)]
            delta = kb.delta if delta is None else delta
        else:
            ins = [t.detach().to(d, dtype=torch.float64).contiguous() for t in kb_or_tensors]
            if delta is None:
                raise ValueError("delta is needed with tensors")
        B, O, N = ins[0].shape[0], ins[0].shape[1], ins[0].shape[2]
        c = lambda t: None if t is None else t.detach().to(d, dtype=torch.float64).contiguous()
        seg_bar, ref_end_bar, dl_bounds_bar = c(seg_bar), c(ref_end_bar), c(dl_bounds_bar)
        if seg_bar is None and seg_stride is None:
            raise ValueError("seg_stride is needed without a seg_bar")
        if seg_bar is not None and seg_stride is not None and int(seg_stride) != seg_bar.shape[2]:
            raise ValueError("seg_stride %d is not seg_bar's, %d" % (seg_stride, seg_bar.shape[2]))
        seg_stride = seg_bar.shape[2] if seg_bar is not None else int(seg_stride)
        like = dict(s_bounds=ins[0], l_bounds=ins[1], ds_bounds=ins[2], dl_bounds_knots=ins[3], s_ref=ins[4], l_ref=ins[5])
        grads = {k: torch.empty_like(like[k]) for k in want}
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.corridor_batch_vjp_device(variant, B, N, O, delta, *ins, seg_stride, seg_bar, ref_end_bar, dl_bounds_bar,
                                           grads, stream=stream)
        grads["_inputs"] = (ins, seg_bar, ref_end_bar, dl_bounds_bar)   # alive until the launch has run
        return grads

    def prism_bounds(self, prisms, N, O, road=None):
        """Obstacle prisms [B, P, 8] (s0, l0, t0, vel_s, vel_l, T, active, -) -> per-knot bounds of the lateral strips
        (btrapz_prism_bounds_device): s_bounds, l_bounds [B, O, N, 2] and n_strips [B], on the device."""
        from .native import CRoad
        d = self.device
        prisms = prisms.to(d, dtype=torch.float64).contiguous()
        B, P = prisms.shape[0], prisms.shape[1]
        sb = torch.empty((B, O, N, 2), dtype=torch.float64, device=d); lb = torch.empty_like(sb)
        n = torch.empty(B, dtype=torch.int32, device=d)
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.prism_bounds_device(B, P, N, road or CRoad.reference(), prisms, O, sb, lb, n, stream=stream)
        return sb, lb, n

    def prism_bounds_vjp(self, prisms, N, O, s_bounds_bar, l_bounds_bar, road=None):
        """Gradients of prism_bounds w.r.t. the prisms (btrapz_prism_bounds_vjp_device, one launch): cotangents
        s_bounds_bar, l_bounds_bar [B, O, N, 2] (either may be None, not both) -> prisms_bar [B, P, 8]: s0, l0, t0, vel_s,
        vel_l, T, then two zeros.  The stage's decisions are frozen and the two-decimal rounding of the faces counts as the
        identity (include/btrapz_hip.h lists the rules); a scene with more than O strips gets zeros."""
        from .native import CRoad
        d = self.device
        prisms = prisms.detach().to(d, dtype=torch.float64).contiguous()
        B, P = prisms.shape[0], prisms.shape[1]
        c = lambda t: None if t is None else t.detach().to(d, dtype=torch.float64).contiguous()
        sbar, lbar = c(s_bounds_bar), c(l_bounds_bar)
        for t in (sbar, lbar):
            if t is not None and tuple(t.shape) != (B, int(O), int(N), 2):
                raise ValueError("a cotangent must be [B, O, N, 2] = %s, not %s" % ((B, O, N, 2), tuple(t.shape)))
        out = torch.empty((B, P, 8), dtype=torch.float64, device=d)
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.prism_bounds_vjp_device(B, P, N, road or CRoad.reference(), prisms, O, sbar, lbar, out, stream=stream)
        return out

    def corridor_batch_tensors(self, variant, N, delta, s_bounds, l_bounds, ds_bounds, dl_bounds, s_ref, l_ref, init,
                               seg_stride=16):
        """corridor_batch on device tensors (e.g. the output of prism_bounds): s_bounds, l_bounds [B, O, N, 2],
        ds_bounds, dl_bounds [B, N, 2], s_ref, l_ref [B, N], init [B, 6]."""
        d = self.device
        B, O = s_bounds.shape[0], s_bounds.shape[1]
        c = lambda t: t.to(d, dtype=torch.float64).contiguous()
        ins = [c(s_bounds), c(l_bounds), c(ds_bounds), c(dl_bounds), c(s_ref), c(l_ref)]
        rec = dict(B=B, seg_stride=seg_stride,
                   seg=torch.zeros((L.NUM_SEG_FIELDS, B, seg_stride), dtype=torch.float64, device=d),
                   seg_count=torch.zeros(B, dtype=torch.int32, device=d), init=c(init),
                   ref_end=torch.zeros((B, 2), dtype=torch.float64, device=d),
                   dl_bounds=torch.zeros((B, 10), dtype=torch.float64, device=d))
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.corridor_batch_device(variant, B, N, O, delta, *ins, seg_stride, rec["seg"], rec["seg_count"],
                                       rec["ref_end"], rec["dl_bounds"], stream=stream)
        rec["_inputs"] = ins
        return rec

    def prism_corridor_batch(self, variant, prisms, N, O, delta, ds_bounds, dl_bounds, s_ref, l_ref, init, seg_stride=16,
                             road=None):
        """prism_bounds + corridor_batch_tensors in one launch (btrapz_prism_corridor_batch_device): the strips are
        evaluated inside the corridor kernel instead of written to memory.  Same record, plus rec["n_strips"]."""
        from .native import CRoad
        d = self.device
        c = lambda t: t.to(d, dtype=torch.float64).contiguous()
        prisms = c(prisms)
        B, P = prisms.shape[0], prisms.shape[1]
        ins = [prisms, c(ds_bounds), c(dl_bounds), c(s_ref), c(l_ref)]
        rec = dict(B=B, seg_stride=seg_stride,
                   seg=torch.zeros((L.NUM_SEG_FIELDS, B, seg_stride), dtype=torch.float64, device=d),
                   seg_count=torch.zeros(B, dtype=torch.int32, device=d), init=c(init),
                   ref_end=torch.zeros((B, 2), dtype=torch.float64, device=d),
                   dl_bounds=torch.zeros((B, 10), dtype=torch.float64, device=d),
                   n_strips=torch.empty(B, dtype=torch.int32, device=d))
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.prism_corridor_batch_device(variant, B, P, N, road or CRoad.reference(), prisms, O, delta, *ins[1:],
                                             seg_stride, rec["seg"], rec["seg_count"], rec["ref_end"], rec["dl_bounds"],
                                             rec["n_strips"], stream=stream)
        rec["_inputs"] = ins
        return rec

    def solve_ragged(self, rec, shared, max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, cap_iter=0, lean=0, compact=0):
        """Solve a ragged batch record (from corridor_batch); outputs stay on the device.  cap_iter:
        btrapz_options.cap_iter (0 automatic, -1 one launch, n two launches with hand-over after n iterations)."""
        d = self.device
        B, st = rec["B"], rec["seg_stride"]
        o = dict(ctrl=torch.zeros((B, 12 * st), dtype=torch.float64, device=d),
                 cost=torch.empty(B, dtype=torch.float64, device=d),
                 status=torch.empty(B, dtype=torch.int32, device=d), iters=torch.empty(B, dtype=torch.int32, device=d))
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.solve_ragged_device(B, st, shared, rec["seg"], rec["seg_count"], rec["init"], rec["ref_end"],
                                     rec["dl_bounds"], o["ctrl"], o["cost"], o["status"], o["iters"], stream=stream,
                                     max_iter=max_iter, eps=eps, elastic=elastic, elastic_tol=elastic_tol, cap_iter=cap_iter, lean=lean, compact=compact)
        return o

    def _sets_call(self, B, S, sets, set_index, rec, seg_count, o, warm, keep_multipliers, options):
        assert set_index.dtype == torch.int32 and set_index.is_contiguous() and set_index.numel() == B
        warm = warm or {}
        x0, lam0 = warm.get("x0"), warm.get("lam")
        if x0 is not None:
            assert x0.dtype == torch.float64 and x0.is_contiguous() and tuple(x0.shape) == (B, 2, S, 3)
        if lam0 is not None:
            assert lam0.dtype == torch.float64 and lam0.is_contiguous() and tuple(lam0.shape) == (2, 36, B, S)
        lam_out = None
        if keep_multipliers:
            lam_out = lam0 if lam0 is not None else torch.empty((2, 36, B, S), dtype=torch.float64, device=self.device)
            o = dict(o); o["lam"] = lam_out
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx.solve_sets_device(B, S, sets, set_index, rec.seg if seg_count is None else rec["seg"], seg_count,
                                   rec.init if seg_count is None else rec["init"],
                                   rec.ref_end if seg_count is None else rec["ref_end"],
                                   rec.dl_bounds if seg_count is None else rec["dl_bounds"], o["ctrl"], o["cost"],
                                   o["status"], o["iters"], x0=x0, lam0=lam0, lam_out=lam_out, mu0=warm.get("mu0", 0.0),
                                   smin=warm.get("smin", 0.0), hint=warm.get("hint"), stream=stream, **options)
        return o

    def solve_sets(self, dbatch, sets, set_index, warm=None, keep_multipliers=False, out=None, **options):
        """A parameter set per candidate (btrapz_solve_sets_device): sets is a list of layout.Shared, set_index an int32
        device tensor [B] naming each candidate's set (outside [0, len(sets)): not solved, status NO_CORRIDOR, cost
        +inf).  warm / keep_multipliers as in solve(); options: max_iter, eps, lean (0 / 1 / -1), cap_iter and compact
        (0 or -1: the sets path runs one launch without the pre-pass).  Returns the dict of device tensors."""
        o = out if out is not None else self._buffers(dbatch.B, dbatch.S)
        return self._sets_call(dbatch.B, dbatch.S, sets, set_index, dbatch, None, o, warm, keep_multipliers, options)

    def solve_sets_ragged(self, rec, sets, set_index, warm=None, keep_multipliers=False, **options):
        """solve_sets for a ragged batch record (from corridor_batch): candidates of up to 64 segments."""
        d = self.device
        B, st = rec["B"], rec["seg_stride"]
        o = dict(ctrl=torch.zeros((B, 12 * st), dtype=torch.float64, device=d),
                 cost=torch.empty(B, dtype=torch.float64, device=d),
                 status=torch.empty(B, dtype=torch.int32, device=d), iters=torch.empty(B, dtype=torch.int32, device=d))
        return self._sets_call(B, st, sets, set_index, rec, rec["seg_count"], o, warm, keep_multipliers, options)

    def solve_vjp(self, dbatch_or_rec, shared_or_sets, out, ctrl_bar, cost_bar, set_index=None):
        """Gradients of a solve (btrapz_solve_vjp_device).  dbatch_or_rec: the DeviceBatch or ragged record that was solved;
        shared_or_sets: its layout.Shared, or the list of sets with set_index (int32 device tensor [B]); out: the solve's
        result dict, from a solve with keep_multipliers=True and elastic=0 (needs "ctrl", "lam", "status"); ctrl_bar
        [B, 12 S] / cost_bar [B]: cotangents (either may be None).  Returns a dict of device tensors: "seg"
        [NUM_SEG_FIELDS, B, S] (field 0 is 0), "init" [B, 6], "ref_end" [B, 2], "dl_bounds" [B, 10], "shared" [B, 20] per
        candidate (layout.Shared.as_array order, without delta)."""
        if isinstance(dbatch_or_rec, dict):
            B, S, seg_count = dbatch_or_rec["B"], dbatch_or_rec["seg_stride"], dbatch_or_rec["seg_count"]
            seg, init, ref_end, dl = (dbatch_or_rec[k] for k in ("seg", "init", "ref_end", "dl_bounds"))
        else:
            B, S, seg_count = dbatch_or_rec.B, dbatch_or_rec.S, None
            seg, init, ref_end, dl = dbatch_or_rec.seg, dbatch_or_rec.init, dbatch_or_rec.ref_end, dbatch_or_rec.dl_bounds
        sets = list(shared_or_sets) if isinstance(shared_or_sets, (list, tuple)) else [shared_or_sets]
        if set_index is not None:
            assert set_index.dtype == torch.int32 and set_index.is_contiguous() and set_index.numel() == B
        if out.get("lam") is None:
            raise ValueError("solve_vjp needs the solve's multipliers: solve with keep_multipliers=True")
        chk = lambda t, shape: None if t is None else (t if (t.dtype == torch.float64 and t.is_contiguous() and
                                                            tuple(t.shape) == shape) else
                                                       t.to(self.device, dtype=torch.float64).reshape(shape).contiguous())
        ctrl_bar = chk(ctrl_bar, (B, 12 * S)); cost_bar = chk(cost_bar, (B,))
        d = self.device
        g = dict(seg=torch.empty((L.NUM_SEG_FIELDS, B, S), dtype=torch.float64, device=d),
                 init=torch.empty((B, 6), dtype=torch.float64, device=d),
                 ref_end=torch.empty((B, 2), dtype=torch.float64, device=d),
                 dl_bounds=torch.empty((B, 10), dtype=torch.float64, device=d),
                 shared=torch.empty((B, 20), dtype=torch.float64, device=d))
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.solve_vjp_device(B, S, sets, set_index, seg, seg_count, init, ref_end, dl, out["ctrl"], out["lam"],
                                  out["status"], ctrl_bar, cost_bar, g_seg=g["seg"], g_init=g["init"],
                                  g_ref_end=g["ref_end"], g_dl_bounds=g["dl_bounds"], g_shared=g["shared"], stream=stream)
        return g

    def solve_jvp(self, dbatch_or_rec, shared_or_sets, out, tangents, set_index=None):
        """Directional derivatives of a solve (btrapz_solve_jvp_device): T input directions per candidate, one launch, one
        factorisation per axis problem.  dbatch_or_rec, shared_or_sets, out, set_index: as in solve_vjp.  tangents: a dict
        with any of "seg" [T, NUM_SEG_FIELDS, B, S] (field 0 is ignored), "init" [T, B, 6], "ref_end" [T, B, 2],
        "dl_bounds" [T, B, 10], "shared" [T, B, 20] (per candidate, layout.Shared.as_array order without delta); a missing
        one is zero.  Returns {"ctrl": [T, B, 12 S], "cost": [T, B]}, device tensors."""
        if isinstance(dbatch_or_rec, dict):
            B, S, seg_count = dbatch_or_rec["B"], dbatch_or_rec["seg_stride"], dbatch_or_rec["seg_count"]
            seg, init, ref_end, dl = (dbatch_or_rec[k] for k in ("seg", "init", "ref_end", "dl_bounds"))
        else:
            B, S, seg_count = dbatch_or_rec.B, dbatch_or_rec.S, None
            seg, init, ref_end, dl = dbatch_or_rec.seg, dbatch_or_rec.init, dbatch_or_rec.ref_end, dbatch_or_rec.dl_bounds
        sets = list(shared_or_sets) if isinstance(shared_or_sets, (list, tuple)) else [shared_or_sets]
        if set_index is not None:
            assert set_index.dtype == torch.int32 and set_index.is_contiguous() and set_index.numel() == B
        if out.get("lam") is None:
            raise ValueError("solve_jvp needs the solve's multipliers: solve with keep_multipliers=True")
        unknown = set(tangents) - {"seg", "init", "ref_end", "dl_bounds", "shared"}
        if unknown:
            raise ValueError("unknown tangents: %s" % sorted(unknown))
        given = {k: v for k, v in tangents.items() if v is not None}
        T = next(iter(given.values())).shape[0] if given else 0
        d = self.device
        shapes = dict(seg=(T, L.NUM_SEG_FIELDS, B, S), init=(T, B, 6), ref_end=(T, B, 2), dl_bounds=(T, B, 10), shared=(T, B, 20))
        tan = {}
        for k, v in given.items():
            if tuple(v.shape) != shapes[k]:
                raise ValueError("tangent %r: shape %s, expected %s" % (k, tuple(v.shape), shapes[k]))
            tan[k] = v.to(d, dtype=torch.float64).contiguous()
        o = dict(ctrl=torch.empty((max(T, 0), B, 12 * S), dtype=torch.float64, device=d),
                 cost=torch.empty((max(T, 0), B), dtype=torch.float64, device=d))
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.solve_jvp_device(B, S, sets, set_index, seg, seg_count, init, ref_end, dl, out["ctrl"], out["lam"],
                                  out["status"], T, seg_dot=tan.get("seg"), init_dot=tan.get("init"),
                                  ref_end_dot=tan.get("ref_end"), dl_bounds_dot=tan.get("dl_bounds"),
                                  shared_dot=tan.get("shared"), ctrl_dot=o["ctrl"], cost_dot=o["cost"], stream=stream)
        return o

    def _cost_args(self, rec, shared_or_sets, ctrl, s_ref, l_ref, status, set_index):
        if isinstance(rec, dict):
            B, S, seg_count, seg, init = rec["B"], rec["seg_stride"], rec["seg_count"], rec["seg"], rec["init"]
        else:
            B, S, seg_count, seg, init = rec.B, rec.S, None, rec.seg, rec.init
        sets = list(shared_or_sets) if isinstance(shared_or_sets, (list, tuple)) else [shared_or_sets]
        d = self.device
        f = lambda t: t.to(d, dtype=torch.float64).contiguous()
        t = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        s_ref, l_ref = f(t(s_ref)), f(t(l_ref))
        if s_ref.shape != l_ref.shape or s_ref.dim() not in (1, 2) or (s_ref.dim() == 2 and s_ref.shape[0] != B):
            raise ValueError("s_ref / l_ref: [N] (one line for every candidate) or [B, N]")
        N = s_ref.shape[-1]
        if set_index is not None:
            assert set_index.dtype == torch.int32 and set_index.is_contiguous() and set_index.numel() == B
        if status is not None:
            assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == B
        ctrl = f(ctrl)
        assert tuple(ctrl.shape) == (B, 12 * S), ctrl.shape
        return dict(B=B, seg_stride=S, sets=sets, set_index=set_index, seg=seg, seg_count=seg_count, init=init, ctrl=ctrl,
                    status=status, N=N, s_ref=s_ref, l_ref=l_ref, ref_stride=N if s_ref.dim() == 2 else 0)

    def traj_cost(self, rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, status=None, set_index=None):
        """a_cost -- the score find_traj returns -- of every candidate's sampled trajectory (btrapz_traj_cost_device).
        rec_or_dbatch: a DeviceBatch or a ragged record; shared_or_sets: the scoring layout.Shared, or a list of sets with
        set_index (int32 device tensor [B]); ctrl [B, 12 S]; s_ref / l_ref: [B, N] or [N] (one line for all); status
        (int32 [B], e.g. the solve's): candidates outside {1, 2} are not scored.  Returns (a_cost [B], n_points [B]) device
        tensors; a candidate that is not scored has +inf and 0."""
        a = self._cost_args(rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, status, set_index)
        cost = torch.empty(a["B"], dtype=torch.float64, device=self.device)
        npts = torch.empty(a["B"], dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx.traj_cost_device(**a, a_cost=cost, n_points=npts, stream=stream)
        return cost, npts

    def traj_cost_vjp(self, rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, a_cost_bar, status=None, set_index=None):
        """Gradients of traj_cost (btrapz_traj_cost_vjp_device) for the cotangent a_cost_bar [B].  Returns a dict of device
        tensors: "ctrl" [B, 12 S], "init" [B, 6], "params" [B, 20] per candidate (layout.Shared.as_array order, without
        delta), "s_ref" / "l_ref" [B, N] per candidate (also for a shared line: sum the rows)."""
        a = self._cost_args(rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, status, set_index)
        B, S, N, d = a["B"], a["seg_stride"], a["N"], self.device
        abar = torch.as_tensor(a_cost_bar).to(d, dtype=torch.float64).reshape(B).contiguous()
        g = dict(ctrl=torch.empty((B, 12 * S), dtype=torch.float64, device=d),
                 init=torch.empty((B, 6), dtype=torch.float64, device=d),
                 params=torch.empty((B, 20), dtype=torch.float64, device=d),
                 s_ref=torch.empty((B, N), dtype=torch.float64, device=d),
                 l_ref=torch.empty((B, N), dtype=torch.float64, device=d))
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.traj_cost_vjp_device(**a, a_cost_bar=abar, ctrl_bar=g["ctrl"], init_bar=g["init"], params_bar=g["params"],
                                      s_ref_bar=g["s_ref"], l_ref_bar=g["l_ref"], stream=stream)
        return g

    def argmin(self, cost, group=None, index_base=0):
        """Arg-min of cost over contiguous groups (default: the whole batch). Device tensors."""
        B = cost.numel()
        group = B if group is None else group
        best_idx = torch.empty(B // group, dtype=torch.int64, device=self.device)
        best_cost = torch.empty(B // group, dtype=torch.float64, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx.argmin_device(B, group, index_base, cost, best_idx, best_cost, stream=stream)
        return best_idx, best_cost

    def sample(self, dbatch, ctrl, sel, delta):
        """Bernstein sampling (solve_3d.cc:1279-1392) of the selected candidates."""
        sel = sel.to(self.device, dtype=torch.int64).contiguous()
        t = dbatch.seg[L.F_T]
        max_points = int(torch.floor(t / delta + 1e-9).sum(1).max().item()) + 2
        out = torch.zeros((sel.numel(), 6, max_points), dtype=torch.float64, device=self.device)
        npts = torch.zeros(sel.numel(), dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.ctx.sample_device(dbatch.B, dbatch.S, delta, dbatch.seg, dbatch.init, ctrl, sel, max_points, out, npts,
                               stream=stream)
        return out, npts

    def _layout_of(self, rec_or_dbatch):
        if isinstance(rec_or_dbatch, dict):
            return rec_or_dbatch["B"], rec_or_dbatch["seg_stride"], rec_or_dbatch.get("seg_count"), rec_or_dbatch["seg"]
        return rec_or_dbatch.B, rec_or_dbatch.S, None, rec_or_dbatch.seg

    def sample_vjp(self, rec_or_dbatch, sel, delta, out_bar, want_ctrl=True, want_init=True):
        """Vector-Jacobian product of sample (btrapz_sample_vjp_device).  rec_or_dbatch: the DeviceBatch or ragged record
        that was sampled; sel: the selection of the forward; out_bar [nsel, 6, max_points]: the cotangent of the samples
        (max_points is read off its shape).  Returns a dict of device tensors with ONE ROW PER SELECTION -- "ctrl"
        [nsel, 12 S] and "init" [nsel, 6]; a candidate that sel names twice has two rows, which the caller sums."""
        B, S, seg_count, seg = self._layout_of(rec_or_dbatch)
        d = self.device
        sel = sel.to(d, dtype=torch.int64).contiguous()
        out_bar = out_bar.to(d, dtype=torch.float64).contiguous()
        n = sel.numel()
        if out_bar.dim() != 3 or out_bar.shape[0] != n or out_bar.shape[1] != 6:
            raise ValueError("out_bar: [nsel, 6, max_points]")
        g = dict(ctrl=torch.empty((n, 12 * S), dtype=torch.float64, device=d) if want_ctrl else None,
                 init=torch.empty((n, 6), dtype=torch.float64, device=d) if want_init else None)
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.sample_vjp_device(B, S, seg_count, delta, seg, sel, out_bar.shape[2], out_bar, ctrl_bar=g["ctrl"],
                                   init_bar=g["init"], stream=stream)
        return g

    def eval_states_vjp(self, rec_or_dbatch, ctrl, times, x_bar, want_ctrl=True, want_times=True):
        """Vector-Jacobian product of eval_states (btrapz_eval_states_vjp_device).  rec_or_dbatch: a DeviceBatch or a ragged
        record; ctrl [B, 12 S]; times [B, n_times]; x_bar [B, 2, n_times, 3]: the cotangent of the states.  Returns a dict
        of device tensors: "ctrl" [B, 12 S] and "times" [B, n_times], the derivative along the trajectory (0 for a time
        that is not > 0)."""
        B, S, seg_count, seg = self._layout_of(rec_or_dbatch)
        d = self.device
        f = lambda t: t.to(d, dtype=torch.float64).contiguous()
        times, x_bar, ctrl = f(times), f(x_bar), f(ctrl)
        n = times.shape[1]
        if tuple(times.shape) != (B, n) or tuple(x_bar.shape) != (B, 2, n, 3) or tuple(ctrl.shape) != (B, 12 * S):
            raise ValueError("times [B, n_times], x_bar [B, 2, n_times, 3], ctrl [B, 12 S]")
        g = dict(ctrl=torch.empty((B, 12 * S), dtype=torch.float64, device=d) if want_ctrl else None,
                 times=torch.empty((B, n), dtype=torch.float64, device=d) if want_times else None)
        stream = torch.cuda.current_stream(d).cuda_stream
        self.ctx.eval_states_vjp_device(B, S, seg_count, seg, ctrl, n, times, x_bar, ctrl_bar=g["ctrl"],
                                        times_bar=g["times"], stream=stream)
        return g
