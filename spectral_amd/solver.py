"""Device-resident batch solver: torch supplies HBM buffers and streams, the HIP library
(libbtrapz_hip.so) does all the work.  No torch ops on the data path."""
import numpy as np
import torch

from . import layout as L
from .native import (Context, CObstacles, CRoad, CRefLine, FRENET_SAMPLES, FRENET_STATES, KIN_AUDIT, MAX_TANGENTS,
                     footprint_struct)


class DeviceBatch:
    """A candidate batch resident in HBM (field-major SoA, see layout.py): B candidates of S segment slots each.
    seg_count None: a uniform batch, every candidate has S segments; an int32 [B] device tensor: a ragged batch of
    stride S.  Arrays a call does not read may be None."""

    def __init__(self, batch, device):
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)
        self.B, self.S, self.seg_count = batch.B, batch.S, None
        self.seg, self.init, self.ref_end, self.dl_bounds = f(batch.seg), f(batch.init), f(batch.ref_end), f(batch.dl_bounds)

    @classmethod
    def from_tensors(cls, seg, init=None, ref_end=None, dl_bounds=None, seg_count=None, B=None, S=None):
        """The record of device tensors that are there already; B and S default to seg's extents [NUM_SEG_FIELDS, B, S]."""
        r = cls.__new__(cls)
        r.B, r.S = seg.shape[1] if B is None else B, seg.shape[2] if S is None else S
        r.seg, r.init, r.ref_end, r.dl_bounds, r.seg_count = seg, init, ref_end, dl_bounds, seg_count
        return r


def _sets_of(shared_or_sets):
    """A layout.Shared, or a list / tuple of them -> the list of parameter sets."""
    return list(shared_or_sets) if isinstance(shared_or_sets, (list, tuple)) else [shared_or_sets]


def _check_index(t, B):
    assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B


class BatchSolver:
    """Solves DeviceBatches on one GPU; outputs stay on the device.  Wherever a method takes a batch it takes either
    shape of one: a DeviceBatch, or a ragged record dict (B, seg_stride, seg, seg_count, init, ref_end, dl_bounds; as
    corridor_batch returns it; seg_count None or absent: uniform)."""

    def __init__(self, device_index=0):
        if not torch.cuda.is_available():
            raise RuntimeError("spectral_amd.BatchSolver needs a HIP device (no CPU path)")
        self.device = torch.device("cuda", device_index)
        self.ctx = Context(device_index)
        self._out = {}

    def upload(self, batch):
        return DeviceBatch(batch, self.device)

    # ---- the one way to do each repeated thing ------------------------------------------------
    @staticmethod
    def _record(x):
        """Either shape of a batch -> DeviceBatch (names B, S, seg_count, seg, init, ref_end, dl_bounds; missing: None)."""
        if isinstance(x, DeviceBatch):
            return x
        if isinstance(x, dict):
            return DeviceBatch.from_tensors(x["seg"], x.get("init"), x.get("ref_end"), x.get("dl_bounds"), x.get("seg_count"),
                                            B=x["B"], S=x["seg_stride"])
        g = lambda k: getattr(x, k, None)     # (an object with the DeviceBatch attributes a call reads)
        return DeviceBatch.from_tensors(x.seg, g("init"), g("ref_end"), g("dl_bounds"), g("seg_count"), B=x.B, S=x.S)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _empty(self, *shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

    def _f64(self, t, detach=False):
        """A tensor as contiguous float64 on this device (itself when it is that already); None -> None."""
        if t is None:
            return None
        return (t.detach() if detach else t).to(self.device, dtype=torch.float64).contiguous()

    def new_result(self, B, S, zero_ctrl=False):
        """A fresh result dict of device tensors: ctrl [B, 12 S], cost, status, iters [B].  zero_ctrl: what a ragged solve
        needs and a uniform one does not -- the slots beyond a candidate's segment count are not written and must read 0."""
        return dict(ctrl=(self._zeros if zero_ctrl else self._empty)(B, 12 * S), cost=self._empty(B),
                    status=self._empty(B, dtype=torch.int32), iters=self._empty(B, dtype=torch.int32))

    def _buffers(self, B, S):
        """The result dict uniform solves of this shape share: a loop of solves allocates nothing."""
        key = (B, S)
        if key not in self._out:
            self._out[key] = self.new_result(B, S)
        return self._out[key]

    def _out_of(self, r, out):
        """The caller's `out`; else the shared buffers of a uniform batch, a fresh zeroed result for a ragged one."""
        if out is not None:
            return out
        return self._buffers(r.B, r.S) if r.seg_count is None else self.new_result(r.B, r.S, zero_ctrl=True)

    def _ragged_record(self, B, seg_stride, init, **more):
        """The dict the corridor stages fill: a ragged batch record, zeroed (a candidate's unused slots read 0)."""
        return dict(B=B, seg_stride=seg_stride, seg=self._zeros(L.NUM_SEG_FIELDS, B, seg_stride),
                    seg_count=self._zeros(B, dtype=torch.int32), init=init, ref_end=self._zeros(B, 2),
                    dl_bounds=self._zeros(B, 10), **more)

    def _warm(self, r, warm, keep_multipliers, o):
        """The btrapz_warm arguments of a solve of record r, shapes checked, and the result dict, which gains "lam" when
        the multipliers are kept."""
        warm = warm or {}
        x0, lam0 = warm.get("x0"), warm.get("lam")
        if x0 is not None:
            assert x0.dtype == torch.float64 and x0.is_contiguous() and tuple(x0.shape) == (r.B, 2, r.S, 3)
        if lam0 is not None:
            assert lam0.dtype == torch.float64 and lam0.is_contiguous() and tuple(lam0.shape) == (2, 36, r.B, r.S)
        lam_out = None
        if keep_multipliers:
            # in place when a previous solve's array is passed in (allowed: include/btrapz_hip.h, btrapz_warm)
            lam_out = lam0 if lam0 is not None else self._empty(2, 36, r.B, r.S)
            o = dict(o); o["lam"] = lam_out
        return dict(x0=x0, lam0=lam0, lam_out=lam_out, mu0=warm.get("mu0", 0.0), smin=warm.get("smin", 0.0),
                    hint=warm.get("hint")), o

    # ---- solves -----------------------------------------------------------------------------
    def solve(self, dbatch, shared, max_iter=0, eps=0.0, out=None, warm=None, keep_multipliers=False, elastic=0,
              elastic_tol=0.0, queue=0, split=0, start=0, cap_iter=0, lean=0, compact=0):
        """Launches the solve on torch's current stream; returns dict of device tensors.

        warm: dict with optional "x0" ([B,2,S,3] joint states, e.g. from eval_states) and "lam" ([2,36,B,S]
        multipliers kept by an earlier solve) plus optional "mu0", "smin" and "hint" ([B] int32 expected difficulty,
        e.g. the previous step's iters: scheduling only) -- btrapz_warm.  keep_multipliers
        adds this solve's multipliers to the result as "lam".  elastic: btrapz_options.elastic (0 off, 1 rescue pass
        over stalled candidates, 2 elastic rows for every candidate).  split: btrapz_options.split (0 automatic: the
        one-candidate-per-wavefront form for batches that leave SIMDs idle; 1 always where it applies; -1 never).  lean:
        btrapz_options.lean (the two-wavefronts-per-SIMD form of cold solves: 0 automatic, 1 where it applies, -1 never).
        A ragged record is taken with warm or keep_multipliers (btrapz_solve_warm_device); its cold solve is solve_ragged."""
        r = self._record(dbatch)
        if warm is None and not keep_multipliers:
            if r.seg_count is not None:
                raise ValueError("solve: the cold solve of a ragged record is solve_ragged")
            o = self._out_of(r, out)
            self.ctx.solve_device(r.B, r.S, shared, r.seg, r.init, r.ref_end, r.dl_bounds, o["ctrl"], o["cost"],
                                  o["status"], o["iters"], stream=self._stream(), max_iter=max_iter, eps=eps,
                                  elastic=elastic, elastic_tol=elastic_tol, queue=queue, split=split, start=start,
                                  cap_iter=cap_iter, lean=lean, compact=compact)
            return o
        return self._warm_solve(self.ctx.solve_warm_device, r, shared, warm, keep_multipliers, out, max_iter=max_iter, eps=eps,
                                elastic=elastic, elastic_tol=elastic_tol, lean=lean)

    def _warm_solve(self, entry, r, shared, warm, keep_multipliers, out, **options):
        """solve() with a warm start or kept multipliers, through `entry` (Context.solve_warm_device or its long sibling)."""
        w, o = self._warm(r, warm, keep_multipliers, self._out_of(r, out))
        if w["hint"] is not None:
            _check_index(w["hint"], r.B)
        entry(r.B, r.S, shared, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, o["ctrl"], o["cost"], o["status"],
              o["iters"], stream=self._stream(), **options, **w)
        return o

    def solve_long(self, dbatch_or_rec, shared, warm=None, keep_multipliers=False, max_iter=0, eps=0.0, out=None):
        """solve(..., warm=, keep_multipliers=) for candidates of up to 256 segments (btrapz_solve_long_warm_device):
        a uniform batch, or a ragged record whose stride may exceed 64.  Candidates of 65..256 segments are warm-started
        from warm["x0"] / warm["lam"] and return their multipliers as "lam" like the shorter ones (up to 64 slots per
        candidate the call is solve()'s own, bit for bit).  warm None and keep_multipliers False: the cold start.  No
        rescue pass; warm["hint"] is not read beyond 64 slots.  Returns the dict solve() returns."""
        return self._warm_solve(self.ctx.solve_long_warm_device, self._record(dbatch_or_rec), shared, warm, keep_multipliers, out,
                                max_iter=max_iter, eps=eps)

    def solve_long_rescue(self, dbatch_or_rec, shared, warm=None, keep_multipliers=False, max_iter=0, eps=0.0, out=None, elastic=1,
                          elastic_tol=0.0):
        """solve_long with the rescue pass (btrapz_solve_long_rescue_device; elastic: 0 or 1, elastic_tol:
        btrapz_options.elastic_tol, 0 = the default): a candidate of up to 256 segments that stalls is solved again with
        elastic rows -- the long candidates of a ragged record too -- and comes back with status 2 where its least violation
        is within the tolerance.  "lam" of a rescued candidate is the stalled solve's.  elastic = 0 is solve_long, bit for
        bit.  (A method of its own: solve_long's signature is part of its contract.)"""
        return self._warm_solve(self.ctx.solve_long_rescue_device, self._record(dbatch_or_rec), shared, warm, keep_multipliers, out,
                                max_iter=max_iter, eps=eps, elastic=elastic, elastic_tol=elastic_tol)

    def prepare(self, dbatch, shared, out=None, **options):
        """solve(dbatch, shared, **options) prepared once: returns (call, out) where call() launches the solve on the
        stream that is current NOW and `out` is the dict of device tensors it fills (cold solves only)."""
        r = self._record(dbatch)
        o = out if out is not None else self._buffers(r.B, r.S)
        call = self.ctx.prepared_solve(r.B, r.S, shared, r.seg, r.init, r.ref_end, r.dl_bounds, o["ctrl"], o["cost"],
                                       o["status"], o["iters"], stream=self._stream(), **options)
        return call, o

    def solve_ragged(self, rec, shared, max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, cap_iter=0, lean=0, compact=0):
        """Solve a ragged batch record (from corridor_batch); outputs stay on the device.  cap_iter:
        btrapz_options.cap_iter (0 automatic, -1 one launch, n two launches with hand-over after n iterations)."""
        r = self._record(rec)
        o = self.new_result(r.B, r.S, zero_ctrl=True)
        self.ctx.solve_ragged_device(r.B, r.S, shared, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, o["ctrl"],
                                     o["cost"], o["status"], o["iters"], stream=self._stream(), max_iter=max_iter, eps=eps,
                                     elastic=elastic, elastic_tol=elastic_tol, cap_iter=cap_iter, lean=lean, compact=compact)
        return o

    def _sets_call(self, r, sets, set_index, o, warm, keep_multipliers, options):
        _check_index(set_index, r.B)
        w, o = self._warm(r, warm, keep_multipliers, o)
        self.ctx.solve_sets_device(r.B, r.S, sets, set_index, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, o["ctrl"],
                                   o["cost"], o["status"], o["iters"], stream=self._stream(), **w, **options)
        return o

    def solve_sets(self, dbatch, sets, set_index, warm=None, keep_multipliers=False, out=None, **options):
        """A parameter set per candidate (btrapz_solve_sets_device): sets is a list of layout.Shared, set_index an int32
        device tensor [B] naming each candidate's set (outside [0, len(sets)): not solved, status NO_CORRIDOR, cost
        +inf).  warm / keep_multipliers as in solve(); options: max_iter, eps, lean (0 / 1 / -1), cap_iter and compact
        (0 or -1: the sets path runs one launch without the pre-pass).  Returns the dict of device tensors."""
        r = self._record(dbatch)
        return self._sets_call(r, sets, set_index, self._out_of(r, out), warm, keep_multipliers, options)

    def solve_sets_ragged(self, rec, sets, set_index, warm=None, keep_multipliers=False, **options):
        """solve_sets for a ragged batch record (from corridor_batch): candidates of up to 64 segments."""
        r = self._record(rec)
        return self._sets_call(r, sets, set_index, self.new_result(r.B, r.S, zero_ctrl=True), warm, keep_multipliers, options)

    def solve_long_sets(self, dbatch_or_rec, sets, set_index, warm=None, keep_multipliers=False, out=None, elastic=0,
                        elastic_tol=0.0, max_iter=0, eps=0.0, lean=0):
        """solve_sets / solve_sets_ragged with what solve_long and solve_long_rescue give one set
        (btrapz_solve_long_sets_device): candidates of up to 256 segments are warm-started from warm["x0"] / warm["lam"] and
        return their multipliers as "lam", and with elastic = 1 a candidate of any width that stalls is solved again with
        elastic rows under its own set (status 2 where its least violation is within elastic_tol).  Each candidate gets, bit
        for bit, what solve_long_rescue gives it with its own set (lean pinned to 1 or -1).  A uniform batch, or a ragged
        record whose stride may exceed 64; warm["hint"] is not read.  Returns the dict solve() returns."""
        r = self._record(dbatch_or_rec)
        _check_index(set_index, r.B)
        w, o = self._warm(r, warm, keep_multipliers, self._out_of(r, out))
        self.ctx.solve_long_sets_device(r.B, r.S, sets, set_index, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, o["ctrl"],
                                        o["cost"], o["status"], o["iters"], stream=self._stream(), elastic=elastic,
                                        elastic_tol=elastic_tol, max_iter=max_iter, eps=eps, lean=lean, **w)
        return o

    def eval_states(self, dbatch, ctrl, times):
        """(p, v, a) of every candidate's solved trajectory at times[b][j] (seconds from the start of its
        horizon) -> [B, 2, n_times, 3]; the x0 of a warm start."""
        r = self._record(dbatch)
        times = self._f64(times)
        n = times.shape[1]
        x = self._empty(r.B, 2, n, 3)
        self.ctx.eval_states_device(r.B, r.S, r.seg_count, r.seg, ctrl, n, times, x, stream=self._stream())
        return x

    # ---- the stages in front of the solve -----------------------------------------------------
    def corridor_batch(self, kb, variant, seg_stride=16):
        """Device corridor stage on a spectral_amd.knots.KnotBatch -> dict of device tensors forming a ragged
        batch record (seg, seg_count, init, ref_end, dl_bounds)."""
        up = self._upload
        rec = self._ragged_record(kb.B, seg_stride, up(kb.init))
        ins = [up(kb.s_bounds), up(kb.l_bounds), up(kb.ds_bounds), up(kb.dl_bounds), up(kb.s_ref), up(kb.l_ref)]
        self.ctx.corridor_batch_device(variant, kb.B, kb.N, kb.num_obs, kb.delta, *ins, seg_stride, rec["seg"],
                                       rec["seg_count"], rec["ref_end"], rec["dl_bounds"], stream=self._stream())
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
        if hasattr(kb_or_tensors, "s_bounds"):
            kb, up = kb_or_tensors, self._upload
            ins = [up(kb.s_bounds), up(kb.l_bounds), up(kb.ds_bounds), up(kb.dl_bounds), up(kb.s_ref), up(kb.l_ref)]
            delta = kb.delta if delta is None else delta
        else:
            ins = [self._f64(t, detach=True) for t in kb_or_tensors]
            if delta is None:
                raise ValueError("delta is needed with tensors")
        B, O, N = ins[0].shape[0], ins[0].shape[1], ins[0].shape[2]
        seg_bar, ref_end_bar, dl_bounds_bar = (self._f64(t, detach=True) for t in (seg_bar, ref_end_bar, dl_bounds_bar))
        if seg_bar is None and seg_stride is None:
            raise ValueError("seg_stride is needed without a seg_bar")
        if seg_bar is not None and seg_stride is not None and int(seg_stride) != seg_bar.shape[2]:
            raise ValueError("seg_stride %d is not seg_bar's, %d" % (seg_stride, seg_bar.shape[2]))
        seg_stride = seg_bar.shape[2] if seg_bar is not None else int(seg_stride)
        like = dict(s_bounds=ins[0], l_bounds=ins[1], ds_bounds=ins[2], dl_bounds_knots=ins[3], s_ref=ins[4], l_ref=ins[5])
        grads = {k: torch.empty_like(like[k]) for k in want}
        self.ctx.corridor_batch_vjp_device(variant, B, N, O, delta, *ins, seg_stride, seg_bar, ref_end_bar, dl_bounds_bar,
                                           grads, stream=self._stream())
        grads["_inputs"] = (ins, seg_bar, ref_end_bar, dl_bounds_bar)   # alive until the launch has run
        return grads

    def prism_bounds(self, prisms, N, O, road=None):
        """Obstacle prisms [B, P, 8] (s0, l0, t0, vel_s, vel_l, T, active, -) -> per-knot bounds of the lateral strips
        (btrapz_prism_bounds_device): s_bounds, l_bounds [B, O, N, 2] and n_strips [B], on the device."""
        prisms = self._f64(prisms)
        B, P = prisms.shape[0], prisms.shape[1]
        sb, lb, n = self._empty(B, O, N, 2), self._empty(B, O, N, 2), self._empty(B, dtype=torch.int32)
        self.ctx.prism_bounds_device(B, P, N, road or CRoad.reference(), prisms, O, sb, lb, n, stream=self._stream())
        return sb, lb, n

    def prism_bounds_vjp(self, prisms, N, O, s_bounds_bar, l_bounds_bar, road=None):
        """Gradients of prism_bounds w.r.t. the prisms (btrapz_prism_bounds_vjp_device, one launch): cotangents
        s_bounds_bar, l_bounds_bar [B, O, N, 2] (either may be None, not both) -> prisms_bar [B, P, 8]: s0, l0, t0, vel_s,
        vel_l, T, then two zeros.  The stage's decisions are frozen and the two-decimal rounding of the faces counts as the
        identity (include/btrapz_hip.h lists the rules); a scene with more than O strips gets zeros."""
        prisms = self._f64(prisms, detach=True)
        B, P = prisms.shape[0], prisms.shape[1]
        sbar, lbar = self._f64(s_bounds_bar, detach=True), self._f64(l_bounds_bar, detach=True)
        for t in (sbar, lbar):
            if t is not None and tuple(t.shape) != (B, int(O), int(N), 2):
                raise ValueError("a cotangent must be [B, O, N, 2] = %s, not %s" % ((B, O, N, 2), tuple(t.shape)))
        out = self._empty(B, P, 8)
        self.ctx.prism_bounds_vjp_device(B, P, N, road or CRoad.reference(), prisms, O, sbar, lbar, out, stream=self._stream())
        return out

    def prism_bounds_jvp(self, prisms, N, O, prisms_dot, road=None):
        """Forward-mode derivative of prism_bounds (btrapz_prism_bounds_jvp_device, one launch): prisms [B, P, 8] and T <= 32
        directions prisms_dot [T, B, P, 8] (entries 6, 7 and inactive slots are not read) -> (s_bounds_dot, l_bounds_dot),
        each [T, B, O, N, 2] = 16 T B O N bytes.  Decisions frozen, rounding straight-through (include/btrapz_hip_stage_jvp.h);
        a scene with more than O strips gets zeros."""
        prisms, prisms_dot = self._f64(prisms, detach=True), self._f64(prisms_dot, detach=True)
        B, P = prisms.shape[0], prisms.shape[1]
        if prisms_dot.dim() != 4 or tuple(prisms_dot.shape[1:]) != (B, P, 8):
            raise ValueError("prisms_dot must be [T, B, P, 8] = [T, %d, %d, 8], not %s" % (B, P, tuple(prisms_dot.shape)))
        T = prisms_dot.shape[0]
        s_dot, l_dot = self._empty(T, B, O, N, 2), self._empty(T, B, O, N, 2)
        self.ctx.prism_bounds_jvp_device(B, P, N, road or CRoad.reference(), prisms, O, T, prisms_dot, s_dot, l_dot,
                                         stream=self._stream())
        return s_dot, l_dot

    def corridor_batch_jvp(self, kb_or_tensors, variant, tangents, delta=None, seg_stride=16):
        """Forward-mode derivative of the device corridor stage (btrapz_corridor_batch_jvp_device).  kb_or_tensors: as in
        corridor_batch_vjp.  tangents: a dict with any of "s_bounds", "l_bounds" [T, B, O, N, 2], "ds_bounds",
        "dl_bounds_knots" [T, B, N, 2], "s_ref", "l_ref" [T, B, N]; a missing one is zero.  Returns {"seg": [T,
        NUM_SEG_FIELDS, B, seg_stride], "ref_end": [T, B, 2], "dl_bounds": [T, B, 10]} -- the dict solve_jvp accepts."""
        if hasattr(kb_or_tensors, "s_bounds"):
            kb, up = kb_or_tensors, self._upload
            ins = [up(kb.s_bounds), up(kb.l_bounds), up(kb.ds_bounds), up(kb.dl_bounds), up(kb.s_ref), up(kb.l_ref)]
            delta = kb.delta if delta is None else delta
        else:
            ins = [self._f64(t, detach=True) for t in kb_or_tensors]
            if delta is None:
                raise ValueError("delta is needed with tensors")
        B, O, N = ins[0].shape[0], ins[0].shape[1], ins[0].shape[2]
        names = ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds_knots", "s_ref", "l_ref")
        unknown = set(tangents) - set(names)
        if unknown:
            raise ValueError("unknown tangents: %s" % sorted(unknown))
        given = {k: v for k, v in tangents.items() if v is not None}
        T = next(iter(given.values())).shape[0] if given else 0
        tan = {}
        for k, v in given.items():
            shape = (T,) + tuple(ins[names.index(k)].shape)
            if tuple(v.shape) != shape:
                raise ValueError("tangent %r: shape %s, expected %s" % (k, tuple(v.shape), shape))
            tan[k] = self._f64(v, detach=True)
        seg_stride = int(seg_stride)
        o = dict(seg=self._empty(max(T, 0), L.NUM_SEG_FIELDS, B, seg_stride), ref_end=self._empty(max(T, 0), B, 2),
                 dl_bounds=self._empty(max(T, 0), B, 10))
        self.ctx.corridor_batch_jvp_device(variant, B, N, O, delta, *ins, seg_stride, T, tan, o["seg"], o["ref_end"],
                                           o["dl_bounds"], stream=self._stream())
        return o   # (ins and tan were allocated on the launch's stream: the allocator hands their memory on in stream order)

    def corridor_batch_tensors(self, variant, N, delta, s_bounds, l_bounds, ds_bounds, dl_bounds, s_ref, l_ref, init,
                               seg_stride=16):
        """corridor_batch on device tensors (e.g. the output of prism_bounds): s_bounds, l_bounds [B, O, N, 2],
        ds_bounds, dl_bounds [B, N, 2], s_ref, l_ref [B, N], init [B, 6]."""
        B, O = s_bounds.shape[0], s_bounds.shape[1]
        ins = [self._f64(t) for t in (s_bounds, l_bounds, ds_bounds, dl_bounds, s_ref, l_ref)]
        rec = self._ragged_record(B, seg_stride, self._f64(init))
        self.ctx.corridor_batch_device(variant, B, N, O, delta, *ins, seg_stride, rec["seg"], rec["seg_count"],
                                       rec["ref_end"], rec["dl_bounds"], stream=self._stream())
        rec["_inputs"] = ins
        return rec

    def prism_corridor_batch(self, variant, prisms, N, O, delta, ds_bounds, dl_bounds, s_ref, l_ref, init, seg_stride=16,
                             road=None):
        """prism_bounds + corridor_batch_tensors in one launch (btrapz_prism_corridor_batch_device): the strips are
        evaluated inside the corridor kernel instead of written to memory.  Same record, plus rec["n_strips"]."""
        ins = [self._f64(t) for t in (prisms, ds_bounds, dl_bounds, s_ref, l_ref)]
        B, P = ins[0].shape[0], ins[0].shape[1]
        rec = self._ragged_record(B, seg_stride, self._f64(init), n_strips=self._empty(B, dtype=torch.int32))
        self.ctx.prism_corridor_batch_device(variant, B, P, N, road or CRoad.reference(), ins[0], O, delta, *ins[1:],
                                             seg_stride, rec["seg"], rec["seg_count"], rec["ref_end"], rec["dl_bounds"],
                                             rec["n_strips"], stream=self._stream())
        rec["_inputs"] = ins
        return rec

    # ---- derivatives of a solve ---------------------------------------------------------------
    def _derivative_args(self, what, r, shared_or_sets, out, set_index):
        """What solve_vjp and solve_jvp check alike; returns the list of parameter sets."""
        if set_index is not None:
            _check_index(set_index, r.B)
        if out.get("lam") is None:
            raise ValueError("%s needs the solve's multipliers: solve with keep_multipliers=True" % what)
        return _sets_of(shared_or_sets)

    def solve_long_vjp(self, dbatch_or_rec, shared_or_sets, out, ctrl_bar, cost_bar, set_index=None):
        """solve_vjp for candidates of up to 256 segments (btrapz_solve_long_vjp_device): `out` is the result dict of
        solve_long(..., keep_multipliers=True).  Arguments, shapes, checks and the returned dict are solve_vjp's; up to 64
        slots per candidate the call is solve_vjp's own, bit for bit."""
        return self._solve_vjp(self.ctx.solve_long_vjp_device, "solve_long_vjp", dbatch_or_rec, shared_or_sets, out, ctrl_bar,
                               cost_bar, set_index)

    def solve_long_jvp(self, dbatch_or_rec, shared_or_sets, out, tangents, set_index=None):
        """solve_jvp for candidates of up to 256 segments (btrapz_solve_long_jvp_device): `out` is the result dict of
        solve_long(..., keep_multipliers=True).  Arguments, shapes, checks and the returned dict are solve_jvp's; up to 64
        slots per candidate the call is solve_jvp's own, bit for bit."""
        return self._solve_jvp(self.ctx.solve_long_jvp_device, "solve_long_jvp", dbatch_or_rec, shared_or_sets, out, tangents,
                               set_index)

    def solve_vjp(self, dbatch_or_rec, shared_or_sets, out, ctrl_bar, cost_bar, set_index=None):
        """Gradients of a solve (btrapz_solve_vjp_device).  dbatch_or_rec: the DeviceBatch or ragged record that was solved;
        shared_or_sets: its layout.Shared, or the list of sets with set_index (int32 device tensor [B]); out: the solve's
        result dict, from a solve with keep_multipliers=True and elastic=0 (needs "ctrl", "lam", "status"); ctrl_bar
        [B, 12 S] / cost_bar [B]: cotangents (either may be None).  Returns a dict of device tensors: "seg"
        [NUM_SEG_FIELDS, B, S] (field 0 is 0), "init" [B, 6], "ref_end" [B, 2], "dl_bounds" [B, 10], "shared" [B, 20] per
        candidate (layout.Shared.as_array order, without delta)."""
        return self._solve_vjp(self.ctx.solve_vjp_device, "solve_vjp", dbatch_or_rec, shared_or_sets, out, ctrl_bar, cost_bar,
                               set_index)

    def _solve_vjp(self, entry, what, dbatch_or_rec, shared_or_sets, out, ctrl_bar, cost_bar, set_index):
        """solve_vjp through `entry` (Context.solve_vjp_device or its long sibling)."""
        r = self._record(dbatch_or_rec)
        B, S = r.B, r.S
        sets = self._derivative_args(what, r, shared_or_sets, out, set_index)
        chk = lambda t, shape: None if t is None else (t if (t.dtype == torch.float64 and t.is_contiguous() and
                                                            tuple(t.shape) == shape) else
                                                       t.to(self.device, dtype=torch.float64).reshape(shape).contiguous())
        ctrl_bar = chk(ctrl_bar, (B, 12 * S)); cost_bar = chk(cost_bar, (B,))
        g = dict(seg=self._empty(L.NUM_SEG_FIELDS, B, S), init=self._empty(B, 6), ref_end=self._empty(B, 2),
                 dl_bounds=self._empty(B, 10), shared=self._empty(B, 20))
        entry(B, S, sets, set_index, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, out["ctrl"], out["lam"], out["status"],
              ctrl_bar, cost_bar, g_seg=g["seg"], g_init=g["init"], g_ref_end=g["ref_end"], g_dl_bounds=g["dl_bounds"],
              g_shared=g["shared"], stream=self._stream())
        return g

    def solve_jvp(self, dbatch_or_rec, shared_or_sets, out, tangents, set_index=None):
        """Directional derivatives of a solve (btrapz_solve_jvp_device): T input directions per candidate, one launch, one
        factorisation per axis problem.  dbatch_or_rec, shared_or_sets, out, set_index: as in solve_vjp.  tangents: a dict
        with any of "seg" [T, NUM_SEG_FIELDS, B, S] (field 0 is ignored), "init" [T, B, 6], "ref_end" [T, B, 2],
        "dl_bounds" [T, B, 10], "shared" [T, B, 20] (per candidate, layout.Shared.as_array order without delta); a missing
        one is zero.  Returns {"ctrl": [T, B, 12 S], "cost": [T, B]}, device tensors."""
        return self._solve_jvp(self.ctx.solve_jvp_device, "solve_jvp", dbatch_or_rec, shared_or_sets, out, tangents, set_index)

    def _solve_jvp(self, entry, what, dbatch_or_rec, shared_or_sets, out, tangents, set_index):
        """solve_jvp through `entry` (Context.solve_jvp_device or its long sibling)."""
        r = self._record(dbatch_or_rec)
        B, S = r.B, r.S
        sets = self._derivative_args(what, r, shared_or_sets, out, set_index)
        unknown = set(tangents) - {"seg", "init", "ref_end", "dl_bounds", "shared"}
        if unknown:
            raise ValueError("unknown tangents: %s" % sorted(unknown))
        given = {k: v for k, v in tangents.items() if v is not None}
        T = next(iter(given.values())).shape[0] if given else 0
        shapes = dict(seg=(T, L.NUM_SEG_FIELDS, B, S), init=(T, B, 6), ref_end=(T, B, 2), dl_bounds=(T, B, 10), shared=(T, B, 20))
        tan = {}
        for k, v in given.items():
            if tuple(v.shape) != shapes[k]:
                raise ValueError("tangent %r: shape %s, expected %s" % (k, tuple(v.shape), shapes[k]))
            tan[k] = self._f64(v)
        o = dict(ctrl=self._empty(max(T, 0), B, 12 * S), cost=self._empty(max(T, 0), B))
        entry(B, S, sets, set_index, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, out["ctrl"], out["lam"], out["status"], T,
              seg_dot=tan.get("seg"), init_dot=tan.get("init"), ref_end_dot=tan.get("ref_end"), dl_bounds_dot=tan.get("dl_bounds"),
              shared_dot=tan.get("shared"), ctrl_dot=o["ctrl"], cost_dot=o["cost"], stream=self._stream())
        return o

    # ---- scores, samples, states and their derivatives ----------------------------------------
    def _cost_args(self, rec, shared_or_sets, ctrl, s_ref, l_ref, status, set_index):
        r = self._record(rec)
        B, S = r.B, r.S
        t = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        s_ref, l_ref = self._f64(t(s_ref)), self._f64(t(l_ref))
        if s_ref.shape != l_ref.shape or s_ref.dim() not in (1, 2) or (s_ref.dim() == 2 and s_ref.shape[0] != B):
            raise ValueError("s_ref / l_ref: [N] (one line for every candidate) or [B, N]")
        N = s_ref.shape[-1]
        if set_index is not None:
            _check_index(set_index, B)
        if status is not None:
            _check_index(status, B)
        ctrl = self._f64(ctrl)
        assert tuple(ctrl.shape) == (B, 12 * S), ctrl.shape
        return dict(B=B, seg_stride=S, sets=_sets_of(shared_or_sets), set_index=set_index, seg=r.seg, seg_count=r.seg_count,
                    init=r.init, ctrl=ctrl, status=status, N=N, s_ref=s_ref, l_ref=l_ref,
                    ref_stride=N if s_ref.dim() == 2 else 0)

    def traj_cost(self, rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, status=None, set_index=None):
        """a_cost -- the score find_traj returns -- of every candidate's sampled trajectory (btrapz_traj_cost_device).
        rec_or_dbatch: a DeviceBatch or a ragged record; shared_or_sets: the scoring layout.Shared, or a list of sets with
        set_index (int32 device tensor [B]); ctrl [B, 12 S]; s_ref / l_ref: [B, N] or [N] (one line for all); status
        (int32 [B], e.g. the solve's): candidates outside {1, 2} are not scored.  Returns (a_cost [B], n_points [B]) device
        tensors; a candidate that is not scored has +inf and 0."""
        a = self._cost_args(rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, status, set_index)
        cost, npts = self._empty(a["B"]), self._empty(a["B"], dtype=torch.int32)
        self.ctx.traj_cost_device(**a, a_cost=cost, n_points=npts, stream=self._stream())
        return cost, npts

    def traj_cost_vjp(self, rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, a_cost_bar, status=None, set_index=None):
        """Gradients of traj_cost (btrapz_traj_cost_vjp_device) for the cotangent a_cost_bar [B].  Returns a dict of device
        tensors: "ctrl" [B, 12 S], "init" [B, 6], "params" [B, 20] per candidate (layout.Shared.as_array order, without
        delta), "s_ref" / "l_ref" [B, N] per candidate (also for a shared line: sum the rows)."""
        a = self._cost_args(rec_or_dbatch, shared_or_sets, ctrl, s_ref, l_ref, status, set_index)
        B, S, N = a["B"], a["seg_stride"], a["N"]
        abar = torch.as_tensor(a_cost_bar).to(self.device, dtype=torch.float64).reshape(B).contiguous()
        g = dict(ctrl=self._empty(B, 12 * S), init=self._empty(B, 6), params=self._empty(B, 20), s_ref=self._empty(B, N),
                 l_ref=self._empty(B, N))
        self.ctx.traj_cost_vjp_device(**a, a_cost_bar=abar, ctrl_bar=g["ctrl"], init_bar=g["init"], params_bar=g["params"],
                                      s_ref_bar=g["s_ref"], l_ref_bar=g["l_ref"], stream=self._stream())
        return g

    # ---- the audit of control points against the rows of their QP --------------------------------
    def check_rows(self, rec_or_dbatch, shared_or_sets, ctrl, set_index=None, unit=0, want=("margin", "worst", "eq_res", "obj")):
        """Audit of ctrl [B, 12 S] against every row of the QP the record states for each candidate
        (btrapz_check_rows_device, one launch, nothing solved).  rec_or_dbatch: a DeviceBatch or a ragged record;
        shared_or_sets: its layout.Shared, or the list of sets with set_index (int32 device tensor [B]); unit 0: every row
        in its own unit, 1: divided by the row's norm (the unit of elastic_tol).  Returns a dict of the device tensors named
        in `want`: "margin" [B, 2, 4] (s axis, l axis; position, velocity, acceleration, jerk rows: the smallest distance
        to a bound, negative = violated, +inf = no bound), "worst" [B, 2, 4] int32 (the row 18 k + r that attains it, -1:
        none), "eq_res" [B, 2, 2] (largest residual of the initial-state rows, of the continuity rows), "obj" [B] (the
        solve's cost at ctrl).  A candidate that cannot be audited -- a non-finite control point, a segment count or set
        out of range, a duration <= 0 -- has margins -inf, worst -1, eq_res +inf, obj +inf."""
        r = self._record(rec_or_dbatch)
        B, S = r.B, r.S
        unknown = set(want) - {"margin", "worst", "eq_res", "obj"}
        if unknown:
            raise ValueError("unknown outputs: %s" % sorted(unknown))
        if set_index is not None:
            _check_index(set_index, B)
        ctrl = self._f64(ctrl, detach=True)
        if tuple(ctrl.shape) != (B, 12 * S):
            raise ValueError("ctrl must be [B, 12 S] = %s, not %s" % ((B, 12 * S), tuple(ctrl.shape)))
        shapes = dict(margin=((B, 2, 4), torch.float64), worst=((B, 2, 4), torch.int32), eq_res=((B, 2, 2), torch.float64),
                      obj=((B,), torch.float64))
        o = {k: self._empty(*shapes[k][0], dtype=shapes[k][1]) for k in want}
        self.ctx.check_rows_device(B, S, _sets_of(shared_or_sets), set_index, r.seg, r.seg_count, r.init, r.ref_end,
                                   r.dl_bounds, ctrl, unit=unit, stream=self._stream(), **o)
        return o

    @staticmethod
    def admissible(check, tol_rows, tol_eq):
        """A check_rows result (with "margin" and "eq_res") -> [B] bool mask: all eight margins >= -tol_rows and all four
        equality residuals <= tol_eq.  Written as comparisons that a NaN fails: NaN and the -inf / +inf of a candidate
        that cannot be audited come out False."""
        m, e = check["margin"], check["eq_res"]
        return (m >= -float(tol_rows)).reshape(m.shape[0], -1).all(dim=1) & (e <= float(tol_eq)).reshape(e.shape[0], -1).all(dim=1)

    @staticmethod
    def kinematic_admissible(audit, kappa_max, alat_max, a_lo, a_hi, frame_margin):
        """A cartesian() audit (with "worst") -> [R] bool mask: |kappa| <= kappa_max, v^2 |kappa| <= alat_max,
        a_lo <= a <= a_hi and 1 - kappa_r l >= frame_margin over the row's samples, no sample outside the reference line,
        and every extreme attained by a sample (worst >= 0).  The last condition is what keeps out a row with nothing to
        judge: a row without samples (count 0: an unsolved candidate), and a row whose samples all hold NaN -- such values
        enter no extreme and are not counted in n_outside, so the row's extremes are the -inf / +inf of "nobody", which
        every comparison above passes.  A row in which only SOME samples hold NaN is judged on the others: keep NaN out of
        the Frenet samples (the sampler and eval_states write none for a solved candidate).  Mask cost with it before topk:
        cost.masked_fill(~mask, inf)."""
        return ((audit["kappa_abs_max"] <= float(kappa_max)) & (audit["alat_abs_max"] <= float(alat_max)) &
                (audit["a_min"] >= float(a_lo)) & (audit["a_max"] <= float(a_hi)) &
                (audit["frame_min"] >= float(frame_margin)) & (audit["n_outside"] == 0) & (audit["worst"] >= 0).all(dim=1))

    # ---- Cartesian states, their kinematic audit and derivatives (include/btrapz_hip_cartesian.h) --
    def _cartesian_args(self, frenet, refline, layout, count, line_index, detach=True):
        f = self._f64(frenet, detach=detach)
        if layout == FRENET_SAMPLES and f.dim() == 3 and f.shape[1] == 6:
            R, n = f.shape[0], f.shape[2]
        elif layout == FRENET_STATES and f.dim() == 4 and f.shape[1] == 2 and f.shape[3] == 3:
            R, n = f.shape[0], f.shape[2]
        else:
            raise ValueError("frenet must be [R, 6, n] (FRENET_SAMPLES) or [R, 2, n, 3] (FRENET_STATES), not %s under layout %r"
                             % (tuple(f.shape), layout))
        for t in (count, line_index):
            if t is not None:
                _check_index(t, R)
        arrays = refline.on(self.device)
        t = CRefLine(refline.n_lines, refline.M, *[a.data_ptr() for a in arrays])
        return f, R, n, t, arrays

    def cartesian(self, frenet, refline, layout=FRENET_SAMPLES, count=None, line_index=None, want=("cart", "audit")):
        """Frenet samples -> Cartesian states and / or their kinematic audit (btrapz_cartesian_device, one launch).
        frenet: [R, 6, n] rows (s, ds, dds, l, dl, ddl) -- sample()'s out -- under FRENET_SAMPLES, or [R, 2, n, 3] --
        eval_states()'s x -- under FRENET_STATES; refline: a layout.RefLine; count: int32 [R] (sample()'s npoints; None:
        n samples per row); line_index: int32 [R] (None: line 0).  Returns a dict: "cart" [R, 6, n], rows (x, y, theta,
        kappa, v, a), NaN at samples outside the line and beyond a row's count; "audit": a dict of "kappa_abs_max",
        "alat_abs_max", "a_min", "a_max", "v_max", "frame_min" [R], "n_outside" [R] int32 and "worst" [R, 6] int32 (the
        sample that attains each extreme, -1: none).  want=("audit",) reads the samples and writes 60 bytes per row."""
        unknown = set(want) - {"cart", "audit"}
        if unknown or not want:
            raise ValueError("want: \"cart\" and / or \"audit\", not %r" % (want,))
        f, R, n, t, keep = self._cartesian_args(frenet, refline, layout, count, line_index)
        out = {}
        if "cart" in want:
            out["cart"] = torch.full((R, 6, n), float("nan"), dtype=torch.float64, device=self.device)
        if "audit" in want:
            out["audit"] = {k: self._empty(R) for k in KIN_AUDIT[:6]}
            out["audit"]["n_outside"] = self._empty(R, dtype=torch.int32)
            out["audit"]["worst"] = self._empty(R, 6, dtype=torch.int32)
        self.ctx.cartesian_device(t, line_index, R, n, layout, f, count, out.get("cart"), out.get("audit"), stream=self._stream())
        return out

    def cartesian_vjp(self, frenet, refline, cart_bar, layout=FRENET_SAMPLES, count=None, line_index=None):
        """Vector-Jacobian product of cartesian (btrapz_cartesian_vjp_device, one launch): cart_bar [R, 6, n] -> the
        cotangent of frenet, in its shape (what sample_vjp / eval_states_vjp take); 0 at samples that are not read or lie
        outside the line.  The interval of the lookup is frozen; the reference line gets no gradient."""
        f, R, n, t, keep = self._cartesian_args(frenet, refline, layout, count, line_index)
        cart_bar = self._f64(cart_bar, detach=True)
        if tuple(cart_bar.shape) != (R, 6, n):
            raise ValueError("cart_bar must be [R, 6, n] = %s, not %s" % ((R, 6, n), tuple(cart_bar.shape)))
        f_bar = torch.empty_like(f)
        self.ctx.cartesian_vjp_device(t, line_index, R, n, layout, f, count, cart_bar, f_bar, stream=self._stream())
        return f_bar

    def cartesian_jvp(self, frenet, refline, frenet_dot, layout=FRENET_SAMPLES, count=None, line_index=None):
        """Forward-mode derivative of cartesian (btrapz_cartesian_jvp_device): frenet_dot [T] x the shape of frenet ->
        cart_dot [T, R, 6, n], the per-sample Jacobian formed once per chunk of 32 directions; 0 at samples outside the line
        and beyond a row's count."""
        f, R, n, t, keep = self._cartesian_args(frenet, refline, layout, count, line_index)
        fd = self._f64(frenet_dot, detach=True)
        if fd.dim() != f.dim() + 1 or tuple(fd.shape[1:]) != tuple(f.shape):
            raise ValueError("frenet_dot must be [T] x %s, not %s" % (tuple(f.shape), tuple(fd.shape)))
        T = fd.shape[0]
        out = self._zeros(T, R, 6, n)
        for t0 in range(0, T, MAX_TANGENTS):
            t1 = min(t0 + MAX_TANGENTS, T)
            self.ctx.cartesian_jvp_device(t, line_index, R, n, layout, f, count, t1 - t0, fd[t0:t1], out[t0:t1], stream=self._stream())
        return out

    # ---- footprint clearance against moving obstacles (include/btrapz_hip_clearance.h) -----------
    @staticmethod
    def collision_free(audit, d_safe):
        """A clearance() audit -> [R] bool mask: the row's smallest clearance is >= d_safe and no sample read had an invalid
        pose -- written as comparisons that a NaN fails.  A row with nothing to judge (count 0: an unsolved candidate, or
        no obstacle present anywhere) has clear_min = +inf and PASSES this mask: combine it with kinematic_admissible,
        which keeps a row without samples out, and mask cost with both before topk:
        cost.masked_fill(~(kin & free), inf)."""
        return (audit["clear_min"] >= float(d_safe)) & (audit["n_invalid"] == 0)

    def _clearance_args(self, cart, obstacles, footprint, scene_index, count):
        c = self._f64(cart, detach=True)
        if c.dim() != 3 or c.shape[1] != 6:
            raise ValueError("cart must be [R, 6, n], not %s" % (tuple(c.shape),))
        R, n = c.shape[0], c.shape[2]
        if obstacles.n != n:
            raise ValueError("obstacles hold %d samples, cart %d" % (obstacles.n, n))
        for t in (count, scene_index):
            if t is not None:
                _check_index(t, R)
        arrays = obstacles.on(self.device)
        ob = CObstacles(obstacles.n_scenes, obstacles.O, obstacles.n, arrays[0].data_ptr(), arrays[1].data_ptr(),
                        arrays[2].data_ptr() if arrays[2] is not None else None)
        return c, R, n, footprint_struct(footprint), ob, arrays

    def clearance(self, cart, obstacles, footprint, scene_index=None, count=None, d_safe=0.0, want=("clear", "which", "audit")):
        """The signed clearance of the ego's rectangle against the scene's obstacle rectangles at every sample, and / or its
        audit per row (btrapz_clearance_device: one kernel launch, behind the two fills that give "clear" and "which" their
        NaN / -1 beyond a row's count).  cart: [R, 6, n] -- cartesian()'s "cart" (rows x, y, theta are
        read); obstacles: a layout.Obstacles with the same n; footprint: (half_length, half_width, centre_offset);
        scene_index: int32 [R] (None: scene 0); count: int32 [R] (None: n samples per row).  Returns a dict: "clear" [R, n]
        (< 0: minus the penetration depth; NaN: invalid pose or beyond the count; +inf: no obstacle), "which" [R, n] int32
        (obstacle * 16 + feature, -1: none), "audit": "clear_min" [R], "worst" [R, 2] int32 (sample, obstacle), "n_below"
        [R] int32 (samples with clearance < d_safe), "n_invalid" [R] int32."""
        unknown = set(want) - {"clear", "which", "audit"}
        if unknown or not want:
            raise ValueError("want: \"clear\", \"which\" and / or \"audit\", not %r" % (want,))
        c, R, n, ft, ob, keep = self._clearance_args(cart, obstacles, footprint, scene_index, count)
        out = {}
        if "clear" in want:
            out["clear"] = torch.full((R, n), float("nan"), dtype=torch.float64, device=self.device)
        if "which" in want:
            out["which"] = torch.full((R, n), -1, dtype=torch.int32, device=self.device)
        if "audit" in want:
            out["audit"] = dict(clear_min=self._empty(R), worst=self._empty(R, 2, dtype=torch.int32),
                                n_below=self._empty(R, dtype=torch.int32), n_invalid=self._empty(R, dtype=torch.int32))
        self.ctx.clearance_device(ft, ob, scene_index, R, n, c, count, d_safe, out.get("clear"), out.get("which"), out.get("audit"),
                                  stream=self._stream())
        return out

    def clearance_vjp(self, cart, obstacles, footprint, which, clear_bar, scene_index=None, count=None):
        """Vector-Jacobian product of clearance under the forward's `which` (btrapz_clearance_vjp_device, one launch):
        clear_bar [R, n] -> cart_bar [R, 6, n] (what cartesian_vjp takes); rows kappa, v, a and every sample that is not
        read, invalid or without an obstacle are 0.  The obstacles get no gradient in reverse mode."""
        c, R, n, ft, ob, keep = self._clearance_args(cart, obstacles, footprint, scene_index, count)
        cb = self._f64(clear_bar, detach=True)
        if tuple(cb.shape) != (R, n) or tuple(which.shape) != (R, n):
            raise ValueError("clear_bar and which must be [R, n] = %s" % ((R, n),))
        _check_index(which, R * n)
        cart_bar = torch.empty_like(c)
        self.ctx.clearance_vjp_device(ft, ob, scene_index, R, n, c, count, which, cb, cart_bar, stream=self._stream())
        return cart_bar

    def clearance_jvp(self, cart, obstacles, footprint, which, cart_dot, obs_dot=None, scene_index=None, count=None):
        """Forward-mode derivative of clearance under the forward's `which` (btrapz_clearance_jvp_device, one launch per 32
        tangents behind a zero fill of the result): cart_dot
        [T, R, 6, n] and obs_dot [T, n_scenes, O, 3, n] (None: the obstacles do not move) -> clear_dot [T, R, n]; 0 at
        samples beyond a row's count, with an invalid pose or without an obstacle."""
        c, R, n, ft, ob, keep = self._clearance_args(cart, obstacles, footprint, scene_index, count)
        cd = self._f64(cart_dot, detach=True)
        if cd.dim() != 4 or tuple(cd.shape[1:]) != (R, 6, n):
            raise ValueError("cart_dot must be [T, R, 6, n], not %s" % (tuple(cd.shape),))
        T = cd.shape[0]
        od = self._f64(obs_dot, detach=True)
        if od is not None and tuple(od.shape) != (T, obstacles.n_scenes, obstacles.O, 3, n):
            raise ValueError("obs_dot must be [T, n_scenes, O, 3, n]")
        if tuple(which.shape) != (R, n):
            raise ValueError("which must be [R, n]")
        _check_index(which, R * n)
        out = self._zeros(T, R, n)
        for t0 in range(0, T, MAX_TANGENTS):
            t1 = min(t0 + MAX_TANGENTS, T)
            self.ctx.clearance_jvp_device(ft, ob, scene_index, R, n, c, count, which, t1 - t0, cd[t0:t1],
                                          od[t0:t1] if od is not None else None, out[t0:t1], stream=self._stream())
        return out

    # ---- Cartesian states projected onto the reference line (include/btrapz_hip_frenet.h) --------
    def _frenet_args(self, cart, refline, layout, order, count, line_index):
        c = self._f64(cart, detach=True)
        if c.dim() != 3 or c.shape[1] != 6:
            raise ValueError("cart must be [R, 6, n], not %s" % (tuple(c.shape),))
        if layout not in (FRENET_SAMPLES, FRENET_STATES):
            raise ValueError("layout: FRENET_SAMPLES or FRENET_STATES, not %r" % (layout,))
        if order not in (0, 1, 2):
            raise ValueError("order: 0, 1 or 2, not %r" % (order,))
        R, n = c.shape[0], c.shape[2]
        for t in (count, line_index):
            if t is not None:
                _check_index(t, R)
        arrays = refline.on(self.device)
        t = CRefLine(refline.n_lines, refline.M, *[a.data_ptr() for a in arrays])
        shape = (R, 6, n) if layout == FRENET_SAMPLES else (R, 2, n, 3)
        return c, R, n, t, arrays, shape

    def frenet(self, cart, refline, layout=FRENET_SAMPLES, order=2, count=None, line_index=None, s_window=None):
        """Cartesian states -> Frenet states on the reference line (btrapz_frenet_device, one launch): the inverse of
        cartesian().  cart: [R, 6, n], rows (x, y, theta, kappa, v, a) -- cartesian()'s "cart"; rows above `order` (0: x, y;
        1: also theta, v; 2: all) are not read.  refline: a layout.RefLine; count, line_index: int32 [R]; s_window: [R, 2]
        (lo, hi) in arc length, the part of the line a row's queries are matched against (None: all of it).  Returns a
        dict: "frenet" under `layout` ([R, 6, n] rows (s, ds, dds, l, dl, ddl), or [R, 2, n, 3]), NaN at samples OUTSIDE
        the line and beyond a row's count, 0 above the order; "interval" [R, n] int32, the matched interval of the table
        (-1: OUTSIDE or not read), which the derivatives take; "n_outside" [R] int32."""
        c, R, n, t, keep, shape = self._frenet_args(cart, refline, layout, order, count, line_index)
        win = self._f64(s_window, detach=True)
        if win is not None and tuple(win.shape) != (R, 2):
            raise ValueError("s_window must be [R, 2] = %s, not %s" % ((R, 2), tuple(win.shape)))
        out = dict(frenet=torch.full(shape, float("nan"), dtype=torch.float64, device=self.device),
                   interval=torch.full((R, n), -1, dtype=torch.int32, device=self.device),
                   n_outside=self._empty(R, dtype=torch.int32))
        self.ctx.frenet_device(t, line_index, R, n, layout, order, c, count, win, out["frenet"], out["interval"], out["n_outside"],
                               stream=self._stream())
        return out

    def frenet_vjp(self, cart, refline, frenet, interval, frenet_bar, layout=FRENET_SAMPLES, order=2, count=None, line_index=None):
        """Vector-Jacobian product of frenet (btrapz_frenet_vjp_device, one launch): frenet_bar, shaped like frenet -> the
        cotangent of cart [R, 6, n]; 0 at samples that are not read or OUTSIDE.  cart, frenet and interval are the
        forward's: nothing is searched again.  The interval is frozen; the reference line gets no gradient."""
        c, R, n, t, keep, shape = self._frenet_args(cart, refline, layout, order, count, line_index)
        f, fb = self._f64(frenet, detach=True), self._f64(frenet_bar, detach=True)
        if tuple(f.shape) != shape or tuple(fb.shape) != shape:
            raise ValueError("frenet and frenet_bar must be %s, not %s and %s" % (shape, tuple(f.shape), tuple(fb.shape)))
        _check_index(interval, R * n)
        cart_bar = self._empty(R, 6, n)
        self.ctx.frenet_vjp_device(t, line_index, R, n, layout, order, c, f, interval, count, fb, cart_bar, stream=self._stream())
        return cart_bar

    def frenet_jvp(self, cart, refline, frenet, interval, cart_dot, layout=FRENET_SAMPLES, order=2, count=None, line_index=None):
        """Forward-mode derivative of frenet (btrapz_frenet_jvp_device): cart_dot [T, R, 6, n] -> frenet_dot [T] x the shape
        of frenet, the per-sample Jacobian formed once per chunk of 32 directions; 0 at OUTSIDE samples and beyond a row's
        count."""
        c, R, n, t, keep, shape = self._frenet_args(cart, refline, layout, order, count, line_index)
        f, cd = self._f64(frenet, detach=True), self._f64(cart_dot, detach=True)
        if tuple(f.shape) != shape:
            raise ValueError("frenet must be %s, not %s" % (shape, tuple(f.shape)))
        if cd.dim() != 4 or tuple(cd.shape[1:]) != (R, 6, n):
            raise ValueError("cart_dot must be [T, R, 6, n] = [T, %d, 6, %d], not %s" % (R, n, tuple(cd.shape)))
        _check_index(interval, R * n)
        T = cd.shape[0]
        out = self._zeros(T, *shape)
        for t0 in range(0, T, MAX_TANGENTS):
            t1 = min(t0 + MAX_TANGENTS, T)
            self.ctx.frenet_jvp_device(t, line_index, R, n, layout, order, c, f, interval, count, t1 - t0, cd[t0:t1], out[t0:t1],
                                       stream=self._stream())
        return out

    def init_from_cartesian(self, states, refline, line_index=None, s_window=None):
        """Cartesian start states [B, 6] = (x, y, theta, kappa, v, a), one per candidate -> (init [B, 6] = (s, ds, dds, l,
        dl, ddl), what a batch's `init` holds, and a [B] bool mask of the rows that are not OUTSIDE; an OUTSIDE row of
        init is NaN).  One btrapz_frenet_device launch at order 2, written in the layout of init."""
        st = self._f64(states, detach=True)
        if st.dim() != 2 or st.shape[1] != 6:
            raise ValueError("states must be [B, 6], not %s" % (tuple(st.shape),))
        B = st.shape[0]
        o = self.frenet(st.reshape(B, 6, 1), refline, layout=FRENET_STATES, order=2, line_index=line_index, s_window=s_window)
        return o["frenet"].reshape(B, 6), o["interval"].reshape(B) >= 0

    def prisms_from_cartesian(self, obstacles, refline, line_index=None, s_window=None):
        """Obstacles in the plane [B, P, 8] = (x, y, t0, theta, v, T, active, reserved) -> (the prisms [B, P, 8] = (s0, l0,
        t0, vel_s, vel_l, T, active, reserved) that prism_bounds takes, and n_outside [B] int64: the active obstacles of a
        scene that are OUTSIDE the line; such an obstacle gets active = 0 and zeros for its four projected entries).  One
        btrapz_frenet_device launch at order 1 (vel_s = ds, vel_l = dl); line_index, s_window: per scene."""
        ob = self._f64(obstacles, detach=True)
        if ob.dim() != 3 or ob.shape[2] != 8:
            raise ValueError("obstacles must be [B, P, 8], not %s" % (tuple(ob.shape),))
        B, P = ob.shape[0], ob.shape[1]
        cart = self._zeros(B, 6, P)
        cart[:, 0], cart[:, 1], cart[:, 2], cart[:, 4] = ob[:, :, 0], ob[:, :, 1], ob[:, :, 3], ob[:, :, 4]
        o = self.frenet(cart, refline, order=1, line_index=line_index, s_window=s_window)
        f, inside = o["frenet"], o["interval"] >= 0
        active = ob[:, :, 6] != 0
        zero = torch.zeros_like(f[:, 0])
        pick = lambda row: torch.where(inside, f[:, row], zero)
        prisms = torch.stack([pick(0), pick(3), ob[:, :, 2], pick(1), pick(4), ob[:, :, 5],
                              torch.where(inside, ob[:, :, 6], zero), ob[:, :, 7]], dim=2).contiguous()
        return prisms, (active & ~inside).sum(dim=1)

    def argmin(self, cost, group=None, index_base=0):
        """Arg-min of cost over contiguous groups (default: the whole batch). Device tensors."""
        B = cost.numel()
        group = B if group is None else group
        best_idx, best_cost = self._empty(B // group, dtype=torch.int64), self._empty(B // group)
        self.ctx.argmin_device(B, group, index_base, cost, best_idx, best_cost, stream=self._stream())
        return best_idx, best_cost

    def topk(self, cost, K, group=None, index_base=0):
        """The K best candidates of every contiguous group (default: the whole batch) in argmin's order -- cost ascending,
        equal costs -> lowest index -- by btrapz_topk_device.  Returns (best_idx [G, K] int64, best_cost [G, K]) device
        tensors; slots beyond the candidates that take part (cost < +inf) hold -1 / +inf.  K == 1 is argmin.  The same on
        every call and every rank: unlike torch.topk the order among equal costs is fixed.

        To sample or evaluate the winners pass `(best_idx - index_base).flatten()` as `sel` to sample / eval_states (put
        -1 back where best_idx is -1: such a selection yields 0 points); a winner that is refused afterwards is followed
        by the next column, without another solve."""
        B = cost.numel()
        group = B if group is None else group
        if group < 1 or B % group != 0:
            raise ValueError("topk: group %r does not divide the %d costs" % (group, B))
        best_idx, best_cost = self._empty(B // group, K, dtype=torch.int64), self._empty(B // group, K)
        self.ctx.topk_device(B, group, K, index_base, self._f64(cost), best_idx, best_cost, stream=self._stream())
        return best_idx, best_cost

    def sample(self, dbatch, ctrl, sel, delta):
        """Bernstein sampling (solve_3d.cc:1279-1392) of the selected candidates of a DeviceBatch or a ragged record
        (btrapz_sample_device / btrapz_sample_ragged_device) -> (out [nsel, 6, max_points], npoints [nsel])."""
        r = self._record(dbatch)
        sel = sel.to(self.device, dtype=torch.int64).contiguous()
        t = r.seg[L.F_T]
        if r.seg_count is not None:
            t = t * (torch.arange(r.S, device=self.device)[None, :] < r.seg_count[:, None])
        max_points = int(torch.floor(t / delta + 1e-9).sum(1).max().item()) + 2
        out, npts = self._zeros(sel.numel(), 6, max_points), self._zeros(sel.numel(), dtype=torch.int32)
        if r.seg_count is None:
            self.ctx.sample_device(r.B, r.S, delta, r.seg, r.init, ctrl, sel, max_points, out, npts, stream=self._stream())
        else:
            self.ctx.sample_ragged_device(r.B, r.S, r.seg_count, delta, r.seg, r.init, ctrl, sel, max_points, out, npts,
                                          stream=self._stream())
        return out, npts

    def sample_vjp(self, rec_or_dbatch, sel, delta, out_bar, want_ctrl=True, want_init=True):
        """Vector-Jacobian product of sample (btrapz_sample_vjp_device).  rec_or_dbatch: the DeviceBatch or ragged record
        that was sampled; sel: the selection of the forward; out_bar [nsel, 6, max_points]: the cotangent of the samples
        (max_points is read off its shape).  Returns a dict of device tensors with ONE ROW PER SELECTION -- "ctrl"
        [nsel, 12 S] and "init" [nsel, 6]; a candidate that sel names twice has two rows, which the caller sums."""
        r = self._record(rec_or_dbatch)
        sel = sel.to(self.device, dtype=torch.int64).contiguous()
        out_bar = self._f64(out_bar)
        n = sel.numel()
        if out_bar.dim() != 3 or out_bar.shape[0] != n or out_bar.shape[1] != 6:
            raise ValueError("out_bar: [nsel, 6, max_points]")
        g = dict(ctrl=self._empty(n, 12 * r.S) if want_ctrl else None, init=self._empty(n, 6) if want_init else None)
        self.ctx.sample_vjp_device(r.B, r.S, r.seg_count, delta, r.seg, sel, out_bar.shape[2], out_bar, ctrl_bar=g["ctrl"],
                                   init_bar=g["init"], stream=self._stream())
        return g

    def eval_states_vjp(self, rec_or_dbatch, ctrl, times, x_bar, want_ctrl=True, want_times=True):
        """Vector-Jacobian product of eval_states (btrapz_eval_states_vjp_device).  rec_or_dbatch: a DeviceBatch or a ragged
        record; ctrl [B, 12 S]; times [B, n_times]; x_bar [B, 2, n_times, 3]: the cotangent of the states.  Returns a dict
        of device tensors: "ctrl" [B, 12 S] and "times" [B, n_times], the derivative along the trajectory (0 for a time
        that is not > 0)."""
        r = self._record(rec_or_dbatch)
        B, S = r.B, r.S
        times, x_bar, ctrl = self._f64(times), self._f64(x_bar), self._f64(ctrl)
        n = times.shape[1]
        if tuple(times.shape) != (B, n) or tuple(x_bar.shape) != (B, 2, n, 3) or tuple(ctrl.shape) != (B, 12 * S):
            raise ValueError("times [B, n_times], x_bar [B, 2, n_times, 3], ctrl [B, 12 S]")
        g = dict(ctrl=self._empty(B, 12 * S) if want_ctrl else None, times=self._empty(B, n) if want_times else None)
        self.ctx.eval_states_vjp_device(B, S, r.seg_count, r.seg, ctrl, n, times, x_bar, ctrl_bar=g["ctrl"],
                                        times_bar=g["times"], stream=self._stream())
        return g
