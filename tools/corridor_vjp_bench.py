#!/usr/bin/env python3
"""The corridor stage's backward pass (btrapz_corridor_batch_vjp_device) beside its forward, timed in ONE run on the shape
of tools/corridor_bench.py: 65 536 jittered copies of c_road_s1_3.txt (N = 71 knots, 3 obstacles).  HIP events, median of
--reps launches each.  Reports backward / forward, the bytes the backward must move (the inputs once, the cotangents, and
every output array written once by the zeroing) with the HBM fraction, and the forward's output hash (the one
corridor_bench.py prints: it must not move).  Writes profiles/corridor_vjp_bench.json.

    python tools/corridor_vjp_bench.py [--input c_road_s1_3] [--batch 65536] [--reps 20] [--parent-forward-ms X --parent-forward-source TEXT]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="c_road_s1_3")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--seg-stride", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-forward-ms", type=float, default=None, help="the forward's time on the commit before this feature, same shape")
    ap.add_argument("--parent-forward-source", default=None, help="where --parent-forward-ms comes from (kept in the JSON)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corridor_vjp_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from spectral_amd import knots, layout as L
    from spectral_amd.native import KNOT_GRADS
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0); d = solver.device
    B, st = a.batch, a.seg_stride
    kb = knots.jittered(knots.parse_corridor_file(os.path.join(ROOT, "tests", "golden", "inputs", a.input + ".txt")), B, seed=3)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(d)
    ins = [f(kb.s_bounds), f(kb.l_bounds), f(kb.ds_bounds), f(kb.dl_bounds), f(kb.s_ref), f(kb.l_ref)]
    seg = torch.zeros((L.NUM_SEG_FIELDS, B, st), dtype=torch.float64, device=d)
    cnt = torch.zeros(B, dtype=torch.int32, device=d); ref_end = torch.zeros((B, 2), dtype=torch.float64, device=d)
    dl10 = torch.zeros((B, 10), dtype=torch.float64, device=d)
    g = torch.Generator(device="cpu").manual_seed(0)
    bars = [torch.randn(t.shape, generator=g, dtype=torch.float64).to(d) for t in (seg, ref_end, dl10)]
    grads = {k: torch.empty_like(t) for k, t in zip(KNOT_GRADS, ins)}
    stream = torch.cuda.current_stream(d).cuda_stream
    fwd = lambda: solver.ctx.corridor_batch_device(a.variant, B, kb.N, kb.num_obs, kb.delta, *ins, st, seg, cnt, ref_end, dl10, stream=stream)
    bwd = lambda: solver.ctx.corridor_batch_vjp_device(a.variant, B, kb.N, kb.num_obs, kb.delta, *ins, st, *bars, grads, stream=stream)

    def timed(run):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record(); torch.cuda.synchronize(); t.append(e0.elapsed_time(e1))
        return float(np.median(t)), float(np.min(t))
    f_ms, f_min = timed(fwd)
    b_ms, b_min = timed(bwd)
    c = cnt.cpu().numpy()
    h = hashlib.sha256(seg.cpu().numpy().tobytes() + c.tobytes() + ref_end.cpu().numpy().tobytes() + dl10.cpu().numpy().tobytes()).hexdigest()[:16]
    in_bytes = (4 * kb.num_obs + 6) * kb.N * 8
    bar_bytes = float(np.mean(np.maximum(c, 0))) * (L.NUM_SEG_FIELDS - 1) * 8 + 16 + 80
    gbs = (2 * in_bytes + bar_bytes) * B / (b_ms * 1e-3) / 1e9      # inputs read, outputs (the inputs' size) zeroed
    out = {"workload": "jittered %s.txt, %d candidates, N = %d, %d obstacles, variant %d" % (a.input, B, kb.N, kb.num_obs, a.variant),
           "forward_ms": f_ms, "forward_min_ms": f_min, "backward_ms": b_ms, "backward_min_ms": b_min, "backward_over_forward": b_ms / f_ms,
           "parent_forward_ms": a.parent_forward_ms, "parent_forward_source": a.parent_forward_source, "forward_hash": h, "mean_segments": float(np.mean(np.maximum(c, 0))),
           "backward_bytes_per_candidate": 2 * in_bytes + bar_bytes,
           "roofline": {"bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0},
           "nonzero_gradient_entries_per_candidate": float(sum(int((t != 0).sum()) for t in grads.values())) / B}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1); fh.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
