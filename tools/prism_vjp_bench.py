#!/usr/bin/env python3
"""The prism stage's backward pass (btrapz_prism_bounds_vjp_device) beside its forward (btrapz_prism_bounds_device), timed
in ONE run on the shape of tools/pipeline_bench.py --prisms: 65 536 scenes of two obstacle prisms, N = 71 knots, O = 5
strips.  HIP events, median of --reps launches each, the two alternating.  The forward WRITES O * N * 32 bytes per scene, the
backward READS them (the two cotangent arrays): the yardstick of the backward is the forward's time.  Reports backward /
forward and each kernel's fraction of the HBM peak on those bytes.  Writes profiles/prism_vjp_bench.json.

    python tools/prism_vjp_bench.py [--batch 65536] [--reps 20]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def scenes(B, seed=11):
    """tools/pipeline_bench.py --prisms: a slower car ahead in the ego's lane, one beside."""
    rng = np.random.default_rng(seed)
    pr = np.zeros((B, 2, 8))
    pr[:, 0, :7] = np.stack([rng.uniform(18, 30, B), np.full(B, 1.2), np.zeros(B), rng.uniform(3, 5, B), np.zeros(B), np.full(B, 4.0), np.ones(B)], 1)
    pr[:, 1, :7] = np.stack([rng.uniform(5, 15, B), np.full(B, 4.2), np.zeros(B), rng.uniform(5, 7, B), np.zeros(B), np.full(B, 4.0), np.ones(B)], 1)
    return pr


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--knots", type=int, default=71)
    ap.add_argument("--strips", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prism_vjp_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from spectral_amd.native import CRoad
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0); d = solver.device
    B, N, O, P = a.batch, a.knots, a.strips, 2
    pr = torch.from_numpy(scenes(B)).to(d)
    sb = torch.empty((B, O, N, 2), dtype=torch.float64, device=d); lb = torch.empty_like(sb)
    ns = torch.empty(B, dtype=torch.int32, device=d)
    g = torch.Generator(device=d).manual_seed(0)
    sbar = torch.randn(sb.shape, generator=g, dtype=torch.float64, device=d); lbar = torch.randn(sb.shape, generator=g, dtype=torch.float64, device=d)
    out = torch.empty((B, P, 8), dtype=torch.float64, device=d)
    road = CRoad.reference()
    stream = torch.cuda.current_stream(d).cuda_stream
    fwd = lambda: solver.ctx.prism_bounds_device(B, P, N, road, pr, O, sb, lb, ns, stream=stream)
    bwd = lambda: solver.ctx.prism_bounds_vjp_device(B, P, N, road, pr, O, sbar, lbar, out, stream=stream)
    for _ in range(3):
        fwd(); bwd()
    torch.cuda.synchronize()
    tf, tb = [], []
    for _ in range(a.reps):
        for run, t in ((fwd, tf), (bwd, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record(); torch.cuda.synchronize(); t.append(e0.elapsed_time(e1))
    f_ms, b_ms = float(np.median(tf)), float(np.median(tb))
    per_scene = O * N * 32
    gbs = lambda ms: per_scene * B / (ms * 1e-3) / 1e9
    grads = out.cpu().numpy()
    res = {"workload": "%d scenes of two obstacle prisms, N = %d, O = %d (tools/pipeline_bench.py --prisms)" % (B, N, O),
           "reps": a.reps, "forward_ms": f_ms, "forward_min_ms": float(np.min(tf)), "backward_ms": b_ms, "backward_min_ms": float(np.min(tb)),
           "backward_over_forward": b_ms / f_ms, "bytes_per_scene": per_scene,
           "forward_roofline": {"bound": "hbm (written)", "achieved": gbs(f_ms), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs(f_ms) / HBM_PEAK_GBS},
           "roofline": {"bound": "hbm (read)", "achieved": gbs(b_ms), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs(b_ms) / HBM_PEAK_GBS},
           "mean_strips": float(ns.cpu().numpy().mean()),
           "forward_hash": hashlib.sha256(sb.cpu().numpy().tobytes() + lb.cpu().numpy().tobytes()).hexdigest()[:16],
           "backward_hash": hashlib.sha256(grads.tobytes()).hexdigest()[:16],
           "nonzero_gradient_entries_per_scene": float((grads != 0).sum()) / B}
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1); fh.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
