#!/usr/bin/env python3
"""The forward-mode derivatives of the prism and corridor stages (btrapz_prism_bounds_jvp_device,
btrapz_corridor_batch_jvp_device) beside their forwards, each stage timed in ONE run with the launches alternating: HIP
events, median of --reps launches each.
  prism run:    65 536 scenes of two obstacle prisms, N = 71, O = 5 (tools/prism_vjp_bench.py's scenes): forward, JVP at T = 1
                and T = 12.  The forward WRITES O * N * 32 bytes per scene, the JVP T times that: reported as GB/s written and
                as a fraction of the HBM peak, beside the forward's figure.
  corridor run: 65 536 jittered copies of c_road_s1_3.txt (N = 71, 3 obstacles; tools/corridor_vjp_bench.py's batch): forward,
                backward (for scale) and JVP at T = 1 and T = 12.
Measured, reported, not asserted.  Writes profiles/stage_jvp_bench.json.

    python tools/stage_jvp_bench.py [--batch 65536] [--reps 20] [--tangents 1 12]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0


def alternating(torch, runs, reps):
    """{name: (median ms, min ms)} of the launches `runs` {name: callable}, alternating in one loop."""
    for _ in range(3):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record(); torch.cuda.synchronize(); t[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in t.items()}


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def prism_run(torch, solver, B, N, O, Ts, reps):
    from prism_vjp_bench import scenes
    from spectral_amd.native import CRoad
    d, P = solver.device, 2
    pr = torch.from_numpy(scenes(B)).to(d)
    sb = torch.empty((B, O, N, 2), dtype=torch.float64, device=d); lb = torch.empty_like(sb)
    ns = torch.empty(B, dtype=torch.int32, device=d)
    road = CRoad.reference()
    stream = torch.cuda.current_stream(d).cuda_stream
    g = torch.Generator(device=d).manual_seed(0)
    runs = {"forward": lambda: solver.ctx.prism_bounds_device(B, P, N, road, pr, O, sb, lb, ns, stream=stream)}
    bufs = {}
    for T in Ts:
        pd = torch.randn((T, B, P, 8), generator=g, dtype=torch.float64, device=d)
        bufs[T] = (pd, torch.empty((T, B, O, N, 2), dtype=torch.float64, device=d), torch.empty((T, B, O, N, 2), dtype=torch.float64, device=d))
        runs["jvp_T%d" % T] = (lambda T=T: solver.ctx.prism_bounds_jvp_device(B, P, N, road, pr, O, T, bufs[T][0], bufs[T][1], bufs[T][2], stream=stream))
    ms = alternating(torch, runs, reps)
    per_scene = O * N * 32
    gbs = lambda bytes_, t: bytes_ * B / (t * 1e-3) / 1e9
    out = {"workload": "%d scenes of two obstacle prisms, N = %d, O = %d" % (B, N, O), "bytes_written_per_scene_forward": per_scene,
           "forward_ms": ms["forward"][0], "forward_min_ms": ms["forward"][1],
           "forward_roofline": {"bound": "hbm (written)", "achieved": gbs(per_scene, ms["forward"][0]), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": gbs(per_scene, ms["forward"][0]) / HBM_PEAK_GBS},
           "forward_hash": digest(sb, lb), "mean_strips": float(ns.cpu().numpy().mean()), "jvp": {}}
    for T in Ts:
        m, mn = ms["jvp_T%d" % T]
        out["jvp"]["T%d" % T] = {"ms": m, "min_ms": mn, "over_forward": m / ms["forward"][0], "over_T_forwards": m / (T * ms["forward"][0]),
                                 "roofline": {"bound": "hbm (written)", "achieved": gbs(T * per_scene, m), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                              "frac": gbs(T * per_scene, m) / HBM_PEAK_GBS},
                                 "hash": digest(bufs[T][1][:1, :1024], bufs[T][2][:1, :1024])}
    return out


def corridor_run(torch, solver, B, Ts, reps, name="c_road_s1_3", variant=0, st=16):
    from spectral_amd import knots, layout as L
    from spectral_amd.native import KNOT_GRADS
    d = solver.device
    kb = knots.jittered(knots.parse_corridor_file(os.path.join(ROOT, "tests", "golden", "inputs", name + ".txt")), B, seed=3)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(d)
    ins = [f(kb.s_bounds), f(kb.l_bounds), f(kb.ds_bounds), f(kb.dl_bounds), f(kb.s_ref), f(kb.l_ref)]
    seg = torch.zeros((L.NUM_SEG_FIELDS, B, st), dtype=torch.float64, device=d)
    cnt = torch.zeros(B, dtype=torch.int32, device=d); ref_end = torch.zeros((B, 2), dtype=torch.float64, device=d)
    dl10 = torch.zeros((B, 10), dtype=torch.float64, device=d)
    g = torch.Generator(device=d).manual_seed(0)
    bars = [torch.randn(t.shape, generator=g, dtype=torch.float64, device=d) for t in (seg, ref_end, dl10)]
    grads = {k: torch.empty_like(t) for k, t in zip(KNOT_GRADS, ins)}
    stream = torch.cuda.current_stream(d).cuda_stream
    shape = (variant, B, kb.N, kb.num_obs, kb.delta)
    runs = {"forward": lambda: solver.ctx.corridor_batch_device(*shape, *ins, st, seg, cnt, ref_end, dl10, stream=stream),
            "backward": lambda: solver.ctx.corridor_batch_vjp_device(*shape, *ins, st, *bars, grads, stream=stream)}
    bufs = {}
    for T in Ts:
        tan = {k: torch.randn((T,) + tuple(t.shape), generator=g, dtype=torch.float64, device=d) for k, t in zip(KNOT_GRADS, ins)}
        outs = (torch.empty((T, L.NUM_SEG_FIELDS, B, st), dtype=torch.float64, device=d), torch.empty((T, B, 2), dtype=torch.float64, device=d),
                torch.empty((T, B, 10), dtype=torch.float64, device=d))
        bufs[T] = (tan, outs)
        runs["jvp_T%d" % T] = (lambda T=T: solver.ctx.corridor_batch_jvp_device(*shape, *ins, st, T, bufs[T][0], *bufs[T][1], stream=stream))
    ms = alternating(torch, runs, reps)
    c = cnt.cpu().numpy()
    in_bytes = (4 * kb.num_obs + 6) * kb.N * 8
    out_bytes = (L.NUM_SEG_FIELDS * st + 12) * 8
    out = {"workload": "jittered %s.txt, %d candidates, N = %d, %d obstacles, variant %d, seg_stride %d" % (name, B, kb.N, kb.num_obs, variant, st),
           "forward_ms": ms["forward"][0], "forward_min_ms": ms["forward"][1], "backward_ms": ms["backward"][0], "backward_min_ms": ms["backward"][1],
           "forward_hash": digest(seg, cnt, ref_end, dl10), "mean_segments": float(np.mean(np.maximum(c, 0))),
           "input_bytes_per_candidate": in_bytes, "output_bytes_per_candidate_and_tangent": out_bytes, "jvp": {}}
    for T in Ts:
        m, mn = ms["jvp_T%d" % T]
        moved = in_bytes + T * out_bytes        # the inputs once, every output entry written once; the tangents are read sparsely
        out["jvp"]["T%d" % T] = {"ms": m, "min_ms": mn, "over_forward": m / ms["forward"][0], "over_backward": m / ms["backward"][0],
                                 "roofline": {"bound": "hbm", "achieved": moved * B / (m * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                              "frac": moved * B / (m * 1e-3) / 1e9 / HBM_PEAK_GBS},
                                 "hash": digest(bufs[T][1][0][:1, :, :1024], bufs[T][1][1][:1, :1024])}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--knots", type=int, default=71)
    ap.add_argument("--strips", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_jvp_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0),
           "prism": prism_run(torch, solver, a.batch, a.knots, a.strips, a.tangents, a.reps)}
    torch.cuda.empty_cache()
    res["corridor"] = corridor_run(torch, solver, a.batch, a.tangents, a.reps)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1); fh.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
