#!/usr/bin/env python3
"""Gradients and directional derivatives of solves with 65..256 segments (btrapz_solve_long_vjp_device / _jvp_device, DESIGN.md
3.16) against the forward solve they differentiate: time of each call by HIP events, on uniform scenario_1 batches of 100 and
200 segments (the batches of tools/long_warm_bench.py).

Per batch, four calls, timed in turn (one event pair per call) --repeat times after two untimed rounds:
    solve      the cold solve_long with its multipliers kept
    vjp        solve_long_vjp, dense ctrl_bar and cost_bar, all five gradient arrays
    jvp_1      solve_long_jvp, T = 1 tangent dense in all five input arrays, ctrl_dot and cost_dot
    jvp_12     the same with T = 12
One JSON object on stdout and, with --out, in a file.  A measurement, not a target.

    python tools/long_grad_bench.py [--batch 4096] [--segments 100,200] [--repeat 20] [--out profiles/long_grad_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import torch
    from spectral_amd import layout as L
    from spectral_amd import native, synth
    from spectral_amd.solver import BatchSolver
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--segments", default="100,200")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    solver = BatchSolver(0)
    dev = torch.device("cuda:0")
    B = a.batch
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "repeat": a.repeat, "workload": "synth.make_scenario1_batch(B, S, 0)",
           "timing": "HIP events around each call, the four calls in turn, two untimed rounds first; medians",
           "kernel_source_hash": native.kernel_source_hash(), "cases": {}}
    for S in [int(s) for s in a.segments.split(",")]:
        batch, sh = synth.make_scenario1_batch(B, S, 0)
        db = solver.upload(batch)
        o = solver.solve_long(db, sh, keep_multipliers=True, out=solver.new_result(B, S))
        gen = torch.Generator(device=dev).manual_seed(S)
        rnd_t = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev, generator=gen)
        xbar, cbar = rnd_t(B, 12 * S), rnd_t(B)
        tan = {T: dict(seg=rnd_t(T, L.NUM_SEG_FIELDS, B, S), init=rnd_t(T, B, 6), ref_end=rnd_t(T, B, 2), dl_bounds=rnd_t(T, B, 10),
                       shared=rnd_t(T, B, 20)) for T in (1, 12)}
        scratch = solver.new_result(B, S)
        calls = [("solve", lambda: solver.solve_long(db, sh, keep_multipliers=True, out=scratch)),
                 ("vjp", lambda: solver.solve_long_vjp(db, sh, o, xbar, cbar)),
                 ("jvp_1", lambda: solver.solve_long_jvp(db, sh, o, tan[1])),
                 ("jvp_12", lambda: solver.solve_long_jvp(db, sh, o, tan[12]))]
        ms = {k: [] for k, _ in calls}
        last = {}
        for rnd in range(a.repeat + 2):
            for k, call in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); last[k] = call(); e1.record()
                torch.cuda.synchronize(dev)
                if rnd >= 2:
                    ms[k].append(e0.elapsed_time(e1))
        st = o["status"].cpu().numpy()
        ok = (st == 1) | (st == 2)
        rec = {k: {"ms_median": float(np.median(v)), "ms_min": float(np.min(v)), "ms_max": float(np.max(v))} for k, v in ms.items()}
        rec["solve"]["mean_iterations"] = float(o["iters"].cpu().numpy()[ok].mean())
        rec["solved"] = int(ok.sum())
        for k in ("vjp", "jvp_1", "jvp_12"):
            rec[k + "_over_solve"] = rec[k]["ms_median"] / rec["solve"]["ms_median"]
        rec["jvp_ms_per_tangent_at_12"] = rec["jvp_12"]["ms_median"] / 12.0
        # the adjoint identity on tangent 0 of the T = 1 call, every solved candidate: the two timed results belong together
        g, j = last["vjp"], last["jvp_1"]
        lhs = (xbar * j["ctrl"][0]).sum(1) + cbar * j["cost"][0]
        mag = (xbar.abs() * j["ctrl"][0].abs()).sum(1) + cbar.abs() * j["cost"][0].abs()
        t1 = tan[1]
        rhs = (g["seg"] * t1["seg"][0]).sum((0, 2)) + sum((g[k] * t1[k][0]).sum(1) for k in ("init", "ref_end", "dl_bounds", "shared"))
        okt = torch.from_numpy(ok).to(dev)
        rec["adjoint_identity_worst"] = float(((lhs - rhs).abs()[okt] / mag[okt]).max())
        out["cases"]["scenario1 x %d" % S] = rec
        print("S=%d done" % S, file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return out


if __name__ == "__main__":
    main()
