#!/usr/bin/env python3
"""The schedules of the lean two-launch solve (btrapz_debug_set_schedule: -1 the two launches, 1 / 2 three launches with
the s / l axis first, 3 / 4 the s / l axis first and the other axis quiet, 0 the library's choice once it has seen a
solve) on the bench batches, all in memory order
(compact = -1): time of the whole solve call by HIP events, hand-over counts per axis, and whether the results are the
one-launch solve's bit for bit.  One JSON object on stdout.

    python tools/schedule_bench.py [--batch 65536] [--cap 6] [--reps 10]
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
    from spectral_amd import synth
    from spectral_amd.solver import BatchSolver
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--cap", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args(argv)
    solver = BatchSolver(0)
    dev = torch.device("cuda:0")
    out = {}
    cases = [("scenario1 x 20 trapezoid", lambda: synth.make_scenario1_batch(a.batch, 20, 0)),
             ("generic x 20 trapezoid", lambda: synth.make_batch(a.batch, 20, config=3)),
             ("scenario1 x 20 cuboid", lambda: synth.make_scenario1_batch(a.batch, 20, 1)),
             ("scenario1 x 10 trapezoid", lambda: synth.make_scenario1_batch(a.batch, 10, 0))]
    for label, make in cases:
        batch, sh = make()
        db = solver.upload(batch)
        kw = dict(split=-1, lean=1, compact=-1)
        o = solver.solve(db, sh, cap_iter=-1, **kw)
        torch.cuda.synchronize(dev)
        ref = {k: o[k].cpu().numpy().copy() for k in ("ctrl", "cost", "status", "iters")}
        ok = ref["status"] > 0
        rec = {}
        for mode in (-1, 1, 2, 3, 4, 0):
            solver.ctx.debug_set_schedule(mode)
            for _ in range(2):
                o = solver.solve(db, sh, cap_iter=a.cap, **kw)
                torch.cuda.synchronize(dev)      # (mode 0: the counts of the solve before have landed)
            best = 1e9
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    o = solver.solve(db, sh, cap_iter=a.cap, **kw)
                e1.record(); torch.cuda.synchronize(dev)
                best = min(best, e0.elapsed_time(e1) / a.reps)
            res = {k: o[k].cpu().numpy().copy() for k in ("ctrl", "cost", "status", "iters")}
            keys = solver.ctx.debug_resume_keys(a.batch)
            rec["mode_%d" % mode] = {
                "solve_ms": best, "launches": solver.ctx.debug_solve_launches(), "form": solver.ctx.last_solve_form(),
                "handed_over": [int((keys[0] > 0).sum()), int((keys[1] > 0).sum())],
                "bit_identical": bool(np.array_equal(ref["status"], res["status"]) and np.array_equal(ref["iters"], res["iters"]) and
                                      np.array_equal(ref["ctrl"][ok], res["ctrl"][ok]) and np.array_equal(ref["cost"], res["cost"]))}
        solver.ctx.debug_set_schedule(0)
        for m in ("mode_1", "mode_2", "mode_3", "mode_4", "mode_0"):
            rec[m]["ratio"] = rec[m]["solve_ms"] / rec["mode_-1"]["solve_ms"]
        out[label] = rec
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
