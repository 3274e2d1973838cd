#!/usr/bin/env python3
"""What the rescue pass of candidates of 193..256 segments costs (btrapz_solve_long_rescue_device): the whole
solve call by HIP events, with and without it, on uniform scenario_1 batches of 200 and 256 segments of which 1 % have no
feasible trajectory (the initial lateral position 0.004 below the first segment's lower line: least violation 0.004, rescued).

Per batch two solves, timed in turn (plain, rescue, plain, rescue, ...: one event pair per call), the median of --repeat
rounds after --warmup untimed ones:
    plain     solver.solve_long(...)            btrapz_solve_long_warm_device, cold start: the call and the kernel that were there
    rescue    solver.solve_long_rescue(...)     the same launch, then the rescue launch: 2 B workgroups of which those of the
                                                stalled axis problems work and the others leave at once
The expectation is "one launch plus the stalled problems".  One JSON object on stdout and, with --out, in a file.  A measurement,
not a target.

    python tools/long_rescue_bench.py [--batch 4096] [--segments 200,256] [--repeat 30] [--warmup 5] [--out profiles/long_rescue_bench.json]
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
    ap.add_argument("--segments", default="200,256")
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--damaged", type=float, default=0.01)
    ap.add_argument("--gap", type=float, default=0.004)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    solver = BatchSolver(0)
    dev = torch.device("cuda:0")
    B = a.batch
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "repeat": a.repeat, "warmup": a.warmup, "damaged_fraction": a.damaged,
           "gap": a.gap, "workload": "synth.make_scenario1_batch(B, S, 0), every 1/damaged-th candidate's initial l below its first lower l line by gap",
           "timing": "HIP events around each solve call, plain and rescue in turn, median",
           "kernel_source_hash": native.kernel_source_hash(), "cases": {}}
    for S in [int(s) for s in a.segments.split(",")]:
        batch, sh = synth.make_scenario1_batch(B, S, 0)
        batch = L.Batch(B=B, S=S, seg=batch.seg.copy(), init=batch.init.copy(), ref_end=batch.ref_end.copy(), dl_bounds=batch.dl_bounds.copy())
        hit = np.arange(0, B, max(1, int(round(1.0 / a.damaged))))
        batch.init[hit, 3] = batch.seg[L.F_L_DOWN_BIAS, hit, 0] - a.gap
        db = solver.upload(batch)
        outs = {k: solver.new_result(B, S) for k in ("plain", "rescue")}
        solves = [("plain", lambda: solver.solve_long(db, sh, out=outs["plain"])),
                  ("rescue", lambda: solver.solve_long_rescue(db, sh, out=outs["rescue"]))]
        ms = {k: [] for k, _ in solves}
        forms = {}
        for rnd in range(a.repeat + a.warmup):
            for k, call in solves:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                torch.cuda.synchronize(dev)
                forms[k] = solver.ctx.last_solve_form()
                if rnd >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        r = {k: {n: v.cpu().numpy() for n, v in o.items()} for k, o in outs.items()}
        ok = r["plain"]["status"] > 0
        same = all(np.array_equal(r["rescue"][n][ok], r["plain"][n][ok]) for n in ("status", "cost", "ctrl", "iters"))
        stalled = int((r["plain"]["status"] == -2).sum())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out["cases"][str(S)] = {
            "ms": med, "ms_min": {k: float(np.min(v)) for k, v in ms.items()}, "forms": forms,
            "rescue_over_plain": med["rescue"] / med["plain"], "rescue_pass_ms": med["rescue"] - med["plain"],
            "damaged": int(len(hit)), "plain_accepted": int(ok.sum()), "plain_stalled": stalled,
            "rescued": int(((r["rescue"]["status"] == 2) & ~ok).sum()), "rescue_refused": int((r["rescue"]["status"] < 0).sum()),
            "answered_candidates_bit_identical": bool(same),
            "mean_iterations_plain": float(r["plain"]["iters"][ok].mean()),
            "mean_iterations_rescued": float(r["rescue"]["iters"][(r["rescue"]["status"] == 2) & ~ok].mean()) if ((r["rescue"]["status"] == 2) & ~ok).any() else None}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
