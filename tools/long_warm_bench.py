#!/usr/bin/env python3
"""Warm starts of candidates of 65..256 segments (btrapz_solve_long_warm_device) against the cold long solve:
time of the whole solve call by HIP events and mean iterations, on uniform scenario_1 batches of 100 and 200 segments.

Per batch, four solves, timed in turn (cold, warm, cold, warm, ...: one event pair per call) --repeat times after two
untimed rounds:
    cold            the cold solve through btrapz_solve_batch_device (the long form as it was: form 2)
    warm_own        from its own solution: x0 = the joint states of the cold solve, lam = its multipliers
    warm_shifted    one replanning step: every line evaluated 0.1 s later, the initial state advanced along the previous
                    solution; x0 = the previous trajectory 0.1 s later, lam = the previous multipliers
    cold_shifted    the cold solve of that shifted problem, for comparison
One JSON object on stdout and, with --out, in a file.  A measurement, not a target.

    python tools/long_warm_bench.py [--batch 4096] [--segments 100,200] [--repeat 20] [--out profiles/long_warm_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shifted(batch, new_init, d):
    """The batch one replanning step later (tests/test_gpu_long_warm.py::test_warm_start_on_the_shifted_problem)."""
    from spectral_amd import layout as L
    nb = batch.slice(0, batch.B)
    seg = nb.seg.copy()
    for bias, skew in ((L.F_DOWN_BIAS, L.F_DOWN_SKEW), (L.F_UPP_BIAS, L.F_UPP_SKEW), (L.F_L_DOWN_BIAS, L.F_L_DOWN_SKEW),
                       (L.F_L_UPP_BIAS, L.F_L_UPP_SKEW), (L.F_X_BIAS, L.F_X_SKEW), (L.F_Y_BIAS, L.F_Y_SKEW)):
        seg[bias] = seg[bias] + seg[skew] * d
    nb.seg = seg
    nb.init = np.concatenate([new_init[:, 0, 0], new_init[:, 1, 0]], axis=1)
    return nb


def main(argv=None):
    import torch
    from spectral_amd import layout as L
    from spectral_amd import native, synth
    from spectral_amd.solver import BatchSolver
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--segments", default="100,200")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--shift", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    solver = BatchSolver(0)
    dev = torch.device("cuda:0")
    B, d = a.batch, a.shift
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "repeat": a.repeat, "shift_s": d, "workload": "synth.make_scenario1_batch(B, S, 0)",
           "timing": "HIP events around each solve call, the four solves in turn, two untimed rounds first",
           "kernel_source_hash": native.kernel_source_hash(), "cases": {}}
    for S in [int(s) for s in a.segments.split(",")]:
        batch, sh = synth.make_scenario1_batch(B, S, 0)
        db = solver.upload(batch)
        res = lambda: solver.new_result(B, S)        # (a result dict per solve: nothing is overwritten between the rounds)
        prev = solver.solve_long(db, sh, keep_multipliers=True, out=res())
        lam = prev["lam"]
        times = torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1))
        x0_own = solver.eval_states(db, prev["ctrl"], times)
        x0_next = solver.eval_states(db, prev["ctrl"], times + d)
        new_init = solver.eval_states(db, prev["ctrl"], torch.full((B, 1), d, dtype=torch.float64)).cpu().numpy()
        ndb = solver.upload(shifted(batch, new_init, d))
        outs = {k: res() for k in ("cold", "warm_own", "warm_shifted", "cold_shifted")}
        solves = [("cold", lambda: solver.solve(db, sh, out=outs["cold"])),
                  ("warm_own", lambda: solver.solve_long(db, sh, warm=dict(x0=x0_own, lam=lam), out=outs["warm_own"])),
                  ("warm_shifted", lambda: solver.solve_long(ndb, sh, warm=dict(x0=x0_next, lam=lam), out=outs["warm_shifted"])),
                  ("cold_shifted", lambda: solver.solve(ndb, sh, out=outs["cold_shifted"]))]
        ms = {k: [] for k, _ in solves}
        forms = {}
        for rnd in range(a.repeat + 2):
            for k, call in solves:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                torch.cuda.synchronize(dev)
                forms[k] = solver.ctx.last_solve_form()
                if rnd >= 2:
                    ms[k].append(e0.elapsed_time(e1))
        host = {k: {f: v.cpu().numpy() for f, v in o.items()} for k, o in outs.items()}
        rec = {}
        for k, _ in solves:
            ref = host["cold" if k in ("cold", "warm_own") else "cold_shifted"]
            ok = ref["status"] > 0
            r = host[k]
            err = np.abs(r["ctrl"][ok] - ref["ctrl"][ok]).max(axis=1) / np.abs(ref["ctrl"][ok]).max(axis=1)
            rec[k] = {"solve_ms_median": float(np.median(ms[k])), "solve_ms_min": float(np.min(ms[k])), "solve_ms_max": float(np.max(ms[k])),
                      "mean_iterations": float(r["iters"][ok].mean()), "max_iterations": int(r["iters"][ok].max()), "form": forms[k],
                      "accepted": int((r["status"] > 0).sum()), "accepted_by_cold": int(ok.sum()),
                      "same_accepted_set": bool(np.array_equal(r["status"] > 0, ok)), "max_rel_err_vs_cold": float(err.max())}
        rec["warm_own_over_cold"] = rec["warm_own"]["solve_ms_median"] / rec["cold"]["solve_ms_median"]
        rec["warm_shifted_over_cold_shifted"] = rec["warm_shifted"]["solve_ms_median"] / rec["cold_shifted"]["solve_ms_median"]
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
