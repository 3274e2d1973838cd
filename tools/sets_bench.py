#!/usr/bin/env python3
"""A parameter set per candidate (btrapz_solve_sets_device) against the one-set entry points, time of the whole solve
call by HIP events:
  g1       the bench batch (scenario_1 x 20) through the sets path with ONE set against btrapz_solve_batch_device, both
           in the same pinned form (cap_iter = -1, compact = -1, lean = 1): the price of the bucketing;
  sweep14  14 logged weight rows, the batch split 14 ways, in one launch against 14 launches;
  config5  128 agents x 512 candidates x 20 segments, warm-started (x0 from eval_states, multipliers kept), a ds_ref and
           limits per agent (128 sets) against the same solve with one set -- each warm-started from ITS OWN cold solve,
           so both solve their own problem from their own start (mean iterations reported beside the times).
Every time is measured --repeat times (runs of --reps solves each, interleaved between the two sides of a comparison):
median, min and max per side, and the ratio of the medians.  One JSON object on stdout.

    python tools/sets_bench.py [--batch 65536] [--reps 5] [--repeat 5]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def compare(a, b, reps, repeat):
    """Interleaved runs of the two sides: their median / min / max ms and median(b) / median(a)."""
    ta, tb = [], []
    for _ in range(repeat):
        ta.append(timed(a, reps)); tb.append(timed(b, reps))
    st = lambda t: dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))
    return st(ta), st(tb), float(np.median(tb) / np.median(ta))


def weight_rows(n):
    rows = []
    for line in open(os.path.join(ROOT, "tests", "golden", "inputs", "all_weights.txt")):
        try:
            v = [float(t) for t in line.split()]
        except ValueError:
            continue
        if len(v) >= 10:
            rows.append(v[:10])
    return rows[:n]


def main(argv=None):
    import torch
    from spectral_amd import layout as L
    from spectral_amd import synth
    from spectral_amd.solver import BatchSolver
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args(argv)
    solver = BatchSolver(0)
    dev = solver.device
    pin = dict(cap_iter=-1, compact=-1, lean=1)
    out = dict(tool="sets_bench", device=torch.cuda.get_device_name(0), batch=args.batch, reps=args.reps, repeat=args.repeat)

    batch, sh = synth.make_scenario1_batch(args.batch, 20)
    db = solver.upload(batch)
    zeros = torch.zeros(batch.B, dtype=torch.int32, device=dev)
    t_uni, t_g1, r = compare(lambda: solver.solve(db, sh, split=-1, **pin), lambda: solver.solve_sets(db, [sh], zeros, **pin),
                             args.reps, args.repeat)
    out["g1"] = dict(uniform=t_uni, sets=t_g1, ratio=r)

    rows = weight_rows(14)
    sets = [synth.shared_params(0, weights=w) for w in rows]
    G = len(sets)
    set_index = torch.from_numpy((np.arange(batch.B) % G).astype(np.int32)).to(dev)
    per = batch.B // G
    parts = [solver.upload(batch.slice(g * per, (g + 1) * per)) for g in range(G)]
    outs = [dict(ctrl=torch.empty((per, 12 * 20), dtype=torch.float64, device=dev),
                 cost=torch.empty(per, dtype=torch.float64, device=dev), status=torch.empty(per, dtype=torch.int32, device=dev),
                 iters=torch.empty(per, dtype=torch.int32, device=dev)) for _ in range(G)]

    def separate():
        for g in range(G):
            solver.solve(parts[g], sets[g], out=outs[g], split=-1, **pin)
    t_sep, t_one, r = compare(separate, lambda: solver.solve_sets(db, sets, set_index, **pin), args.reps, args.repeat)
    out["sweep14"] = dict(sets=G, separate_launches=t_sep, one_launch=t_one, ratio=r)

    AG, CAND = 128, 512
    b5, sh5 = synth.make_batch(AG * CAND, 20, config=5, agents=AG)
    d5 = solver.upload(b5)
    agent_sets = [dataclasses.replace(sh5, ds_ref=6.0 + 2.0 * a / AG, dds=(-2.0 - 0.5 * a / AG, 2.0 + 0.5 * a / AG),
                                      ddl=(-0.7 - 0.1 * a / AG, 0.7 + 0.1 * a / AG)) for a in range(AG)]
    si_agents = torch.from_numpy(np.repeat(np.arange(AG), CAND).astype(np.int32)).to(dev)
    si_one = torch.zeros(AG * CAND, dtype=torch.int32, device=dev)
    times = torch.from_numpy(np.cumsum(b5.seg[L.F_T], axis=1))
    res, calls = {}, {}
    for name, ss, si in (("one_set", [sh5], si_one), ("per_agent_sets", agent_sets, si_agents)):
        o = solver.solve_sets(d5, ss, si, keep_multipliers=True, **pin)          # its own cold solve ...
        x0 = solver.eval_states(d5, o["ctrl"], times)                           # ... is its own warm start
        lam = o["lam"].clone()
        torch.cuda.synchronize()
        calls[name] = (lambda ss=ss, si=si, x0=x0, lam=lam:
                       solver.solve_sets(d5, ss, si, warm=dict(x0=x0, lam=lam.clone()), keep_multipliers=True, **pin))
        w = calls[name]()
        torch.cuda.synchronize()
        res[name + "_solved"] = float((w["status"] > 0).float().mean().item())
        res[name + "_mean_iters"] = float(w["iters"].float().mean().item())
    # (the clone of the multipliers is in both timed calls: the warm start stays the same at every repetition)
    res["one_set"], res["per_agent_sets"], res["ratio"] = compare(calls["one_set"], calls["per_agent_sets"], args.reps, args.repeat)
    out["config5_warm"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
