#!/usr/bin/env python3
"""One replanning step of 16 agents with 256 candidates each at 100 and 200 segments, every agent with its own ds_ref and
acceleration limits, warm-started from the previous plan, with the rescue pass:

    sets      ONE btrapz_solve_long_sets_device call over the 4 096 candidates (solver.solve_long_sets, elastic = 1)
    per_agent what a caller had to do before it: 16 btrapz_solve_long_rescue_device calls, one per agent's slice
              (solver.solve_long_rescue, elastic = 1)

Workload: synth.make_scenario1_batch(B, S, 0); the previous plan is the cold sets solve with its multipliers kept; the step
evaluates every line --shift seconds later, moves the initial state along the previous solution and starts from the previous
trajectory that much later (tools/long_warm_bench.py); then every 1/--damaged-th candidate's initial lateral position is put
--gap below its first lower line (tools/long_rescue_bench.py): it stalls and is rescued.

The two sides must agree bit for bit on ctrl, cost, status and iters: checked before anything is timed, and the bench refuses to
time results that differ.  Timing: HIP events around the one call and around the sixteen, the two in turn in one process,
median / min / max of --repeat rounds after --warmup untimed ones.  A measurement, not a target.  One JSON object on stdout
and, with --out, in a file.

    python tools/long_sets_bench.py [--batch 4096] [--agents 16] [--segments 100,200] [--repeat 20] [--warmup 3] [--out profiles/long_sets_bench.json]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    import torch
    from long_warm_bench import shifted
    from spectral_amd import layout as L
    from spectral_amd import native, synth
    from spectral_amd.solver import BatchSolver, DeviceBatch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--segments", default="100,200")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shift", type=float, default=0.1)
    ap.add_argument("--damaged", type=float, default=0.01)
    ap.add_argument("--gap", type=float, default=0.004)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    solver = BatchSolver(0)
    dev = torch.device("cuda:0")
    B, G, d = a.batch, a.agents, a.shift
    per = B // G
    assert per * G == B
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "agents": G, "repeat": a.repeat, "warmup": a.warmup, "shift_s": d,
           "damaged_fraction": a.damaged, "gap": a.gap,
           "workload": "synth.make_scenario1_batch(B, S, 0), agent g = candidates [g B / agents, (g + 1) B / agents) with ds_ref + 0.25 g and dds widened by 0.05 g; "
                       "one replanning step, warm-started; every 1/damaged-th candidate's initial l below its first lower l line by gap",
           "timing": "HIP events around the one sets call and around the per-agent calls, the two in turn, median / min / max",
           "kernel_source_hash": native.kernel_source_hash(), "cases": {}}
    idx = torch.from_numpy((np.arange(B) // per).astype(np.int32)).to(dev)
    for S in [int(s) for s in a.segments.split(",")]:
        batch, sh = synth.make_scenario1_batch(B, S, 0)
        sets = [dataclasses.replace(sh, ds_ref=sh.ds_ref + 0.25 * g, dds=(sh.dds[0] - 0.05 * g, sh.dds[1] + 0.05 * g)) for g in range(G)]
        db = solver.upload(batch)
        prev = solver.solve_long_sets(db, sets, idx, keep_multipliers=True, out=solver.new_result(B, S))
        lam = prev["lam"]
        times = torch.from_numpy(np.cumsum(batch.seg[L.F_T], axis=1))
        x0 = solver.eval_states(db, prev["ctrl"], times + d)
        new_init = solver.eval_states(db, prev["ctrl"], torch.full((B, 1), d, dtype=torch.float64)).cpu().numpy()
        nb = shifted(batch, new_init, d)
        hit = np.arange(0, B, max(1, int(round(1.0 / a.damaged))))
        nb.init[hit, 3] = nb.seg[L.F_L_DOWN_BIAS, hit, 0] - a.gap
        ndb = solver.upload(nb)
        # the agents' slices, made once (a caller that solves agent by agent holds them that way)
        slices = []
        for g in range(G):
            r = slice(g * per, (g + 1) * per)
            slices.append((DeviceBatch.from_tensors(ndb.seg[:, r].contiguous(), ndb.init[r].contiguous(), ndb.ref_end[r].contiguous(),
                                                    ndb.dl_bounds[r].contiguous()),
                           dict(x0=x0[r].contiguous(), lam=lam[:, :, r].contiguous()), solver.new_result(per, S)))
        o_sets = solver.new_result(B, S)

        def run_sets():
            solver.solve_long_sets(ndb, sets, idx, warm=dict(x0=x0, lam=lam), elastic=1, out=o_sets)

        def run_agents():
            for g, (sb, w, o) in enumerate(slices):
                solver.solve_long_rescue(sb, sets[g], warm=w, out=o)

        run_sets(); run_agents()
        torch.cuda.synchronize(dev)
        form = solver.ctx.last_solve_form()
        hs = {k: v.cpu().numpy() for k, v in o_sets.items()}
        ha = {k: np.concatenate([o[k].cpu().numpy() for _, _, o in slices]) for k in hs}
        same = {k: bool(np.array_equal(hs[k].view(np.uint8) if hs[k].dtype == np.float64 else hs[k],
                                       ha[k].view(np.uint8) if ha[k].dtype == np.float64 else ha[k])) for k in hs}
        if not all(same.values()):
            raise SystemExit("S=%d: the sets call and the per-agent calls differ: %s -- nothing timed" % (S, same))
        solves = [("sets", run_sets), ("per_agent", run_agents)]
        ms = {k: [] for k, _ in solves}
        for rnd in range(a.repeat + a.warmup):
            for k, call in solves:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); call(); e1.record()
                torch.cuda.synchronize(dev)
                if rnd >= a.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        st = hs["status"]
        stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
        rec = {"ms": {k: stat(v) for k, v in ms.items()}, "form_sets": form, "bit_equal": same,
               "sets_over_per_agent": float(np.median(ms["sets"]) / np.median(ms["per_agent"])),
               "sets_over_per_agent_range": [float(np.min(ms["sets"]) / np.max(ms["per_agent"])), float(np.max(ms["sets"]) / np.min(ms["per_agent"]))],
               "damaged": int(len(hit)), "solved": int((st == 1).sum()), "rescued": int((st == 2).sum()), "refused": int((st < 0).sum()),
               "mean_iterations_solved": float(hs["iters"][st == 1].mean()) if (st == 1).any() else None}
        out["cases"]["scenario1 x %d" % S] = rec
        print("S=%d done" % S, file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return out


if __name__ == "__main__":
    main()
