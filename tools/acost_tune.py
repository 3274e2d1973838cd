"""The reference's weight sweep, on the device, on one bundled input (tests/golden/inputs/c1.txt), two ways:
  (a) random rows U(0, 50)^10, --rows-per-launch per btrapz_solve_sets_device launch, scored by btrapz_traj_cost_device;
  (b) multi-start projected Adam on the weights, every start a parameter set of one launch, gradients through
      diff.solve + diff.traj_cost (spectral_amd.tune.descend).
Reports the best a_cost against the number of solves and the wall time, and rows / s against a find_traj loop over the
same rows on a subset.

The trapezoid objective is degenerate: every term of its a_cost carries one of the weights it is scored with, and the
corridor, speed, acceleration and jerk rows bound each term, so a_cost goes to 0 as those weights shrink -- minimising it
over the weights the solve uses only shrinks them (the reference's sweep has the same property, held off only by its box).
Trapezoid runs are therefore scored with FIXED weights (--score-weights, default tests/golden/inputs/weights.txt); the
cuboid's a_cost has no weights and is used as is.

    python tools/acost_tune.py --out profiles/acost_tune.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def random_rows(solver, variant, n_rows, per_launch, score_w, seed):
    import numpy as np
    import torch
    from spectral_amd import knots, native
    from spectral_amd.tune import replicated_record, shared_of
    kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", "c1.txt"))
    rec = replicated_record(solver, kb, variant, per_launch)
    rng = np.random.default_rng(seed)
    W = rng.uniform(0, 50, (n_rows, 10))
    score = shared_of(score_w, kb.header, kb.delta, variant)
    idx = torch.arange(per_launch, dtype=torch.int32, device=solver.device)
    best, curve, costs = np.inf, [], []
    warm = solver.solve_sets_ragged(rec, [score] * per_launch, idx)   # (warm-up: first calls)
    solver.traj_cost(rec, score, warm["ctrl"], kb.s_ref[0], kb.l_ref[0], status=warm["status"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lo in range(0, n_rows, per_launch):
        sets = [shared_of(w, kb.header, kb.delta, variant) for w in W[lo:lo + per_launch]]
        o = solver.solve_sets_ragged(rec, sets, idx)
        # scored with the fixed weights (trapezoid) / none (cuboid): one set for every candidate
        a, _ = solver.traj_cost(rec, score, o["ctrl"], kb.s_ref[0], kb.l_ref[0], status=o["status"])
        c = a.cpu().numpy()
        costs.append(c)
        best = min(best, float(c.min()))
        curve.append({"solves": lo + per_launch, "best": best, "wall_s": time.perf_counter() - t0})
    wall = time.perf_counter() - t0
    # find_traj over the first rows (scored with their own weights: what the reference's loop returns; timing only)
    n_ft = 64
    t1 = time.perf_counter()
    for w in W[:n_ft]:
        native.find_traj_mem(variant, list(w) + [1], kb)
    ft = time.perf_counter() - t1
    allc = np.concatenate(costs)
    return {"rows": n_rows, "rows_per_launch": per_launch, "wall_s": wall, "rows_per_s": n_rows / wall,
            "find_traj_rows_per_s": n_ft / ft, "find_traj_rows": n_ft, "best": best, "curve": curve,
            "scored": int(np.isfinite(allc).sum()), "best_at_solves": lambda n: float(np.min(allc[:n]))}


def main():
    import numpy as np
    import torch
    from spectral_amd import knots
    from spectral_amd.solver import BatchSolver
    from spectral_amd.tune import descend
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--rows-per-launch", type=int, default=1024)
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--score-weights", default=os.path.join(GOLD, "inputs", "weights.txt"))
    a = ap.parse_args()
    score_w = np.loadtxt(a.score_weights)[:10]
    W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))[:10]
    kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", "c1.txt"))
    solver = BatchSolver(0)
    res = {"input": "tests/golden/inputs/c1.txt", "score_weights": score_w.tolist(),
           "note": "trapezoid a_cost scored with fixed weights (its objective over the solve's own weights is degenerate); "
                   "cuboid a_cost has no weights"}
    for variant, name in ((0, "trapezoid"), (1, "cuboid")):
        r = random_rows(solver, variant, a.rows, a.rows_per_launch, score_w, seed=variant)
        descend(solver, kb, variant, W, starts=a.starts, steps=1, seed=5, score_weights=score_w)   # (warm-up: first calls)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = descend(solver, kb, variant, W, starts=a.starts, steps=a.steps, seed=5, score_weights=score_w)
        torch.cuda.synchronize()
        gw = time.perf_counter() - t0
        at = r.pop("best_at_solves")
        res[name] = {"random": r,
                     "adam": {"starts": a.starts, "steps": a.steps, "solves": g["solves"], "wall_s": gw,
                              "start_mean": g["start_mean"], "final_mean": g["final_mean"],
                              "mean_reduction": 1 - g["final_mean"] / g["start_mean"], "best": g["best"],
                              "means": g["means"]},
                     "random_best_at_adam_solves": at(min(g["solves"], a.rows))}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
