"""spectral_amd.tune.fit_trajectory -- multi-start projected Adam on the ten weights with the gradient through
diff.solve + diff.sample -- against the reference's saved scenario_1 trajectories (tests/golden/ref_outputs/, inputs
under tests/golden/inputs/; the pairs tests/golden/weight_fit.json lists as fitted), starting from the bundled
weights.txt.  Per file: the loss at the start and the end, the per-column maximum deviation of the best start, the number
of solves and the wall time, beside the residual weight_fit.json records for the same file from the Nelder-Mead fit over
the CPU oracle.  --synthetic: a target sampled from a solve with known weights instead (the measured reduction factor of
the mean loss is what tests/test_gpu_states.py holds a third of).  A record, not a threshold.
--method lm: spectral_amd.tune.fit_trajectory_lm (Levenberg-Marquardt on the Jacobian of btrapz_solve_jvp_device) on the
same targets and starts; --steps then counts LM steps (default 25), and the record holds the JVP launches and the work
(candidates solved + candidates of JVP launches) as well.

    python tools/fit_trajectory.py --synthetic --out profiles/fit_trajectory.json
    python tools/fit_trajectory.py --method lm --synthetic --out profiles/fit_trajectory_lm.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
COLUMNS = ("s", "ds", "dds", "l", "dl", "ddl")


def saved_trajectory(path):
    """A saved file's rows t, s, l, ds, dl, dds, ddl -> [6, n] in the order s, ds, dds, l, dl, ddl."""
    import numpy as np
    a = np.loadtxt(path)
    return a[:, [1, 3, 5, 2, 4, 6]].T.copy()


def synthetic_target(solver, kb, W, variant=0):
    import torch
    from spectral_amd import diff, tune
    rec = tune.replicated_record(solver, kb, variant, 1)
    o = solver.solve_sets_ragged(rec, [tune.shared_of(W, kb.header, kb.delta, variant)],
                                 torch.zeros(1, dtype=torch.int32, device=solver.device))
    with torch.no_grad():
        traj, npts = diff.sample(o["ctrl"], rec["seg"], rec["init"], solver, seg_count=rec["seg_count"], delta=kb.delta)
    return traj[0, :, :int(npts[0])].cpu().numpy()


def run(solver, kb, variant, target, W, starts, steps, seed, spread, method="adam"):
    import torch
    from spectral_amd import tune
    fit = tune.fit_trajectory_lm if method == "lm" else tune.fit_trajectory
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fit(solver, kb, variant, target, W, starts=starts, steps=steps, seed=seed, spread=spread)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    extra = {}
    if method == "lm":
        extra = {"jvp_launches": r["jvp_launches"], "work": r["solves"] + starts * r["jvp_launches"],
                 "accepted_steps_per_start": [int(v) for v in r["accepted"]], "loss_mean_per_step": [float(v) for v in r["means"]]}
    return {**extra, "starts": starts, "steps": steps, "solves": r["solves"], "wall_s": wall, "samples_compared": r["samples"],
            "loss_start_mean": r["start_mean"], "loss_final_mean": r["final_mean"], "loss_best": r["best"],
            "reduction": r["start_mean"] / r["final_mean"] if r["final_mean"] > 0 else float("inf"),
            "max_abs_dev_of_best_start": dict(zip(COLUMNS, (float(v) for v in r["max_dev"]))),
            "best_weights": [float(v) for v in r["weights"][int(r["losses"].argmin())]]}


def main():
    import numpy as np
    from spectral_amd import knots
    from spectral_amd.solver import BatchSolver
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=None, help="default: 100 (adam), 25 (lm)")
    ap.add_argument("--method", choices=("adam", "lm"), default="adam")
    ap.add_argument("--synthetic", action="store_true", help="also fit a target sampled from a solve with known weights")
    ap.add_argument("--no-files", action="store_true", help="skip the saved trajectories")
    a = ap.parse_args()
    if a.steps is None:
        a.steps = 25 if a.method == "lm" else 100
    W = np.loadtxt(os.path.join(GOLD, "inputs", "weights.txt"))[:10]
    solver = BatchSolver(0)
    res = {"method": "tune.fit_trajectory_lm: Levenberg-Marquardt on the log-weights, one JVP launch of ten tangents and one "
                     "trial solve per step, every start a parameter set of one launch" if a.method == "lm" else
                     "tune.fit_trajectory: Adam on the log-weights, lr 0.05, every start a parameter set of one launch",
           "columns": list(COLUMNS)}
    kb1 = knots.parse_corridor_file(os.path.join(GOLD, "inputs", "c1.txt"))
    run(solver, kb1, 0, synthetic_target(solver, kb1, W), W, a.starts, 1, 0, 0.3, a.method)   # (warm-up: first calls)
    if a.synthetic:
        res["synthetic"] = dict(run(solver, kb1, 0, synthetic_target(solver, kb1, W), W, a.starts, a.steps, 6, float(np.log(1.3)), a.method),
                                input="tests/golden/inputs/c1.txt", variant=0,
                                target="sampled from the solve with tests/golden/inputs/weights.txt; starts at +-ln 1.3 per log-weight")
    if not a.no_files:
        fit = json.load(open(os.path.join(GOLD, "weight_fit.json")))
        res["files"] = {}
        for name, info in sorted(fit["targets"].items()):
            if not info.get("fitted"):
                continue
            kb = knots.parse_corridor_file(os.path.join(GOLD, "inputs", info["input"] + ".txt"))
            target = saved_trajectory(os.path.join(GOLD, "ref_outputs", name))
            r = run(solver, kb, int(info["variant"]), target, W, a.starts, a.steps, 0, 0.3, a.method)
            nm = fit["fits"].get(name, {})
            r["nelder_mead_max_abs_diff"] = {k: nm[k]["max_abs_diff"] for k in ("s", "l", "exact") if k in nm}
            r["input"], r["variant"], r["rows_saved"] = info["input"], int(info["variant"]), int(target.shape[1])
            res["files"][name] = r
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
