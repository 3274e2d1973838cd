"""Forward mode against reverse mode on BASELINE config 3's batch (65 536 scenario_1 candidates x 20 segments) and its
cuboid variant: the solve with the multipliers kept, btrapz_solve_vjp_device, btrapz_solve_jvp_device at T = 1 and at
T = 10 in one call, and ten separate T = 1 calls.  The tangents are dense in the 20 parameters of every candidate (the
fit's case).  HIP events, warm-up, median / min / max of --reps repetitions; kernel times from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--no-rocprof: skip).

    python tools/jvp_bench.py --out profiles/jvp_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(variant, reps, warmup):
    import numpy as np
    import torch
    import bench
    from spectral_amd.solver import BatchSolver
    B, S = 65536, 20
    batch, sh = bench.make_workload("scenario1", B, S, variant, 0)
    solver = BatchSolver(0)
    db = solver.upload(batch)
    d = solver.device
    rng = np.random.default_rng(0)
    xbar = torch.tensor(rng.standard_normal((B, 12 * S)), device=d)
    cbar = torch.tensor(rng.standard_normal(B), device=d)
    tan10 = torch.tensor(rng.standard_normal((10, B, 20)), device=d)
    tan1 = [tan10[t:t + 1].contiguous() for t in range(10)]
    o = solver.solve(db, sh, keep_multipliers=True)
    names = ("forward", "vjp", "jvp_T1", "jvp_T10", "jvp_10_calls_of_T1")
    times = {k: [] for k in names}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for i in range(warmup + reps):
        e = [ev() for _ in range(6)]
        e[0].record()
        o = solver.solve(db, sh, keep_multipliers=True, out=o)
        e[1].record()
        solver.solve_vjp(db, sh, o, xbar, cbar)
        e[2].record()
        solver.solve_jvp(db, sh, o, {"shared": tan1[0]})
        e[3].record()
        solver.solve_jvp(db, sh, o, {"shared": tan10})
        e[4].record()
        for t in range(10):
            solver.solve_jvp(db, sh, o, {"shared": tan1[t]})
        e[5].record()
        torch.cuda.synchronize()
        if i >= warmup:
            for j, k in enumerate(names):
                times[k].append(e[j].elapsed_time(e[j + 1]))
    st = o["status"].cpu().numpy()
    res = {"B": B, "S": S, "variant": variant, "solved": int(((st == 1) | (st == 2)).sum())}
    for k, v in times.items():
        v = sorted(v)
        res[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1], "reps": len(v)}
    res["jvp_T1_over_vjp"] = res["jvp_T1"]["median_ms"] / res["vjp"]["median_ms"]
    res["ten_calls_over_one_call_of_T10"] = res["jvp_10_calls_of_T1"]["median_ms"] / res["jvp_T10"]["median_ms"]
    return res


def main():
    from vjp_bench import kernel_stats
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    res = {"workload": "bench.make_workload('scenario1', 65536, 20, variant, 0): BASELINE config 3 (variant 0) and its "
                       "cuboid variant; tangents dense in the 20 parameters of every candidate",
           "note": "the output buffers of a call are allocated inside the timed region (torch's caching allocator), as in "
                   "tools/vjp_bench.py",
           "config3": measure(0, a.reps, a.warmup), "config3_cuboid": measure(1, a.reps, a.warmup)}
    if a.child:
        return
    if not a.no_rocprof:
        res["kernels_rocprofv3"] = kernel_stats(5, script=os.path.abspath(__file__))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
