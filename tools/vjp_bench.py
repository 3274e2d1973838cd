"""Forward (solve with the multipliers kept) against backward (btrapz_solve_vjp_device) on BASELINE config 3's batch
(65 536 scenario_1 candidates x 20 segments) and its cuboid variant.  HIP events, warm-up, median / min / max of --reps
repetitions; kernel times from a separate `rocprofv3 --kernel-trace --stats` run of this script (--no-rocprof: skip).

    python tools/vjp_bench.py --out profiles/vjp_bench.json
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s, MI355X_MICROARCH.md


def _bytes(B, S, fwd):
    """Bytes a launch must move, from the shapes.  Forward: record in, ctrl + multipliers + cost / status out.
    Backward: record, ctrl, multipliers, status and cotangents in, grad_seg and the per-candidate gradients out."""
    rec = (17 * S + 6 + 2 + 10) * 8
    ctrl, lam, grads = 12 * S * 8, 2 * 36 * S * 8, (17 * S + 6 + 2 + 10 + 20) * 8
    if fwd:
        return B * (rec + ctrl + lam + 12)
    return B * (rec + 2 * ctrl + lam + 8 + 4 + grads)


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
    o = solver.solve(db, sh, keep_multipliers=True)
    times = {"forward": [], "backward": []}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for i in range(warmup + reps):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        o = solver.solve(db, sh, keep_multipliers=True, out=o)
        e1.record()
        solver.solve_vjp(db, sh, o, xbar, cbar)
        e2.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times["forward"].append(e0.elapsed_time(e1)); times["backward"].append(e1.elapsed_time(e2))
    st = o["status"].cpu().numpy()
    res = {"B": B, "S": S, "variant": variant, "solved": int(((st == 1) | (st == 2)).sum())}
    for k, v in times.items():
        v = sorted(v)
        med = float(np.median(v))
        nbytes = _bytes(B, S, k == "forward")
        res[k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "reps": len(v), "bytes": nbytes,
                  "hbm_share_at_median": nbytes / (med * 1e-3) / HBM_PEAK}
    res["backward_over_forward"] = res["backward"]["median_ms"] / res["forward"]["median_ms"]
    return res


def kernel_stats(reps, script=None, args=()):
    """Kernel times from rocprofv3 --kernel-trace --stats over a short run of `script` (default: this one) with --child
    (a child process)."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="vjp_prof_")
    cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "vjp", "--", sys.executable, os.path.abspath(script or __file__),
           "--child", "--reps", str(reps), "--warmup", "2", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        return {"error": "rocprofv3 exit %d" % r.returncode, "tail": r.stderr[-2000:]}
    stats = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = next((v for k, v in row.items() if k and "name" in k.lower()), "")
                num = lambda key: float(next((v for k, v in row.items() if k and k.lower() == key), 0) or 0)
                stats[name.split("(")[0][-80:]] = {"calls": int(num("calls")), "average_ms": num("averagens") * 1e-6,
                                                   "min_ms": num("minns") * 1e-6, "max_ms": num("maxns") * 1e-6,
                                                   "share_percent": num("percentage")}
    if not stats:
        stats = {"error": "no kernel statistics found", "files": sorted(glob.glob(os.path.join(out, "**", "*"), recursive=True))[:20]}
    shutil.rmtree(out, ignore_errors=True)
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    res = {"workload": "bench.make_workload('scenario1', 65536, 20, variant, 0): BASELINE config 3 (variant 0) and its "
                       "cuboid variant", "hbm_peak_bytes_per_s": HBM_PEAK,
           "config3": measure(0, a.reps, a.warmup), "config3_cuboid": measure(1, a.reps, a.warmup)}
    if a.child:
        return
    if not a.no_rocprof:
        res["kernels_rocprofv3"] = kernel_stats(5)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
