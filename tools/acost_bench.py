"""a_cost of sampled trajectories (btrapz_traj_cost_device) and its VJP (btrapz_traj_cost_vjp_device) on the knot-level
pipeline workload: synth.scenario1_knots(65536, 20) through the device corridor stage and a ragged solve, scored with
per-candidate reference lines ([B, N]) and with one shared line ([N]), both variants.  HIP events, warm-up, median / min
/ max of --reps repetitions, the solve of the same batch timed the same way; kernel times from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--no-rocprof: skip).

    python tools/acost_bench.py --out profiles/acost_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X_MICROARCH.md


def _bytes(counts, stride, N, B, per_candidate_lines, vjp):
    """Bytes a launch must move, from the shapes: per candidate its count, status, S durations, 12 S control points and
    the initial state in, and the reference lines (2 N per candidate, or 2 N once); a_cost and n_points out.  The VJP
    reads a_cost_bar instead and writes ctrl_bar (12 seg_stride), init_bar, params_bar and two rows of N."""
    S = counts.clip(min=0).sum()
    lines = 16 * N * (B if per_candidate_lines else 1)
    common = B * (4 + 4 + 48) + S * (8 + 96) + lines
    if not vjp:
        return int(common + B * 12)
    return int(common + B * 8 + B * (96 * stride + 48 + 160 + 16 * N))


def _median(f, reps, warmup):
    import numpy as np
    import torch
    ts = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    ts = sorted(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": ts[0], "max_ms": ts[-1], "reps": len(ts)}


def measure(variant, reps, warmup, B=65536):
    import numpy as np
    import torch
    from spectral_amd import synth
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    kb = synth.scenario1_knots(B, 20, seed=0)
    rec = solver.corridor_batch(kb, variant, seg_stride=32)
    sh = synth.shared_params(variant)
    o = solver.solve_ragged(rec, sh)
    torch.cuda.synchronize()
    solve_t = _median(lambda: solver.solve_ragged(rec, sh), max(5, reps // 4), 1)
    d = solver.device
    counts = rec["seg_count"].cpu().numpy()
    st = o["status"]
    s_b = torch.tensor(kb.s_ref, device=d); l_b = torch.tensor(kb.l_ref, device=d)
    lines = {"per_candidate": (s_b, l_b), "shared": (s_b[0].contiguous(), l_b[0].contiguous())}
    abar = torch.ones(B, dtype=torch.float64, device=d)
    res = {"B": B, "N": kb.N, "seg_stride": 32, "variant": variant, "mean_segments": float(counts.mean()),
           "solved": int(((st == 1) | (st == 2)).sum()), "solve": solve_t}
    for name, (sr, lr) in lines.items():
        cost, npts = solver.traj_cost(rec, sh, o["ctrl"], sr, lr, status=st)
        torch.cuda.synchronize()
        fwd = _median(lambda: solver.traj_cost(rec, sh, o["ctrl"], sr, lr, status=st), reps, warmup)
        bwd = _median(lambda: solver.traj_cost_vjp(rec, sh, o["ctrl"], sr, lr, abar, status=st), reps, warmup)
        for r, vjp in ((fwd, False), (bwd, True)):
            r["bytes"] = _bytes(counts, 32, kb.N, B, name == "per_candidate", vjp)
            r["hbm_share_at_median"] = r["bytes"] / (r["median_ms"] * 1e-3) / HBM_PEAK
        c = cost.cpu().numpy()
        res[name] = {"forward": fwd, "vjp": bwd, "vjp_over_forward": bwd["median_ms"] / fwd["median_ms"],
                     "forward_over_solve": fwd["median_ms"] / solve_t["median_ms"],
                     "mean_samples": float(npts.cpu().numpy()[np.isfinite(c)].mean()),
                     "scored": int(np.isfinite(c).sum())}
    return res


def main():
    from vjp_bench import kernel_stats
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--variant", type=int, choices=(0, 1), default=None, help="one variant only (default: both)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    res = {"workload": "synth.scenario1_knots(65536, 20) -> btrapz_corridor_batch_device (seg_stride 32) -> "
                       "btrapz_solve_ragged_device, scored with synth.shared_params(variant)", "hbm_peak_bytes_per_s": HBM_PEAK}
    for v, name in ((0, "trapezoid"), (1, "cuboid")):
        if a.variant is None or a.variant == v:
            res[name] = measure(v, a.reps, a.warmup)
    if a.child:
        return
    if not a.no_rocprof:
        res["kernels_rocprofv3"] = kernel_stats(5, script=__file__)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
