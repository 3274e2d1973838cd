"""Sampling and state evaluation with their vector-Jacobian products (btrapz_sample_ragged_device /
btrapz_sample_vjp_device, btrapz_eval_states_device / btrapz_eval_states_vjp_device) on the knot-level workload of
tools/acost_bench.py: synth.scenario1_knots(65536, 20) through the device corridor stage and a ragged solve; every
candidate is selected once, the states are taken at every joint (n_times = seg_stride) and at one time.  HIP events,
warm-up, median / min / max of --reps repetitions; per launch the bytes it must move (from the shapes) and their share
of the HBM peak at the median.

    python tools/states_bench.py --out profiles/states_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12   # bytes / s, MI355X_MICROARCH.md


def measure(variant, reps, warmup, B=65536):
    import numpy as np
    import torch
    from acost_bench import _median
    from spectral_amd import layout as L, synth
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    d = solver.device
    stride = 32
    kb = synth.scenario1_knots(B, 20, seed=0)
    rec = solver.corridor_batch(kb, variant, seg_stride=stride)
    o = solver.solve_ragged(rec, synth.shared_params(variant))
    torch.cuda.synchronize()
    ctrl, cnt = o["ctrl"], rec["seg_count"]
    counts = cnt.cpu().numpy().clip(min=0)
    S_sum = int(counts.sum())
    t = (rec["seg"][L.F_T] * (torch.arange(stride, device=d)[None, :] < cnt[:, None])).cpu().numpy()
    samples = np.floor(t / kb.delta + 1e-9).sum(1)
    mp = int(samples.max()) + 2
    sel = torch.arange(B, dtype=torch.int64, device=d)
    out = torch.zeros((B, 6, mp), dtype=torch.float64, device=d)
    npts = torch.zeros(B, dtype=torch.int32, device=d)
    stream = lambda: torch.cuda.current_stream(d).cuda_stream
    fwd_s = lambda: solver.ctx.sample_ragged_device(B, stride, cnt, kb.delta, rec["seg"], rec["init"], ctrl, sel, mp, out, npts,
                                                    stream=stream())
    fwd_s()
    ob = torch.randn((B, 6, mp), dtype=torch.float64, device=d)
    cb = torch.empty((B, 12 * stride), dtype=torch.float64, device=d)
    ib = torch.empty((B, 6), dtype=torch.float64, device=d)
    vjp_s = lambda: solver.ctx.sample_vjp_device(B, stride, cnt, kb.delta, rec["seg"], sel, mp, ob, ctrl_bar=cb, init_bar=ib,
                                                 stream=stream())
    written = int(6 * 8 * (samples.sum() + B))   # rows the forward writes / the VJP reads
    common = B * (8 + 4) + S_sum * 8
    res = {"B": B, "seg_stride": stride, "variant": variant, "mean_segments": float(counts.mean()),
           "mean_samples": float(samples.mean()) + 1, "max_points": mp}
    pair = {"forward": _median(fwd_s, reps, warmup), "vjp": _median(vjp_s, reps, warmup)}
    pair["forward"]["bytes"] = int(common + S_sum * 96 + B * 48 + written + B * 4)
    pair["vjp"]["bytes"] = int(common + written + B * (96 * stride + 48))
    res["sample"] = pair
    for name, n in (("eval_states_joints", stride), ("eval_states_one_time", 1)):
        times = torch.cumsum(rec["seg"][L.F_T], 1)[:, :n].contiguous() if n > 1 else (0.5 * torch.as_tensor(t.sum(1), device=d))[:, None].contiguous()
        x = torch.empty((B, 2, n, 3), dtype=torch.float64, device=d)
        xb = torch.randn((B, 2, n, 3), dtype=torch.float64, device=d)
        tb = torch.empty((B, n), dtype=torch.float64, device=d)
        fwd = lambda: solver.ctx.eval_states_device(B, stride, cnt, rec["seg"], ctrl, n, times, x, stream=stream())
        vjp = lambda: solver.ctx.eval_states_vjp_device(B, stride, cnt, rec["seg"], ctrl, n, times, xb, ctrl_bar=cb, times_bar=tb,
                                                        stream=stream())
        pair = {"forward": _median(fwd, reps, warmup), "vjp": _median(vjp, reps, warmup)}
        # the forward reads, per time, the walked durations (cached after the first) and 12 control points, writes 6 values
        pair["forward"]["bytes"] = int(B * 4 + S_sum * 8 + B * n * (8 + 96 + 48))
        pair["vjp"]["bytes"] = int(B * 4 + S_sum * 8 + B * n * (8 + 96 + 48 + 8) + B * 96 * stride)
        res[name] = dict(pair, n_times=n)
    for key in ("sample", "eval_states_joints", "eval_states_one_time"):
        for r in (res[key]["forward"], res[key]["vjp"]):
            r["hbm_share_at_median"] = r["bytes"] / (r["median_ms"] * 1e-3) / HBM_PEAK
        res[key]["vjp_over_forward"] = res[key]["vjp"]["median_ms"] / res[key]["forward"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", type=int, choices=(0, 1), default=None, help="one variant only (default: both)")
    a = ap.parse_args()
    res = {"workload": "synth.scenario1_knots(65536, 20) -> btrapz_corridor_batch_device (seg_stride 32) -> "
                       "btrapz_solve_ragged_device; every candidate selected once; states at every joint slot and at one time",
           "forward_kernels": "sample_kernel, eval_states_kernel (unchanged)", "vjp_kernels": "sample_vjp_kernel, eval_states_vjp_kernel",
           "hbm_peak_bytes_per_s": HBM_PEAK}
    for v, name in ((0, "trapezoid"), (1, "cuboid")):
        if a.variant is None or a.variant == v:
            res[name] = measure(v, a.reps, a.warmup)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
