#!/usr/bin/env python3
"""The Cartesian stage (btrapz_cartesian_device, _vjp_device, _jvp_device; include/btrapz_hip_cartesian.h) beside the
sampler that feeds it and beside the same map written the way a caller writes it today: torch elementwise operations and a
searchsorted.  ONE run, the launches alternating, HIP events around each launch (launch overhead included: microseconds
against milliseconds), median and min / max of --reps launches.

Workload: --batch scenario_1 candidates of 7 one-second segments solved on the GPU, sampled every 0.1 s -- 71 samples per
row, the scenario_1 horizon, in the sampler's [B, 6, 72] array with its npoints as count -- on an arc of radius 80 m
tabulated at 1 000 points.

Reported per launch: time, the bytes the algorithm has to move (inputs read once, outputs written once, the table not
counted: 48 KB that stay in cache), their rate and its fraction of the HBM peak (8 TB/s by the data sheet) and of 6.29 TB/s,
the rate published for a float4 copy on this chip -- a REFERENCE figure: no copy is timed in this run.  The times are
HIP-event times of a launch, not kernel times of a profiler.  Which bound holds is read off two figures, not assumed: the
fraction of that reference rate, and the audit-only call, which moves half the forward's bytes with the same arithmetic -- a bandwidth-bound kernel gets faster by
about that half, an arithmetic-bound one does not.  Measured, reported, not asserted.  Writes profiles/cartesian_bench.json.

    python tools/cartesian_bench.py [--batch 65536] [--reps 20] [--tangents 1 12]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
HBM_COPY_GBS = 6290.0      # published float4-copy rate of the MI355X: a reference figure, not measured here


def alternating(torch, runs, reps):
    """{name: [ms] * reps} of the launches `runs` {name: callable}, alternating in one loop after three warm-up rounds."""
    for _ in range(3):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record(); torch.cuda.synchronize(); t[k].append(e0.elapsed_time(e1))
    return t


def torch_map(torch, tab, f, valid):
    """The documented map as elementwise torch operations: f [R, 6, n], tab the six [M] tensors, valid [R, n] bool.
    Returns cart [R, 6, n] (NaN outside the line and where not valid) -- what a caller writes without this stage."""
    rs, rx, ry, rth, rk, rdk = tab
    s, sd, sdd, l, ld, ldd = f.unbind(1)
    inside = valid & (s >= rs[0]) & (s <= rs[-1])
    sc = torch.where(inside, s, rs[0])
    i = (torch.searchsorted(rs, sc.contiguous(), right=True) - 1).clamp(0, rs.numel() - 2)
    h = rs[i + 1] - rs[i]
    w = (sc - rs[i]) / h
    lin = lambda q: q[i] + w * (q[i + 1] - q[i])
    wrap = lambda a: torch.remainder(a + math.pi, 2 * math.pi) - math.pi
    th = rth[i] + w * wrap(rth[i + 1] - rth[i])
    k, kp = lin(rk), lin(rdk)
    om = 1 - k * l
    vt, vn = sd * om, ld
    at = sdd * om - sd * sd * kp * l - 2 * k * sd * ld
    an = ldd + k * sd * sd * om
    v2 = vt * vt + vn * vn
    v = torch.sqrt(v2)
    cart = torch.stack([lin(rx) - torch.sin(th) * l, lin(ry) + torch.cos(th) * l, wrap(th + torch.atan2(vn, vt)),
                        (vt * an - vn * at) / (v2 * v), v, (vt * at + vn * an) / v], 1)
    return torch.where(inside[:, None, :], cart, torch.full_like(cart, float("nan")))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cartesian_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from spectral_amd import synth
    from spectral_amd.native import CRefLine, KIN_AUDIT
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    d = solver.device
    B, S = a.batch, 7
    batch, sh = synth.make_scenario1_batch(B, S, 0)
    db = solver.upload(batch)
    o = solver.solve(db, sh)
    sel = torch.arange(B, device=d)
    traj, npts = solver.sample(db, o["ctrl"], sel, sh.delta)
    torch.cuda.synchronize()
    n = traj.shape[2]
    valid_rows = int((npts > 0).sum())
    samples = int(npts.sum())
    rl = synth.refline_arc(200.0, 200.0 / 999.0, 80.0)
    assert rl.M == 1000, rl.M
    tab = rl.on(d)
    t = CRefLine(rl.n_lines, rl.M, *[x.data_ptr() for x in tab])
    stream = torch.cuda.current_stream(d).cuda_stream
    cart = torch.empty((B, 6, n), dtype=torch.float64, device=d)
    audit = {k: torch.empty(B, dtype=torch.float64, device=d) for k in KIN_AUDIT[:6]}
    audit["n_outside"] = torch.empty(B, dtype=torch.int32, device=d); audit["worst"] = torch.empty((B, 6), dtype=torch.int32, device=d)
    g = torch.Generator(device=d).manual_seed(0)
    cart_bar = torch.randn((B, 6, n), generator=g, dtype=torch.float64, device=d)
    f_bar = torch.empty_like(traj)
    out_s, np_s = torch.zeros_like(traj), torch.zeros_like(npts)
    fwd = lambda c, au: solver.ctx.cartesian_device(t, None, B, n, 0, traj, npts, c, au, stream=stream)
    runs = {"sampler": lambda: solver.ctx.sample_device(B, S, sh.delta, db.seg, db.init, o["ctrl"], sel, n, out_s, np_s, stream=stream),
            "forward_cart_audit": lambda: fwd(cart, audit), "forward_cart": lambda: fwd(cart, None), "audit_only": lambda: fwd(None, audit),
            "vjp": lambda: solver.ctx.cartesian_vjp_device(t, None, B, n, 0, traj, npts, cart_bar, f_bar, stream=stream)}
    bufs = {}
    for T in a.tangents:
        bufs[T] = (torch.randn((T, B, 6, n), generator=g, dtype=torch.float64, device=d), torch.zeros((T, B, 6, n), dtype=torch.float64, device=d))
        runs["jvp_T%d" % T] = lambda T=T: solver.ctx.cartesian_jvp_device(t, None, B, n, 0, traj, npts, T, bufs[T][0], bufs[T][1], stream=stream)
    valid = torch.arange(n, device=d)[None, :] < npts[:, None]
    line = [x[0] for x in tab]
    keep = {}

    def torch_forward():
        with torch.no_grad():
            keep["cart"] = torch_map(torch, line, traj, valid)

    def torch_vjp():
        f = traj.detach().clone().requires_grad_(True)
        c = torch_map(torch, line, f, valid)
        keep["f_bar"], = torch.autograd.grad(torch.where(valid[:, None, :], c, torch.zeros_like(c)), f, torch.where(valid[:, None, :], cart_bar, torch.zeros_like(cart_bar)))
    runs["torch_forward"] = torch_forward
    runs["torch_forward_and_vjp"] = torch_vjp
    ms = alternating(torch, runs, a.reps)
    # what the two implementations computed, side by side (the yardstick is the tests' business, not this tool's)
    fwd(cart, audit); torch_forward(); torch.cuda.synchronize()
    both = ~torch.isnan(cart) & ~torch.isnan(keep["cart"])
    agree = float(((cart - keep["cart"]).abs()[both] / (1 + keep["cart"].abs()[both])).max())
    per = 48   # bytes of one sample's six doubles
    moved = {"sampler": samples * per + B * (12 * S + 6 + S) * 8, "forward_cart_audit": 2 * samples * per + B * 76, "forward_cart": 2 * samples * per,
             "audit_only": samples * per + B * 76, "vjp": 2 * samples * per + B * n * per, "torch_forward": 2 * samples * per,
             "torch_forward_and_vjp": 4 * samples * per}
    for T in a.tangents:
        moved["jvp_T%d" % T] = (1 + 2 * T) * samples * per
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "workload": "%d scenario_1 candidates of %d segments, %d solved; rows of %d slots, %d samples in all (71 per solved row); arc of radius 80 m, %d points"
                       % (B, S, valid_rows, n, samples, rl.M),
           "timing": "HIP events around one launch (launch overhead included); not a profiler's kernel time",
           "hbm_peak_gbs": HBM_PEAK_GBS, "hbm_copy_gbs_reference": HBM_COPY_GBS,
           "hbm_copy_gbs_reference_source": "published float4-copy rate of the MI355X; no copy was timed in this run", "kernel_and_torch_agree_to": agree, "launches": {}}
    for k, v in ms.items():
        med = float(np.median(v))
        gbs = moved[k] / (med * 1e-3) / 1e9
        res["launches"][k] = {"ms": med, "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "algorithmic_bytes": int(moved[k]), "gbs": gbs,
                              "frac_of_hbm_peak": gbs / HBM_PEAK_GBS, "frac_of_reference_copy": gbs / HBM_COPY_GBS}
    L_ = res["launches"]
    ratio = L_["audit_only"]["ms"] / L_["forward_cart_audit"]["ms"]
    res["audit_only_over_forward"] = ratio
    res["forward_over_sampler"] = L_["forward_cart_audit"]["ms"] / L_["sampler"]["ms"]
    res["torch_forward_over_forward"] = L_["torch_forward"]["ms"] / L_["forward_cart"]["ms"]
    res["bound"] = ("bandwidth: the forward reaches %.0f %% of the reference copy rate" % (100 * L_["forward_cart_audit"]["frac_of_reference_copy"])
                    if L_["forward_cart_audit"]["frac_of_reference_copy"] >= 0.6 else
                    "FP64 arithmetic (sincos, atan2, fmod) or latency, not bandwidth: the forward reaches %.0f %% of the reference copy rate (not measured here) and the "
                    "audit-only call, with half the bytes, takes %.0f %% of its time" % (100 * L_["forward_cart_audit"]["frac_of_reference_copy"], 100 * ratio))
    res["not_measured"] = "kernel time without launch overhead (no profiler run); FP64 operation counts; a torch JVP"
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1); fh.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
