#!/usr/bin/env python3
"""The clearance stage (btrapz_clearance_device, _vjp_device, _jvp_device; include/btrapz_hip_clearance.h) beside the
Cartesian stage that feeds it and beside the same quantity written the way a caller writes it today: torch elementwise
operations, one obstacle after the other.  ONE run, the launches alternating, HIP events around each launch (launch
overhead included), median and min / max of --reps launches -- the method of tools/cartesian_bench.py.

Workload: --scenes x --per-scene scenario_1 candidates of 7 one-second segments solved on the GPU, sampled every 0.1 s (71
samples per solved row in rows of 72 slots) and placed on an arc of radius 80 m; rows of one scene are consecutive.  Every
scene has O obstacles (4 and 16) that keep lane and speed along the arc (synth.obstacles_on_line), headings off the
road's by up to 0.2 rad.

Reported per launch: time, rectangle pairs per second (forward launches), the bytes the algorithm has to move (the poses
read once, the outputs written once, a scene's obstacle columns counted once per scene: they are shared through the
caches) and their rate against 6.29 TB/s, the float4-copy rate published for this chip -- a REFERENCE figure, no copy is
timed here.  Which limit the forward sits nearest to is read off two figures: that fraction, and how the time grows from 4
to 16 obstacles, which multiplies the arithmetic by four and leaves the bytes almost alone.  Measured once, reported, not
asserted.  Writes profiles/clearance_bench.json.

    python tools/clearance_bench.py [--scenes 128] [--per-scene 512] [--reps 10] [--obstacles 4 16]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GBS = 6290.0      # published float4-copy rate of the MI355X: a reference figure, not measured here
FOOT = (2.4, 0.95, 1.3)
SIGNS = ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))


def alternating(torch, runs, reps):
    """{name: [ms] * reps} of the launches `runs` {name: callable}, alternating in one loop after two warm-up rounds."""
    for _ in range(2):
        for run in runs.values():
            run()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); run(); e1.record(); torch.cuda.synchronize(); t[k].append(e0.elapsed_time(e1))
    return t


def torch_pair(torch, x, y, th, ox, oy, oth, hlb, hwb):
    """The header's definition for one obstacle per row, elementwise: everything [R, n] (hlb, hwb [R, 1])."""
    hla, hwa, off = FOOT
    ca, sa, cb, sb = torch.cos(th), torch.sin(th), torch.cos(oth), torch.sin(oth)
    dx, dy = ox - (x + off * ca), oy - (y + off * sa)
    dau, dan, dbu, dbn = dx * ca + dy * sa, dy * ca - dx * sa, dx * cb + dy * sb, dy * cb - dx * sb
    c, s = ca * cb + sa * sb, ca * sb - sa * cb
    ac, as_ = c.abs(), s.abs()
    g = torch.stack([dau.abs() - hla - (hlb * ac + hwb * as_), dan.abs() - hwa - (hlb * as_ + hwb * ac),
                     dbu.abs() - (hla * ac + hwa * as_) - hlb, dbn.abs() - (hla * as_ + hwa * ac) - hwb]).amax(0)
    dist = None
    zero = torch.zeros_like(x)
    for sx, sy in SIGNS:
        pu, pn = sx * hla * c + sy * hwa * s - dbu, sy * hwa * c - sx * hla * s - dbn
        da = torch.sqrt(torch.maximum(pu.abs() - hlb, zero) ** 2 + torch.maximum(pn.abs() - hwb, zero) ** 2 + 1e-300)
        qu, qn = sx * hlb * c - sy * hwb * s + dau, sx * hlb * s + sy * hwb * c + dan
        db = torch.sqrt(torch.maximum(qu.abs() - hla, zero) ** 2 + torch.maximum(qn.abs() - hwa, zero) ** 2 + 1e-300)
        m = torch.minimum(da, db)
        dist = m if dist is None else torch.minimum(dist, m)
    return torch.where(g > 0, dist, g)


def torch_clearance(torch, cart, pose, half, scene):
    """min over the scene's obstacles, one obstacle at a time: cart [R, 6, n], pose [K, O, 3, n], half [K, O, 2], scene [R]."""
    x, y, th = cart[:, 0], cart[:, 1], cart[:, 2]
    best = torch.full_like(x, float("inf"))
    for o in range(pose.shape[1]):
        p, h = pose[scene, o], half[scene, o]
        cl = torch_pair(torch, x, y, th, p[:, 0], p[:, 1], p[:, 2], h[:, :1], h[:, 1:])
        best = torch.minimum(best, torch.where(torch.isnan(cl) & ~torch.isnan(x), torch.full_like(cl, float("inf")), cl))
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=128)
    ap.add_argument("--per-scene", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--obstacles", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from spectral_amd import synth
    from spectral_amd.native import CRefLine, CObstacles, footprint_struct
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    d = solver.device
    K, B, S = a.scenes, a.scenes * a.per_scene, 7
    batch, sh = synth.make_scenario1_batch(B, S, 0)
    db = solver.upload(batch)
    o = solver.solve(db, sh)
    traj, npts = solver.sample(db, o["ctrl"], torch.arange(B, device=d), sh.delta)
    rl = synth.refline_arc(200.0, 200.0 / 999.0, 80.0)
    tab = rl.on(d)
    t = CRefLine(rl.n_lines, rl.M, *[x.data_ptr() for x in tab])
    n = traj.shape[2]
    cart = torch.full((B, 6, n), float("nan"), dtype=torch.float64, device=d)     # NaN beyond a row's count: not valid, on both sides
    stream = torch.cuda.current_stream(d).cuda_stream
    solver.ctx.cartesian_device(t, None, B, n, 0, traj, npts, cart, None, stream=stream)
    torch.cuda.synchronize()
    samples, rows = int(npts.sum()), int((npts > 0).sum())
    scene = (torch.arange(B, device=d) // a.per_scene).to(torch.int32)
    ft = footprint_struct(FOOT)
    g = torch.Generator(device=d).manual_seed(0)
    clear = torch.full((B, n), float("nan"), dtype=torch.float64, device=d)
    which = torch.full((B, n), -1, dtype=torch.int32, device=d)
    valid = torch.arange(n, device=d)[None, :] < npts[:, None]
    audit = dict(clear_min=torch.empty(B, dtype=torch.float64, device=d), worst=torch.empty((B, 2), dtype=torch.int32, device=d),
                 n_below=torch.empty(B, dtype=torch.int32, device=d), n_invalid=torch.empty(B, dtype=torch.int32, device=d))
    clear_bar = torch.randn((B, n), generator=g, dtype=torch.float64, device=d)
    cart_bar = torch.empty_like(cart)
    res = {"device": torch.cuda.get_device_name(0), "label": "measured once on one MI355X", "reps": a.reps,
           "workload": "%d scenes x %d scenario_1 candidates of %d segments, %d solved; rows of %d slots, %d samples in all; arc of radius 80 m"
                       % (K, a.per_scene, S, rows, n, samples),
           "timing": "HIP events around one launch (launch overhead included); not a profiler's kernel time",
           "hbm_copy_gbs_reference": HBM_COPY_GBS,
           "hbm_copy_gbs_reference_source": "published float4-copy rate of the MI355X; no copy was timed in this run", "by_obstacles": {}}
    rng = np.random.default_rng(0)
    for O in a.obstacles:
        ob = synth.obstacles_on_line(rl, rng.uniform(5.0, 60.0, (K, O)), rng.uniform(-6.0, 6.0, (K, O)), rng.uniform(1.0, 9.0, (K, O)), n=n,
                                     dt=sh.delta, half=(2.3, 0.9), dtheta=rng.uniform(-0.2, 0.2, (K, O)))
        pose, half, _ = ob.on(d)
        cob = CObstacles(K, O, n, pose.data_ptr(), half.data_ptr(), None)
        fwd = lambda c, w, au: solver.ctx.clearance_device(ft, cob, scene, B, n, cart, npts, 0.5, c, w, au, stream=stream)
        fwd(clear, which, audit)
        torch.cuda.synchronize()
        runs = {"cartesian_forward": lambda: solver.ctx.cartesian_device(t, None, B, n, 0, traj, npts, cart_bar, None, stream=stream),
                "forward_all": lambda: fwd(clear, which, audit), "audit_only": lambda: fwd(None, None, audit),
                "vjp": lambda: solver.ctx.clearance_vjp_device(ft, cob, scene, B, n, cart, npts, which, clear_bar, cart_bar, stream=stream)}
        bufs = {}
        for T in a.tangents:
            bufs[T] = (torch.randn((T, B, 6, n), generator=g, dtype=torch.float64, device=d), torch.zeros((T, B, n), dtype=torch.float64, device=d))
            runs["jvp_T%d" % T] = lambda T=T: solver.ctx.clearance_jvp_device(ft, cob, scene, B, n, cart, npts, which, T, bufs[T][0], None, bufs[T][1],
                                                                             stream=stream)
        keep = {}
        idx = scene.long()

        def torch_forward():
            with torch.no_grad():
                keep["clear"] = torch_clearance(torch, cart, pose, half, idx)

        def torch_backward():
            c = cart.detach().clone().requires_grad_(True)
            cl = torch_clearance(torch, c, pose, half, idx)
            ok = torch.isfinite(cl)
            keep["cart_bar"], = torch.autograd.grad(torch.where(ok, cl, torch.zeros_like(cl)), c, torch.where(ok, clear_bar, torch.zeros_like(clear_bar)))
        runs["torch_forward"] = torch_forward
        runs["torch_forward_and_backward"] = torch_backward
        # the torch statement must say what the kernel says BEFORE either is timed: finite in the same places and within 1e-9 m
        # (rounding alone is 1e-13 m at these coordinates; a wrong statement is off by metres)
        fwd(clear, which, audit); torch_forward(); torch.cuda.synchronize()
        both = valid & torch.isfinite(clear) & torch.isfinite(keep["clear"])
        agree = float((clear - keep["clear"]).abs()[both].max())
        same_nan = bool((torch.isfinite(clear) == torch.isfinite(keep["clear"]))[valid].all())
        assert same_nan and agree <= 1e-9, ("the torch statement and the kernel disagree", O, agree, same_nan)
        ms = alternating(torch, runs, a.reps)
        solver.ctx.clearance_vjp_device(ft, cob, scene, B, n, cart, npts, which, clear_bar, cart_bar, stream=stream)
        torch_backward(); torch.cuda.synchronize()
        gb = torch.nan_to_num(keep["cart_bar"][:, :3])
        off_tie = (gb - cart_bar[:, :3]).abs().amax(1) <= 1e-6 * (1 + cart_bar[:, :3].abs().amax(1))
        obs_bytes = K * O * 3 * n * 8 + K * O * 16
        moved = {"cartesian_forward": 2 * samples * 48, "forward_all": samples * (24 + 12) + obs_bytes + B * 24, "audit_only": samples * 24 + obs_bytes + B * 24,
                 "vjp": samples * (24 + 4 + 8) + B * n * 48 + obs_bytes, "torch_forward": samples * (24 + 8) + obs_bytes,
                 "torch_forward_and_backward": samples * (24 + 8 + 8 + 48) + obs_bytes}
        for T in a.tangents:
            moved["jvp_T%d" % T] = samples * (24 + 4 + T * 32) + obs_bytes
        pairs = samples * O
        r = {"pairs": pairs, "kernel_and_torch_agree_to_m": agree, "finite_in_the_same_places": same_nan,
             "share_of_samples_whose_gradient_agrees_with_autograd": float(off_tie[npts > 0].float().mean()), "launches": {}}
        for k, v in ms.items():
            med = float(np.median(v))
            gbs = moved[k] / (med * 1e-3) / 1e9
            r["launches"][k] = {"ms": med, "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "algorithmic_bytes": int(moved[k]), "gbs": gbs,
                                "frac_of_reference_copy": gbs / HBM_COPY_GBS}
            if k in ("forward_all", "audit_only", "torch_forward"):
                r["launches"][k]["pairs_per_s"] = pairs / (med * 1e-3)
        r["torch_forward_over_forward"] = r["launches"]["torch_forward"]["ms"] / r["launches"]["forward_all"]["ms"]
        r["torch_backward_over_forward_and_vjp"] = r["launches"]["torch_forward_and_backward"]["ms"] / (r["launches"]["forward_all"]["ms"] + r["launches"]["vjp"]["ms"])
        r["forward_over_cartesian"] = r["launches"]["forward_all"]["ms"] / r["launches"]["cartesian_forward"]["ms"]
        res["by_obstacles"][str(O)] = r
        del bufs, keep
        torch.cuda.empty_cache()
    Os = [str(O) for O in a.obstacles]
    if len(Os) >= 2:
        lo, hi = res["by_obstacles"][Os[0]]["launches"]["forward_all"], res["by_obstacles"][Os[-1]]["launches"]["forward_all"]
        growth = hi["ms"] / lo["ms"]
        res["forward_time_growth_%s_to_%s_obstacles" % (Os[0], Os[-1])] = growth
        res["bound"] = ("FP64 arithmetic of the obstacle loop (sincos, the twelve features), not bandwidth: %.1f x the obstacles cost %.2f x the time, and the "
                        "forward moves %.1f %% (O = %s) and %.1f %% (O = %s) of the reference copy rate (not measured here)"
                        % (int(Os[-1]) / int(Os[0]), growth, 100 * lo["frac_of_reference_copy"], Os[0], 100 * hi["frac_of_reference_copy"], Os[-1])
                        if growth >= 0.5 * int(Os[-1]) / int(Os[0]) else
                        "launch and memory latency rather than arithmetic: %.1f x the obstacles cost only %.2f x the time" % (int(Os[-1]) / int(Os[0]), growth))
    res["not_measured"] = "kernel time without launch overhead (no profiler run); FP64 operation counts; obstacle sines and cosines staged in LDS or read from a side array"
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1); fh.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
