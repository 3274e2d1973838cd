#!/usr/bin/env python3
"""The projection onto the reference line (btrapz_frenet_device, _vjp_device, _jvp_device; include/btrapz_hip_frenet.h)
beside the forward it inverts (btrapz_cartesian_device on the same rows) and beside the same projection written the way
a caller writes it today: torch operations -- chord distances to every interval, argmin, a fixed number of Newton steps.
ONE run, the launches alternating, HIP events around each launch (launch overhead included), min / median / max of --reps
launches.  Informative: nothing is asserted.  Writes profiles/frenet_bench.json.

Workloads, on an arc of radius 80 m tabulated at 1 000 points:
  - round trip: --batch rows of 71 samples, each row a trajectory of 7 s (s = s0 + ds t, a lateral sine), placed in the
    plane by btrapz_cartesian_device and projected back at order 2, without a window and with one of 5 m either side of
    the row's span;
  - obstacles: --batch rows of 16 poses anywhere along the line, at order 1.
The torch projection holds a [queries, M - 1] array of distances: it is timed on --torch-rows rows, in slices, and its
time per query is what is compared.  The mean number of refinement steps is counted by a NumPy replica of the
iteration of frenet_core.h on a sample of the queries (the kernel does not report it).

    python tools/frenet_bench.py [--batch 65536] [--reps 20] [--torch-rows 2048]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cartesian_bench import alternating  # noqa: E402


def torch_project(torch, tab, x, y, newton=4):
    """(s, l) of the queries x, y [Q] against the table (six [M] tensors): nearest chord, then `newton` Newton steps."""
    rs, rx, ry, rth = tab[0], tab[1], tab[2], tab[3]
    ax, ay, ex, ey = rx[:-1], ry[:-1], rx[1:] - rx[:-1], ry[1:] - ry[:-1]
    px, py = x[:, None] - ax[None, :], y[:, None] - ay[None, :]
    t = ((px * ex + py * ey) / (ex * ex + ey * ey)).clamp(0.0, 1.0)
    i = ((px - t * ex) ** 2 + (py - t * ey) ** 2).argmin(1)
    w = t.gather(1, i[:, None])[:, 0]
    wrap = lambda a: torch.remainder(a + math.pi, 2 * math.pi) - math.pi
    dth = wrap(rth[i + 1] - rth[i])
    for _ in range(newton):
        th = rth[i] + w * dth
        c, s = torch.cos(th), torch.sin(th)
        qx, qy = x - (ax[i] + w * ex[i]), y - (ay[i] + w * ey[i])
        g = qx * c + qy * s
        l = qy * c - qx * s
        w = (w - g / (l * dth - (ex[i] * c + ey[i] * s))).clamp(0.0, 1.0)
    th = rth[i] + w * dth
    return rs[i] + w * (rs[i + 1] - rs[i]), (y - (ay[i] + w * ey[i])) * torch.cos(th) - (x - (ax[i] + w * ex[i])) * torch.sin(th)


def refinement_steps(line, x, y, iv):
    """The steps refine() of frenet_core.h takes, per query: a NumPy replica (secant start, Newton, bisection when a step
    leaves the bracket, a Newton step below 2^-30 ends it)."""
    rx, ry, rth = line["rx"], line["ry"], line["rtheta"]
    g_at = lambda k: (x - rx[k]) * np.cos(rth[k]) + (y - ry[k]) * np.sin(rth[k])
    ga, gb = g_at(iv), g_at(iv + 1)
    ax, ay, ex, ey = rx[iv], ry[iv], rx[iv + 1] - rx[iv], ry[iv + 1] - ry[iv]
    dth = np.remainder(rth[iv + 1] - rth[iv] + np.pi, 2 * np.pi) - np.pi
    with np.errstate(all="ignore"):
        w = ga / (ga - gb)
    w = np.where((w >= 0) & (w <= 1), w, 0.5)
    lo, hi = np.zeros_like(w), np.ones_like(w)
    steps, live = np.zeros(len(w), dtype=np.int64), np.ones(len(w), dtype=bool)
    for _ in range(64):
        if not live.any():
            break
        steps[live] += 1
        th = rth[iv] + w * dth
        c, s = np.cos(th), np.sin(th)
        qx, qy = x - (ax + w * ex), y - (ay + w * ey)
        g = qx * c + qy * s
        live &= g != 0
        lo, hi = np.where(live & (g > 0), w, lo), np.where(live & (g < 0), w, hi)
        with np.errstate(all="ignore"):
            dw = g / ((qy * c - qx * s) * dth - (ex * c + ey * s))
        wn = w - dw
        small = np.abs(dw) <= 2.0 ** -30
        wn = np.where(small | ((wn > lo) & (wn < hi)), wn, 0.5 * (lo + hi))
        w = np.where(live, wn, w)
        live &= ~small
    return steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-rows", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frenet_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from spectral_amd import synth
    from spectral_amd.native import CRefLine
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    d = solver.device
    B, n, P = a.batch, 71, 16
    rl = synth.refline_arc(200.0, 200.0 / 999.0, 80.0)
    assert rl.M == 1000, rl.M
    tab = rl.on(d)
    t = CRefLine(rl.n_lines, rl.M, *[x.data_ptr() for x in tab])
    stream = torch.cuda.current_stream(d).cuda_stream
    g = torch.Generator(device=d).manual_seed(0)
    U = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64, device=d)
    tt = 0.1 * torch.arange(n, device=d, dtype=torch.float64)[None, :]
    s0, ds, l0, ph = U(5.0, 140.0, B, 1), U(3.0, 7.0, B, 1), U(-3.0, 3.0, B, 1), U(0.0, 6.28, B, 1)
    traj = torch.stack([s0 + ds * tt, ds.expand(B, n), torch.zeros((B, n), dtype=torch.float64, device=d), l0 + torch.sin(0.6 * tt + ph),
                        0.6 * torch.cos(0.6 * tt + ph), -0.36 * torch.sin(0.6 * tt + ph)], 1).contiguous()
    window = torch.cat([s0 - 5.0, s0 + ds * 7.0 + 5.0], 1).contiguous()
    cart = torch.empty((B, 6, n), dtype=torch.float64, device=d)
    solver.ctx.cartesian_device(t, None, B, n, 0, traj, None, cart, None, stream=stream)
    obs_f = torch.stack([U(1.0, 199.0, B, P), U(0.0, 10.0, B, P), torch.zeros((B, P), dtype=torch.float64, device=d), U(-6.0, 6.0, B, P),
                         U(-1.0, 1.0, B, P), torch.zeros((B, P), dtype=torch.float64, device=d)], 1).contiguous()
    obs = torch.empty((B, 6, P), dtype=torch.float64, device=d)
    solver.ctx.cartesian_device(t, None, B, P, 0, obs_f, None, obs, None, stream=stream)
    fr, iv, no = torch.empty_like(traj), torch.empty((B, n), dtype=torch.int32, device=d), torch.empty(B, dtype=torch.int32, device=d)
    fo, io = torch.empty_like(obs_f), torch.empty((B, P), dtype=torch.int32, device=d)
    fbar = torch.randn((B, 6, n), generator=g, dtype=torch.float64, device=d)
    cbar, cdot, fdot = torch.empty_like(cart), torch.randn((1, B, 6, n), generator=g, dtype=torch.float64, device=d), torch.empty((1, B, 6, n), dtype=torch.float64, device=d)
    cart2 = torch.empty_like(cart)
    fwd = lambda win: solver.ctx.frenet_device(t, None, B, n, 0, 2, cart, None, win, fr, iv, no, stream=stream)
    fwd(None); torch.cuda.synchronize()
    runs = {"cartesian_forward": lambda: solver.ctx.cartesian_device(t, None, B, n, 0, traj, None, cart2, None, stream=stream),
            "frenet_forward": lambda: fwd(None), "frenet_forward_window": lambda: fwd(window),
            "frenet_obstacles_order1": lambda: solver.ctx.frenet_device(t, None, B, P, 0, 1, obs, None, None, fo, io, no, stream=stream),
            "frenet_vjp": lambda: solver.ctx.frenet_vjp_device(t, None, B, n, 0, 2, cart, fr, iv, None, fbar, cbar, stream=stream),
            "frenet_jvp_T1": lambda: solver.ctx.frenet_jvp_device(t, None, B, n, 0, 2, cart, fr, iv, None, 1, cdot, fdot, stream=stream)}
    line = [x[0] for x in tab]
    rows = min(a.torch_rows, B)
    keep = {}

    def torch_run():
        with torch.no_grad():
            out = [torch_project(torch, line, cart[r0:r0 + 256, 0].reshape(-1), cart[r0:r0 + 256, 1].reshape(-1)) for r0 in range(0, rows, 256)]
            keep["s"], keep["l"] = torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
    runs["torch_projection_subset"] = torch_run
    ms = alternating(torch, runs, a.reps)
    fwd(None); torch_run(); torch.cuda.synchronize()
    err = lambda got, want: float((got - want).abs().max())
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "workload": "%d rows of %d samples (round trip) and of %d poses (obstacles, order 1); arc of radius 80 m, %d points" % (B, n, P, rl.M),
           "timing": "HIP events around one launch (launch overhead included); not a profiler's kernel time",
           "round_trip_max_abs_error": {"s": err(fr[:, 0], traj[:, 0]), "l": err(fr[:, 3], traj[:, 3]), "ds": err(fr[:, 1], traj[:, 1]),
                                        "dl": err(fr[:, 4], traj[:, 4]), "dds": err(fr[:, 2], traj[:, 2]), "ddl": err(fr[:, 5], traj[:, 5])},
           "outside": int(no.sum()), "torch_rows": rows,
           "torch_projection_max_abs_error": {"s": err(keep["s"], traj[:rows, 0].reshape(-1)), "l": err(keep["l"], traj[:rows, 3].reshape(-1))},
           "launches": {}}
    for k, v in ms.items():
        q = rows * n if k == "torch_projection_subset" else B * (P if "obstacles" in k else n)
        res["launches"][k] = {"ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "queries": q,
                              "ns_per_query": float(np.median(v)) * 1e6 / q}
    L_ = res["launches"]
    res["torch_over_kernel_per_query"] = L_["torch_projection_subset"]["ns_per_query"] / L_["frenet_forward"]["ns_per_query"]
    res["window_over_whole_line"] = L_["frenet_forward_window"]["ms"] / L_["frenet_forward"]["ms"]
    res["inverse_over_forward"] = L_["frenet_forward"]["ms"] / L_["cartesian_forward"]["ms"]
    pick = np.random.default_rng(0).choice(B, min(B, 512), replace=False)
    host_line = {k: rl.host[k][0] for k in ("rx", "ry", "rtheta")}
    c_h, iv_h = cart[pick].cpu().numpy(), iv[pick].cpu().numpy().astype(np.int64)
    ok = iv_h.reshape(-1) >= 0
    steps = refinement_steps(host_line, c_h[:, 0].reshape(-1)[ok], c_h[:, 1].reshape(-1)[ok], iv_h.reshape(-1)[ok])
    res["refinement_steps"] = {"mean": float(steps.mean()), "max": int(steps.max()), "queries": int(ok.sum()), "how": "NumPy replica of the iteration"}
    res["not_measured"] = "kernel time without launch overhead (no profiler run); FP64 operation counts; the torch projection on the whole batch"
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1); fh.write("\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
