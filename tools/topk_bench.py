"""K-best selection (btrapz_topk_device) beside its two yardsticks, in ONE run: btrapz_argmin_device, and
torch.topk(cost.view(G, group), K, largest=False) with the index fix-up a user would write (global indices, -1 where the
cost is not finite).  Shapes: 1 x 65 536 (one arg-min group over the batch) and 128 x 512 (BASELINE config 5).

Costs: the solved costs of bench.make_workload("scenario1", 65536, 20) ("solved": +inf where the solve failed), and
seeded normal costs with 25 % +inf, the pipeline's unsolved share ("normal25").

Timing: HIP events around --calls back-to-back calls on one stream (a single call of a few microseconds is below what an
event pair resolves), divided by the number of calls; the variants alternate inside every repetition; warm-up first;
median / min / max over --reps repetitions (at least 20).  The time of a call therefore includes its launch overhead(s)
-- two launches for the split shapes of argmin and topk, several for the torch path -- which is what a caller pays.

    python tools/topk_bench.py --out profiles/topk_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 4, 16, 64)
SHAPES = ((1, 65536), (128, 512))


def variants(solver, cost, G, group):
    import torch
    row0 = (torch.arange(G, device=cost.device, dtype=torch.int64) * group)[:, None]

    def torch_topk(K):
        v, j = torch.topk(cost.view(G, group), K, dim=1, largest=False)
        return torch.where(v < float("inf"), j + row0, torch.full_like(j, -1)), v

    out = {"argmin": lambda: solver.argmin(cost, group=group)}
    for K in KS:
        out["topk_K%d" % K] = lambda K=K: solver.topk(cost, K, group=group)
        out["torch_topk_K%d" % K] = lambda K=K: torch_topk(K)
    return out


def measure(fns, reps, warmup, calls):
    import numpy as np
    import torch
    ts = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ts[k].append(e0.elapsed_time(e1) / calls)
    return {k: {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * min(v), "max_us": 1e3 * max(v), "reps": len(v)} for k, v in ts.items()}


def check(solver, cost, G, group):
    """topk == the numpy yardstick on these costs (K = 16), and K = 1 == argmin: a time of a wrong result is no time."""
    import numpy as np
    import torch
    bi, bc = solver.topk(cost, 16, group=group)
    ai, ac = solver.argmin(cost, group=group)
    b1, c1 = solver.topk(cost, 1, group=group)
    torch.cuda.synchronize()
    c = cost.cpu().numpy()
    for g in range(G):
        cg = c[g * group:(g + 1) * group]
        idx = np.arange(g * group, (g + 1) * group)
        m = cg < np.inf
        order = np.lexsort((idx[m], cg[m]))[:16]
        wi = np.full(16, -1, np.int64); wi[:order.size] = idx[m][order]
        assert np.array_equal(bi[g].cpu().numpy(), wi), g
    assert torch.equal(b1[:, 0], ai) and torch.equal(c1[:, 0].view(torch.int64), ac.view(torch.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20")
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("topk_bench.py needs a HIP device: there is no CPU path")
    import bench
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    B = 65536
    batch, shared = bench.make_workload("scenario1", B, 20, 0, 0)
    o = solver.solve(solver.upload(batch), shared)
    torch.cuda.synchronize()
    rng = np.random.default_rng(2024)
    normal = rng.normal(size=B)
    normal[rng.random(B) < 0.25] = np.inf
    sources = {"solved": o["cost"].clone(), "normal25": torch.from_numpy(normal).to(solver.device)}
    res = {"device": torch.cuda.get_device_name(0), "calls_per_timing": a.calls, "warmup": a.warmup,
           "unit": "microseconds per call, HIP events around calls_per_timing back-to-back calls",
           "sources": {"solved": "bench.make_workload('scenario1', 65536, 20, 0, 0) solved; share of +inf %.4f" % float(torch.isinf(sources["solved"]).double().mean()),
                       "normal25": "numpy default_rng(2024) normal, 25 % +inf"}}
    for name, cost in sources.items():
        res[name] = {}
        for G, group in SHAPES:
            check(solver, cost, G, group)
            res[name]["%dx%d" % (G, group)] = measure(variants(solver, cost, G, group), a.reps, a.warmup, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for name in sources:
        for shape, r in res[name].items():
            print(name, shape, " ".join("%s %.1f" % (k, v["median_us"]) for k, v in r.items()))


if __name__ == "__main__":
    main()
