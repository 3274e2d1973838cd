#!/usr/bin/env python3
"""The row audit (btrapz_check_rows_device) timed beside the cold solve of the same batch, on BASELINE config 3's batch
(65 536 x 20, both variants: bench.make_workload) and on the knot-level pipeline's ragged record
(synth.scenario1_knots(65536, 20) through the device corridor stage at stride 32):

  * HIP-event time of the audit, median of --reps launches; the bytes it must move -- (17 + 12) doubles read per segment
    (the record's fields and the control points), 18 per candidate, and its 136 bytes of results -- and that figure over the
    time as a fraction of HBM peak, the way tools/corridor_bench.py computes it; the cold solve's time in the same run;
  * reported, not asserted: on every candidate the solve accepted (status 1 or 2) the worst margin per class in unit 1 and
    the worst equality residual (tests/test_gpu_check_rows.py takes these as the tolerances of BatchSolver.admissible),
    and the share of an MPC-style step's winners (the arg-min of every group of --cand candidates) that stay admissible when
    the bounds of their record move as spectral_amd.knots.jittered moves them by default (the upper s bound of a candidate
    by U(-0.4, 0.4) m): the question a receding-horizon planner asks before it spends a solve.

Writes profiles/check_rows_bench.json and prints it as one JSON line.

    python tools/check_rows_bench.py [--batch 65536] [--reps 20] [--out profiles/check_rows_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
CLASSES = ("position", "velocity", "acceleration", "jerk")


def audit_bytes(B, mean_segments):
    """What the audit must move for B candidates: per segment 17 record fields and 12 control points, per candidate the
    initial state, ref_end and dl_bounds (6 + 2 + 10 doubles) and the results (8 margins, 8 rows, 4 residuals, obj)."""
    return B * (mean_segments * (17 + 12) * 8 + 18 * 8 + 8 * 8 + 8 * 4 + 4 * 8 + 8)


def median_ms(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(np.min(t))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--segments", type=int, default=20)
    ap.add_argument("--cand", type=int, default=512, help="candidates per agent of the MPC-style step (tools/mpc_bench.py's default)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_rows_bench.json"))
    a = ap.parse_args(argv)
    import torch
    import bench
    from spectral_amd import layout as L, synth
    from spectral_amd.solver import BatchSolver, DeviceBatch
    solver = BatchSolver(0)
    B, S = a.batch, a.segments
    stream = torch.cuda.current_stream(solver.device).cuda_stream

    def timed_audit(r, sh, ctrl):
        o = dict(margin=solver._empty(r.B, 2, 4), worst=solver._empty(r.B, 2, 4, dtype=torch.int32), eq_res=solver._empty(r.B, 2, 2), obj=solver._empty(r.B))
        run = lambda: solver.ctx.check_rows_device(r.B, r.S, [sh], None, r.seg, r.seg_count, r.init, r.ref_end, r.dl_bounds, ctrl, unit=1, stream=stream, **o)
        return median_ms(torch, run, a.reps), o

    def accepted(o, status):
        ok = (status == 1) | (status == 2)
        m = o["margin"][ok]
        worst = m.reshape(-1, 2, 4).amin(dim=(0, 1)).cpu().numpy() if bool(ok.any()) else np.full(4, np.inf)
        eq = float(o["eq_res"][ok].max()) if bool(ok.any()) else 0.0
        return ok, {"candidates": int(ok.sum()), "worst_margin_unit1": dict(zip(CLASSES, (float(v) for v in worst))),
                    "worst_equality_residual": eq, "tol_rows_unit1": float(max(0.0, -worst.min())), "tol_eq": eq}

    out = {"note": "measured once on one MI355X; medians of %d launches between HIP events; no gate is put on these numbers" % a.reps,
           "bytes": "per segment (17 + 12) doubles read, per candidate 18 doubles read and 136 bytes written; HBM peak %.0f GB/s" % HBM_PEAK_GBS,
           "uniform": {}, "accepted_results": {}, "mpc_step": {}}
    for variant in (0, 1):
        batch, sh = bench.make_workload("scenario1", B, S, variant, 0)
        db = solver.upload(batch)
        (solve_ms, solve_min) = median_ms(torch, lambda: solver.solve(db, sh), a.reps)
        res = solver.solve(db, sh)
        (ms, mn), o = timed_audit(db, sh, res["ctrl"])
        nbytes = audit_bytes(B, S)
        gbs = nbytes / (ms * 1e-3) / 1e9
        out["uniform"][str(variant)] = {"workload": "BASELINE config %d: %d x %d scenario_1 candidates, variant %d" % (3 + variant, B, S, variant),
                                        "audit_ms": ms, "audit_min_ms": mn, "cold_solve_ms": solve_ms, "cold_solve_min_ms": solve_min,
                                        "audit_over_solve": ms / solve_ms, "bytes": nbytes,
                                        "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}}
        ok, rep = accepted(o, res["status"])
        out["accepted_results"][str(variant)] = rep
        # ---- an MPC-style step: the winner of every group of --cand candidates, audited against its jittered record ----
        if B % a.cand == 0 and bool(ok.any()):
            idx, _ = solver.argmin(res["cost"], group=a.cand)
            torch.cuda.synchronize()
            win = idx[idx >= 0].cpu().numpy()
            rng = np.random.default_rng(0)
            sub = L.Batch(B=len(win), S=S, seg=np.ascontiguousarray(batch.seg[:, win]), init=batch.init[win].copy(), ref_end=batch.ref_end[win].copy(),
                          dl_bounds=batch.dl_bounds[win].copy())
            wctrl = res["ctrl"][torch.from_numpy(win).to(solver.device)].contiguous()
            before = solver.admissible(solver.check_rows(solver.upload(sub), sh, wctrl, unit=1), rep["tol_rows_unit1"], rep["tol_eq"])
            sub.seg[L.F_UPP_BIAS] += rng.uniform(-0.4, 0.4, (len(win), 1))           # knots.jittered: s_shift = 0.4 on the upper s bound
            after = solver.admissible(solver.check_rows(solver.upload(sub), sh, wctrl, unit=1), rep["tol_rows_unit1"], rep["tol_eq"])
            out["mpc_step"][str(variant)] = {"winners": int(len(win)), "admissible_under_their_own_record": float(before.double().mean()),
                                             "still_admissible_under_the_jittered_record": float(after.double().mean())}
    # ---- the knot-level pipeline's ragged record ----
    kb = synth.scenario1_knots(B, 20)
    rec = solver.corridor_batch(kb, 0, seg_stride=32)
    sh = synth.shared_params(0)
    sh.ds_ref, sh.dl_ref = kb.header["ds_ref"], kb.header["dl_ref"]
    sh.dds, sh.ddds, sh.ddl, sh.dddl = kb.header["dds"], kb.header["ddds"], kb.header["ddl"], kb.header["dddl"]
    r = DeviceBatch.from_tensors(rec["seg"], rec["init"], rec["ref_end"], rec["dl_bounds"], rec["seg_count"], B=B, S=32)
    (solve_ms, solve_min) = median_ms(torch, lambda: solver.solve_ragged(rec, sh), max(3, a.reps // 4))
    res = solver.solve_ragged(rec, sh)
    (ms, mn), o = timed_audit(r, sh, res["ctrl"])
    counts = rec["seg_count"].cpu().numpy()
    mean_seg = float(np.maximum(counts, 0).mean())
    nbytes = audit_bytes(B, mean_seg)
    gbs = nbytes / (ms * 1e-3) / 1e9
    out["ragged"] = {"workload": "synth.scenario1_knots(%d, 20) through the device corridor stage, stride 32, %.2f segments per candidate" % (B, mean_seg),
                     "audit_ms": ms, "audit_min_ms": mn, "cold_solve_ms": solve_ms, "cold_solve_min_ms": solve_min, "audit_over_solve": ms / solve_ms,
                     "bytes": nbytes, "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}}
    out["accepted_results"]["ragged"] = accepted(o, res["status"])[1]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
