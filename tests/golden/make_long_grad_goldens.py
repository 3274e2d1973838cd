"""Writes tests/golden/long_grad_yardstick.npz: the yardstick of btrapz_solve_long_vjp_device / _jvp_device
(tests/vjp_reference.py, tests/jvp_reference.py -- the oracle's dense exact solve and the adjoint / tangent KKT systems by
least squares) at the widths where it is too slow to run in a test: 15 s a candidate at 129 segments, two minutes at 256.

    python tests/golden/make_long_grad_goldens.py [first_case [last_case]]
    python tests/golden/make_long_grad_goldens.py strict

Per case `c<i>_`: `hash` of the candidate's inputs (case_hash: tests/test_long_grad_goldens.py holds the file to the
generator), `seed`, `xbar` (standard normal from that seed) and `cbar` = 0.7, the oracle's `x` and the rows it counts as
active (`act`, `lower`), the five gradient arrays `g_*` with their unique masks `um_*`, and two random directions
(`d<t>_*`, jvp_reference.random_direction from the same generator) with `dx<t>`, `dcost<t>`, `dcost_scale<t>`.  Every case
written is strictly complementary and every tangent consistent (or its active rows independent: see generate); the generic cases have every gradient unique
(Adjoint.nondegenerate), the scenario_1 case has ties at joints: its masks mark them and its directions are 0 there.

`strict`: adds `strict_<generator>_<segments>` [5], which candidates of the batches the GPU tests run at every seam are solved
and strictly complementary by the oracle, and `weak_<generator>_<segments>` [5], which of them have a weakly active row
(strict_of says what that is and why the central differences of tests/test_gpu_long_grad.py leave such a candidate out)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, "long_grad_yardstick.npz")
# (generator, segments, candidate)
CASES = [("generic", 129, 0), ("generic", 129, 1), ("scenario1", 129, 0), ("generic", 256, 0)]
CBAR = 0.7
KEYS = ("seg", "init", "ref_end", "dl_bounds", "shared")


def make(gen, S):
    from spectral_amd import synth
    return synth.make_scenario1_batch(5, S, 0) if gen == "scenario1" else synth.make_batch(5, S, config=3)


def case_seed(S, b):
    return 7000 + 10 * S + b


def case_hash(batch, sh, b):
    h = hashlib.sha256()
    for a in (batch.seg[:, b], batch.init[b], batch.ref_end[b], batch.dl_bounds[b], sh.as_array()):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def generate(i):
    from jvp_reference import Tangent, random_direction
    from vjp_reference import Adjoint, one
    gen, S, b = CASES[i]
    batch, sh = make(gen, S)
    seed = case_seed(S, b)
    rng = np.random.default_rng(seed)
    xbar = rng.standard_normal(12 * S)
    bt = one(batch, b)
    adj = Adjoint(bt, sh, xbar, CBAR)
    g = adj.grads()
    # strictly complementary; the generic candidates with every gradient unique (nondegenerate) too.  The scenario_1 candidate
    # has joints at which two fields tie: those entries are masked out (um_*), as the tests of the 64-segment kernels do,
    # and its directions are 0 there.
    assert adj.status in (1, 2) and adj.strict and (adj.unique or gen == "scenario1"), (CASES[i], adj.status, adj.strict, adj.unique)
    um = adj.unique_mask()
    p = "c%d_" % i
    out = {p + "hash": np.array(case_hash(batch, sh, b)), p + "seed": np.array(seed), p + "xbar": xbar, p + "cbar": np.array(CBAR),
           p + "x": adj.x, p + "act": adj.act, p + "lower": adj.lower}
    for k in KEYS:
        out[p + "g_" + k] = g[k]
        out[p + "um_" + k] = um[k]
    for t in range(2):
        dr = random_direction(rng, S)
        for k in KEYS:
            dr[k] = dr[k] * um[k]
        tg = Tangent(bt, sh, dr, adj=adj)
        # consistent: the targets of DEPENDENT active rows (a joint stated twice) agree, measured by the least-squares solve's
        # residual against 1e-7.  Where the active rows are independent (full_rank) every target is consistent, and the residual
        # is that solve's rounding alone: 1.4e-6 on a |dx| of 3.9 for one direction at 256 segments (a 4 600 x 4 600 system).
        assert tg.consistent or adj.full_rank, (CASES[i], t)
        for k in KEYS:
            out[p + "d%d_%s" % (t, k)] = dr[k]
        out[p + "dx%d" % t] = tg.dx
        out[p + "dcost%d" % t] = np.array(tg.dcost)
        out[p + "dcost_scale%d" % t] = np.array(tg.dcost_scale)
    ineq = (adj.u - adj.l) > 1e-12
    segs = sorted(set(int(s) for s in adj.row_seg[adj.act & ineq]))
    print("case %d %s: status %d, %d active inequality rows in segments %s" % (i, CASES[i], adj.status, int((adj.act & ineq).sum()), segs), flush=True)
    return out


# The shapes tests/test_gpu_long_grad.py runs at every seam of the lane mapping, five candidates each.
SEAMS = [("generic", S) for S in (65, 127, 128, 129, 192, 193, 255, 256)] + [("scenario1", 128)]


def strict_of(task):
    """(status, strictly complementary) of one candidate by the oracle's exact solve alone: vjp_reference.Adjoint's rule and
    margin, without its adjoint system (whose least-squares solve is most of the two minutes at 256 segments)."""
    from vjp_reference import dense, one
    gen, S, b = task
    batch, sh = make(gen, S)
    qp, P, A, q, l, u = dense(one(batch, b), sh)
    x, y, info = qp.solve_exact()
    margin = 1e-6
    Ax = A @ x
    eq = (u - l) <= 1e-12
    ymax = max(np.abs(y).max(), 1e-300)
    scale = 1.0 + np.maximum(np.abs(np.where(np.abs(l) < 1e9, l, 0)), np.abs(np.where(np.abs(u) < 1e9, u, 0)))
    slack = np.minimum(Ax - l, u - Ax)
    strict = bool(np.all(eq | (np.abs(y) > margin * ymax) | (slack > margin * scale)))
    # a weakly active row: an ACTIVE inequality row (Adjoint's rule: |y| above 1e-6 of the largest multiplier) whose multiplier
    # is at most 1e-4 of the largest inequality multiplier -- the upper end of the band tests/test_gpu_long_warm.py leaves out of
    # its support comparison.  Such a row is active at the optimum, and so for the derivative kernels, but an interior-point
    # iterate holds it at the slack mu / lambda and it gives way under a finite step: a difference quotient of the solve
    # does not see the optimum's derivative there.  (generic 193, candidate 0: one row at 3.0e-3 of 456, slack 5e-4 in the
    # oracle's own solution; generic 192, candidate 2: 1.8e-2 of 1 161; the next smallest multipliers: 1.36 and 0.84.)
    active = (~eq) & (np.abs(y) > margin * ymax)
    weak = bool((np.abs(y[active]) <= 1e-4 * np.abs(y[~eq]).max()).any())
    return gen, S, b, int(info.status), strict, weak


def strict_flags(procs=8):
    """`strict_<gen>_<S>` [5] bool for every shape of SEAMS: the candidates that are solved and strictly complementary -- the
    ones a derivative is defined on and a central difference can be held to.  45 exact solves, 1 s to 40 s each."""
    import multiprocessing
    tasks = sorted(((gen, S, b) for gen, S in SEAMS for b in range(5)), key=lambda t: -t[1])
    with multiprocessing.Pool(procs) as pool:
        res = pool.map(strict_of, tasks, chunksize=1)
    out = {}
    for gen, S in SEAMS:
        out["strict_%s_%d" % (gen, S)] = np.array([next(r[3] in (1, 2) and r[4] for r in res if r[:3] == (gen, S, b)) for b in range(5)])
        out["weak_%s_%d" % (gen, S)] = np.array([next(r[5] for r in res if r[:3] == (gen, S, b)) for b in range(5)])
        print("%s %d: (status, strict, weakly active row) %s" % (gen, S, [r[3:] for r in sorted(res) if r[:2] == (gen, S)]), flush=True)
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "strict":
        data = dict(np.load(OUT)) if os.path.exists(OUT) else {}
        data.update(strict_flags())
        np.savez_compressed(OUT, **data)
        print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
        return
    lo = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    hi = int(sys.argv[2]) if len(sys.argv) > 2 else len(CASES) - 1
    data = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    for i in range(lo, hi + 1):
        data.update(generate(i))
        np.savez_compressed(OUT, **data)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
