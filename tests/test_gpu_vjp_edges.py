"""btrapz_solve_vjp_device (vjp_kernel) at every edge of its lane mapping: the cases of tests/grad_edge_cases.py -- the
families and seeds of test_gpu_vjp.py at 3, 5, 10, 20, 21, 32, 33 and 63 segments, B = 253 -- with the oracle-based
yardstick (tests/vjp_reference.py) at the last group of wavefront 0 (next to the aliased spare lanes), at the first group of
wavefront 1 and at candidate B - 1, alone in the last wavefront beside the lanes clamped onto it.  Beside the yardstick:
the neighbouring slot's gradient must fail the same comparison, a candidate's gradient does not depend on B (bit for
bit), and records that mix segment counts 1 ... stride in strides 21 and 33 give the gradients of uniform calls (bit
for bit).  The tolerances are those of test_gpu_vjp.py."""
import numpy as np
import pytest
import torch

import grad_edge_cases as C
from grad_edge_cases import KEYS, PRIMAL_SEG, PRIMAL_SHARED, _cand, _close
from spectral_amd import layout as L
from vjp_reference import reference_vjp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def _ratios(mine, ref, um):
    """Per array: the largest error on the entries where the gradient is unique, relative to the array's norm for the
    candidate (the measure of test_vjp_against_the_yardstick)."""
    return {k: float((np.abs(mine[k] - ref[k]) * um[k]).max() / max(np.abs(ref[k]).max(), 1e-300)) for k in KEYS}


def _passes(mine, ref, um, keys=KEYS):
    """The assertions of test_vjp_against_the_yardstick as one verdict per array."""
    r = _ratios(mine, ref, um)
    ok = {k: r[k] <= 1e-4 for k in keys}
    if "seg" in keys:
        ok["seg"] = ok["seg"] and all(_close(mine["seg"][f], ref["seg"][f]) for f in PRIMAL_SEG)
    if "shared" in keys:
        ok["shared"] = ok["shared"] and _close(mine["shared"][PRIMAL_SHARED], ref["shared"][PRIMAL_SHARED])
    return ok


@pytest.mark.parametrize("family,S", C.CASES)
def test_vjp_at_the_lane_edges(solver, family, S):
    """One kept solve per form (lean 1, -1) and its solve_vjp, then on the packed form's gradients:

    the yardstick at every target slot -- primal-side fields by _close, every array on unique_mask() entries within 1e-4
    of the candidate's array norm; compared == len(targets), nothing skipped; the gradient returned for slot b - 1 fails
    slot b's comparison on seg or shared; lean and packed within 1e-5 of max(norm, 1), exact zeros for status outside
    {1, 2} and for field 0, over the whole batch; the same solve as the first 253 of 256 candidates gives every output
    row of candidates 0 ... 252 bit for bit.

    Then every kept multiplier of the target slots is set to NaN (what the solve itself can return: DESIGN 3.7, Active
    rows): the same yardstick assertions hold, every other candidate keeps its bits.

    Measured on an MI355X, one run, worst over the three families and the target slots (bound 1e-4):

        segments                         3       5       10      20      21      32      33      63
        ratio to the yardstick           6.9e-6  1.3e-5  2.3e-5  1.4e-5  1.3e-5  1.3e-5  1.2e-5  1.2e-5
        the same, multipliers NaN        6.9e-6  1.3e-5  2.3e-5  1.4e-5  1.3e-5  1.3e-5  1.2e-5  1.2e-5
        slot b - 1 against it, smallest  0.49    0.56    0.78    0.82    0.45    0.96    1.0     3.7     (seg)
                                         0.21    0.16    1.1     1.0     0.076   0.96    1.0     3.4     (shared)"""
    batch, sh, targets, _, _ = C.build(family, S)
    B = C.B
    d = solver.device
    rng = np.random.default_rng(S)
    xb, cb = rng.standard_normal((B, 12 * S)), rng.standard_normal(B)
    xbar, cbar = torch.tensor(xb, device=d), torch.tensor(cb, device=d)
    results = {}
    for lean in (1, -1):
        o, g = C._solve_and_vjp(solver, batch, sh, xbar, cbar, lean=lean)
        st = o["status"].cpu().numpy()
        results[lean] = (st, g, o)
        bad = (st != 1) & (st != 2)
        for k in KEYS:   # status outside {1, 2}: exactly 0; field 0: exactly 0
            arr = g[k] if k != "seg" else np.moveaxis(g[k], 1, 0)
            assert (arr[bad] == 0).all(), k
        assert (g["seg"][L.F_T] == 0).all()
    st, g, o = results[-1]
    for k in KEYS:   # the two forms solve to rounding: their gradients agree
        a, r = results[1][1][k], g[k]
        assert np.abs(a - r).max() <= 1e-5 * max(np.abs(r).max(), 1.0), k

    # ---- the yardstick at every target slot, and the neighbour's gradient against it ----
    compared, worst, refs = 0, 0.0, {}
    for b in targets:
        assert st[b] == 1, (family, S, b, st[b])
        ref, adj = reference_vjp(batch, sh, b, xb[b], cb[b])
        assert adj.strict, (family, S, b)
        um = adj.unique_mask()
        refs[b] = (ref, um)
        mine = _cand(g, b)
        for f in PRIMAL_SEG:
            assert _close(mine["seg"][f], ref["seg"][f]), (family, S, b, f)
        assert _close(mine["ref_end"], ref["ref_end"]), (family, S, b)
        assert _close(mine["shared"][PRIMAL_SHARED], ref["shared"][PRIMAL_SHARED]), (family, S, b)
        for k in KEYS:
            scale = max(np.abs(ref[k]).max(), 1e-300)
            bad_ = np.argwhere(um[k] & (np.abs(mine[k] - ref[k]) > 1e-4 * scale))
            assert bad_.size == 0, (family, S, b, k, [(tuple(i), mine[k][tuple(i)], ref[k][tuple(i)]) for i in bad_[:6]])
        r = _ratios(mine, ref, um)
        worst = max(worst, max(r.values()))
        verdict = _passes(mine, ref, um)
        assert all(verdict.values()), (family, S, b, verdict)
        # a kernel that read the neighbouring group would hand slot b the gradient of slot b - 1: that must not pass
        other = _passes(_cand(g, b - 1), ref, um, keys=("seg", "shared"))
        rn = _ratios(_cand(g, b - 1), ref, um)
        print("yardstick %s S=%d b=%d: %s; slot %d's gradient against it: seg %.1e shared %.1e" %
              (family, S, b, " ".join("%s %.1e" % (k, r[k]) for k in KEYS), b - 1, rn["seg"], rn["shared"]))
        assert not (other["seg"] and other["shared"]), (family, S, b, rn)
        compared += 1
    print("yardstick %s S=%d: %d slots compared, worst ratio %.3e" % (family, S, compared, worst))
    assert compared == len(targets) == len(C.target_slots(S))

    # ---- multipliers that are no numbers: the solve keeps its LAST iterate's, and that may be the non-finite one that
    #      ended it (cuboid, 10 segments, candidate 203 of this batch in the packed form).  The rows of such a candidate
    #      are classified by their slack; here every kept multiplier of the target slots is NaN ----
    db = solver.upload(batch)
    lam = o["lam"].clone(); lam[:, :, list(targets), :] = float("nan")
    gn = solver.solve_vjp(db, sh, dict(o, lam=lam), xbar, cbar)
    torch.cuda.synchronize()
    gn = {k: v.cpu().numpy() for k, v in gn.items()}
    others = np.setdiff1d(np.arange(B), targets)
    for k in KEYS:
        assert np.array_equal(gn[k][:, others] if k == "seg" else gn[k][others], g[k][:, others] if k == "seg" else g[k][others]), k
    for b in targets:
        ref, um = refs[b]
        rn = _ratios(_cand(gn, b), ref, um)
        print("yardstick %s S=%d b=%d, multipliers NaN: %s" % (family, S, b, " ".join("%s %.1e" % (k, rn[k]) for k in KEYS)))
        verdict = _passes(_cand(gn, b), ref, um)
        assert all(verdict.values()), (family, S, b, verdict, rn)

    # ---- a candidate's gradient does not depend on B: the lanes clamped onto B - 1 take no part ----
    rec, oe = C.extended_solve(db, o)
    g256 = solver.solve_vjp(rec, sh, oe, C.extended(xbar, 0), C.extended(cbar, 0))
    torch.cuda.synchronize()
    assert g256["shared"].shape[0] == C.B_EXT
    for k in KEYS:
        part = g256[k][:, :B] if k == "seg" else g256[k][:B]
        assert np.array_equal(part.cpu().numpy(), g[k]), (family, S, k)
    solved = torch.tensor((st == 1) | (st == 2), device=d)
    assert solved[:C.B_EXT - B].any() and (g256["shared"][B:][solved[:C.B_EXT - B]] != 0).any()   # (the added candidates are real work)


@pytest.mark.parametrize("family", C.RAGGED_FAMILIES)
@pytest.mark.parametrize("stride", C.RAGGED_STRIDES)
def test_mixed_counts_in_strides_that_do_not_divide_64(solver, family, stride):
    """A ragged record of stride 21 / 33 whose segment counts cycle over 1 ... stride, solved (kept) and differentiated in one
    call; then, for the counts 1, 2, stride - 1, stride and those either side of 64 / 3 and 64 / 2, the candidates of that
    count as a uniform record of that stride: the uniform call's gradients equal the ragged call's bit for bit, and the
    ragged seg slots beyond the count are exactly 0."""
    d = solver.device
    rec, sh, o, counts = C.ragged_solve(solver, family, stride)
    B = C.B
    rng = np.random.default_rng(stride)
    xbar = torch.tensor(rng.standard_normal((B, 12 * stride)), device=d); cbar = torch.tensor(rng.standard_normal(B), device=d)
    idx0 = torch.zeros(B, dtype=torch.int32, device=d)
    gr = solver.solve_vjp(rec, [sh], o, xbar, cbar, set_index=idx0)
    st = o["status"].cpu().numpy()
    solved = (st == 1) | (st == 2)
    assert solved.sum() >= B // 2, solved.sum()
    beyond = torch.arange(stride, device=d)[None, :] >= rec["seg_count"][:, None]
    assert (gr["seg"][:, beyond] == 0).all()
    done = 0
    for n in C.ragged_counts(stride):
        sel, u, ou = C.uniform_part(rec, o, counts, n)
        assert solved[counts == n].any(), (family, stride, n)
        gu = solver.solve_vjp(u, sh, ou, xbar[sel, :12 * n].contiguous(), cbar[sel].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(gu["seg"], gr["seg"][:, sel, :n]), (family, stride, n)
        assert (gr["seg"][:, sel, n:] == 0).all(), (family, stride, n)
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            assert torch.equal(gu[k], gr[k][sel]), (family, stride, n, k)
        assert (gu["shared"] != 0).any(), (family, stride, n)
        done += 1
    assert done == len(C.ragged_counts(stride))
