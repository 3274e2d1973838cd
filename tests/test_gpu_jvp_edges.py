"""btrapz_solve_jvp_device (jvp_kernel) at every edge of its lane mapping: the cases and target slots of
tests/grad_edge_cases.py (see test_gpu_vjp_edges.py) with the oracle-based yardstick (tests/jvp_reference.py) at the last
group of wavefront 0, the first group of wavefront 1 and candidate B - 1 alone in the last wavefront; the adjoint
identity against the VJP -- two separately written kernels -- on every solved candidate of the batch at every width
and on mixed-count records of strides 21 and 33; and the structure, bit for bit: a candidate's derivative does not
depend on B, ragged = uniform, T tangents in one call = T calls of one.  The tolerances are those of test_gpu_jvp.py
(DESIGN 3.10)."""
import numpy as np
import pytest
import torch

import grad_edge_cases as C
from grad_edge_cases import KEYS, SHAPES, _dev, _directions, _fmt, _identity, _per_tangent_ratios
from jvp_reference import Tangent
from spectral_amd import layout as L
from vjp_reference import one

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


@pytest.mark.parametrize("family,S", C.CASES)
def test_jvp_at_the_lane_edges(solver, family, S):
    """T = 2 tangents -- one dense in all five arrays, one dense in seg only, the entries of non-unique derivatives zeroed
    through unique_mask() at the compared slots -- on the kept solve of either form:

    the yardstick at every target slot, ctrl_dot and cost_dot of each tangent within 1e-4 of its own reference's norm
    (_per_tangent_ratios with its FLOOR), compared == len(targets), nothing skipped, and both references non-zero at a
    compared slot; exact zeros for status outside {1, 2}; the adjoint identity against the VJP on every solved candidate of
    the batch within 1e-4 (_identity as test_gpu_jvp.py has it); the same solve as the first 253 of 256 candidates gives
    ctrl_dot and cost_dot of candidates 0 ... 252 bit for bit; with every kept multiplier of the target slots NaN the
    yardstick assertions hold and every other candidate keeps its bits; at 21 segments T tangents = T calls, bit for bit.

    Measured on an MI355X, one run, worst over the three families, the forms and the target slots (bounds 1e-4):

        segments                   3        5        10       20       21       32       33       63
        yardstick, per tangent     7.3e-8   6.3e-6   7.0e-8   4.0e-7   2.2e-7   2.2e-6   1.3e-6   1.6e-7
        the same, multipliers NaN  7.3e-8   6.3e-6   7.0e-8   4.0e-7   2.2e-7   2.2e-6   1.3e-6   1.6e-7
        adjoint identity           1.9e-11  4.0e-10  8.4e-11  1.8e-10  6.7e-11  3.0e-10  2.9e-10  4.8e-11"""
    batch, sh, targets, _, adjoints = C.build(family, S)
    masks = C.unique_masks(family, S)
    B, T = C.B, 2
    rng = np.random.default_rng(S)
    tan = {k: np.zeros(SHAPES(T, B, S)[k]) for k in KEYS}
    for k in KEYS:
        tan[k][0] = rng.standard_normal(tan[k][0].shape)
    tan["seg"][1] = rng.standard_normal(tan["seg"][1].shape)
    for b in targets:
        um = masks[b]
        tan["seg"][:, :, b, :] *= um["seg"][None]
        for k in ("init", "ref_end", "dl_bounds", "shared"):
            tan[k][:, b] *= um[k][None]
    # the references: once per slot and tangent, for both forms
    refs = {}
    for b in targets:
        bt = one(batch, b)
        ref_x = np.zeros((T, 12 * S)); ref_c = np.zeros(T)
        for t in range(T):
            dr = {k: (tan[k][t, :, b, :] if k == "seg" else tan[k][t, b]).copy() for k in KEYS}
            dr["seg"][L.F_T] = 0.0
            tg = Tangent(bt, sh, dr, adj=adjoints[b])
            ref_x[t], ref_c[t] = tg.dx, tg.dcost
        refs[b] = (ref_x, ref_c)
    seen = np.zeros(T)
    tan_d = _dev(solver, tan)
    for lean in (-1, 1):
        db, o = C._solve(solver, batch, sh, lean=lean)
        st = o["status"].cpu().numpy()
        j = solver.solve_jvp(db, sh, o, tan_d)
        torch.cuda.synchronize()
        cd, cs = j["ctrl"].cpu().numpy(), j["cost"].cpu().numpy()
        bad = (st != 1) & (st != 2)
        assert (cd[:, bad] == 0).all() and (cs[:, bad] == 0).all()
        compared, worst = 0, 0.0
        for b in targets:
            assert st[b] == 1, (family, S, lean, b, st[b])
            ref_x, ref_c = refs[b]
            ex, ec = _per_tangent_ratios(cd[:, b], cs[:, b], ref_x, ref_c)
            worst = max(worst, ex.max(), ec.max())
            print("yardstick %s S=%d lean=%d b=%d: ctrl_dot %s cost_dot %s of each tangent's norm; |ref dx| %s" %
                  (family, S, lean, b, _fmt(ex), _fmt(ec), _fmt(np.abs(ref_x).max(1))))
            assert (ex <= 1e-4).all() and (ec <= 1e-4).all(), (family, S, lean, b, ex, ec)
            # the neighbouring slot's derivative is another one: a kernel that read the wrong group would not pass
            nx, nc = _per_tangent_ratios(cd[:, b - 1], cs[:, b - 1], ref_x, ref_c)
            assert (nx > 1e-4).all(), (family, S, lean, b, nx, nc)
            seen = np.maximum(seen, np.abs(ref_x).max(1))
            compared += 1
        print("yardstick %s S=%d lean=%d: %d slots compared, worst ratio %.3e" % (family, S, lean, compared, worst))
        assert compared == len(targets) == len(C.target_slots(S))
    # 0 == 0 is no agreement: both tangents must have moved a compared candidate
    assert (seen > 0).all(), seen

    # ---- multipliers that are no numbers (test_gpu_vjp_edges.py): every kept multiplier of the target slots NaN, their
    #      rows classified by the slack; every other candidate bit for bit as before ----
    lam = o["lam"].clone(); lam[:, :, list(targets), :] = float("nan")
    jn = solver.solve_jvp(db, sh, dict(o, lam=lam), tan_d)
    torch.cuda.synchronize()
    others = torch.tensor(np.setdiff1d(np.arange(B), targets), device=solver.device)
    assert torch.equal(jn["ctrl"][:, others], j["ctrl"][:, others]) and torch.equal(jn["cost"][:, others], j["cost"][:, others])
    for b in targets:
        ex, ec = _per_tangent_ratios(jn["ctrl"][:, b].cpu().numpy(), jn["cost"][:, b].cpu().numpy(), *refs[b])
        print("yardstick %s S=%d b=%d, multipliers NaN: ctrl_dot %s cost_dot %s" % (family, S, b, _fmt(ex), _fmt(ec)))
        assert (ex <= 1e-4).all() and (ec <= 1e-4).all(), (family, S, b, ex, ec)

    # ---- the adjoint identity against the VJP on every solved candidate (the last solve: the lean form's) ----
    worst = _identity(solver, db, sh, o, None, S, seed=S)
    print("adjoint identity %s S=%d: worst |lhs - rhs| / sum |terms| = %.3e" % (family, S, worst))
    assert worst <= 1e-4, (family, S, worst)

    # ---- a candidate's derivative does not depend on B: the lanes clamped onto B - 1 take no part ----
    rec, oe = C.extended_solve(db, o)
    j256 = solver.solve_jvp(rec, sh, oe, {k: C.extended(v, 2 if k == "seg" else 1) for k, v in tan_d.items()})
    torch.cuda.synchronize()
    assert j256["ctrl"].shape[1] == C.B_EXT
    assert torch.equal(j256["ctrl"][:, :B], j["ctrl"]) and torch.equal(j256["cost"][:, :B], j["cost"]), (family, S)
    solved = torch.tensor((st == 1) | (st == 2), device=solver.device)[:C.B_EXT - B]
    assert solved.any() and (j256["ctrl"][:, B:][:, solved] != 0).any()   # (the added candidates are real work)

    # ---- T tangents in one call = T calls of one tangent (the factor stays in registers across the tangent loop) ----
    if S == 21:
        for t in range(T):
            jt = solver.solve_jvp(db, sh, o, {k: v[t:t + 1].contiguous() for k, v in tan_d.items()})
            assert torch.equal(jt["ctrl"][0], j["ctrl"][t]) and torch.equal(jt["cost"][0], j["cost"][t]), (family, t)


@pytest.mark.parametrize("family", C.RAGGED_FAMILIES)
@pytest.mark.parametrize("stride", C.RAGGED_STRIDES)
def test_mixed_counts_in_strides_that_do_not_divide_64(solver, family, stride):
    """The ragged records of test_gpu_vjp_edges.py (stride 21 / 33, segment counts cycling over 1 ... stride), T = 3 dense
    tangents: the adjoint identity against the VJP on every solved candidate within 1e-4; for the counts 1, 2, stride - 1,
    stride and those either side of 64 / 3 and 64 / 2 the candidates of that count as a uniform record give ctrl_dot and
    cost_dot of the ragged call bit for bit, and the ragged ctrl_dot slots beyond 12 x count are exactly 0; at stride 33,
    T tangents in one call = T calls of one tangent, bit for bit.

    Measured on an MI355X, one run: adjoint identity 2.5e-10 (stride 21) and 3.5e-9 (stride 33), worst of the two
    families."""
    d = solver.device
    rec, sh, o, counts = C.ragged_solve(solver, family, stride)
    B, T = C.B, 3
    idx0 = torch.zeros(B, dtype=torch.int32, device=d)
    worst = _identity(solver, rec, [sh], o, idx0, stride, seed=stride)
    print("adjoint identity %s ragged stride %d: worst |lhs - rhs| / sum |terms| = %.3e" % (family, stride, worst))
    assert worst <= 1e-4, (family, stride, worst)
    tan = _dev(solver, _directions(np.random.default_rng(stride + 1), T, B, stride))
    jr = solver.solve_jvp(rec, [sh], o, tan, set_index=idx0)
    st = o["status"].cpu().numpy()
    solved = (st == 1) | (st == 2)
    beyond = torch.arange(12 * stride, device=d)[None, :] >= 12 * rec["seg_count"][:, None]
    assert (jr["ctrl"][:, beyond] == 0).all()
    done = 0
    for n in C.ragged_counts(stride):
        sel, u, ou = C.uniform_part(rec, o, counts, n)
        assert solved[counts == n].any(), (family, stride, n)
        tu = {k: (v[:, :, sel, :n] if k == "seg" else v[:, sel]).contiguous() for k, v in tan.items()}
        ju = solver.solve_jvp(u, sh, ou, tu)
        torch.cuda.synchronize()
        assert torch.equal(ju["ctrl"], jr["ctrl"][:, sel, :12 * n]), (family, stride, n)
        assert (jr["ctrl"][:, sel, 12 * n:] == 0).all(), (family, stride, n)
        assert torch.equal(ju["cost"], jr["cost"][:, sel]), (family, stride, n)
        assert (ju["ctrl"] != 0).any(), (family, stride, n)
        done += 1
    assert done == len(C.ragged_counts(stride))
    if stride == 33:
        for t in range(T):
            jt = solver.solve_jvp(rec, [sh], o, {k: v[t:t + 1].contiguous() for k, v in tan.items()}, set_index=idx0)
            assert torch.equal(jt["ctrl"][0], jr["ctrl"][t]) and torch.equal(jt["cost"][0], jr["cost"][t]), (family, t)
