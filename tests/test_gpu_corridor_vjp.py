"""The backward pass of the device corridor stage (btrapz_corridor_batch_vjp_device) on the GPU: against the yardstick of
tests/corridor_vjp_reference.py (central differences of the oracle's record, computed tolerance), against its host twin,
on inputs with more than 16 selected segments and a span moved by the overlap step, its defined cases, determinism, refusals,
and the autograd layer diff.corridor: alone, and in front of diff.solve and diff.traj_cost against central differences of
the whole pipeline."""
import numpy as np
import pytest
import torch

import corridor_vjp_cases as K
import corridor_vjp_reference as R
from spectral_amd import diff, layout as L, synth
from spectral_amd.native import BtrapzError, KNOT_GRADS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


def dev(solver, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(solver.device, dtype=torch.float64).contiguous()


def device_grads(solver, kb, variant, sb, rb, db, want=KNOT_GRADS, seg_stride=K.SEG_STRIDE):
    g = solver.corridor_batch_vjp(kb, variant, dev(solver, sb), dev(solver, rb), dev(solver, db), want=want, seg_stride=seg_stride)
    torch.cuda.synchronize()
    return {k: g[k].cpu().numpy() for k in want}


def batches():
    return [("scenario", K.scenario(4))] + [("c1", K.c1(4))] + [("fuzz%d" % s, K.fuzz(s)) for s in K.FUZZ_SEEDS]


@pytest.mark.parametrize("variant", [0, 1])
def test_kernel_against_yardstick(solver, variant):
    floor, h_max, shared = 0, 0.0, False
    for name, kb in batches():
        sb, rb, db = K.cotangents(kb.B)
        g = device_grads(solver, kb, variant, sb, rb, db)
        rec = solver.corridor_batch(kb, variant, seg_stride=K.SEG_STRIDE)
        counts = rec["seg_count"].cpu().numpy()
        checked = [b for b in range(kb.B) if counts[b] >= 1][:2]
        assert checked, name
        for b in checked:
            jac = R.jacobian(kb, b, variant, key=(name, kb.B, b, variant))
            assert jac["n"] == counts[b], (name, b)
            floor += R.check_caps(jac)
            h_max = max(h_max, R.max_pieces_in_front(jac) * kb.delta); shared = shared or R.shared_origin(jac)
            worst = R.compare(jac, {k: v[b] for k, v in g.items()}, R.flat_cotangent(jac["n"], sb[:, b], rb[b], db[b]), (name, b, variant))
            print(name, b, "worst error / tolerance:", worst)
    assert floor >= 15 and h_max >= 2.0 - 1e-6 and shared, (floor, h_max, shared)


def equals_host_twin(solver, kb, variant, g, sb, rb, db, seg_stride, name=""):
    """Every candidate of the batch: the forward's seg_count is the host twin's, the gradients agree to the yardstick's computed
    tolerance (from the forward's own record).  Returns the counts."""
    rec = solver.corridor_batch(kb, variant, seg_stride=seg_stride)
    counts = rec["seg_count"].cpu().numpy(); seg = rec["seg"].cpu().numpy()
    for b in range(kb.B):
        h, n = K.host_grads(kb, b, variant, sb, rb, db, seg_stride=seg_stride)
        assert n == counts[b], (name, b, n, counts[b])
        y = np.concatenate([seg[1:, b, :max(n, 0)].ravel(), rec["ref_end"][b].cpu().numpy(), rec["dl_bounds"][b].cpu().numpy()])
        yb = R.flat_cotangent(max(n, 0), sb[:, b], rb[b], db[b])
        tol = 4.0 * float(np.sum(np.abs(yb) * 4.0 * np.spacing(np.abs(y)))) / (2 * R.H_STEP)
        for k in KNOT_GRADS:
            assert np.abs(g[k][b] - h[k]).max() <= tol, (name, b, k)
    return counts, seg


@pytest.mark.parametrize("variant", [0, 1])
def test_device_against_host_twin(solver, variant):
    for name, kb in batches() + [("mixed", K.fuzz(K.MIXED_SEED))]:
        sb, rb, db = K.cotangents(kb.B, seed=3)
        g = device_grads(solver, kb, variant, sb, rb, db)
        equals_host_twin(solver, kb, variant, g, sb, rb, db, K.SEG_STRIDE, name)


def test_provenance_through_sort_reorder_and_overlap(solver):
    """More than 16 selected segments (std::sort's order is not the stable one there), tied first knots, and an overlap step
    that moves a beg_t: the ds walk is over the final span.  Candidate 0 against the yardstick, all four against the host twin."""
    kb = K.tied(K.TIED_SEED)
    sb, rb, db = K.cotangents(kb.B, seed=7, seg_stride=K.TIED_STRIDE)
    g = device_grads(solver, kb, 0, sb, rb, db, seg_stride=K.TIED_STRIDE)
    counts, seg = equals_host_twin(solver, kb, 0, g, sb, rb, db, K.TIED_STRIDE, "tied")
    assert ((counts >= 17) & (counts <= 26)).all(), counts
    jac = R.jacobian(kb, 0, 0, key=("tied", K.TIED_SEED, 0, 0))
    (n, spans, _), _ = R.record(R.one_candidate(kb, 0), 0)
    assert n == counts[0] and n > 16 and R.check_caps(jac) >= 15
    moved = K.moved_spans(jac, spans, kb.N, kb.delta)
    assert moved, "the overlap step moved no beg_t"
    assert all(seg[L.F_T, 0, k] == (spans[k][1] - spans[k][0]) * kb.delta for k in moved)   # the device's span is the moved one
    print("n", n, "moved", moved, "worst error / tolerance:",
          R.compare(jac, {k: v[0] for k, v in g.items()}, R.flat_cotangent(n, sb[:, 0], rb[0], db[0]), "tied"))


def test_every_output_slot_in_use(solver):
    """seg_stride 64 with a corridor of 64 segments (the ref_end terms sit in a 65th row of the ordered pass), neighbours of 60
    and 63, and a selection beyond the stage's 64 (seg_count -1: zeros) -- against the host twin."""
    kb = K.full()
    sb, rb, db = K.cotangents(kb.B, seed=8, seg_stride=64)
    g = device_grads(solver, kb, 0, sb, rb, db, seg_stride=64)
    counts, _ = equals_host_twin(solver, kb, 0, g, sb, rb, db, 64, "full")
    assert 64 in counts and -1 in counts, counts
    for b in range(kb.B):
        assert g["s_ref"][b, kb.N - 1] != 0 if counts[b] > 0 else not any(g[k][b].any() for k in KNOT_GRADS), b


def test_defined_cases(solver):
    kb = K.fuzz(K.MIXED_SEED)
    rec = solver.corridor_batch(kb, 0, seg_stride=K.SEG_STRIDE)
    counts = rec["seg_count"].cpu().numpy()
    assert 0 in counts and -1 in counts and (counts >= 1).sum() >= 2, counts
    sb, rb, db = K.cotangents(kb.B, seed=4)
    g = device_grads(solver, kb, 0, sb, rb, db)
    for b in range(kb.B):
        if counts[b] < 1:   # no corridor: zeros in every entry
            assert all(not g[k][b].any() for k in KNOT_GRADS), b
        else:               # the neighbours: what they get alone
            one = R.one_candidate(kb, b)
            g1 = device_grads(solver, one, 0, sb[:, b:b + 1], rb[b:b + 1], db[b:b + 1])
            assert g["s_bounds"][b].any() and all(np.array_equal(g[k][b], g1[k][0]) for k in KNOT_GRADS), b
    # cotangents in slots >= seg_count, and of field 0, are ignored
    sb2 = sb.copy(); sb2[0] = 1e30
    for b in range(kb.B):
        sb2[:, b, max(counts[b], 0):] = -1e30
    g2 = device_grads(solver, kb, 0, sb2, rb, db)
    assert all(np.array_equal(g[k], g2[k]) for k in KNOT_GRADS)
    # the tie rule: on a plateau of ds_bounds the earliest knot of the final span gets the gradient
    kb = K.scenario(4)
    kb.ds_bounds[..., 0] = 0.5; kb.ds_bounds[..., 1] = 7.0
    sb = np.zeros((L.NUM_SEG_FIELDS, kb.B, K.SEG_STRIDE)); sb[L.F_DS_LO] = 1.0; sb[L.F_DS_HI] = -1.0
    g = device_grads(solver, kb, 0, sb, None, None, want=("ds_bounds",))["ds_bounds"]
    for b in range(kb.B):
        (n, spans, _), _ = R.record(R.one_candidate(kb, b), 0)
        want = np.zeros((kb.N, 2))
        for bt, et in spans:
            want[min(max(bt, 0), kb.N - 1)] += (1.0, -1.0)
        assert np.array_equal(g[b], want), b


def test_deterministic_and_any_subset_of_outputs(solver):
    kb = K.c1(8, seed=2)
    sb, rb, db = K.cotangents(kb.B, seed=5)
    g = device_grads(solver, kb, 0, sb, rb, db)
    again = device_grads(solver, kb, 0, sb, rb, db)
    assert all(np.array_equal(g[k], again[k]) for k in KNOT_GRADS) and g["s_bounds"].any()
    for want in (("s_bounds",), ("l_ref", "ds_bounds"), ("dl_bounds_knots",), ("l_bounds", "s_ref")):
        part = device_grads(solver, kb, 0, sb, rb, db, want=want)
        assert all(np.array_equal(part[k], g[k]) for k in want), want
    only_seg = device_grads(solver, kb, 0, sb, None, None)
    only_rest = device_grads(solver, kb, 0, None, rb, db)   # (no segment cotangent: the stride is given)
    with pytest.raises(ValueError):
        solver.corridor_batch_vjp(kb, 0, None, dev(solver, rb), dev(solver, db))
    assert not only_seg["dl_bounds_knots"].any() and only_rest["dl_bounds_knots"].any() and not only_rest["s_bounds"].any()


def test_refusals(solver):
    d = solver.device
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=d)

    def call(B=2, N=21, O=2, S=16, bars=(True, True, True), want=KNOT_GRADS):
        ins = [z(B, O, N, 2), z(B, O, N, 2), z(B, N, 2), z(B, N, 2), z(B, N), z(B, N)]
        like = dict(zip(KNOT_GRADS, ins))
        grads = {k: torch.empty_like(like[k]) for k in want}
        solver.ctx.corridor_batch_vjp_device(0, B, N, O, 0.1, *ins, S, z(L.NUM_SEG_FIELDS, B, S) if bars[0] else None,
                                             z(B, 2) if bars[1] else None, z(B, 10) if bars[2] else None, grads)
    call()
    for kw, text in ((dict(N=513), "not differentiated"), (dict(O=65), "not differentiated"), (dict(S=65), "not differentiated"),
                     (dict(bars=(False, False, False)), "all null"), (dict(want=()), "no output"), (dict(N=2), "N >= 3")):
        with pytest.raises(BtrapzError, match=text):
            call(**kw)


def test_diff_corridor_backward_is_the_direct_call(solver):
    kb = K.scenario(4)
    names = ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds", "s_ref", "l_ref")
    ins = [dev(solver, getattr(kb, n)).requires_grad_(True) for n in names]
    seg, count, ref_end, dl10 = diff.corridor(solver, *ins, variant=0, delta=kb.delta, seg_stride=K.SEG_STRIDE)
    rec = solver.corridor_batch(kb, 0, seg_stride=K.SEG_STRIDE)
    assert torch.equal(seg, rec["seg"]) and torch.equal(count, rec["seg_count"]) and not count.requires_grad
    sb, rb, db = K.cotangents(kb.B, seed=6)
    torch.autograd.backward([seg, ref_end, dl10], [dev(solver, sb), dev(solver, rb), dev(solver, db)])
    g = device_grads(solver, kb, 0, sb, rb, db)
    for t, k in zip(ins, KNOT_GRADS):
        assert np.array_equal(t.grad.cpu().numpy(), g[k]), k


def test_diff_corridor_solve_traj_cost_against_central_differences(solver):
    """knots -> diff.corridor -> diff.solve -> diff.traj_cost, the sum of the scores of the candidates that are solved and
    strictly complementary (the criterion of tests/vjp_reference.py on the record the stage wrote): its gradient w.r.t. a
    dozen s_bounds entries with a non-zero Jacobian against central differences of the whole GPU pipeline, to 1e-3 of the norm
    of the gradient over the checked entries (DESIGN 3.7's tolerance for central differences of the solve).  Which entries have
    a non-zero Jacobian is read off the forward stage alone: one launch over copies of a candidate with one entry moved each."""
    from vjp_reference import Adjoint
    kb = synth.scenario1_knots(8, 8)
    sh = synth.shared_params(0, delta=kb.delta)
    d = solver.device
    prm = torch.tensor(diff.params_from_shared(sh), device=d)
    base = [dev(solver, getattr(kb, n)) for n in ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds", "s_ref", "l_ref")]
    init = dev(solver, kb.init)

    def pipeline(ins, init):
        seg, cnt, ref_end, dl10 = diff.corridor(solver, *ins, variant=0, delta=kb.delta, seg_stride=K.SEG_STRIDE)
        ctrl, _, st = diff.solve(solver, seg, init, ref_end, dl10, prm, seg_count=cnt, variant=0, delta=kb.delta)
        cost = diff.traj_cost(ctrl, seg, init, ins[4], ins[5], prm, solver, seg_count=cnt, status=st, variant=0, delta=kb.delta)
        return cost, st, cnt, seg, ref_end, dl10

    s = base[0].clone().requires_grad_(True)
    cost, st, cnt, seg, ref_end, dl10 = pipeline([s] + base[1:], init)
    stn, cn, segn = st.cpu().numpy(), cnt.cpu().numpy(), seg.detach().cpu().numpy()
    ren, dln = ref_end.detach().cpu().numpy(), dl10.detach().cpu().numpy()
    kept = []
    for b in range(kb.B):
        if stn[b] in (1, 2) and cn[b] >= 1:
            n = int(cn[b])
            one = L.Batch(B=1, S=n, seg=np.ascontiguousarray(segn[:, b:b + 1, :n]), init=kb.init[b:b + 1].copy(), ref_end=ren[b:b + 1].copy(),
                          dl_bounds=dln[b:b + 1].copy())
            if Adjoint(one, sh, np.zeros(12 * n), 0.0).strict:
                kept.append(b)
    print("solved and strictly complementary:", kept, "status", stn, "segments", cn)
    assert len(kept) >= 2
    cost[torch.tensor(kept, device=d)].sum().backward()
    grad = s.grad.cpu().numpy()
    assert not grad[[b for b in range(kb.B) if b not in kept]].any()

    # the entries of a kept candidate whose move changes the record and no decision (segment count, durations)
    O_, N = kb.num_obs, kb.N
    step = lambda x: 1e-4 * (1.0 + abs(x))
    entries = []
    with torch.no_grad():
        for b in kept[:6]:
            copies = [t[b:b + 1].repeat(O_ * N * 2, *([1] * (t.dim() - 1))).contiguous() for t in base]
            flat = copies[0].reshape(O_ * N * 2, O_ * N * 2)
            flat += torch.diag(dev(solver, [step(x) for x in kb.s_bounds[b].reshape(-1)]))
            sg, ct, _, _ = diff.corridor(solver, *copies, variant=0, delta=kb.delta, seg_stride=K.SEG_STRIDE)
            sg, ct = sg.cpu().numpy(), ct.cpu().numpy()
            n = int(cn[b])   # (slots beyond the count are not the stage's to write)
            same = (ct == n) & (sg[L.F_T, :, :n] == segn[L.F_T, b, :n]).all(axis=1)
            moves = (sg[1:, :, :n] != segn[1:, b, None, :n]).any(axis=(0, 2))
            hits = np.flatnonzero(same & moves)
            entries += [(b, int(c)) for c in hits]
    assert len(entries) >= 12

    # central differences of the whole pipeline: one run over the moved copies of every such entry.  An entry stays only if
    # both moved pipelines are solved with the decisions of the centre (elsewhere there is no central difference).  Most
    # bounds are not active in the solve, so their central difference is round-off: the dozen takes up to eight entries whose
    # central difference is above 1e-3 of the largest -- chosen by the reference, not by the gradient under test -- and
    # fills up with the others; both lists thinned evenly.
    M = len(entries)
    with torch.no_grad():
        idx = torch.tensor([b for b, _ in entries] * 2, device=d)
        copies = [t[idx].contiguous() for t in base]
        hs = np.array([step(kb.s_bounds[b].reshape(-1)[c]) for b, c in entries])
        flat = copies[0].reshape(2 * M, -1)
        for i, (b, c) in enumerate(entries):
            flat[i, c] += hs[i]; flat[M + i, c] -= hs[i]
        c2, st2, cnt2, seg2, _, _ = pipeline(copies, init[idx].contiguous())
        c2, st2, cnt2, seg2 = c2.cpu().numpy(), st2.cpu().numpy(), cnt2.cpu().numpy(), seg2.cpu().numpy()
    rows = [b for b, _ in entries] * 2
    ok = np.array([st2[i] in (1, 2) and cnt2[i] == cn[b] and (seg2[L.F_T, i, :cn[b]] == segn[L.F_T, b, :cn[b]]).all() for i, b in enumerate(rows)])
    usable = np.flatnonzero(ok[:M] & ok[M:])
    print("entries with a non-zero Jacobian: %d, with a central difference: %d" % (M, usable.size))
    assert usable.size >= 12
    with np.errstate(invalid="ignore"):   # (an unsolved copy scores +inf)
        fd_all = (c2[:M] - c2[M:]) / (2 * hs)
    thin = lambda v, k: v[np.linspace(0, v.size - 1, min(k, v.size)).astype(int)] if v.size else v
    big = usable[np.abs(fd_all[usable]) > 1e-3 * np.abs(fd_all[usable]).max()]
    big = thin(big, 8)
    pick = np.sort(np.concatenate([big, thin(np.setdiff1d(usable, big), 12 - big.size)]))
    assert pick.size == 12 and big.size >= 2
    print("checked entries (candidate, o, knot, side):", [(entries[i][0],) + tuple(int(v) for v in np.unravel_index(entries[i][1], (O_, N, 2))) for i in pick])
    entries, fd = [entries[i] for i in pick], fd_all[pick]
    an = np.array([grad[b].reshape(-1)[c] for b, c in entries])
    norm = float(np.linalg.norm(an))
    print("autograd", an, "central differences", fd, "worst error / norm: %.3e" % (np.abs(fd - an).max() / norm))
    assert norm > 0 and np.abs(fd - an).max() <= 1e-3 * norm
