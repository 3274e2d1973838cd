"""The lean two-launch solve with one axis QUIET (spectral_amd/csrc/btrapz_lean_quiet.hip): the capped launch
of the first axis and the bucketing of its lists, then ONE grid of that axis's resume wavefronts and, behind them, the
other axis through the plain one-launch body -- no cap, no lists, no resume launch for it.  Forced with
btrapz_debug_set_schedule (3: s first, l quiet; 4: l first, s quiet) and held, bit for bit, to the one-launch lean solve:
status, iteration counts, costs, and the control points of the solved candidates.  Then the rule that chooses the
schedule by itself, and the estimate that brings a context back from it when the quiet axis starts to talk."""
import functools

import numpy as np
import pytest

from spectral_amd import synth
from test_gpu_lean_pipeline import fetch, run, same

pytestmark = pytest.mark.gpu
MODES = (3, 4)       # mode m: axis m - 3 first, axis 4 - m quiet


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    s = BatchSolver(0)
    yield s
    s.ctx.debug_set_schedule(0)


@functools.lru_cache(maxsize=None)
def scenario1(B, S, variant):
    return synth.make_scenario1_batch(B, S, variant)


@functools.lru_cache(maxsize=None)
def generic(B, S, config):
    return synth.make_batch(B, S, config=config)


def quiet_against_one_launch(solver, batch, sh, cap, **kw):
    """Both forced orders against the one-launch solve; the quiet axis never hands over.  Returns {mode: keys}."""
    one, n1, f1, _ = run(solver, batch, sh, 0, cap_iter=-1, **kw)
    assert (n1, f1) == (1, 8)
    keys = {}
    for mode in MODES:
        res, n, form, keys[mode] = run(solver, batch, sh, mode, cap_iter=cap, **kw)
        assert (n, form) == (3, 11), (mode, n, form)
        same(one, res, ("mode", mode))
        assert (keys[mode][4 - mode] == 0).all(), (mode, keys[mode][4 - mode])
    return keys


@pytest.mark.parametrize("B", [1, 2, 3, 4, 64, 1000])
def test_grid_edges(solver, B):
    """A last wavefront that is partly filled (three groups per wavefront at 20 segments) and a group that is alone from
    the first iteration on: under the cap such a group hands over (at B = 1 both axes do, test_gpu_lean_pipeline.py); on
    the quiet axis it goes on to the end where it is."""
    batch, sh = scenario1(B, 20, 0)
    keys = quiet_against_one_launch(solver, batch, sh, 3)
    if B == 1:
        for mode in MODES:
            assert (keys[mode][mode - 3] > 0).all(), keys[mode]


@pytest.mark.parametrize("S", [16, 21, 32, 33, 64])
def test_groups_per_wavefront(solver, S):
    """4, 3, 2, 1 and 1 groups per wavefront, on a batch of which BOTH axes spread: three launches with the cap on both
    axes (modes 1 / 2) hand over on either, the quiet schedule on the first axis only -- what tells it from them."""
    batch, sh = generic(257, S, 2)
    keys = quiet_against_one_launch(solver, batch, sh, 4)
    capped = {mode: run(solver, batch, sh, mode, cap_iter=4)[3] for mode in (1, 2)}
    print("S", S, "handed over (s, l): quiet", {m: (keys[m] > 0).sum(axis=1).tolist() for m in MODES},
          "capped", {m: (capped[m] > 0).sum(axis=1).tolist() for m in (1, 2)})
    for mode in MODES:
        first, quiet = mode - 3, 4 - mode
        assert (keys[mode][first] > 0).any()
        assert (capped[mode - 2][quiet] > 0).any()       # the premise: under the cap this axis does hand over
        assert np.array_equal(keys[mode][first], capped[mode - 2][first])   # the first axis goes exactly today's way


def test_nothing_handed_over(solver):
    """The resume part of the grid finds an empty list."""
    batch, sh = scenario1(512, 20, 0)
    keys = quiet_against_one_launch(solver, batch, sh, 22)
    for mode in MODES:
        assert (keys[mode] > 0).sum() == 0


def test_cuboid_variant_in_memory_order(solver):
    """The cuboid variant without its pre-pass (compact = -1: the memory-order path).  A quarter of its candidates cannot
    start: groups that are alone from the first iteration on, which the quiet axis carries to the end."""
    batch, sh = scenario1(6144, 20, 1)
    keys = quiet_against_one_launch(solver, batch, sh, 5, compact=-1)
    assert (keys[3][0] > 0).sum() > 0


@pytest.mark.parametrize("mode", MODES)
def test_back_to_back_without_a_host_sync(solver, mode):
    """6 144 candidates, then 64, then 6 144 of another family on one context and stream, nothing in between: no list,
    table, count or estimate of the call before leaks into the next."""
    import torch
    batches = [scenario1(6144, 20, 0), scenario1(64, 20, 0), generic(6144, 20, 3)]
    dbs = [solver.upload(b) for b, _ in batches]
    ones = []
    for db, (b, sh) in zip(dbs, batches):
        o = solver.solve(db, sh, split=-1, lean=1, cap_iter=-1, out=solver.new_result(b.B, b.S))
        torch.cuda.synchronize()
        ones.append(fetch(o))
    outs = [solver.new_result(b.B, b.S) for b, _ in batches]
    torch.cuda.synchronize()
    solver.ctx.debug_set_schedule(mode)
    launches = []
    for db, (b, sh), out in zip(dbs, batches, outs):
        solver.solve(db, sh, split=-1, lean=1, cap_iter=6, out=out)
        launches.append(solver.ctx.debug_solve_launches())
    torch.cuda.synchronize()
    solver.ctx.debug_set_schedule(0)
    assert launches == [3, 3, 3]
    for i, (one, out) in enumerate(zip(ones, outs)):
        same(one, fetch(out), ("solve", i))


def test_automatic_rule():
    """A fresh context knows nothing: two launches.  scenario_1 hands over on the s axis only (1 067 : 0 at this shape), so
    the next solve runs s first and l quiet.  A generic batch of the same shape still runs that schedule once -- its l axis
    spreads but hands nothing over: empty keys -- and the ESTIMATE that solve leaves for l (of the order of what s handed
    over) brings the next one back to two launches.  The results never depend on any of it."""
    import torch
    from spectral_amd.solver import BatchSolver
    s1, sh1 = scenario1(6144, 20, 0)
    gen, shg = generic(6144, 20, 3)

    def solve(solver, db, sh, **kw):
        o = solver.solve(db, sh, split=-1, lean=1, **kw)
        torch.cuda.synchronize()
        return fetch(o), solver.ctx.debug_solve_launches()

    solver = BatchSolver(0)
    d1, dg = solver.upload(s1), solver.upload(gen)
    one, n = solve(solver, d1, sh1, cap_iter=-1)
    assert n == 1
    first, n = solve(solver, d1, sh1, cap_iter=6)
    assert n == 2
    second, n = solve(solver, d1, sh1, cap_iter=6)
    assert n == 3
    same(one, first, "two launches"); same(one, second, "s first, l quiet")
    keys = solver.ctx.debug_resume_keys(6144)
    assert (keys[0] > 0).sum() > 0 and (keys[1] > 0).sum() == 0

    fresh = BatchSolver(0)
    dg2 = fresh.upload(gen)
    gone, n = solve(fresh, dg2, shg, cap_iter=-1)
    g1, n1 = solve(fresh, dg2, shg, cap_iter=6)
    two_launch_keys = fresh.ctx.debug_resume_keys(6144)
    g2, n2 = solve(fresh, dg2, shg, cap_iter=6)
    assert (n1, n2) == (2, 2)
    same(gone, g1, "generic, first"); same(gone, g2, "generic, second")
    assert (two_launch_keys[1] > 0).sum() > 0            # the premise: under the cap the generic batch's l axis talks

    g3, n3 = solve(solver, dg, shg, cap_iter=6)
    keys = solver.ctx.debug_resume_keys(6144)
    g4, n4 = solve(solver, dg, shg, cap_iter=6)
    print("generic: handed over under the cap (s, l)", (two_launch_keys > 0).sum(axis=1), "quiet schedule", (keys > 0).sum(axis=1))
    assert n3 == 3 and (keys[0] > 0).sum() > 0 and (keys[1] > 0).sum() == 0     # the quiet schedule ran
    assert n4 == 2                                                               # ... and its estimate said that l talks
    same(gone, g3, "generic after scenario_1"); same(gone, g4, "generic, its own counts")
