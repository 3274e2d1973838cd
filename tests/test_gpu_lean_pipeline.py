"""The lean two-launch solve as THREE launches on one stream (spectral_amd/csrc/btrapz_lean_pipe.hip): the
capped launch of one axis, one grid of that axis's resume wavefronts and the other axis's capped launch, the other axis's
resume launch.  Forced with btrapz_debug_set_schedule (1: s axis first, 2: l axis first) and held, bit for bit, to the
one-launch lean solve: status, iteration counts, costs, and the control points of the solved candidates.  Then the rule
that chooses the schedule by itself: from what the context's last finished solve of the same shape handed over per axis."""
import numpy as np
import pytest

from spectral_amd import synth

pytestmark = pytest.mark.gpu
SLOT_PERCENT = 15      # BTRAPZ_SUSP_PERCENT: hand-over slots for this share of the 2 B axis problems, at least 1024


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    s = BatchSolver(0)
    yield s
    s.ctx.debug_set_schedule(0)


def fetch(o):
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def run(solver, batch, sh, mode, **kw):
    """One solve with the schedule set to `mode`: (results on the host, launches of the solve, resume keys [2, B])."""
    import torch
    solver.ctx.debug_set_schedule(mode)
    o = solver.solve(solver.upload(batch), sh, split=-1, lean=1, **kw)
    torch.cuda.synchronize()
    launches, form = solver.ctx.debug_solve_launches(), solver.ctx.last_solve_form()
    keys = solver.ctx.debug_resume_keys(batch.B) if launches > 1 else None
    solver.ctx.debug_set_schedule(0)
    return fetch(o), launches, form, keys


def same(one, other, what):
    assert np.array_equal(one["status"], other["status"]), what
    assert np.array_equal(one["iters"], other["iters"]), what
    assert np.array_equal(one["cost"], other["cost"]), what
    ok = one["status"] > 0
    assert np.array_equal(one["ctrl"][ok], other["ctrl"][ok]), what


def pipelined_against_one_launch(solver, batch, sh, cap, **kw):
    """Both forced orders against the one-launch solve; returns {mode: keys}."""
    one, n1, f1, _ = run(solver, batch, sh, 0, cap_iter=-1, **kw)
    assert (n1, f1) == (1, 8)
    keys = {}
    for mode in (1, 2):
        res, n, form, keys[mode] = run(solver, batch, sh, mode, cap_iter=cap, **kw)
        assert (n, form) == (3, 11), (mode, n, form)
        same(one, res, ("mode", mode))
    return keys


@pytest.mark.parametrize("B", [1, 2, 3, 4, 64, 1000])
def test_grid_edges(solver, B):
    """A last wavefront that is partly filled (three groups per wavefront at 20 segments), a group that is alone from the
    first iteration on; at B = 1 both axes hand over, so the third launch has work."""
    batch, sh = synth.make_scenario1_batch(B, 20, 0)
    keys = pipelined_against_one_launch(solver, batch, sh, 3)
    if B == 1:
        for mode in (1, 2):
            assert (keys[mode] > 0).all(), keys[mode]


@pytest.mark.parametrize("S", [16, 21, 32, 33, 64])
def test_groups_per_wavefront(solver, S):
    """4, 3, 2, 1 and 1 groups per wavefront; with one group every group is alone in its wavefront."""
    batch, sh = synth.make_batch(257, S, config=2)
    keys = pipelined_against_one_launch(solver, batch, sh, 4)
    assert (keys[1] > 0).any()


def test_one_axis_silent(solver):
    """scenario_1, trapezoid corridors: every lateral problem takes the same number of iterations and hands nothing over
    (measured: 0 of 6 144, 1 of 65 536), the longitudinal ones spread -- the case the schedule exists for.  With the
    silent axis first the first resume part finds an empty list and the third launch does all the resuming."""
    batch, sh = synth.make_scenario1_batch(6144, 20, 0)
    keys = pipelined_against_one_launch(solver, batch, sh, 6)
    for mode in (1, 2):
        assert (keys[mode][0] > 0).sum() > 0
        assert (keys[mode][1] > 0).sum() == 0
    assert np.array_equal(keys[1], keys[2])


def test_both_axes_talk(solver):
    """A generic batch: both axes hand over about as much (9 936 and 9 724 of 65 536 at this cap), so each resume part
    and each capped part has work whichever axis goes first."""
    batch, sh = synth.make_batch(6144, 20, config=3)
    keys = pipelined_against_one_launch(solver, batch, sh, 6)
    for mode in (1, 2):
        assert (keys[mode][0] > 0).sum() > 0 and (keys[mode][1] > 0).sum() > 0


def test_cuboid_variant_in_memory_order(solver):
    """The cuboid variant without its pre-pass (compact = -1: the memory-order path; with the pre-pass the batch goes
    through a.order and keeps its two launches).  A quarter of its candidates cannot start: groups that are alone from the
    first iteration on.  (Measured: its lateral axis hands over as little as the trapezoid variant's, 1 of 65 536.)"""
    batch, sh = synth.make_scenario1_batch(6144, 20, 1)
    keys = pipelined_against_one_launch(solver, batch, sh, 5, compact=-1)
    for mode in (1, 2):
        assert (keys[mode][0] > 0).sum() > 0


def test_nothing_handed_over(solver):
    """Both resume parts find empty lists."""
    batch, sh = synth.make_scenario1_batch(512, 20, 0)
    keys = pipelined_against_one_launch(solver, batch, sh, 22)
    for mode in (1, 2):
        assert (keys[mode] > 0).sum() == 0


def slot_count(B):
    return max(1024, 2 * B * SLOT_PERCENT // 100)


def test_low_cap_stays_within_the_slots(solver):
    """cap_iter = 3: every group still iterating four iterations later asks for a slot; no more keys than slots."""
    B = 8192
    batch, sh = synth.make_scenario1_batch(B, 20, 0)
    keys = pipelined_against_one_launch(solver, batch, sh, 3)
    for mode in (1, 2):
        assert 0 < (keys[mode] > 0).sum() <= slot_count(B)


def test_slots_run_out_during_the_second_axis(solver):
    """A generic batch at cap_iter = 4 asks for more slots than the workspace has.  The axis that goes first is served in
    full (what it asks for does not depend on the other axis); the other axis gets what is left, its remaining groups find
    no slot and go on where they are -- every slot is handed out exactly once, and the results are the same.
    (Measured at this shape: 1 239 + 604 of 1 843 slots with the s axis first.)"""
    B = 6144
    batch, sh = synth.make_batch(B, 20, config=3)
    keys = pipelined_against_one_launch(solver, batch, sh, 4)
    n = {mode: (keys[mode] > 0).sum(axis=1) for mode in (1, 2)}
    print("handed over per axis (s, l): s first", n[1], "l first", n[2], "slots", slot_count(B))
    wanted_s, wanted_l = int(n[1][0]), int(n[2][1])      # what each axis hands over when nothing has been taken before it
    assert 0 < wanted_s < slot_count(B) and 0 < wanted_l < slot_count(B)
    assert wanted_s + wanted_l > slot_count(B)           # the premise: together they do not fit
    assert int(n[1][1]) == slot_count(B) - wanted_s and int(n[2][0]) == slot_count(B) - wanted_l


@pytest.mark.parametrize("mode", [1, 2])
def test_back_to_back_without_a_host_sync(solver, mode):
    """6 144 candidates, then 64, then 6 144 of another family on one context and stream, nothing in between: no list,
    table or count of the call before leaks into the next."""
    import torch
    batches = [synth.make_scenario1_batch(6144, 20, 0), synth.make_scenario1_batch(64, 20, 0), synth.make_batch(6144, 20, config=3)]
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
    """A fresh context knows nothing: two launches.  Once that solve's per-axis counts have landed, the next solve of
    the same shape runs the longitudinal axis first when the counts are lopsided (scenario_1) and stays at two launches
    when they are not (generic batch).  The results never depend on it."""
    import torch
    from spectral_amd.solver import BatchSolver
    s1, sh1 = synth.make_scenario1_batch(6144, 20, 0)
    gen, shg = synth.make_batch(6144, 20, config=3)

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
    same(one, first, "two launches"); same(one, second, "three launches")
    keys = solver.ctx.debug_resume_keys(6144)
    assert (keys[0] > 0).sum() >= 4 * (keys[1] > 0).sum() and (keys[0] > 0).sum() > 0
    # never: two launches whatever is remembered
    solver.ctx.debug_set_schedule(-1)
    never, n = solve(solver, d1, sh1, cap_iter=6)
    assert n == 2
    same(one, never, "never")
    solver.ctx.debug_set_schedule(0)

    fresh = BatchSolver(0)
    dg2 = fresh.upload(gen)
    gone, n = solve(fresh, dg2, shg, cap_iter=-1)
    g1, n1 = solve(fresh, dg2, shg, cap_iter=6)
    g2, n2 = solve(fresh, dg2, shg, cap_iter=6)
    assert (n1, n2) == (2, 2)
    same(gone, g1, "generic, first"); same(gone, g2, "generic, second")
    # the context that remembers scenario_1: the generic batch of the same shape still runs (three launches, its counts are
    # not known yet), gives the same results, and its own counts bring the next one back to two
    g3, n3 = solve(solver, dg, shg, cap_iter=6)
    g4, n4 = solve(solver, dg, shg, cap_iter=6)
    assert (n3, n4) == (3, 2)
    same(gone, g3, "generic after scenario_1"); same(gone, g4, "generic, its own counts")
