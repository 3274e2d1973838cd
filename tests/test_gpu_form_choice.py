"""Which form the host driver chooses (btrapz_last_solve_form) for a table of shapes and options, for the plain entry
points and for btrapz_solve_sets_device with a single set: the two drivers must choose alike wherever both serve a shape.

The batch sizes are derived from R = 4 x multi_processor_count, the wavefronts the device holds at one per SIMD
(btrapz_ctx.resident_waves), which is what the rules compare with:
  split   uniform cold, at most 21 segments, 2 B <= R (or split = 1)
  lean    4 x est_waves >= 5 R with est_waves = 2 (B / (64 / S) + 1), 3..64 segments (or lean = 1)
  capped  uniform cold, 16..32 segments, launch of at least 8 R wavefronts (or cap_iter > 0); never by itself with sets
  long    uniform, 65..256 segments; + 16: the candidates of more than 64 segments of a ragged batch"""
import numpy as np
import pytest

from spectral_amd import layout as L, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from spectral_amd.solver import BatchSolver
    return BatchSolver(0)


@pytest.fixture(scope="module")
def R():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def lean_threshold_batch(R):
    """The smallest multiple of 6 (candidates of 10 segments per wavefront) with 4 * 2 * (B / 6 + 1) >= 5 R."""
    B = 6
    while 4 * 2 * (B // 6 + 1) < 5 * R:
        B += 6
    return B


def ragged_with_one_long(solver):
    """Slots for 80 segments: one candidate of 70 segments among short ones (each keeps its first count segments)."""
    import torch
    batch, sh = synth.make_batch(6, 70, config=2)
    d = solver.device
    seg = np.zeros((L.NUM_SEG_FIELDS, batch.B, 80)); seg[:, :, :batch.S] = batch.seg
    counts = [70, 10, 12, 8, 20, 15]
    rec = dict(B=batch.B, seg_stride=80, seg=torch.tensor(seg, device=d), seg_count=torch.tensor(counts, dtype=torch.int32, device=d),
               init=torch.tensor(batch.init, device=d), ref_end=torch.tensor(batch.ref_end, device=d),
               dl_bounds=torch.tensor(batch.dl_bounds, device=d))
    return rec, sh


# (row of the table, B as a function of R, S, options, expected form)
ROWS = [
    (1, lambda R: 8, 20, {}, 1),
    (2, lambda R: 8, 22, {}, 0),
    (3, lambda R: 8, 20, dict(split=-1), 0),
    (4, lambda R: 8, 20, dict(keep_multipliers=True), 0),
    (5, lean_threshold_batch, 10, {}, 8),
    (6, lean_threshold_batch, 10, dict(lean=-1), 0),
    (7, lambda R: 12 * R, 20, {}, 11),
    (8, lambda R: 12 * R, 20, dict(lean=-1), 3),
    (9, lambda R: 12 * R, 20, dict(cap_iter=-1), 8),
    (10, lambda R: 8 * R, 40, {}, 8),
    (11, lambda R: 4, 70, {}, 2),
]


@pytest.mark.parametrize("row,B_of,S,options,expected", ROWS, ids=["row%d" % r[0] for r in ROWS])
def test_form_of_the_plain_entry_points(solver, R, row, B_of, S, options, expected):
    import torch
    batch, sh = synth.make_batch(B_of(R), S, config=2)
    solver.solve(solver.upload(batch), sh, **options)
    torch.cuda.synchronize()
    form = solver.ctx.last_solve_form()
    print("row %d: B %d S %d %r -> form %d" % (row, batch.B, S, options, form))
    assert form == expected


def test_form_of_a_ragged_batch_with_a_long_candidate(solver):
    import torch
    rec, sh = ragged_with_one_long(solver)
    solver.solve_ragged(rec, sh)
    torch.cuda.synchronize()
    form = solver.ctx.last_solve_form()
    print("row 12: form %d" % form)
    assert form >= 0 and form & 16


SETS_EXPECTED = {1: 1, 5: 8, 7: 8, 11: 2}   # (row 7: the sets path never caps by itself)
SETS_ROWS = [(r[0], r[1], r[2], SETS_EXPECTED[r[0]]) for r in ROWS if r[0] in SETS_EXPECTED]


@pytest.mark.parametrize("row,B_of,S,expected", SETS_ROWS, ids=["row%d" % r[0] for r in SETS_ROWS])
def test_form_of_the_sets_solve_with_a_single_set(solver, R, row, B_of, S, expected):
    import torch
    batch, sh = synth.make_batch(B_of(R), S, config=2)
    solver.solve_sets(solver.upload(batch), [sh], torch.zeros(batch.B, dtype=torch.int32, device=solver.device))
    torch.cuda.synchronize()
    form = solver.ctx.last_solve_form()
    print("sets row %d: B %d S %d -> form %d" % (row, batch.B, S, form))
    assert form == expected


def test_form_of_the_sets_solve_of_a_ragged_batch_with_a_long_candidate(solver):
    import torch
    rec, sh = ragged_with_one_long(solver)
    solver.solve_sets_ragged(rec, [sh], torch.zeros(rec["B"], dtype=torch.int32, device=solver.device))
    torch.cuda.synchronize()
    form = solver.ctx.last_solve_form()
    print("sets row 12: form %d" % form)
    assert form >= 0 and form & 16
