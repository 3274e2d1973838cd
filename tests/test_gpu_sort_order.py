"""The device corridor stage where the order of tied segments decides the corridor (more than 16 selected segments, lanes
that open segments at the same knots): every field of its cubes against the oracle, whose sort is the C++ library's own
std::sort (src/solve_3d.cc:630; oracle/std_sort_order.cpp) -- exactly, on the shapes that select each code path: the
wave-wide kernel (rank sort, std_sort_core on one lane when keys tie, the in-order shortcut), the kernel with one lane per
candidate (sort_segments_core), the launch that evaluates its bounds from prisms.  Every generated batch meets the
sensitivity floor of tests/test_sort_order.py: the oracle's stable switch gives at least 10 % of its candidates another
corridor, so a device that sorted stably -- as it did until this test existed -- fails on dozens of candidates."""
import numpy as np
import pytest

from helpers import (CUBE_ATTRS, O, TIED_SHAPES, assert_sensitivity_floor, cube_rows, max_obstacle_segments, oracle_corridors_both_orders,
                     order_sensitive, tied_lanes_knot_batch, tied_prism_scenes, tied_shape_batch)
from spectral_amd import knots, layout as L, synth

pytestmark = pytest.mark.gpu

FIELDS = [(L.F_T, "t"), (L.F_DOWN_BIAS, "down_bias"), (L.F_DOWN_SKEW, "down_skew"), (L.F_UPP_BIAS, "upp_bias"), (L.F_UPP_SKEW, "upp_skew"),
          (L.F_L_DOWN_BIAS, "l_down_bias"), (L.F_L_DOWN_SKEW, "l_down_skew"), (L.F_L_UPP_BIAS, "l_upp_bias"), (L.F_L_UPP_SKEW, "l_upp_skew"),
          (L.F_BEG_L, "beg_l"), (L.F_END_L, "end_l")]
B = 256


def assert_record_equals(rec, want, what):
    """Counts and every cube field of the device's record against [(n, rows)] of the oracle, bit for bit."""
    import torch
    torch.cuda.synchronize()
    cnt = rec["seg_count"].cpu().numpy(); seg = rec["seg"].cpu().numpy()
    assert cnt.tolist() == [n for n, _ in want], (what, [(b, int(c), n) for b, (c, (n, _)) in enumerate(zip(cnt, want)) if c != n][:5])
    wrong = []
    for b, (n, rows) in enumerate(want):
        for f, name in FIELDS:
            if not np.array_equal(seg[f, b, :n], rows[:, CUBE_ATTRS.index(name)]):
                wrong.append((b, name))
                break
    assert not wrong, (what, len(wrong), wrong[:5])


@pytest.mark.parametrize("shape", sorted(TIED_SHAPES))
def test_device_corridors_equal_the_oracle_where_the_tie_order_decides(shape):
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    kb = tied_shape_batch(shape, B)
    real, stable = oracle_corridors_both_orders(kb, (shape, B))
    counts = np.array([n for n, _ in real])
    lo, hi = (65, 128) if kb.N > 512 else (17, 64)
    assert counts.min() >= lo and counts.max() <= hi and len(set(counts.tolist())) >= 6, counts
    if kb.N <= 512:   # within the lists of the wave-wide kernel (beyond them it reports -1 and sorts nothing)
        assert max_obstacle_segments(kb) <= 160 // kb.num_obs, (shape, max_obstacle_segments(kb))
    assert_sensitivity_floor(real, stable, shape)
    assert_record_equals(solver.corridor_batch(kb, 0, seg_stride=128 if kb.N > 512 else 64), real, shape)


def test_fused_prism_corridor_launch_where_the_tie_order_decides():
    """btrapz_prism_corridor_batch_device at N = 201 with up to 7 strips (O N <= 1536: the fused kernel itself): a reference
    that runs on the edge two strips share is inside both, 21-29 selected segments."""
    import torch
    from test_gpu_prism_bounds import pack
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    N, Omax = 201, 7
    scenes, bounds, s_ref, l_ref = tied_prism_scenes(31, B, N)

    def oracle_all():
        out = []
        for b in range(B):
            lists = [O.corridor_generation(0, N, 0.1, np.array(s), np.array(l)) for s, l in bounds[b]]
            n, cubes = O.collision_check(0, N, 0.1, lists, s_ref[b], l_ref[b])
            out.append((n, cube_rows(cubes[:max(n, 0)])))
        return out
    real = oracle_all()
    with O.stable_sort():
        stable = oracle_all()
    counts = np.array([n for n, _ in real])
    assert counts.min() > 16 and counts.max() <= 40 and len(set(counts.tolist())) >= 6 and max(len(s) for s in bounds) <= Omax
    assert_sensitivity_floor(real, stable, "prisms")
    init = np.zeros((B, 6)); init[:, 1] = 1.0
    dsb = np.tile(np.array([0.0, 20.0]), (B, N, 1)); dlb = np.tile(np.array([-3.0, 3.0]), (B, N, 1))
    t = torch.from_numpy
    rec = solver.prism_corridor_batch(0, t(pack(scenes, 3)), N, Omax, 0.1, t(dsb), t(dlb), t(s_ref), t(l_ref), t(init), seg_stride=40)
    torch.cuda.synchronize()
    assert rec["n_strips"].cpu().numpy().tolist() == [len(s) for s in bounds]
    assert_record_equals(rec, real, "prisms")


def test_scenario1_knots_as_the_bench_draws_it():
    """synth.scenario1_knots(256, 20): 18-24 segments on every candidate, the lanes' one-second pieces tied where the
    reference changes lanes.  (In this draw the tie order reaches no final corridor -- 9 of the 2 000 of
    tests/test_sort_order.py, none of these 256: the floor is a property of the generated batches, this one is the
    workload as it is; what it does hold the device to is the permutation of the tied pairs inside the stage, which the
    reorder and overlap steps see, with the in-order shortcut on the way.)"""
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    kb = synth.scenario1_knots(B, 20)
    real, _ = oracle_corridors_both_orders(kb, "scenario1_knots(256, 20)")
    counts = np.array([n for n, _ in real])
    assert counts.min() > 16 and counts.max() <= 24
    assert_record_equals(solver.corridor_batch(kb, 0, seg_stride=32), real, "scenario1_knots")


def test_a_batch_mixing_short_and_long_corridors_equals_the_uniform_ones_bit_for_bit():
    """Candidates of at most 16 segments (the stable insertion pass is the whole sort) beside candidates of more (introsort)
    in one launch: each gets the bits it gets in a batch of its own kind -- and those are the oracle's."""
    import torch
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    N, half = 121, 64
    long_ = tied_lanes_knot_batch(15, half, N, 2, (20, 32), 6)
    short = tied_lanes_knot_batch(16, half, N, 2, (5, 14), 2)
    mix = lambda a, b: np.stack([a, b], 1).reshape((2 * half,) + a.shape[1:])      # long, short, long, short, ...
    both = knots.KnotBatch(2 * half, N, 2, 0.1, *[mix(getattr(long_, k), getattr(short, k)) for k in
                                                    ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds", "s_ref", "l_ref", "init")], dict(long_.header))
    real_long, stable_long = oracle_corridors_both_orders(long_, "mix long")
    real_short, _ = oracle_corridors_both_orders(short, "mix short")
    assert min(n for n, _ in real_long) > 16 and max(n for n, _ in real_short) <= 16 and min(n for n, _ in real_short) > 0
    assert_sensitivity_floor(real_long, stable_long, "mix long")
    recs = {k: solver.corridor_batch(kb, 0, seg_stride=32) for k, kb in (("long", long_), ("short", short), ("both", both))}
    torch.cuda.synchronize()
    seg = {k: r["seg"].cpu().numpy() for k, r in recs.items()}; cnt = {k: r["seg_count"].cpu().numpy() for k, r in recs.items()}
    assert np.array_equal(cnt["both"][0::2], cnt["long"]) and np.array_equal(cnt["both"][1::2], cnt["short"])
    assert seg["both"][:, 0::2].tobytes() == seg["long"].tobytes() and seg["both"][:, 1::2].tobytes() == seg["short"].tobytes()
    assert_record_equals(recs["both"], [r for pair in zip(real_long, real_short) for r in pair], "mixed")


def test_tied_batch_from_knots_to_control_points(tmp_path):
    """End to end on a tied batch: knots -> device corridor -> ragged solve, against the oracle's optimum of the QP of the
    oracle's own corridor, at the parity tests' 1e-5 |x*|inf.  (A corridor the tie order rearranges is no longer in order of
    time -- in the reference too -- and its QP has no solution: two such candidates are held to that verdict, the control
    points are compared on the candidates the device solved.)"""
    import torch
    from test_gpu_long_ragged import shared_for
    from spectral_amd.solver import BatchSolver
    solver = BatchSolver(0)
    kb = tied_shape_batch("N201_2lanes", B)
    real, stable = oracle_corridors_both_orders(kb, ("N201_2lanes", B))
    sens = order_sensitive(real, stable)
    rec = solver.corridor_batch(kb, 0, seg_stride=32)
    sh = shared_for(kb, 0)
    o = solver.solve_ragged(rec, sh)
    torch.cuda.synchronize()
    ctrl = o["ctrl"].cpu().numpy(); status = o["status"].cpu().numpy(); counts = rec["seg_count"].cpu().numpy()
    checked = 0
    for b in np.nonzero(status > 0)[0][:8].tolist() + sens[:2]:
        path = str(tmp_path / ("c%d.txt" % b))
        knots.write_corridor_file(path, kb, b)
        inp = O.ParsedInput(path)
        n, cubes = O.pipeline(0, inp)
        assert n == counts[b] == real[b][0] and n > 16
        x, _, info = O.AssembledQp(0, cubes, O.params_from_weights(synth.REFERENCE_WEIGHTS), inp).solve_exact(max_iter=120)
        assert (info.status in (1, 2)) == (status[b] > 0), (b, info.status, status[b])
        if status[b] > 0:
            err = np.abs(ctrl[b, :12 * n] - x).max()
            assert err <= 1e-5 * np.abs(x).max(), (b, err / np.abs(x).max())
            checked += 1
    assert checked >= 6, checked
