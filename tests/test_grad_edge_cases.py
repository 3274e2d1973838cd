"""tests/grad_edge_cases.py on the CPU: every target slot of every (family, width) case holds a solved, strictly
complementary candidate -- judged here by a fresh yardstick solve of the slot, not by what build() remembers -- and the
batch build() returns is a permutation of the generated one.  The GPU tests (test_gpu_vjp_edges.py,
test_gpu_jvp_edges.py) compare every target slot and skip none; this file is why they never run with fewer
comparisons than stated."""
import numpy as np
import pytest

import grad_edge_cases as C
from vjp_reference import Adjoint, one


def test_the_slots_sit_at_the_edges_of_the_lane_mapping():
    assert C.B_EXT > C.B
    for S in C.WIDTHS:
        g = 64 // S
        t = C.target_slots(S)
        assert C.B % g == (1 if g > 1 else 0) and t[-1] == C.B - 1          # B - 1: alone in the last wavefront
        if S == 63:
            assert t == (C.B - 1,)
        elif g == 1:
            assert t == (1, C.B - 1)
        else:
            assert t == (g - 1, g, C.B - 1)                                  # last group of wavefront 0, first of wavefront 1
            assert (g - 1) // g == 0 and g // g == 1 and (g - 1) % g == g - 1
    assert C.ragged_counts(21) == (1, 2, 20, 21) and C.ragged_counts(33) == (1, 2, 21, 22, 32, 33)
    assert all(64 % s for s in C.RAGGED_STRIDES)
    assert len(C.CASES) == 3 * (len(C.WIDTHS) - 1) + 1 and ("scenario_1", 63) in C.CASES


@pytest.mark.parametrize("family,S", C.CASES)
def test_every_target_slot_holds_a_solved_strict_candidate(family, S):
    batch, sh, targets, perm, adjoints = C.build(family, S)
    assert targets == C.target_slots(S) and set(adjoints) == set(targets)
    swapped = np.flatnonzero(perm != np.arange(C.B))
    print("targets %s S=%d: slots %s, swapped %s" % (family, S, targets, [(int(b), int(perm[b])) for b in swapped]))
    for b in targets:
        adj = Adjoint(one(batch, b), sh, np.zeros(12 * S), 0.0)
        assert adj.status == 1 and adj.strict, (family, S, b)
    # a permutation of the generated batch: every candidate still there, once, whole
    gen, sh0 = C.generate(family, S)
    assert sh0 == sh and batch.B == C.B and batch.S == S
    assert np.array_equal(np.sort(perm), np.arange(C.B))
    assert np.array_equal(batch.seg, gen.seg[:, perm]) and np.array_equal(batch.init, gen.init[perm])
    assert np.array_equal(batch.ref_end, gen.ref_end[perm]) and np.array_equal(batch.dl_bounds, gen.dl_bounds[perm])
    # a swap only where a target slot needed one, and only with a slot that is no target
    assert len(swapped) % 2 == 0 and len(swapped) <= 2 * len(targets)
    assert len(set(swapped) & set(targets)) == len(swapped) // 2
