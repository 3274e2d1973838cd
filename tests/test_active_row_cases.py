"""The cases of tests/test_gpu_active_rows.py, without a GPU: the census conditions of DESIGN.md 7 ("What is held at which
widths") on the widths the oracle solves live and on the stored ones, the stored answers' 64-segment slice regenerated bit for
bit, and the helpers the GPU tests read rows with held to the oracle's assembled matrix."""
import numpy as np
import pytest

import active_row_cases as A
import row_check_reference as R
from helpers import oracle_qp_from_batch


@pytest.mark.parametrize("S", [1, 3, 5, 21, 33])
def test_census_of_the_live_widths(S):
    w = A.width(S)
    for c in A.CASES:
        print(A.census_line(S, w["cases"][c]))
    counting = A.assert_census(S, w)
    assert (w["base"]["status"] == 1).all()
    # every solved candidate's status is 1 or a rejection: an accept decision never hangs on an "inaccurate" answer
    for c in A.CASES:
        assert np.isin(w["cases"][c]["sol"]["status"], (1, -2, -3)).all(), (S, c)
    assert len(counting) >= 9


def test_census_of_the_cuboid_variant():
    w = A.width(21, variant=1)
    for c in A.CASES:
        print(A.census_line(21, w["cases"][c]))
    A.assert_census(21, w)


def test_census_of_the_stored_widths():
    for S, (B, pairs, _) in A.STORED.items():
        w = A.stored(S)
        assert w["batch"].B == B
        for case, c in w["cases"].items():
            print(A.census_line(S, c))
            assert np.isin(c["sol"]["status"], (1, -2, -3)).all(), (S, case)
        if pairs is None:
            A.assert_census(S, w)
        else:
            assert [case[:2] for case in w["cases"]] == list(pairs), S
            for case, c in w["cases"].items():
                assert c["counts"] and 2 * c["n_solved"] > B, A.census_line(S, c)


def test_the_stored_64_segment_slice_is_what_the_generator_writes():
    g = np.load(A.golden_path())
    fresh = A.generate_stored(64)
    assert sorted(k for k in g.files if k.startswith("S64/")) == sorted(fresh)
    for k, v in fresh.items():
        a, b = np.asarray(v), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_the_ragged_record_counts_at_every_width():
    """One batch-wide limit -- the 21-segment width's -- on the 1-, 3-, 21- and 33-segment candidates."""
    for case in (("jrk", "s", "hi"), ("acc", "l", "lo")):
        limit = A.width(21)["cases"][case]["limit"]
        for S in (1, 3, 21, 33):
            batch, sh = A.family(S)
            c = A.with_solution(batch, sh, case, limit)
            print(A.census_line(S, c))
            assert c["counts"] and 2 * c["n_solved"] > batch.B, A.census_line(S, c)


@pytest.mark.parametrize("S", [1, 3, 21])
def test_rows_are_read_where_the_oracle_has_them(S):
    """class_rows() / row_values() against the assembled QP: the row order the audit's yardstick asserts, and A x itself."""
    w = A.width(S)
    rng = np.random.default_rng(S)
    for case in (("vel", "s", "hi"), ("jrk", "l", "lo")):
        c = w["cases"][case]
        qp = oracle_qp_from_batch(c["batch"], c["sh"], 1)
        R.row_order_identities(qp)
        x = rng.standard_normal(12 * S)
        Ax = R.csc(qp) @ x
        for cls in A.CLASSES:
            for axis in A.AXES:
                rows = A.class_rows(S, cls, axis)
                assert np.allclose(A.row_values(x, S, cls, axis), Ax[rows], rtol=0, atol=1e-12 * A.ROW_L1[cls] * np.abs(x).max())
        # the tightened bound is the one the oracle's rows carry
        cls, axis, side = case
        limit = A.tightened_bound(case, c["limit"], 1)
        if np.isfinite(limit):
            bound = (qp.u if side == "hi" else qp.l)[A.class_rows(S, cls, axis)]
            assert (bound == limit).all(), (case, bound, limit)


def test_a_wrong_jerk_coefficient_moves_the_optimum_of_a_jerk_case_only():
    """What the GPU tests rely on, shown on the CPU with the oracle alone: the optimum of a jerk-active candidate moves by more
    than the control-point bound when a jerk limit is off by 1 / 60, the optimum of the family's own candidate does not."""
    S = 21
    w = A.width(S)
    c = w["cases"][("jrk", "s", "hi")]
    b = int(np.nonzero(c["good"])[0][0])
    moved = lambda batch, sh, x: np.abs(A._solve_one((batch, sh, b))["x"] - x).max() / np.abs(x).max()
    import copy
    off = copy.deepcopy(c["sh"]); off.ddds = (off.ddds[0], off.ddds[1] * 60.0 / 59.0)
    assert moved(c["batch"], off, c["sol"]["x"][b]) > 1e-5
    base_off = copy.deepcopy(w["sh"]); base_off.ddds = (base_off.ddds[0], base_off.ddds[1] * 60.0 / 59.0)
    assert moved(w["batch"], base_off, w["base"]["x"][b]) <= 1e-7
