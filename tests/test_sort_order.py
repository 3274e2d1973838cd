"""The order of the selected corridor segments beyond 16 of them (a4 / f1).  The reference sorts them with std::sort and a
comparator on beg_t alone (src/solve_3d.cc:630); libstdc++'s introsort keeps tied keys in input order only up to 16
elements, and two lanes that open segments at the same knots tie all the time.  Three statements of that order are held
together here, on the CPU:
  * the C++ library's own std::sort (oracle/std_sort_order.cpp) -- pinned by tests/golden/std_sort_order.json;
  * the product's restatement (sort_segments_core, corridor_core.h), through the sanitizer build of the host code, on
    thousands of key arrays including ones that drive it into the heap-sort fallback;
  * the host corridor stage (btrapz_corridor_from_file) against the oracle on inputs where the order decides the corridor --
    which the oracle's stable switch counts (a floor, asserted: a batch where the tie order never matters checks nothing).
tests/test_gpu_sort_order.py holds the device to the same oracle."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import (O, TIED_SHAPES, assert_sensitivity_floor, cube_rows, fuzz_knot_batch, oracle_corridor,
                     oracle_corridors_both_orders, order_sensitive, tied_shape_batch)
from spectral_amd import knots, native, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectral_amd", "csrc")
BIN = os.path.join(ROOT, "spectral_amd", "lib", "host_check_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "std_sort_order.json")))


def test_the_live_std_sort_reproduces_the_committed_permutations():
    """Another libstdc++ (or another C++ library) that orders ties differently is a red test here, not silent drift."""
    assert len(FIXTURE) >= 100 and {len(c["keys"]) for c in FIXTURE} >= {1, 16, 17, 64, 65, 256}
    for c in FIXTURE:
        perm = O.std_sort_order(c["keys"])
        assert perm.tolist() == c["perm"], (c["kind"], len(c["keys"]))
        assert sorted(c["perm"]) == list(range(len(c["keys"]))) and (np.diff(np.array(c["keys"])[perm]) >= 0).all()


def test_std_sort_is_stable_up_to_16_keys_and_not_beyond():
    """The sort-level fact: two lanes opening at the same knots, listed lane after lane.  The two sorts agree for every
    n <= 16 and part ways at 17, 19, 21-26, ... but not at 18 or 20 -- which is why no test here uses one fixed n."""
    def lanes(n):
        half = (n + 1) // 2
        return np.concatenate([np.arange(half), np.arange(n - half)]) * 10
    differs = {n for n in range(1, 129) if not np.array_equal(O.std_sort_order(lanes(n)), O.std_sort_order(lanes(n), stable=True))}
    assert not any(n <= 16 for n in differs)
    assert {17, 19, 21, 22, 23, 24, 25, 26, 32, 48, 64, 65, 80, 96, 100, 112, 128} <= differs and not ({18, 20} & differs)
    rng = np.random.default_rng(3)
    for _ in range(300):
        k = rng.integers(0, 4, int(rng.integers(1, 17)))
        assert np.array_equal(O.std_sort_order(k), O.std_sort_order(k, stable=True))


@pytest.fixture(scope="module")
def restatement():
    """sort_segments_core on key arrays: [(heap-sort fallback taken, permutation)], through host_check_asan (g++,
    AddressSanitizer + UBSan: the unguarded loops of the algorithm rely on a smaller key in front of them)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "host_asan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]

    def run(arrays, path):
        with open(path, "w") as f:
            f.write("".join("%d %s\n" % (len(k), " ".join(str(int(v)) for v in k)) for k in arrays))
        p = subprocess.run([BIN, "sort", path], capture_output=True, text=True, env=ENV, timeout=600)
        out = p.stdout + p.stderr
        assert p.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
        rows = [[int(v) for v in line.split()] for line in p.stdout.splitlines()]
        assert len(rows) == len(arrays)
        return [(row[0] == 1, row[1:]) for row in rows]
    return run


def random_key_arrays():
    rng = np.random.default_rng(16)
    arrays = [np.zeros(n, dtype=int) for n in (1, 2, 16, 17, 64, 65, 255, 256)]              # all equal
    for n in range(1, 257):                                                                   # every n once, heavy ties
        arrays.append(rng.integers(0, 3, n))
    for t in range(5000):
        n = int(rng.integers(1, 257))
        k = rng.integers(0, int(rng.choice([1, 2, 3, 5, 8, 20, 300])), n)                    # small alphabets: ties are heavy
        kind = t % 6
        if kind == 1:
            k = np.sort(k)                                                                    # already sorted
        elif kind == 2:
            k = np.sort(k)[::-1]                                                              # reversed
        elif kind == 3:
            half = (n + 1) // 2                                                               # lanes opening at the same knots
            k = np.concatenate([np.sort(k[:half]), np.sort(k[:n - half])])
        arrays.append(k)
    return arrays


def test_the_restatement_gives_std_sorts_permutation_on_random_keys(restatement, tmp_path):
    arrays = random_key_arrays()
    assert len(arrays) >= 5000 and {len(k) for k in arrays} == set(range(1, 257))
    got = restatement(arrays, str(tmp_path / "keys.txt"))
    unstable = 0
    for k, (_, perm) in zip(arrays, got):
        want = O.std_sort_order(k)
        assert perm == want.tolist(), (len(k), k.tolist())
        unstable += not np.array_equal(want, O.std_sort_order(k, stable=True))
    assert unstable >= 2000          # (the arrays do tell the two orders apart)


def test_the_heap_sort_fallback_is_taken_and_gives_std_sorts_permutation(restatement, tmp_path):
    """McIlroy's adversary, run against the live std::sort, builds keys on which every pivot is among the smallest of its
    range: the depth limit 2 floor(lg n) runs out and what is left is heap-sorted.  The restatement must report that it
    went there -- otherwise the branch is untested -- and give the library's permutation, with ties too (keys halved)."""
    arrays = []
    for n in (65, 100, 128, 200, 256):
        adv = O.std_sort_adversary(n)
        arrays += [adv, adv >> 1]
    got = restatement(arrays, str(tmp_path / "adv.txt"))
    for k, (fell_back, perm) in zip(arrays, got):
        assert fell_back, (len(k), k.tolist())
        assert perm == O.std_sort_order(k).tolist(), (len(k), k.tolist())
    assert any(not np.array_equal(O.std_sort_order(k), O.std_sort_order(k, stable=True)) for k in arrays[1::2])
    plain = restatement([np.arange(100) % 7, np.arange(256)[::-1] // 3], str(tmp_path / "plain.txt"))
    assert not any(fell_back for fell_back, _ in plain)      # ... and ordinary inputs do not take it


def host_corridor(kb, b, path):
    knots.write_corridor_file(path, kb, b)
    return native.corridor_from_file(0, path, cap=512)


@pytest.mark.parametrize("shape", sorted(TIED_SHAPES))
def test_host_corridor_stage_equals_the_oracle_where_the_tie_order_decides(shape, tmp_path):
    """tied_lanes_knot_batch: 17-64 selected segments (N = 201, 512) and 65-256 (N = 700), most of them tied.  Count and
    every field of test_corridor_fuzz.py's ATTRS, exactly."""
    B = 64
    kb = tied_shape_batch(shape, B)
    real, stable = oracle_corridors_both_orders(kb, (shape, B))
    counts = np.array([n for n, _ in real])
    lo, hi = (65, 256) if kb.N > 512 else (17, 64)
    assert counts.min() >= lo and counts.max() <= hi and len(set(counts.tolist())) >= 6, counts       # spread, never one fixed n
    sens = assert_sensitivity_floor(real, stable, shape)
    path = str(tmp_path / "c.txt")
    for b in range(B):
        segs = host_corridor(kb, b, path)
        assert len(segs) == real[b][0], (shape, b)
        assert np.array_equal(cube_rows(segs), real[b][1]), (shape, b)
    b = sens[0]                                             # (and the stable order is NOT what the host path computes)
    assert not np.array_equal(cube_rows(host_corridor(kb, b, path)), stable[b][1])


def test_scenario1_knots_candidate_609(tmp_path):
    """The bench's knot-level workload, 2 000 candidates of 18-24 segments: nine get another corridor under std::sort than
    under a stable sort.  Candidate 609: the lane-1 twin (31, 41, l in [1, 3]) lands at position 14, not 3."""
    kb = synth.scenario1_knots(2000, 20)
    real, stable = oracle_corridors_both_orders(kb, "scenario1_knots(2000, 20)")
    counts = np.array([n for n, _ in real])
    assert counts.min() > 16 and counts.max() <= 24
    sens = order_sensitive(real, stable)
    assert sens == [609, 885, 888, 978, 1410, 1623, 1821, 1910, 1912]
    path = str(tmp_path / "c.txt")
    for b in sens + [0, 1, 2, 1999]:
        segs = host_corridor(kb, b, path)
        assert len(segs) == real[b][0] and np.array_equal(cube_rows(segs), real[b][1]), b
    segs = host_corridor(kb, 609, path)
    span = lambda c: (c.beg_t, c.end_t, c.beg_l, c.end_l)
    assert span(segs[14]) == (31, 41, 1.0, 3.0) and span(segs[3]) == (31, 41, 3.0, 4.5)
    n, rows = stable[609]                                   # what a stable sort would have made of it: the twins split the span
    assert (rows[3][0], rows[3][1], rows[3][11], rows[3][12]) == (31, 36, 1.0, 3.0)


def test_up_to_16_segments_the_oracle_equals_its_stable_switch_on_the_fuzz_cases():
    from test_corridor_fuzz import CASES
    checked = small = 0
    for seed, b in CASES:
        kb = fuzz_knot_batch(seed)
        n, cubes = oracle_corridor(kb, b, 0)
        if n is None:
            continue
        with O.stable_sort():
            m, cubes_stable = oracle_corridor(kb, b, 0)
        checked += 1
        if n <= 16:
            small += 1
            assert n == m
            a, s = cube_rows(cubes[:max(n, 0)]), cube_rows(cubes_stable[:max(n, 0)])
            assert a.tobytes() == s.tobytes() or np.array_equal(a, s, equal_nan=True), (seed, b)
    assert checked >= 50 and small >= 25
