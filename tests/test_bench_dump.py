"""bench.py --dump-outputs without a device: what dump_outputs writes for a batch that fits (every candidate) and for the
flagship batch (65 536 candidates x 20 segments: a fixed seeded sample under 64 MB), and --steps below 1 refused."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rows", "status", "iters", "solved_rows", "cost", "ctrl", "winner_index", "winner_cost", "winner_ctrl"}


def fake_step(B, S, seed=0):
    """A step's results as the library returns them: candidates without status 1 / 2 have cost +inf (and here NaN
    control points, so that a dump of them would show)."""
    rng = np.random.default_rng(seed)
    status = rng.integers(-2, 3, B).astype(np.int32)
    bad = (status != 1) & (status != 2)
    ctrl = rng.standard_normal((B, 12 * S)); ctrl[bad] = np.nan
    cost = rng.standard_normal(B); cost[bad] = np.inf
    w = int(np.flatnonzero(~bad)[0])
    return ctrl, cost, status, rng.integers(0, 30, B).astype(np.int32), w


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_a_batch_that_fits_is_dumped_whole(tmp_path):
    ctrl, cost, status, iters, w = fake_step(600, 20)
    bench.dump_outputs(str(tmp_path), ctrl, cost, status, iters, 1200, 1200 + w, cost[w], ctrl[w])
    got = load(str(tmp_path))
    assert set(got) == NAMES and all(v.dtype == np.float64 and np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["rows"], np.arange(1200, 1800))
    assert np.array_equal(got["status"], status) and np.array_equal(got["iters"], iters)
    ok = (status == 1) | (status == 2)
    assert 0 < ok.sum() < 600 and np.array_equal(got["solved_rows"], 1200 + np.flatnonzero(ok))
    assert np.array_equal(got["cost"], cost[ok]) and np.array_equal(got["ctrl"], ctrl[ok])
    assert got["winner_index"].tolist() == [1200 + w] and np.array_equal(got["winner_ctrl"], ctrl[w])


def test_a_step_without_a_winner_dumps_its_index_only(tmp_path):
    ctrl, cost, status, iters, _ = fake_step(50, 10)
    status[:] = -2; cost[:] = np.inf; ctrl[:] = np.nan
    bench.dump_outputs(str(tmp_path), ctrl, cost, status, iters, 0, -1, np.inf, np.full(120, np.nan))
    got = load(str(tmp_path))
    assert set(got) == NAMES - {"winner_cost", "winner_ctrl"} and all(np.isfinite(v).all() for v in got.values())
    assert got["winner_index"].tolist() == [-1] and got["solved_rows"].size == got["cost"].size == 0
    assert got["ctrl"].shape == (0, 120)


def test_the_flagship_batch_is_a_fixed_sample_under_64_mb(tmp_path):
    B, S = 65536, 20
    ctrl, cost, status, iters, w = fake_step(B, S)
    status[:B // 2] = 1; ctrl[:B // 2] = 0.5; cost[:B // 2] = 1.5          # (the budget holds when every row is solved)
    dumps = []
    for k in range(2):
        d = str(tmp_path / str(k))
        bench.dump_outputs(d, ctrl, cost, status, iters, 0, w, cost[w], ctrl[w])
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
        dumps.append(load(d))
    rows = dumps[0]["rows"].astype(np.int64)
    assert B // 3 < len(rows) < B and (np.diff(rows) > 0).all() and rows[-1] < B
    assert np.array_equal(dumps[0]["status"], status[rows]) and np.array_equal(dumps[0]["iters"], iters[rows])
    solved = dumps[0]["solved_rows"].astype(np.int64)
    assert np.array_equal(solved, rows[(status[rows] == 1) | (status[rows] == 2)])
    assert np.array_equal(dumps[0]["ctrl"], ctrl[solved]) and np.array_equal(dumps[0]["cost"], cost[solved])
    for n in NAMES:                                  # the same arguments, the same files
        assert np.isfinite(dumps[0][n]).all() and np.array_equal(dumps[0][n], dumps[1][n])
    # every row solved: the largest dump a sample of this batch can make stays within the budget
    status[:] = 1; ctrl[:] = 0.5; cost[:] = 1.5
    d = str(tmp_path / "all")
    bench.dump_outputs(d, ctrl, cost, status, iters, 0, 0, 1.5, ctrl[0])
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6


def test_steps_below_one_are_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr and p.stdout == ""
