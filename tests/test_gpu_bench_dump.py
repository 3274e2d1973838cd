"""bench.py --dump-outputs on the device: the last timed step's results, the same from run to run and from either host,
consistent with the JSON line (its winner is the dumped winner, and that winner's row of the dumped batch), and finite:
the candidates without a solution (cost +inf) are in status.npy, not in cost.npy / ctrl.npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"rows", "status", "iters", "solved_rows", "cost", "ctrl", "winner_index", "winner_cost", "winner_ctrl"}


def run(d, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "6000",
                        "--no-cpu-baseline", "--latency-reps", "0", "--no-secondary", "--lean", "1", "--dump-outputs", str(d), *args],
                       capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]      # (the one-process host lets RCCL's banner through)
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(str(d), f)) for f in os.listdir(str(d))}


def check(line, got):
    assert set(got) == NAMES and all(v.dtype == np.float64 and np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["rows"], np.arange(6000)) and got["status"].shape == got["iters"].shape == (6000,)
    ok = (got["status"] == 1) | (got["status"] == 2)
    assert np.array_equal(got["solved_rows"], np.flatnonzero(ok)) and got["ctrl"].shape == (ok.sum(), 240) and got["cost"].shape == (ok.sum(),)
    w = int(got["winner_index"][0])
    assert w == line["winner"]["index"] and got["winner_cost"][0] == line["winner"]["cost"]
    j = int(np.searchsorted(got["solved_rows"], w))
    assert got["solved_rows"][j] == w and got["cost"][j] == got["winner_cost"][0] == got["cost"].min()
    assert np.array_equal(got["winner_ctrl"], got["ctrl"][j])
    assert line["status_counts"] == {str(int(k)): int((got["status"] == k).sum()) for k in np.unique(got["status"])}
    return ok


def test_dumped_outputs_are_the_last_step_and_reproducible(tmp_path):
    line, got = run(tmp_path / "a")
    assert line["steps"] == 3
    check(line, got)
    again, got2 = run(tmp_path / "b")
    one, got3 = run(tmp_path / "c", "--host", "one-process")
    for n, v in got.items():
        assert np.array_equal(v, got2[n]), n
        assert np.array_equal(v, got3[n]), n
    # the cuboid variant (BASELINE config 4), where a good part of the candidates has no solution
    line4, got4 = run(tmp_path / "d", "--variant", "1")
    ok4 = check(line4, got4)
    assert 0 < ok4.sum() < 6000
