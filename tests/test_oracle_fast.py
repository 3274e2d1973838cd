"""The -O3 -march=native oracle of bench.py's CPU baseline (oracle.fast_lib) in a tree its user cannot write to: the
library is compiled into a private temporary directory, the tree gains no file, and it solves as the checker build does."""
import os
import tempfile

import numpy as np

from helpers import O
from spectral_amd import synth


def test_fast_oracle_in_a_tree_that_cannot_be_written(monkeypatch):
    missing = os.path.join(O._HERE, "libbtrapz_oracle_fast_no_such_cpu.so")
    assert not os.path.exists(missing)
    monkeypatch.setattr(O, "_fast", None)
    monkeypatch.setattr(O, "_fast_path", lambda: missing)
    real_access = os.access
    monkeypatch.setattr(os, "access", lambda p, m, **kw: False if os.path.abspath(p) == O._HERE else real_access(p, m, **kw))
    ours = lambda: (set(os.listdir(O._HERE)), {f for f in os.listdir(tempfile.gettempdir()) if f.startswith("btrapz_oracle_fast_")})
    before = ours()
    assert O.build_fast() is None
    batch, sh = synth.make_batch(6, 10, config=2)
    x_fast, obj_fast, st_fast, _ = O.batch_solve(batch, sh, 0, 6, threads=2, fast=True)
    assert O._fast is not None and not os.path.exists(missing)
    assert ours() == before                                     # nothing left behind, in the tree or in the temporary directory
    x, obj, st, _ = O.batch_solve(batch, sh, 0, 6)
    assert np.array_equal(st_fast, st) and (st > 0).any()
    assert np.allclose(x_fast, x, rtol=1e-9, atol=1e-9) and np.allclose(obj_fast, obj, rtol=1e-9, atol=1e-9)
