"""Writes tests/golden/active_rows_yardstick.npz: the oracle's answers to the cases of tests/active_row_cases.py -- candidates
whose optimum sits on velocity, acceleration or jerk rows -- at the widths where its dense exact solve is too slow to run in a
test: about a second a candidate at 64 and 65 segments, 15 s at 130, minutes at 256.

    python tests/golden/make_active_row_goldens.py [width ...]        (default: 64 65 130 256)

Per width `S<n>/`: `B`, `cases` (the case names, e.g. jrk_s_hi) and per case `S<n>/<case>/` the tightened `limit` (one
batch-wide value, or [B] per-candidate values with nan where the family's limit stays), the oracle's `x` [B, 12 S], `obj`,
`status` and `strict` [B], and the active-row masks `act_lo` / `act_hi` [B, 42 S] as packed bits.  The batches themselves are
not stored: active_row_cases.family() regenerates them from spectral_amd.synth.  active_row_cases.STORED says which cases a
width holds; tests/test_active_row_cases.py regenerates the 64-segment slice and compares it with the file bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import active_row_cases as A
    out = A.golden_path()
    widths = [int(a) for a in sys.argv[1:]] or sorted(A.STORED)
    data = dict(np.load(out)) if os.path.exists(out) else {}
    for S in widths:
        data = {k: v for k, v in data.items() if not k.startswith("S%d/" % S)}
        data.update(A.generate_stored(S, log=lambda line: print(line, flush=True)))
        np.savez_compressed(out, **data)
        print("width %d written: %d bytes" % (S, os.path.getsize(out)), flush=True)
        w = A.stored(S, data)
        short = [A.case_id(c) for c, v in w["cases"].items() if not v["counts"]]
        assert not short or S == 64, (S, "cases that do not count", short)
    assert os.path.getsize(out) < 1000000, os.path.getsize(out)


if __name__ == "__main__":
    main()
