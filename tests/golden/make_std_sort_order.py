"""Writes tests/golden/std_sort_order.json: key arrays and the permutations the C++ library's std::sort gave them
(oracle/std_sort_order.cpp; comparator on the key alone, perm[r] = input index at position r) where this was run --
libstdc++ of GCC 11, the introsort the reference's GCC 7.5 build has too.  tests/test_sort_order.py holds the live
function to it, so a machine whose C++ library orders ties differently shows up as a red test.
    python tests/golden/make_std_sort_order.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O  # noqa: E402


def key_arrays():
    rng = np.random.default_rng(630)
    out = []
    for n in (1, 2, 3, 15, 16, 17, 18, 19, 20, 21, 24, 26, 32, 33, 48, 63, 64, 65, 80, 96, 100, 112, 128, 129, 200, 255, 256):
        half = (n + 1) // 2
        out.append(("two lanes opening at the same knots", np.concatenate([np.arange(half), np.arange(n - half)]) * 10))
        out.append(("random, alphabet of 3", rng.integers(0, 3, n)))
        out.append(("random, alphabet of n / 2", rng.integers(0, max(n // 2, 1), n)))
    for n in (17, 40, 64, 100, 256):
        k = rng.integers(0, 5, n)
        out += [("all equal", np.zeros(n, dtype=int)), ("sorted with ties", np.sort(k)), ("reversed with ties", np.sort(k)[::-1]),
                ("organ pipe", np.minimum(np.arange(n), n - 1 - np.arange(n)) // 2)]
    for n in (65, 100, 128, 200, 256):
        adv = O.std_sort_adversary(n)
        out += [("McIlroy adversary (heap-sort fallback)", adv), ("McIlroy adversary, keys halved (fallback with ties)", adv >> 1)]
    return out


if __name__ == "__main__":
    cases = [dict(kind=kind, keys=[int(v) for v in k], perm=[int(v) for v in O.std_sort_order(k)]) for kind, k in key_arrays()]
    with open(os.path.join(HERE, "std_sort_order.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]\n")
    print(len(cases), "cases")
