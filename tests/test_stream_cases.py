"""Every exported entry point that takes a `void *stream` (include/*.h) has a case in tests/stream_cases.py -- what
tests/test_gpu_streams.py holds to the stream contract -- or an exemption that says why: a new entry point cannot arrive
without one.  No GPU."""
import glob
import os
import re

import stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entry_points():
    """The functions declared in include/*.h with a `void *stream` parameter."""
    names = []
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        text = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"\b(btrapz_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
                names.append(m.group(1))
    return names


def test_the_headers_are_read():
    names = stream_entry_points()
    assert len(names) == len(set(names)) and len(names) >= 38, names
    for known in ("btrapz_solve_batch_device", "btrapz_rescue_violations_device", "btrapz_topk_device", "btrapz_frenet_jvp_device",
                  "btrapz_corridor_batch_jvp_device", "btrapz_solve_long_sets_device"):
        assert known in names, known


def test_every_entry_point_with_a_stream_has_a_case_or_an_exemption():
    named = {e for c in SC.CASES for e in c.entries}
    missing = [n for n in stream_entry_points() if n not in named and n not in SC.EXEMPT]
    assert not missing, missing
    for n, why in SC.EXEMPT.items():
        assert isinstance(why, str) and len(why.split()) >= 5 and why.rstrip().endswith("."), (n, "an exemption is a sentence that says why")


def test_every_name_in_the_table_is_an_entry_point():
    declared = set(stream_entry_points())
    for c in SC.CASES:
        assert c.entries, c.name
        for e in c.entries:
            assert e in declared, (c.name, e)
    for n in SC.EXEMPT:
        assert n in declared, n


def test_the_flags_are_stated():
    names = [c.name for c in SC.CASES]
    assert len(names) == len(set(names))
    for c in SC.CASES:
        assert c.asynchronous or c.blocking_doc.strip(), (c.name, "a blocking case names the line that says so")
    # the one documented block of the batched entry points: the long candidates of a ragged record with slots beyond 64
    assert [c.name for c in SC.CASES if not c.asynchronous] == ["ragged solve, stride beyond 64: the long candidates"]
    quoted = re.search(r'"([^"]+)"', SC.by_name("ragged solve, stride beyond 64: the long candidates").blocking_doc).group(1)
    header = " ".join(re.sub(r"^\s*\*", " ", l) for l in open(os.path.join(ROOT, "include", "btrapz_hip.h")).read().splitlines())
    assert " ".join(quoted.split()) in " ".join(header.split()), quoted


def test_the_split_threshold_is_read_from_the_source():
    assert SC.split_group() >= 2
