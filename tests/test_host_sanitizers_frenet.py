"""btrapz_frenet_host, _vjp_host and _jvp_host under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host
program (spectral_amd/csrc/host_check/frenet_check.cpp, `make -C spectral_amd/csrc host_asan_frenet`; g++, no HIP, no GPU,
nothing loaded into Python) with every buffer at exactly its documented size, over the edges of the shapes -- 1 row,
1 query, tables of 2 and 3 points, both layouts, the three orders, counts 0, 1, n and beyond n, a line_index out of range,
windows that are whole, narrow, NaN and reversed, queries on table normals, off the line and NaN, intervals of wild values
handed to the derivatives, a table that is not increasing -- and the refusals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectral_amd", "csrc")
BIN = os.path.join(ROOT, "spectral_amd", "lib", "frenet_check_asan")


def test_frenet_host_runs_clean_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "host_asan_frenet"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "runtime error" not in p.stderr, (p.stdout[-1500:], p.stderr[-1500:])
    cases = [line for line in p.stdout.splitlines() if " -> rc 0 " in line]
    refusals = [line for line in p.stdout.splitlines() if line.startswith("refusal") and line.endswith("rc -1")]
    assert len(cases) >= 16 and len(refusals) >= 17, p.stdout[-1500:]
    assert any(" outside 0 " not in line for line in cases) and any(" kept 0 " not in line for line in cases)
