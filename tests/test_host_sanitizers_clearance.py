"""btrapz_clearance_host, _vjp_host and _jvp_host under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host
program (spectral_amd/csrc/host_check/clearance_check.cpp, `make -C spectral_amd/csrc host_asan_clearance`; g++, no HIP, no
GPU, nothing loaded into Python) with every buffer at exactly its documented size, over the edges of the shapes -- 1 row,
1 sample, 1 and 17 obstacles, counts 0, 1, n and beyond n, a scene_index out of range, obstacle counts 0, ragged and beyond
O, NaN ego and obstacle poses, a `which` that names nothing -- and the refusals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectral_amd", "csrc")
BIN = os.path.join(ROOT, "spectral_amd", "lib", "clearance_check_asan")


def test_clearance_host_runs_clean_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "host_asan_clearance"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "runtime error" not in p.stderr, (p.stdout[-1500:], p.stderr[-1500:])
    cases = [line for line in p.stdout.splitlines() if " -> rc 0 " in line]
    refusals = [line for line in p.stdout.splitlines() if line.startswith("refusal") and line.endswith("rc -1")]
    assert len(cases) >= 8 and len(refusals) >= 23, p.stdout[-1500:]
    assert any(" invalid 0 " not in line for line in cases) and any(" kept 0 " not in line for line in cases)
    assert any(" nobody 0 " not in line for line in cases)
