"""btrapz_prism_bounds_jvp_host and btrapz_corridor_jvp_host under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
host program (spectral_amd/csrc/host_check/stage_jvp_check.cpp, `make -C spectral_amd/csrc host_asan_stage_jvp`; g++, no HIP,
no GPU, nothing loaded into Python) over the edges of the two stages' shapes with 1, 2 and 32 directions, subsets of the
tangents and outputs, NaN-prefilled outputs, and the refusals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectral_amd", "csrc")
BIN = os.path.join(ROOT, "spectral_amd", "lib", "stage_jvp_check_asan")


def test_stage_jvp_host_twins_run_clean_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "host_asan_stage_jvp"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "runtime error" not in p.stderr, (p.stdout[-1500:], p.stderr[-1500:])
    lines = [line for line in p.stdout.splitlines() if " -> rc " in line]
    assert len(lines) >= 40 and sum("rc -1" in line for line in lines) >= 11, lines
    assert any(line.startswith("prism") and "rc -1" in line for line in lines) and any(line.startswith("corridor") and "rc -1" in line for line in lines)
