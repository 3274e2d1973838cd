"""btrapz_prism_bounds_vjp_host under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program
(spectral_amd/csrc/host_check/prism_vjp_check.cpp, `make -C spectral_amd/csrc host_asan_prism_vjp`; g++, no HIP, no GPU, nothing
loaded into Python) over the edges of the backward pass's shapes -- 1 knot, 1 and 16 cars, 33 strips with O = 32, 33 and 34,
inactive slots, identical cars, either cotangent missing, the refusals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectral_amd", "csrc")
BIN = os.path.join(ROOT, "spectral_amd", "lib", "prism_vjp_check_asan")


def test_prism_vjp_host_runs_clean_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "host_asan_prism_vjp"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "runtime error" not in p.stderr, (p.stdout[-1500:], p.stderr[-1500:])
    lines = [line for line in p.stdout.splitlines() if " -> rc " in line]
    assert len(lines) >= 14 and any("rc -1" in line for line in lines), lines
