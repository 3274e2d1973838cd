"""btrapz_corridor_vjp_host under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone host program
(spectral_amd/csrc/host_check/corridor_vjp_check.cpp, `make -C spectral_amd/csrc host_asan_vjp`; g++, no HIP, no GPU) over the
edges of the backward pass's shapes -- 3 and 512 knots, 64 obstacles, lists that overflow, no selection, subsets of outputs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spectral_amd", "csrc")
BIN = os.path.join(ROOT, "spectral_amd", "lib", "corridor_vjp_check_asan")


def test_corridor_vjp_host_runs_clean_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-C", CSRC, "host_asan_vjp"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok") and "runtime error" not in p.stderr, (p.stdout[-1500:], p.stderr[-1500:])
    counts = [int(line.split("seg_count")[1].split()[0]) for line in p.stdout.splitlines() if "seg_count" in line]
    assert -1 in counts and 0 in counts and max(counts) >= 7, counts
