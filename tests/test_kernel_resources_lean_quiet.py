"""What the compiler made of the kernels of the quiet-axis schedule (spectral_amd/csrc/btrapz_lean_quiet.hip), read from
the code object the build produced (no GPU).  The solve kernels run beside and in place of the lean solve kernels and are
held to what those are held to (test_kernel_resources.py): two wavefronts per SIMD -- at most 256 registers, none of them
accumulation registers, 20 KB of LDS per wavefront -- and a bound on scratch."""
from test_kernel_resources import kernels_of


def test_quiet_axis_kernels_fit_two_wavefronts_per_simd():
    ks = kernels_of("btrapz_lean_quiet.o")
    for name, r in sorted(ks.items()):
        print(name, r)
    solve = {n: r for n, r in ks.items() if "ipm_solve_lean_quiet" in n}
    plain = [n for n in solve if "plain" in n]
    fused = [n for n in solve if "plain" not in n]
    counts = [n for n in ks if "quiet_counts_kernel" in n]
    assert len(plain) == 1 and len(fused) == 1 and len(counts) == 1, sorted(ks)
    assert len(ks) == 3, sorted(ks)
    for name, r in solve.items():
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (name, r)
        assert r["lds"] == 20480, (name, r)
    # Scratch.  The single-body kernel is the plain body of ipm_solve_lean_kernel: the 120 B of the cold lean
    # instantiations (92 B when this was written).  The fused kernel carries the resume body and the plain body under one
    # register allocation and takes the place of ipm_solve_lean_pipe_kernel (resume + capped body): it is held to that
    # kernel's 132 B (104 B when this was written).
    assert solve[plain[0]]["scratch"] <= 120, solve[plain[0]]
    assert solve[fused[0]]["scratch"] <= 132, solve[fused[0]]
    # the count kernel declares no shared memory and keeps everything in registers
    r = ks[counts[0]]
    assert r["lds"] == 0 and r["scratch"] == 0 and r["agpr"] == 0, r
