"""What the compiler made of the kernels of the three-launch schedule (spectral_amd/csrc/btrapz_lean_pipe.hip), read from
the code object the build produced (no GPU): they run beside and in place of the lean solve kernels, so they are held to
what those are held to (test_kernel_resources.py) -- two wavefronts per SIMD: at most 256 registers, none of them
accumulation registers, 20 KB of LDS per wavefront, and a bound on scratch."""
from test_kernel_resources import kernels_of


def test_pipeline_kernels_fit_two_wavefronts_per_simd():
    ks = kernels_of("btrapz_lean_pipe.o")
    solve = {n: r for n, r in ks.items() if "ipm_solve_lean_pipe" in n}
    assert len(solve) == 3, sorted(ks)       # one axis's capped launch, one axis's resume launch, the fused grid
    assert len(ks) == 4, sorted(ks)          # ... and the copy of the two list lengths
    for name, r in ks.items():
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (name, r)
        assert r["lds"] == (20480 if name in solve else 0), (name, r)
        # Scratch.  The single-body kernels (launches 1 and 3): the 120 B of the cold lean instantiations, whose bodies they
        # are (112 and 92 B).  The fused kernel of launch 2 carries TWO loop bodies under one register allocation and does
        # not reach that (132 B: 96 in its resume part, 128 in its capped part, against 92 and 112 alone) -- which is why
        # launches 1 and 3 have kernels of their own; it is held to the bound test_kernel_resources.py sets for the lean
        # kernels that carry a second body (the warm-start instantiations' in-loop cold restart): 200 B, far below a
        # kernel that spills its state (744 B).
        fused = name in solve and "capped" not in name and "resume" not in name
        assert r["scratch"] <= (200 if fused else 120), (name, r)
