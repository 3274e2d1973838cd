"""The instantiations of btrapz_solve_sets_device (a parameter set per candidate), read from the code objects the build
produced (no GPU): the lean ones keep the lean form's budget -- two wavefronts per SIMD -- and the packed ones do not
spill, as the instantiations they are built from (tests/test_kernel_resources.py)."""
from test_kernel_resources import kernels_of


def test_lean_sets_kernels_fit_two_wavefronts_per_simd():
    lean = {n: r for n, r in kernels_of("btrapz_sets.o").items() if "ipm_solve_lean_sets" in n}
    assert len(lean) == 2, sorted(lean)
    for name, r in lean.items():
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (name, r)
        assert r["lds"] == 20480, (name, r)
        assert r["scratch"] <= (200 if "warm" in name else 120), (name, r)


def test_packed_sets_kernels_do_not_spill():
    solve = {n: r for n, r in kernels_of("btrapz_kernels.o").items() if "ipm_solve_sets" in n or "ipm_solve_long_sets" in n}
    assert len(solve) == 4, sorted(solve)   # ordered cold / warm, split, long
    for name, r in solve.items():
        assert r["scratch"] <= (48 if "warm" in name else 0) and 256 < r["vgpr"] <= 512 and r["agpr"] > 0, (name, r)
