"""What the compiler made of the long form's two rescue kernels, read from the code object the build produced (no GPU): the
four-wavefront one (ipm_solve_long_rescue_kernel) fits the CU's 160 KB of LDS because its wavefronts carry no
reduction rows -- 4 x 72 x 512 + (8 + 4 x 256) x 8 = 155 712 B -- and, like the three-wavefront one, does not spill."""
from test_kernel_resources import kernels_of

CU_LDS = 160 * 1024


def test_the_fourth_wavefront_fits_the_cu_and_nothing_spills():
    ks = kernels_of("btrapz_kernels.o")
    four = [r for n, r in ks.items() if "ipm_solve_long_rescue_kernel" in n]
    three = [r for n, r in ks.items() if "ipm_solve_long_elastic_kernel" in n]
    assert len(four) == 1 and len(three) == 1, sorted(ks)
    assert four[0]["lds"] == 4 * 72 * 512 + (8 + 4 * 256) * 8 == 155712 and four[0]["lds"] <= CU_LDS, four
    assert 4 * 76 * 512 + (8 + 4 * 256) * 8 > CU_LDS               # with the reduction rows it would not
    assert three[0]["lds"] == 3 * 76 * 512 + (8 + 4 * 256) * 8, three
    for r in four + three:
        assert r["scratch"] == 0 and 256 < r["vgpr"] <= 512 and r["agpr"] > 0, r
