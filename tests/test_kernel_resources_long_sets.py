"""What the compiler made of the four instantiations behind btrapz_solve_long_sets_device, read from the code
object the build produced (no GPU): each is there once, none spills, the four-wavefront rescue kernel keeps the LDS trick of
ipm_solve_long_rescue_kernel (no reduction rows: it fits the CU's 160 KB) and the three-wavefront one has the LDS of
ipm_solve_long_elastic_kernel -- a set's scalars and its M'QM table come through scalar loads and cost no LDS row."""
from test_kernel_resources import kernels_of

CU_LDS = 160 * 1024
NEW = ("ipm_solve_long_warm_sets_kernel", "ipm_solve_elastic_sets_kernel", "ipm_solve_long_elastic_sets_kernel",
       "ipm_solve_long_rescue_sets_kernel")


def named(ks, name):
    """The kernels whose mangled name holds `name` as a whole identifier (<length><name>E...)."""
    return [r for n, r in ks.items() if "%d%sE" % (len(name), name) in n]


def test_the_four_new_kernels_are_there_once_and_do_not_spill():
    ks = kernels_of("btrapz_kernels.o")
    for name in NEW:
        found = named(ks, name)
        assert len(found) == 1, (name, sorted(ks))
        r = found[0]
        assert r["scratch"] == 0 and 256 < r["vgpr"] <= 512 and r["agpr"] > 0, (name, r)


def test_lds_of_the_rescue_kernels():
    ks = kernels_of("btrapz_kernels.o")
    four, three = named(ks, "ipm_solve_long_rescue_sets_kernel")[0], named(ks, "ipm_solve_long_elastic_sets_kernel")[0]
    assert four["lds"] <= CU_LDS and four["lds"] == named(ks, "ipm_solve_long_rescue_kernel")[0]["lds"] == 155712, four
    assert three["lds"] == named(ks, "ipm_solve_long_elastic_kernel")[0]["lds"], three
    assert named(ks, "ipm_solve_elastic_sets_kernel")[0]["lds"] == named(ks, "ipm_solve_elastic_kernel")[0]["lds"]
    assert named(ks, "ipm_solve_long_warm_sets_kernel")[0]["lds"] == named(ks, "ipm_solve_long_warm_kernel")[0]["lds"]
