"""The kernels of btrapz_traj_cost_device / btrapz_traj_cost_vjp_device, read from the code object the build produced (no
GPU): no scratch (tests/test_kernel_resources.py reads the code objects)."""
from test_kernel_resources import kernels_of


def test_acost_kernels_have_no_scratch():
    ks = kernels_of("btrapz_acost.o")
    names = sorted(n for n in ks if "acost" in n)
    assert len(names) == 2 and any("vjp" in n for n in names), names
    for name in names:
        r = ks[name]
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512, (name, r)
