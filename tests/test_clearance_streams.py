"""The three entry points of include/btrapz_hip_clearance.h in the table of stream cases (tests/stream_cases.py), entered from
here with that module's own `case` decorator: tests/test_stream_cases.py demands a case of every entry point that takes a
`void *stream`, and tests/test_gpu_streams.py then holds each case to the stream contract (T1 ... T6) on side streams.

The cases are entered when this module is IMPORTED, which pytest does while it collects -- before any test runs, and,
module names being collected in order, before tests/test_gpu_streams.py reads the table for its parameters.  They are
therefore in the table whenever the suite or the directory is run; tests/test_stream_cases.py run ALONE does not import
this module and reports the three entry points as missing.

Shapes: R = 4 rows of n = 33 samples against one scene of 3 obstacles (the plane cases' R and n)."""
import numpy as np

import stream_cases as SC

CR, CN, CO = SC.CR, SC.CN, 3
NAMES = {"plane: clearance": "btrapz_clearance_device", "plane: clearance vjp": "btrapz_clearance_vjp_device",
         "plane: clearance jvp": "btrapz_clearance_jvp_device"}


class DeviceObstacles:
    """What BatchSolver.clearance reads of a layout.Obstacles, over working tensors (layout.Obstacles copies to the host
    when it is made, which a run() must not do)."""

    def __init__(self, pose, half):
        self.n_scenes, self.O, _, self.n = pose.shape
        self._arrays = (pose, half, None)

    def on(self, device):
        return self._arrays


def clearance_builder(kind):
    def build(solver):
        import clearance_cases as CL
        import torch
        half = torch.tensor([[[2.3, 0.9], [1.1, 0.6], [4.0, 1.2]]], dtype=torch.float64, device=solver.device)

        def make(seed):
            rng = SC.rng_of(seed, 16)
            c = CL.make_case(CR, CN, CO, seed=70 + seed)
            a = dict(cart=c["cart"], pose=c["obstacles"].host["pose"], count=rng.integers(CN // 2, CN + 1, CR).astype(np.int32),
                     scene_index=np.zeros(CR, dtype=np.int32))
            if kind != "clearance":
                up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(solver.device)
                o = solver.clearance(up(a["cart"]), DeviceObstacles(up(a["pose"]), half), CL.FOOT, want=("which",))
                torch.cuda.synchronize()
                a["which"] = o["which"].reshape(-1).contiguous()
            if kind == "clearance vjp":
                a["clear_bar"] = rng.standard_normal((CR, CN))
            if kind == "clearance jvp":
                a["cart_dot"] = rng.standard_normal((2, CR, 6, CN)); a["obs_dot"] = rng.standard_normal((2, 1, CO, 3, CN))
            return a
        X, Y = SC.both(make)

        def run(w):
            ob = DeviceObstacles(w["pose"], half)
            kw = dict(count=w["count"], scene_index=w["scene_index"])
            if kind == "clearance":
                o = solver.clearance(w["cart"], ob, CL.FOOT, d_safe=0.5, **kw)
                return dict(o["audit"], clear=o["clear"], which=o["which"])
            which = w["which"].reshape(CR, CN)
            if kind == "clearance vjp":
                return dict(cart_bar=solver.clearance_vjp(w["cart"], ob, CL.FOOT, which, w["clear_bar"], **kw))
            return dict(clear_dot=solver.clearance_jvp(w["cart"], ob, CL.FOOT, which, w["cart_dot"], obs_dot=w["obs_dot"], **kw))
        return X, Y, run, dict(ranges=dict(count=(0, CN), scene_index=(0, 0), which=(-1, 16 * (CO - 1) + 11)))
    return build


for _name, _entry in NAMES.items():
    if all(c.name != _name for c in SC.CASES):          # (a second import of this module under another name enters nothing twice)
        SC.case(_name, _entry)(clearance_builder(_name.split(": ")[1]))


def test_the_three_entry_points_are_in_the_table():
    for name, entry in NAMES.items():
        c = SC.by_name(name)
        assert c.entries == (entry,) and c.asynchronous and not c.workspace


def test_no_entry_point_with_a_stream_is_left_without_a_case():
    import test_stream_cases as T
    named = {e for c in SC.CASES for e in c.entries}
    assert not [n for n in T.stream_entry_points() if n not in named and n not in SC.EXEMPT]
    assert set(NAMES.values()) <= set(T.stream_entry_points())
