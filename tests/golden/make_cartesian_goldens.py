#!/usr/bin/env python3
"""Golden vectors for the Cartesian stage (include/btrapz_hip_cartesian.h), produced by the REFERENCE'S OWN code.

`NormalizeAngle` and `frenet_to_cartesian3D` are taken out of /root/reference/src/cart_frenet.py with `ast` at run time
(the module itself cannot be imported: commonroad is absent and it loads a scenario at import) and executed with the
names of `math` that the module imports.  Nothing of that source is stored here: the output, cartesian_goldens.json, holds
the reference lines, the inputs and the six numbers the reference returned.

Samples sit ON table points (s == rs[i]: no interpolation enters, the reference takes the point's own values) of a
straight line, an arc and a clothoid (spectral_amd.synth), with ds >= 0.5.  The reference takes the lateral state over
arc length (d, d', d''), the library over time (l, dl, ddl); d', d'', ds and dds are drawn as small dyadic rationals so
that dl = d' ds and ddl = d'' ds^2 + d' dds are exact in float64: both sets describe the same state to the last bit.

    python tests/golden/make_cartesian_goldens.py          # needs /root/reference (build container only)
"""
import ast
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SRC = "/root/reference/src/cart_frenet.py"
FIELDS = ("rs", "rx", "ry", "rtheta", "rkappa", "rdkappa")


def reference_functions():
    tree = ast.parse(open(SRC).read())
    want = {"NormalizeAngle", "frenet_to_cartesian3D"}
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    ns = {k: getattr(math, k) for k in dir(math) if not k.startswith("_")}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), SRC, "exec"), ns)
    return ns["frenet_to_cartesian3D"]


def main():
    from spectral_amd import synth
    f2c = reference_functions()
    rng = np.random.default_rng(20261021)
    lines = dict(straight=synth.refline_straight(60.0, 0.5, x0=3.0, y0=-2.0, theta0=0.0),
                 straight_rotated=synth.refline_straight(60.0, 0.5, x0=-1.0, y0=4.0, theta0=2.5),
                 arc_left=synth.refline_arc(60.0, 0.5, 25.0, theta0=0.3),
                 arc_right=synth.refline_arc(60.0, 0.5, -40.0, x0=10.0, theta0=-2.9),     # (its heading crosses -pi)
                 clothoid=synth.refline_clothoid(60.0, 0.5, -0.02, 0.002, theta0=1.0))
    dy = lambda lo, hi, q: float(rng.integers(int(lo * q), int(hi * q) + 1)) / q     # a dyadic rational in [lo, hi]
    samples = []
    for name, rl in lines.items():
        t = {k: rl.host[k][0] for k in FIELDS}
        for i in rng.choice(rl.M, 64, replace=False):
            i = int(i)
            ds, dds = dy(0.5, 12.0, 16), dy(-3.0, 3.0, 16)
            d, d1, d2 = float(rng.uniform(-3.0, 3.0)), dy(-0.75, 0.75, 64), dy(-0.25, 0.25, 64)
            dl, ddl = d1 * ds, d2 * ds * ds + d1 * dds
            assert dl / ds == d1 and (ddl - d1 * dds) / (ds * ds) == d2
            x, y, v, a, theta, kappa = f2c(t["rs"][i], t["rx"][i], t["ry"][i], t["rtheta"][i], t["rkappa"][i], t["rdkappa"][i],
                                           [t["rs"][i], ds, dds], [d, d1, d2])
            samples.append(dict(line=name, i=i, frenet=[float(t["rs"][i]), ds, dds, d, dl, ddl],
                                out=[float(x), float(y), float(theta), float(kappa), float(v), float(a)]))
    out = dict(order_in=["s", "ds", "dds", "l", "dl", "ddl"], order_out=["x", "y", "theta", "kappa", "v", "a"],
               lines={name: {k: [float(v) for v in rl.host[k][0]] for k in FIELDS} for name, rl in lines.items()}, samples=samples)
    json.dump(out, open(os.path.join(HERE, "cartesian_goldens.json"), "w"), separators=(",", ":"))
    print("wrote cartesian_goldens.json:", len(samples), "samples on", len(lines), "lines")


if __name__ == "__main__":
    main()
