#!/usr/bin/env python3
"""Golden vectors for the projection onto the reference line (include/btrapz_hip_frenet.h), produced by the REFERENCE'S
OWN code.

`cartesian_to_frenet3D` is taken out of /root/reference/src/cart_frenet.py with `ast` at run time (the module itself
cannot be imported: commonroad is absent and it loads a scenario at import) and executed with numpy and the names of
`math` that the module imports.  Nothing of that source is stored here: the output, frenet_goldens.json, holds the
reference lines, the inputs and the six numbers the reference returned.

The reference leaves the matched point on the line to the caller.  Queries therefore sit ON THE NORMALS OF TABLE POINTS,
where the table point is the projection: p = r_k + l n_k with |l| >= 0.01 (below that the reference snaps l to 0, which
the library does not keep), on a straight line, two arcs and a clothoid (spectral_amd.synth).  The reference returns the
lateral state over arc length (d, d', d''); the file also stores it over time, dl = d' ds and ddl = d'' ds^2 + d' dds,
formed in float64 from the reference's numbers.

    python tests/golden/make_frenet_goldens.py          # needs /root/reference (build container only)
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


def reference_function():
    tree = ast.parse(open(SRC).read())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "cartesian_to_frenet3D"]
    ns = {k: getattr(math, k) for k in dir(math) if not k.startswith("_")}
    ns["np"] = np
    exec(compile(ast.Module(body=nodes, type_ignores=[]), SRC, "exec"), ns)
    return ns["cartesian_to_frenet3D"]


def main():
    from spectral_amd import synth
    c2f = reference_function()
    rng = np.random.default_rng(20261021)
    lines = dict(straight_rotated=synth.refline_straight(60.0, 0.5, x0=-1.0, y0=4.0, theta0=2.5),
                 arc_left=synth.refline_arc(60.0, 0.5, 30.0, theta0=0.3),
                 arc_right=synth.refline_arc(60.0, 0.5, -40.0, x0=10.0, theta0=-2.9),     # (its heading crosses -pi)
                 clothoid=synth.refline_clothoid(60.0, 0.5, -0.02, 0.002, theta0=1.0))
    samples = []
    for name, rl in lines.items():
        t = {k: rl.host[k][0] for k in FIELDS}
        for i in rng.choice(np.arange(1, rl.M - 1), 48, replace=False):
            i = int(i)
            l = float(rng.uniform(0.01, 6.0)) * (1.0 if rng.random() < 0.5 else -1.0)
            x = float(t["rx"][i] - math.sin(t["rtheta"][i]) * l)
            y = float(t["ry"][i] + math.cos(t["rtheta"][i]) * l)
            theta = float(t["rtheta"][i] + rng.uniform(-1.0, 1.0))
            kappa, v, a = float(rng.uniform(-0.05, 0.05)), float(rng.uniform(0.5, 12.0)), float(rng.uniform(-3.0, 3.0))
            sc, dc = c2f(t["rs"][i], t["rx"][i], t["ry"][i], t["rtheta"][i], t["rkappa"][i], t["rdkappa"][i], x, y, v, a, theta, kappa)
            sc, dc = [float(q) for q in sc], [float(q) for q in dc]
            samples.append(dict(line=name, i=i, cart=[x, y, theta, kappa, v, a], s_condition=sc, d_condition=dc,
                                frenet=[sc[0], sc[1], sc[2], dc[0], dc[1] * sc[1], dc[2] * sc[1] * sc[1] + dc[1] * sc[2]]))
    out = dict(order_in=["x", "y", "theta", "kappa", "v", "a"], order_out=["s", "ds", "dds", "l", "dl", "ddl"],
               lines={name: {k: [float(v) for v in rl.host[k][0]] for k in FIELDS} for name, rl in lines.items()}, samples=samples)
    json.dump(out, open(os.path.join(HERE, "frenet_goldens.json"), "w"), separators=(",", ":"))
    print("wrote frenet_goldens.json:", len(samples), "samples on", len(lines), "lines")


if __name__ == "__main__":
    main()
