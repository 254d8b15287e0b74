#!/usr/bin/env python3
"""Writes tests/golden/measure_tiny.npz (run once, the fixture is committed):

    python tests/golden/make_measure_golden.py

The fixture holds the scenes tests/test_measure.py holds the fp32 restatements of pies_measure_elements / pies_measure_nodes to
fp64 on - 600 loose tetrahedra with the strain limits (tet_*) and with the volume limits (vol_*), every special element among
them, and 600 nodes in 64 ranges (node_*) - and the deviation from fp64 the restatements showed on them when it was written
(dev_*: each a fraction of the quantity's natural scale, see element_deviation / node_deviation).  The tests' gates are four
times these figures.  The rest data is the library's own (pies_get_rest of a host-only handle): inputs, no GPU is needed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "benchlib")):
    sys.path.insert(0, p)

import test_measure as T  # noqa: E402


def main():
    out, worst = {}, {}
    for prefix, volume in (("tet_", False), ("vol_", True)):
        scene = T.make_element_scene(600, volume)
        dev, margin, differing = T.element_deviation(scene)
        assert differing == 0 and margin >= T.MARGIN, (prefix, differing, margin)
        print(prefix, dev, "smallest margin %.3g" % margin)
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k in ("pos0", "pos1", "ids", "rest"):
            out[prefix + k] = scene[k]
        out[prefix + "lo"], out[prefix + "hi"], out[prefix + "volume"] = T.F(scene["lo"]), T.F(scene["hi"]), np.bool_(volume)
    pos, vel, inv_mass = T.make_node_scene(600)
    ranges, about = T.make_ranges(600, 64)
    out.update(node_pos=pos, node_vel=vel, node_inv_mass=inv_mass, node_ranges=ranges, node_about=about)
    worst["nodes"] = T.node_deviation(pos, vel, inv_mass, ranges, about)
    for k, v in worst.items():
        out["dev_" + k] = np.float64(v)
        print("dev_%s = %.3g" % (k, v))
    np.savez_compressed(os.path.join(HERE, "measure_tiny.npz"), **out)


if __name__ == "__main__":
    main()
