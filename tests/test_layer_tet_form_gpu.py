"""The tetrahedral projection of k_layer on row pairs (tet_rows.h, the default) computes bit for bit what tet_core computes
(PIES_LAYER_TET_FORM=0) and what the oracle computes replaying the exported order: every scene of the rest-dictionary tests, and
beams with the headline's cross-section and wave roles.

The planner levels a body along its longest axis.  _beam((20, 20, 6)), _beam((24, 24, 5)) and _beam((28, 28, 4)) as they stand are
levelled along x (classes of 109 - 117, the 256-thread instantiation); the same beams with their layers spaced so that z is the
longest axis are levelled across the 20 x 20 (24 x 24, 28 x 28) section as BASELINE config 2 is, and give the roles meant:
  tall_20x20x6   512 threads, tetrahedral classes of about 180, distance classes up to 389
  tall_22x22x5   512 threads, a distance class of 472: beyond 448, every wavefront busy in a distance colour
  tall_24x24x5   a class of 563: the 1 024-thread instantiation
  tall_28x28x4   a class of 769: the 1 024-thread instantiation
and tall_20x20x6 once more with the workgroup forced to 256 threads: the loop for the rest of a class larger than the workgroup.
(24 x 24 already exceeds 512, so the case between 448 and 512 is 22 x 22.)  All collapse onto the floor within the first tick as
config 2 does: flat and inverted elements."""
import os

import numpy as np
import pytest

import layer_rest_scenes
import scenes

STATE = ("positions", "prev_positions", "velocities")


def _tall_beam(dims, spacing, seed=3):
    def build(s):
        scenes.build_beam(s, dims)
        p = s.positions.copy()
        p[:, 2] *= spacing  # (the rest state is taken at finalize: the spaced lattice is at rest)
        s.set_positions(p)
        scenes.perturb(s, seed, 0.05)
    return build


CASES = dict(layer_rest_scenes.CASES)
for _dims in ((20, 20, 6), (24, 24, 5), (28, 28, 4)):
    CASES["beam_%dx%dx%d" % _dims] = {"build": layer_rest_scenes._beam(_dims), "iterations": 20, "ticks": 3}
for _dims, _spacing in (((20, 20, 6), 4.0), ((22, 22, 5), 6.0), ((24, 24, 5), 6.0), ((28, 28, 4), 10.0)):
    CASES["tall_%dx%dx%d" % _dims] = {"build": _tall_beam(_dims, _spacing), "iterations": 20, "ticks": 3}
# a workgroup smaller than the class: the loop for the rest of a class, in the row-pair form
CASES["tall_20x20x6_block256"] = {"build": _tall_beam((20, 20, 6), 4.0), "iterations": 6, "ticks": 2, "tuning": {"PIES_LAYER_BLOCK": "256"}}

# what launch_layer selects for the case: (threads of the workgroup, row-pair form available, bounds of the largest colour class).
# More than 256 tiles, or a colour class beyond 512, run the 128-register instantiations, which keep tet_core.
VARIANT = {
    "headline_4x4x12": (256, True, (1, 256)),
    "wpe4_3x3x600": (256, False, (1, 256)),
    "tail_loop_24x24x4_block256": (256, True, (1, 256)),
    "materials": (256, True, (1, 256)),
    "delaunay_no_dictionary": (256, True, (1, 256)),
    "over_the_cap": (256, True, (1, 256)),
    "beam_20x20x6": (256, True, (1, 256)),
    "beam_24x24x5": (256, True, (1, 256)),
    "beam_28x28x4": (256, True, (1, 256)),
    "tall_20x20x6": (512, True, (257, 448)),
    "tall_20x20x6_block256": (256, True, (257, 448)),
    "tall_22x22x5": (512, True, (449, 512)),
    "tall_24x24x5": (1024, False, (513, 1024)),
    "tall_28x28x4": (1024, False, (513, 1024)),
}


def _run(pies, case, oracle=None):
    g = pies.Solver(scenes.pbd_options(pies, case["iterations"]))
    case["build"](g)
    g.set_flag(1, 0)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    g.finalize()
    o = None
    if oracle is not None:
        o = oracle.OracleSolver(scenes.pbd_options(oracle, case["iterations"]))
        case["build"](o)
        o.set_flag(1, 0)
        for t in (pies.POSITION, pies.DISTANCE, pies.TET, pies.BEND):
            if g.count(t):
                o.permute(t, g.order(t))
        o.tick(case["ticks"])
    layer = g.launch_counts()["layer"]
    g.tick(case["ticks"])
    out = {k: getattr(g, k) for k in STATE}
    g.close()
    return out, layer, o


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_row_pairs_equal_tet_core_and_the_oracle(pies, oracle, tune, name):
    case = CASES[name]
    for k, v in case.get("tuning", {}).items():
        tune(k, v)
    new, layer, o = _run(pies, case, oracle)
    assert layer > 0  # schedule LAYERED is what ran
    tune("PIES_LAYER_TET_FORM", "0")
    old, layer0, _ = _run(pies, case)
    assert layer0 == layer
    for k in STATE:
        assert np.isfinite(new[k]).all()
        assert np.array_equal(new[k].view(np.uint32), old[k].view(np.uint32)), k
        assert np.array_equal(new[k].view(np.uint32), getattr(o, k).view(np.uint32)), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_selects_its_variant(pies, tune, name):
    """(host only) launch_layer's choice from the plan: the workgroup from the largest colour class, the 128-register variants from
    more than 256 tiles; a forced workgroup smaller than the class runs the loop for the rest of a class."""
    case = CASES[name]
    for k, v in case.get("tuning", {}).items():
        tune(k, v)
    g = pies.Solver(scenes.pbd_options(pies, 1), device=pies.DEVICE_NONE)
    case["build"](g)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    g.finalize()
    tiles, cls = g.count(pies.LAYER_MAX_TILES), g.count(pies.LAYER_MAX_CLASS)
    assert tiles > 0 and cls > 0, (tiles, cls)
    forced = int(case.get("tuning", {}).get("PIES_LAYER_BLOCK", 0))
    want = forced or cls
    if tiles > 256:
        want = min(want, 512)
    threads = 256 if want <= 256 else 512 if want <= 512 else 1024
    rows = tiles <= 256 and threads <= 512
    assert (threads, rows) == VARIANT[name][:2], (name, tiles, cls, threads, rows)
    lo, hi = VARIANT[name][2]
    assert lo <= cls <= hi, (name, cls)


@pytest.mark.gpu
def test_tet_goldens_through_the_row_pairs(pies, tune):
    """The tetrahedral golden vectors (tests/golden/tet_projection.npz) through k_layer with the projection on row pairs, as
    test_tet_goldens_through_the_dictionary runs them (32 sets x 16 copies, the same tolerance); bitwise equal to tet_core's."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tet_projection.npz"))
    nset, copies = 32, 16
    x, q, exp = (np.repeat(d[k][:nset], copies, axis=0) for k in ("x", "qinv", "expected"))
    n = len(x)

    def run():
        g = pies.Solver(pies.Options(solver=pies.PBD, iterations=1, timeSubsteps=1, fixedTimestepSize=0.012, gravity=0.0,
                                     floorHeight=-1.0e6, damping=0.0), device=0)
        g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
        g.set_schedule(pies.SCHEDULE_LAYERED)
        g.add_nodes_raw(x.reshape(-1, 3), radius=0.01)
        g.add_tet(np.arange(4 * n, dtype=np.uint32).reshape(n, 4), 1.0, float(d["lo"]), float(d["hi"]))
        g.set_rest(pies.TET, q)
        g.finalize()
        layer, cls, tiles = g.launch_counts()["layer"], g.count(pies.LAYER_MAX_CLASS), g.count(pies.LAYER_MAX_TILES)
        g.tick(1)
        out = g.positions.reshape(n, 4, 3)
        g.close()
        return out, layer, cls, tiles
    out, layer, cls, tiles = run()
    assert layer > 0 and cls <= 512 and tiles <= 256, (layer, cls, tiles)  # (an instantiation that has the row-pair form)
    for k in range(n):
        err = np.abs(out[k] - exp[k]).max()
        assert err <= 5e-5 * max(1.0, np.abs(exp[k]).max()) + np.abs(x[k]).max() * 2.4e-7, (k, err)
    tune("PIES_LAYER_TET_FORM", "0")
    out0, _, _, _ = run()
    assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))
