"""GPU tests of the tetrahedral rest dictionary of schedule LAYERED: k_layer reading Qinv, the strain limits and w from the table in
LDS (PIES_LAYER_REST_DICT unset) computes bit for bit what it computes streaming them per element (PIES_LAYER_REST_DICT=0), and
what the oracle computes replaying the exported order.  Every k_layer variant that reads the table has a case: the 256-register
path, the 128-register four-wavefronts-per-SIMD path, and the tail loop for colour classes larger than the workgroup."""
import os

import numpy as np
import pytest

import layer_rest_scenes
import scenes

pytestmark = pytest.mark.gpu

STATE = ("positions", "prev_positions", "velocities")


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
    sets, layer = g.count(pies.LAYER_REST_SETS), g.launch_counts()["layer"]
    g.tick(case["ticks"])
    out = {k: getattr(g, k) for k in STATE}
    g.close()
    return out, sets, layer, o


@pytest.mark.parametrize("name", sorted(layer_rest_scenes.CASES))
def test_dictionary_equals_streamed_records_and_the_oracle(pies, oracle, tune, name):
    case = layer_rest_scenes.CASES[name]
    for k, v in case.get("tuning", {}).items():
        tune(k, v)
    on, sets, layer, o = _run(pies, case, oracle)
    assert layer > 0  # schedule LAYERED is what ran
    assert case["sets"](sets), sets
    tune("PIES_LAYER_REST_DICT", "0")
    off, sets0, layer0, _ = _run(pies, case)
    assert sets0 == 0 and layer0 == layer
    for k in STATE:
        assert np.isfinite(on[k]).all()
        assert np.array_equal(on[k].view(np.uint32), off[k].view(np.uint32)), k
        assert np.array_equal(on[k].view(np.uint32), getattr(o, k).view(np.uint32)), k
    assert np.abs(on["positions"] - o.positions).max() == 0.0


def test_wpe4_case_has_more_tiles_than_compute_units(pies):
    """(what selects the 128-register variants in launch_layer: more than 256 tiles - workgroups - in a launch's phase)"""
    g = pies.Solver(scenes.pbd_options(pies, 1), device=pies.DEVICE_NONE)
    layer_rest_scenes.CASES["wpe4_3x3x600"]["build"](g)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    g.finalize()
    assert g.count(pies.NODES) == 3 * 3 * 600 and g.count(pies.LAYER_MAX_TILES) > 256, g.count(pies.LAYER_MAX_TILES)
    small = pies.Solver(scenes.pbd_options(pies, 1), device=pies.DEVICE_NONE)
    layer_rest_scenes.CASES["headline_4x4x12"]["build"](small)
    small.set_schedule(pies.SCHEDULE_LAYERED)
    small.finalize()
    assert 0 < small.count(pies.LAYER_MAX_TILES) <= 256  # (the 256-register path's case)


def test_tet_goldens_through_the_dictionary(pies, tune):
    """The tetrahedral golden vectors (tests/golden/tet_projection.npz) through k_layer with the dictionary: 32 of them, each over
    16 copies of its nodes, so that 32 sets cover 512 elements; the same tolerance as tests/test_golden_gpu.py."""
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
        sets, layer = g.count(pies.LAYER_REST_SETS), g.launch_counts()["layer"]
        g.tick(1)
        out = g.positions.reshape(n, 4, 3)
        g.close()
        return out, sets, layer
    out, sets, layer = run()
    assert layer > 0 and sets == nset, (layer, sets)
    for k in range(n):
        err = np.abs(out[k] - exp[k]).max()
        assert err <= 5e-5 * max(1.0, np.abs(exp[k]).max()) + np.abs(x[k]).max() * 2.4e-7, (k, err)
    tune("PIES_LAYER_REST_DICT", "0")
    out0, sets0, _ = run()
    assert sets0 == 0 and np.array_equal(out.view(np.uint32), out0.view(np.uint32))
