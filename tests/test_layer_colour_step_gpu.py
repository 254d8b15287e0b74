"""The tetrahedral colour step of k_layer, piece by piece, at the smallest shapes at which each piece can go wrong: after 3 ticks
positions, previous positions and velocities equal, byte for byte, the oracle replaying the exported order, the same build with
the projection in tet_core's form (PIES_LAYER_TET_FORM=0) and the same build streaming the rest constants (PIES_LAYER_REST_DICT=0).

  headline_4x4x12   classes of 4 - 5 elements: most lanes are masked, and their look-ahead reads the clamped slot
  beam_2x2x12       one cube per slab: segments whose classes hold a single element
  lattice_w9        54 sets: set indices that use the second 3-bit field of the record's first word
  lattice_w64       64 w values: 6 orientations x 64 = 384 sets, over the cap of 64, the streamed path
  lattice_64_sets   4 orientations x 16 w values = 64 sets exactly: indices up to 63, all six bits
  lattice_w65       over the cap: the streamed records, the edges as pair subtractions without the table
  tall_17x17x3_block256  the smallest cross-section whose largest colour class (280, a distance class) exceeds a workgroup forced to
                    256 threads - 16 x 16 gives 247: the distance segment's loop for the rest of a class runs in some colours
  tall_28x28x3_block256  a largest class of about 769 (a distance class; the tetrahedral ones are smaller and not asserted)
  tall_24x24x3_tets_block256  the same beam shape WITHOUT distance constraints: every class is tetrahedral, and the largest (276;
                    23 x 23 gives 242) exceeds the 256 threads: the tetrahedral loop for the rest of a class (the set index from the first word and the
                    pair-ordered row there too), asserted through PIES_LAYER_MAX_CLASS

(The cases' figures - sets, largest class - were found on host-only handles and are asserted below on such handles, without a GPU.)"""
import numpy as np
import pytest

import layer_rest_scenes
import scenes

STATE = ("positions", "prev_positions", "velocities")


def _lattice(nw, seed, tets_per_cell=6):
    def build(s):
        if tets_per_cell == 6:
            layer_rest_scenes.lattice_with_w(s, nw)
        else:
            _lattice_some_orientations(s, nw, tets_per_cell)
        scenes.perturb(s, seed, 0.03)
    return build


def _tall_beam(dims, seed=3, **kw):
    """a beam whose layers are spaced so that z is its longest axis: levelled across its cross-section, as BASELINE config 2 is"""
    def build(s):
        scenes.build_beam(s, dims, **kw)
        p = s.positions.copy()
        p[:, 2] *= 2.0 * dims[0]  # (the rest state is taken at finalize: the spaced lattice is at rest)
        s.set_positions(p)
        scenes.perturb(s, seed, 0.05)
    return build


def _lattice_some_orientations(s, nw, per_cell, dims=(6, 6, 14)):
    """lattice_with_w with only the first `per_cell` of a cell's six tetrahedra (fewer orientations, so that orientations x nw
    can hit the cap exactly), the w value changing from slab to slab so that every w meets every orientation"""
    W, H, D = dims
    idx = lambda x, y, z: (z * H + y) * W + x  # noqa: E731
    s.add_nodes_raw(np.float32([[x, y + 1.0, z] for z in range(D) for y in range(H) for x in range(W)]), radius=0.3)
    kinds = ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7))[:per_cell]
    by_w = [[] for _ in range(nw)]
    edges = set()
    cell = 0
    for z in range(D - 1):
        for y in range(H - 1):
            for x in range(W - 1):
                c = [idx(x + (b & 1), y + ((b >> 1) & 1), z + (b >> 2)) for b in range(8)]
                for t in kinds:
                    by_w[cell % nw].append([c[i] for i in t])
                    edges.update((min(c[t[a]], c[t[b]]), max(c[t[a]], c[t[b]])) for a in range(4) for b in range(a + 1, 4))
                cell += 1
    s.add_distance(np.uint32(sorted(edges)), 0.5)
    for part, w in zip(by_w, np.linspace(0.02, 0.9, nw)):
        s.add_tet(np.uint32(part), float(w))


# "sets": PIES_LAYER_REST_SETS with the dictionary allowed (a number, or its bounds: a lattice has one set per orientation; the
# 2 x 2 beam is too small for a dictionary to be a compression); "block": the workgroup launch_layer takes; "cls": bounds of the largest class
CASES = {
    "headline_4x4x12": {"build": layer_rest_scenes._beam((4, 4, 12)), "iterations": 20, "sets": (1, 12), "block": 256, "cls": (1, 256)},
    "beam_2x2x12": {"build": layer_rest_scenes._beam((2, 2, 12)), "iterations": 20, "sets": (0, 12), "block": 256, "cls": (1, 256)},
    "lattice_w9": {"build": _lattice(9, 6), "iterations": 4, "sets": 54, "block": 256, "cls": (1, 256)},
    "lattice_w64": {"build": _lattice(64, 6), "iterations": 4, "sets": 0, "block": 256, "cls": (1, 256)},
    "lattice_64_sets": {"build": _lattice(16, 6, tets_per_cell=4), "iterations": 4, "sets": 64, "block": 256, "cls": (1, 256)},
    "lattice_w65": {"build": _lattice(65, 6), "iterations": 4, "sets": 0, "block": 256, "cls": (1, 256)},
    "tall_17x17x3_block256": {"build": _tall_beam((17, 17, 3)), "iterations": 3, "sets": (1, 12), "block": 256, "cls": (257, 300),
                              "tuning": {"PIES_LAYER_BLOCK": "256"}},
    "tall_28x28x3_block256": {"build": _tall_beam((28, 28, 3)), "iterations": 3, "sets": (1, 12), "block": 256, "cls": (700, 800),
                              "tuning": {"PIES_LAYER_BLOCK": "256"}},
    "tall_24x24x3_tets_block256": {"build": _tall_beam((24, 24, 3), distance=False), "iterations": 3, "sets": (1, 12), "block": 256,
                                   "cls": (257, 300), "tets_only": True, "tuning": {"PIES_LAYER_BLOCK": "256"}},
}
TICKS = 3


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
        o.tick(TICKS)
    sets, layer, cls = g.count(pies.LAYER_REST_SETS), g.launch_counts()["layer"], g.count(pies.LAYER_MAX_CLASS)
    g.tick(TICKS)
    out = {k: getattr(g, k) for k in STATE}
    g.close()
    return out, sets, layer, cls, o


def _check_figures(case, sets, cls):
    lo, hi = case["sets"] if isinstance(case["sets"], tuple) else (case["sets"], case["sets"])
    assert lo <= sets <= hi, sets
    lo, hi = case["cls"]
    assert lo <= cls <= hi, cls
    if "tuning" in case:
        assert cls > int(case["tuning"]["PIES_LAYER_BLOCK"]), cls  # the largest class exceeds the workgroup


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_colour_step_equals_the_oracle_tet_core_and_streamed_records(pies, oracle, tune, name):
    case = CASES[name]
    for k, v in case.get("tuning", {}).items():
        tune(k, v)
    new, sets, layer, cls, o = _run(pies, case, oracle)
    assert layer > 0  # schedule LAYERED is what ran
    _check_figures(case, sets, cls)
    tune("PIES_LAYER_TET_FORM", "0")
    core, sets_core, layer_core, _, _ = _run(pies, case)
    tune("PIES_LAYER_TET_FORM", None)
    tune("PIES_LAYER_REST_DICT", "0")
    streamed, sets_streamed, layer_streamed, _, _ = _run(pies, case)
    assert sets_core == sets and sets_streamed == 0 and layer_core == layer and layer_streamed == layer
    for k in STATE:
        assert np.isfinite(new[k]).all()
        assert new[k].tobytes() == getattr(o, k).astype(new[k].dtype, copy=False).tobytes(), k
        assert new[k].tobytes() == core[k].tobytes(), k
        assert new[k].tobytes() == streamed[k].tobytes(), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_has_its_figures(pies, tune, name):
    """(host only) the sets of the rest dictionary, the largest colour class against the workgroup, and the 256-register
    instantiations (at most 256 tiles) that hold the code under test"""
    case = CASES[name]
    for k, v in case.get("tuning", {}).items():
        tune(k, v)
    g = pies.Solver(scenes.pbd_options(pies, 1), device=pies.DEVICE_NONE)
    case["build"](g)
    g.set_flag(1, 0)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    g.finalize()
    tiles, cls, sets = g.count(pies.LAYER_MAX_TILES), g.count(pies.LAYER_MAX_CLASS), g.count(pies.LAYER_REST_SETS)
    assert 0 < tiles <= 256, tiles
    _check_figures(case, sets, cls)
    if case.get("tets_only"):
        assert g.count(pies.DISTANCE) == 0 and g.count(pies.TET) > 0  # the largest class is a tetrahedral one
    want = int(case.get("tuning", {}).get("PIES_LAYER_BLOCK", 0)) or cls
    assert (256 if want <= 256 else 512 if want <= 512 else 1024) == case["block"]
