"""Scenes of the rest-dictionary tests (test_layer_rest_dict.py on host-only handles, test_layer_rest_dict_gpu.py on the device).
CASES[name] = {"build": scene builder, "iterations", "ticks", "tuning": switches of the case, "sets": predicate on
PIES_LAYER_REST_SETS with the dictionary allowed}."""
import numpy as np

import scenes

CAP = 64  # kLayerRestMaxSets


def lattice_with_w(s, nw, dims=(5, 5, 14)):
    """a lattice of 6 tetrahedra per cell whose elements take nw distinct w values (one add_tet call per value) + its edges"""
    W, H, D = dims
    idx = lambda x, y, z: (z * H + y) * W + x  # noqa: E731
    s.add_nodes_raw(np.float32([[x, y + 1.0, z] for z in range(D) for y in range(H) for x in range(W)]), radius=0.3)
    tets, edges = [], set()
    for z in range(D - 1):
        for y in range(H - 1):
            for x in range(W - 1):
                c = [idx(x + (b & 1), y + ((b >> 1) & 1), z + (b >> 2)) for b in range(8)]
                for t in ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7)):
                    tets.append([c[i] for i in t])
                    edges.update((min(c[t[a]], c[t[b]]), max(c[t[a]], c[t[b]])) for a in range(4) for b in range(a + 1, 4))
    tets = np.uint32(tets)
    s.add_distance(np.uint32(sorted(edges)), 0.5)
    for part, w in zip(np.array_split(tets, nw), np.linspace(0.02, 0.9, nw)):
        s.add_tet(part, float(w))


def _beam(dims, seed=3, **kw):
    def build(s):
        scenes.build_beam(s, dims, **kw)
        scenes.perturb(s, seed, 0.05)
    return build


def _materials(s):
    # two boxes of different scale and w, and one whose strain limits differ: lanes of one wavefront hold different set indices
    scenes.build_beam(s, (4, 4, 9), w_tet=0.05, translation=(0.0, 5.0, 0.0))
    scenes.build_beam(s, (4, 4, 9), w_tet=0.3, scale=0.5, translation=(8.0, 5.0, 0.0))
    first = s.count(9)
    s.create_tet_box(3, 3, 9, translation=(16.0, 5.0, 0.0), w=0.05)
    ids = s.ids(2)
    own = ids[(ids >= first).all(axis=1)]
    s.add_tet(own, 0.2, 0.6, 1.3)  # the same elements again with other strain limits (and w)
    scenes.perturb(s, 4, 0.05)


_MESH = {}


def _delaunay(s):
    if "m" not in _MESH:
        _MESH["m"] = scenes.delaunay_beam((4, 4, 10))
    scenes.build_unstructured(s, _MESH["m"])
    scenes.perturb(s, 5, 0.02)


def _over_cap(s):
    lattice_with_w(s, CAP + 1)
    scenes.perturb(s, 6, 0.03)


few = lambda n: 0 < n <= 12  # noqa: E731  (a lattice: one set per element orientation)
CASES = {
    "headline_4x4x12": {"build": _beam((4, 4, 12)), "iterations": 20, "ticks": 3, "sets": few},
    "wpe4_3x3x600": {"build": _beam((3, 3, 600)), "iterations": 4, "ticks": 2, "sets": few},
    "tail_loop_24x24x4_block256": {"build": _beam((24, 24, 4)), "iterations": 3, "ticks": 2, "tuning": {"PIES_LAYER_BLOCK": "256"}, "sets": few},
    "materials": {"build": _materials, "iterations": 6, "ticks": 3, "sets": lambda n: 12 < n <= CAP},
    "delaunay_no_dictionary": {"build": _delaunay, "iterations": 5, "ticks": 3, "sets": lambda n: n == 0},
    "over_the_cap": {"build": _over_cap, "iterations": 4, "ticks": 2, "sets": lambda n: n == 0},
}
