"""The distance projection of k_layer with its three quotients from one reciprocal and its square root without range scaling
(distance_quotient.h, round 14).

Every scene runs schedule LAYERED for 2 ticks and must equal, byte for byte, the oracle replaying the exported order and the same
build with the distance projection dividing three times (PIES_LAYER_DIST_FORM=0); the inverse masses (.w of the node records,
distinct per node) must come back as they went in.

  lattice_3x3x4, tet_box_3x3x4   a createBox lattice (distance constraints only; unperturbed, so axis-aligned pairs with two zero
                                 numerators) and a createTetBox body, perturbed
  class_1 .. class_65            N fans of 2 distance constraints that share their moving node: 2 colour classes of N constraints
                                 (1, 63, 64 and 65: the wavefront's edge) against the 256-thread workgroup
  range                          fans whose pairs sit on and beside the range test: coincident nodes, an axis-aligned pair, a pair
                                 of which one component is -0, coordinates of magnitude 1e-20 and 1e18, numerators of 1e-20 and just
                                 below 2^-32 beside ordinary ones, pairs at a distance of 1e-5 less / more a few units in the last place

(The two other parts of the round - 12-byte scatters, the tile descriptor in the launch's arguments - measured under the bar and
are not in the build: DESIGN.md section 4.)"""
import numpy as np
import pytest

import scenes

STATE = ("positions", "prev_positions", "velocities")
CLASS_SIZES = (1, 63, 64, 65)


def _inv_masses(n):
    return (0.25 + np.arange(n, dtype=np.float32) / 64.0).astype(np.float32)


def _lattice(s):
    scenes.build_beam(s, (3, 3, 4), tets=False)


def _tet_box(s):
    scenes.build_beam(s, (3, 3, 4), distance=False)
    scenes.perturb(s, 5, 0.05)


def _fans(moving, partners, rest=1.0):
    """moving: F x 3, partners: F x K x 3.  Constraint (fan f, k) moves node f towards / away from its k-th partner: the K constraints
    of a fan conflict, those of different fans do not - K colour classes of F constraints."""
    moving, partners = np.float32(moving), np.float32(partners)
    f, k = partners.shape[:2]

    def build(s):
        s.add_nodes_raw(np.concatenate([moving, partners.reshape(-1, 3)]), radius=0.01)
        ids = np.uint32([[i, f + i * k + j] for i in range(f) for j in range(k)])
        s.add_distance(ids, 0.5)
        s.set_rest(1, np.full(len(ids), rest, np.float32))  # DISTANCE
    return build


def _class_scene(n):
    rng = np.random.default_rng(100 + n)
    moving = np.zeros((n, 3))
    moving[:, 1:] = rng.uniform(-0.5, 0.5, (n, 2))  # the moving nodes at x = 0, where the levelling starts; x is the longest axis: one tile
    partners = moving[:, None, :] + rng.uniform(0.3, 1.0, (n, 2, 3)) * [5.0, 1.0, -1.0]
    partners[0, 0, 0] = 5.0  # (the longest constraint spans the scene: no slabs by position)
    return _fans(moving, partners)


def _range_scene():
    tiny, below = 1.0e-20, float(np.nextafter(np.float32(2.0 ** -32), np.float32(0.0)))
    e = float(np.float32(1.0e-5))
    d_lo, d_hi = float(np.nextafter(np.float32(e), np.float32(0.0))), float(np.nextafter(np.float32(e), np.float32(1.0)))
    pairs = [  # the two partners of a fan, relative to its moving node
        ((0.0, 0.0, 0.0), (0.7, 0.0, 0.0)),           # coincident nodes; an axis-aligned pair (two zero numerators)
        ((0.0, 0.9, 0.0), (0.0, 0.0, -1.1)),          # axis-aligned along y and z
        ((tiny, 0.0, 0.0), (tiny, tiny, tiny)),       # coordinates of magnitude 1e-20: dist below the threshold
        ((tiny, 0.8, 0.0), (0.6, -tiny, 0.3)),        # a numerator of 1e-20 beside ordinary ones: the fallback divides
        ((below, 0.5, 0.0), (0.5, 2.0 ** -32, 0.25)),  # a numerator just below 2^-32, and one at it
        ((1.0e18, 0.0, 1.0e18), (1.0e18, 0.0, 0.0)),  # coordinates of magnitude 1e18: dist beyond 2^32
        ((e, 0.0, 0.0), (d_hi, 0.0, 0.0)),            # dist at the 1e-5 threshold, and one unit in the last place above it
        ((d_lo, 0.0, 0.0), (0.0, 0.0, 2.0 * e)),      # one unit below it; twice the threshold
        ((6.0e-6, 6.0e-6, 6.0e-6), (5.0e-6, 5.0e-6, 5.0e-6)),  # components below the threshold, dist above / below it
        ((0.3, 0.4, 1.2), (-0.2, 0.5, 0.1)),          # ordinary
    ]
    f = len(pairs)
    moving = np.zeros((f, 3), np.float32)
    moving[:, 1] = 4.0 * np.arange(f)
    partners = moving[:, None, :] + np.float32(pairs)
    # a partner at z = -0 against a moving node at z = +0: a -0 numerator (and +0 in y), which the chain must hand on as -0
    moving = np.concatenate([moving, np.float32([[0.0, 4.0 * f, 0.0]])])
    partners = np.concatenate([partners, np.float32([[[0.5, 4.0 * f, -0.0], [0.25, 4.0 * f, 0.0]]])])
    return _fans(moving, partners, rest=0.75)


SCENES = {"lattice_3x3x4": (_lattice, {}), "tet_box_3x3x4": (_tet_box, {}), "range": (_range_scene(), dict(gravity=0.0, floorHeight=-1.0e6))}
for _n in CLASS_SIZES:
    SCENES["class_%d" % _n] = (_class_scene(_n), dict(gravity=0.0, floorHeight=-1.0e6))


def _run(pies, build, options, oracle=None, device=0, ticks=2):
    g = pies.Solver(scenes.pbd_options(pies, 3, **options), device=device)
    build(g)
    n = g.count(pies.NODES)
    g.set_inv_masses(_inv_masses(n))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    g.finalize()
    if device != 0:
        return g, None
    assert g.launch_counts()["layer"] > 0  # schedule LAYERED is what runs
    o = None
    if oracle is not None:
        o = oracle.OracleSolver(scenes.pbd_options(oracle, 3, **options))
        build(o)
        o.set_inv_masses(_inv_masses(n))
        o.set_flag(oracle.FLAG_NODE_COLLISIONS, 0)
        for t in (pies.POSITION, pies.DISTANCE, pies.TET, pies.BEND):
            if g.count(t):
                o.permute(t, g.order(t))
        o.tick(ticks)
    g.tick(ticks)
    out = {k: getattr(g, k) for k in STATE}
    out["inv_masses"] = g.inv_masses
    out["tiles"], out["class"] = g.count(pies.LAYER_MAX_TILES), g.count(pies.LAYER_MAX_CLASS)
    g.close()
    return out, o


def _same(a, b, what):
    assert np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_oracle_and_three_divisions(pies, oracle, tune, name):
    build, options = SCENES[name]
    new, o = _run(pies, build, options, oracle)
    assert new["tiles"] <= 256 and new["class"] <= 256  # the 256-thread instantiation that has both forms of the distance projection
    if name.startswith("class_"):
        assert new["class"] == int(name[6:]), new["class"]
    tune("PIES_LAYER_DIST_FORM", "0")
    old, _ = _run(pies, build, options)
    for k in STATE:
        _same(new[k], old[k], k + ": three quotients from one reciprocal against three divisions")
        _same(new[k], getattr(o, k), k + ": against the oracle")
    if name != "range":  # (its 1e18 coordinates stay finite as well, but that is not what it is about)
        assert all(np.isfinite(new[k]).all() for k in STATE)
    _same(new["inv_masses"], _inv_masses(len(new["inv_masses"])), ".w of the node records")
    _same(old["inv_masses"], _inv_masses(len(old["inv_masses"])), ".w of the node records, three divisions")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_plans(pies, name):
    """(host only) the scenes are what the GPU tests take them for: one launch's tiles and the largest colour class"""
    build, options = SCENES[name]
    g, _ = _run(pies, build, options, device=pies.DEVICE_NONE)
    tiles, cls = g.count(pies.LAYER_MAX_TILES), g.count(pies.LAYER_MAX_CLASS)
    g.close()
    assert 0 < tiles <= 256 and 0 < cls <= 256, (tiles, cls)
    if name.startswith("class_"):
        assert cls == int(name[6:]), cls
