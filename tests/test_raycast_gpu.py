"""GPU tests of pies_raycast.  The yardstick is the numpy fp32 restatement of the pair rule (tests/test_raycast.py: cast), run on
the positions read back from the device: triangle, t, u and v must be equal BIT FOR BIT - the rule uses only fp32 + - x / and
comparisons, which the device and numpy round alike.  Every kernel variant and every split of the triangles must give those same
bits as well (a minimum of keys does not depend on the order it is taken in)."""
import numpy as np
import pytest

import scenes
from test_node_renumber import shuffled_beam
from test_raycast import F, MISS, cast
from test_skin import T0, box_surface, lattice

pytestmark = pytest.mark.gpu

RAYS = (1, 63, 65, 257, 1025)  # lane tails of a wavefront and of a workgroup, more than one workgroup, narrow ray groups of 64
# (variant, chunks): None = automatic.  The triangle counts 255 / 257 / 600 are 1 / 2 / 3 tiles of the wide variant, so 1, 2 and
# 3 chunks cover one chunk per tile, several tiles per chunk and chunks without a tile.
VARIANTS = ((None, None), ("narrow", None), ("wide", 1), ("wide", 2), ("wide", 3))


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def rays_for(P, tris, count, seed):
    """Random rays around the scene: a third at random (many misses), a third aimed at triangle corners and edge midpoints
    (grazing: u, v or u + v at the rim, hit or miss by the last bit), a third at interior points"""
    rng = np.random.default_rng(seed)
    lo, hi = P.min(0) - 1.0, P.max(0) + 1.0
    o = rng.uniform(lo, hi, (count, 3)).astype(F)
    d = rng.normal(size=(count, 3)).astype(F)
    if len(tris):
        k = rng.integers(0, len(tris), count)
        corner = P[tris[k, rng.integers(0, 3, count)]]
        mid = (0.5 * (P[tris[k, 0]].astype(np.float64) + P[tris[k, 1]])).astype(F)
        w = rng.dirichlet([1.0, 1.0, 1.0], count)
        inner = (w[:, :1] * P[tris[k, 0]] + w[:, 1:2] * P[tris[k, 1]] + w[:, 2:] * P[tris[k, 2]]).astype(F)
        kind = np.arange(count) % 6
        for sel, target in ((kind == 1, corner), (kind == 2, mid), (kind >= 4, inner)):
            d[sel] = ((target[sel] - o[sel]) * rng.uniform(0.3, 2.0, (int(sel.sum()), 1)).astype(F)).astype(F)
    return o, d


def check(pies, tune, g, P, tris, count, seed, t_max=np.inf, cull_back=False, variants=VARIANTS, **kw):
    """Every variant against the restatement on positions P, and so against each other; returns the restatement's result"""
    o, d = rays_for(P, tris, count, seed)
    want = cast(o, d, P, tris, t_max, cull_back)
    for variant, chunks in variants:
        tune("PIES_RAY_VARIANT", variant)
        tune("PIES_RAY_CHUNKS", chunks)
        got = g.raycast(o, d, t_max=t_max, cull_back=cull_back, **kw)
        assert np.array_equal(got[0], want[0]), (variant, chunks, count, np.nonzero(got[0] != want[0])[0][:8])
        assert same_bits(got[1:], want[1:]), (variant, chunks, count)
    tune("PIES_RAY_VARIANT", None)
    tune("PIES_RAY_CHUNKS", None)
    return want


def soup(pies, n_triangles, seed=3):
    """n_triangles random triangles over loose nodes in a 4-cube (PBD, no constraints): every ray crosses many of them"""
    rng = np.random.default_rng(seed)
    n = max(3, min(200, 3 * n_triangles))
    g = pies.Solver(scenes.pbd_options(pies, 2))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(rng.uniform(0.5, 4.5, (n, 3)).astype(F), radius=0.05)
    tris = np.stack([rng.permutation(n)[:3] for _ in range(n_triangles)]).astype(np.uint32)
    g.add_triangles(tris)
    return g, tris


@pytest.mark.parametrize("n_triangles", [1, 48, 255, 257, 600])
def test_every_variant_gives_the_restatements_bits(pies, tune, n_triangles):
    if n_triangles == 48:  # createTetBox 3 x 3 x 3 with its surface triangles
        g = pies.Solver(pies.Options(solver=pies.PD))
        lattice(g)
    else:
        g, _ = soup(pies, n_triangles)
    tris = g.ids(pies.TRIANGLES)
    assert len(tris) == n_triangles
    P = g.positions
    hits = 0
    for count in RAYS:
        want = check(pies, tune, g, P, tris, count, seed=count)
        hits += int((want[0] != MISS).sum())
    misses = sum(RAYS) - hits
    print("%d triangles: %d hits, %d misses over %d rays" % (n_triangles, hits, misses, sum(RAYS)))
    assert hits > 0 and misses > 0
    # a finite t_max and back-face culling, all variants again
    t_max = 0.5 * float(np.median(want[1][np.isfinite(want[1])])) if np.isfinite(want[1]).any() else 1.0
    cut = check(pies, tune, g, P, tris, 257, seed=7, t_max=t_max)
    assert (cut[1][cut[0] != MISS] <= F(t_max)).all()
    check(pies, tune, g, P, tris, 257, seed=7, cull_back=True)
    # outputs are optional
    o, d = rays_for(P, tris, 65, 9)
    full = g.raycast(o, d)
    L, C = pies.load(), __import__("ctypes")
    only_t = np.empty(65, F)
    assert L.pies_raycast(g._h, 0, 0, 65, o.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.POINTER(C.c_float)), float("inf"), 0,
                          None, only_t.ctypes.data_as(C.POINTER(C.c_float)), None) == pies.OK
    assert same_bits([only_t], [full[1]])


def moving_run(pies, tune, kind):
    if kind == "pbd":
        g = pies.Solver(scenes.pbd_options(pies, 4))
        g.set_schedule(pies.SCHEDULE_LAYERED)
        g.create_tet_box(4, 4, 6, translation=(0.25, 1.5, 0.5), w=0.5)
    else:
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        g.create_tet_box(4, 4, 6, translation=(0.25, 1.5, 0.5), w=1.0)
    tris = g.ids(pies.TRIANGLES)
    scenes.perturb(g, 3, 0.05)
    g.set_prev_positions(g.positions)
    P0 = g.positions
    g.tick(3)
    assert not g.failed
    P = g.positions
    assert np.abs(P - P0).max() > 1e-3
    want = check(pies, tune, g, P, tris, 257, seed=11)
    assert (want[0] != MISS).any()
    return P, want


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_moving_state_and_reproducibility(pies, tune, kind):
    """3 ticks of the perturbed lattice (PBD under schedule LAYERED, PD): casts are the restatement on `positions`; a second fresh
    run gives the same bits."""
    a, b = moving_run(pies, tune, kind), moving_run(pies, tune, kind)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1][0], b[1][0]) and same_bits(a[1][1:], b[1][1:])


def test_renumbered_nodes_keep_host_triangle_indices(pies, tune):
    from test_node_renumber_gpu import beam, pd_options
    mesh = shuffled_beam()
    g = pies.Solver(pd_options(pies))
    g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    beam(g, mesh)
    g.tick(2)
    assert g.count(pies.NODES_RENUMBERED) == 1
    tris = g.ids(pies.TRIANGLES)  # host order, host ids
    want = check(pies, tune, g, g.positions, tris, 257, seed=13)
    assert (want[0] != MISS).sum() > 50


def test_skin_target(pies, tune):
    """Rays against a skin on the 3 x 3 x 3 lattice, at rest and with every node at A p + t (dyadic: the mapped nodes are exact);
    the yardstick runs on read_skin's positions, triangle indices are the skin's own."""
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    tets = lattice(g)
    lo, hi = F(T0) + 0.05, F(T0) + 1.95
    v0, tri0 = box_surface(lo + 0.5, hi - 0.5, 2)  # a first skin, so that the second one's triangles do not start at 0
    v, tri = box_surface(lo, hi, 5)                # 300 triangles: two tiles
    assert g.add_skin(v0, tets, tri0) == 0 and g.add_skin(v, tets, tri) == 1
    for skin, t in ((0, tri0), (1, tri)):
        x = g.read_skin(skin, normals=False)
        want = check(pies, tune, g, x, t, 257, seed=17 + skin, target=pies.RAY_SKIN, skin=skin)
        assert (want[0] != MISS).sum() > 50 and want[0][want[0] != MISS].max() < len(t)
    A = np.float64([[1.5, 0.25, 0.0], [0.0, 1.25, 0.5], [0.25, 0.0, 1.0]])
    P1 = g.positions.astype(np.float64) @ A.T + np.float64([0.5, 2.0, 0.25])
    assert np.array_equal(P1.astype(F).astype(np.float64), P1)
    g.set_positions(P1.astype(F))
    x1 = g.read_skin(1, normals=False)
    assert np.abs(x1 - x).max() > 0.1
    want = check(pies, tune, g, x1, tri, 257, seed=19, target=pies.RAY_SKIN, skin=1)
    assert (want[0] != MISS).sum() > 50
    # the scene target still sees the lattice's own 48 triangles
    check(pies, tune, g, g.positions, g.ids(pies.TRIANGLES), 65, seed=23)


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_a_cast_changes_nothing_else(pies, kind):
    """Ticks with a cast between them end in the same node state, bit for bit, and the same launch counts as ticks without"""
    runs = []
    for casting in (False, True):
        if kind == "pbd":
            g = pies.Solver(scenes.pbd_options(pies, 4))
            g.create_tet_box(4, 4, 6, translation=(0.25, 1.5, 0.5), w=0.5)
        else:
            g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
            g.create_tet_box(4, 4, 6, translation=(0.25, 1.5, 0.5), w=1.0)
        scenes.perturb(g, 8, 0.05)
        g.set_prev_positions(g.positions)
        g.finalize()
        counts = g.launch_counts()
        o, d = rays_for(g.positions, g.ids(pies.TRIANGLES), 257, 29)
        for _ in range(3):
            g.tick()
            launched = g.launch_counts()
            if casting:
                g.raycast(o, d)
                assert g.launch_counts() == launched
        runs.append(((counts, launched), g.positions.copy(), g.velocities.copy()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_a_cast_behind_tick_async_sees_that_tick(pies):
    def make():
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        g.create_tet_box(4, 4, 6, translation=(0.25, 1.5, 0.5), w=1.0)
        scenes.perturb(g, 5, 0.05)
        g.set_prev_positions(g.positions)
        return g
    g, twin = make(), make()
    tris = g.ids(pies.TRIANGLES)
    o, d = rays_for(g.positions, tris, 257, 31)
    g.tick_async()
    got = g.raycast(o, d)  # queued behind the tick, no synchronisation in between
    twin.tick()
    P = twin.positions
    assert np.array_equal(g.positions, P)
    want = cast(o, d, P, tris)
    assert np.array_equal(got[0], want[0]) and same_bits(got[1:], want[1:])
    assert (got[0] != MISS).any()


def test_empty_targets_give_all_misses(pies):
    g = pies.Solver(pies.Options(solver=pies.PD))
    g.create_tet_box(3, 3, 3, translation=T0, triangles=False)
    o, d = np.zeros((65, 3), F), np.ones((65, 3), F)
    for got in (g.raycast(o, d), g.raycast(o[:0], d[:0])):
        assert (got[0] == MISS).all() and np.isposinf(got[1]).all() and not got[2].any()
    assert g.add_skin(F([[1.0, 2.0, 1.0]]), g.ids(pies.TET)) == 0  # a skin without triangles
    got = g.raycast(o, d, target=pies.RAY_SKIN, skin=0)
    assert (got[0] == MISS).all() and np.isposinf(got[1]).all() and not got[2].any()
