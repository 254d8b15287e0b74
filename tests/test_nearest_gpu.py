"""GPU tests of pies_closest_points.  The yardstick of the distance pass is the numpy fp32 restatement of the pair rule
(tests/test_nearest.py: nearest), run on the positions read back from the device: triangle, distance, u, v and the closest point
must be equal BIT FOR BIT - the rule uses only fp32 + - x / sqrt and comparisons, which the device and numpy round alike.  Every
kernel variant and every split of the triangles must give those same bits as well (a minimum of keys does not depend on the order
it is taken in).  The winding number goes through atan2f, so it is held to numpy fp64 within test_trimesh.gate_of, and to itself
bit for bit from call to call."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_nearest import F, NONE, WINDING_GROW, box_points, nearest, winding32, winding64
from test_node_renumber import shuffled_beam
from test_raycast import turned_box
from test_raycast_gpu import same_bits, soup
from test_skin import T0, box_surface, lattice
from test_trimesh import gate_of

pytestmark = pytest.mark.gpu

POINTS = (1, 63, 65, 257, 1025)  # lane tails of a wavefront and of a workgroup, more than one workgroup, narrow groups of 64
# (variant, chunks): None = automatic.  The triangle counts 255 / 257 / 600 are 1 / 2 / 3 tiles of the wide variant, so 1, 2 and
# 3 chunks cover one chunk per tile, several tiles per chunk and chunks without a tile.
VARIANTS = ((None, None), ("narrow", None), ("wide", 1), ("wide", 2), ("wide", 3))


def points_for(P, tris, count, seed):
    """Query points around the scene, by index modulo 6: 0 and 5 uniform in the bounding box grown by 1 on every side, 1 exact
    copies of triangle corners (dd == 0, shared by every triangle at that corner), 2 fp32 midpoints of edges (ties at dd == 0 or
    at the last bit), 3 points on triangle interiors, 4 the point two places before it once more"""
    rng = np.random.default_rng(seed)
    lo, hi = P.min(0) - 1.0, P.max(0) + 1.0
    p = rng.uniform(lo, hi, (count, 3)).astype(F)
    if len(tris):
        k = rng.integers(0, len(tris), count)
        e = rng.integers(0, 3, count)
        corner = P[tris[k, e]]
        mid = (0.5 * (P[tris[k, e]].astype(np.float64) + P[tris[k, (e + 1) % 3]])).astype(F)
        w = rng.dirichlet([1.0, 1.0, 1.0], count)
        inner = (w[:, :1] * P[tris[k, 0]] + w[:, 1:2] * P[tris[k, 1]] + w[:, 2:] * P[tris[k, 2]]).astype(F)
        kind = np.arange(count) % 6
        for sel, source in ((kind == 1, corner), (kind == 2, mid), (kind == 3, inner)):
            p[sel] = source[sel]
        again = np.nonzero(kind == 4)[0]
        p[again] = p[again - 2]
    return p


def query(g, p, tune, variant, chunks, **kw):
    tune("PIES_NEAR_VARIANT", variant)
    tune("PIES_NEAR_CHUNKS", chunks)
    return g.closest_points(p, **kw)


def check(tune, g, P, tris, count, seed, max_distance=np.inf, variants=VARIANTS, **kw):
    """Every variant against the restatement on positions P, and so against each other; returns the points and the restatement's
    result (with the winner's region)"""
    p = points_for(P, tris, count, seed)
    want = nearest(p, P, tris, max_distance, with_region=True)
    for variant, chunks in variants:
        got = query(g, p, tune, variant, chunks, max_distance=max_distance, **kw)
        assert np.array_equal(got[0], want[0]), (variant, chunks, count, np.nonzero(got[0] != want[0])[0][:8])
        assert same_bits(got[1:], want[1:4]), (variant, chunks, count)
    tune("PIES_NEAR_VARIANT", None)
    tune("PIES_NEAR_CHUNKS", None)
    return p, want


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
    regions = set()
    for count in POINTS:
        p, want = check(tune, g, P, tris, count, seed=count)
        assert (want[0] != NONE).all()  # max_distance = +inf: every point has an answer
        regions |= set(want[4].tolist())
    print("%d triangles: winners' regions %s" % (n_triangles, sorted(regions)))
    assert regions == set(range(7))
    # a finite max_distance (half the median distance of the uniform points: found and not found both occur among them) and 0,
    # all variants again
    uniform = np.isin(np.arange(POINTS[-1]) % 6, (0, 5))
    cut = 0.5 * float(np.median(want[1][uniform]))
    assert cut > 0.01
    p, near = check(tune, g, P, tris, 257, seed=7, max_distance=cut)
    found = near[0] != NONE
    assert found[uniform[:257]].any() and (~found[uniform[:257]]).any()
    assert (near[1][found] <= F(cut) * F(1 + 2.0 ** -22)).all() and np.array_equal(near[3][~found], p[~found])
    p, zero = check(tune, g, P, tris, 257, seed=7, max_distance=0.0)
    found = zero[0] != NONE
    assert found.any() and (~found).any() and not zero[1][found].any()
    # outputs are optional: one call with out_distance alone
    p = points_for(P, tris, 65, 9)
    full = g.closest_points(p)
    only = np.empty(65, F)
    fp = C.POINTER(C.c_float)
    assert pies.load().pies_closest_points(g._h, 0, 0, 65, p.ctypes.data_as(fp), float("inf"), None, only.ctypes.data_as(fp), None, None,
                                           None) == pies.OK
    assert same_bits([only], [full[1]])


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
    _, want = check(tune, g, P, tris, 257, seed=11)
    return P, want


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_moving_state_and_reproducibility(pies, tune, kind):
    """3 ticks of the perturbed lattice (PBD under schedule LAYERED, PD): the answers are the restatement on `positions`; a second
    fresh run gives the same bits."""
    a, b = moving_run(pies, tune, kind), moving_run(pies, tune, kind)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1][0], b[1][0]) and same_bits(a[1][1:4], b[1][1:4])


def test_renumbered_nodes_keep_host_triangle_indices(pies, tune):
    from test_node_renumber_gpu import beam, pd_options
    mesh = shuffled_beam()
    g = pies.Solver(pd_options(pies))
    g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    beam(g, mesh)
    g.tick(2)
    assert g.count(pies.NODES_RENUMBERED) == 1
    tris = g.ids(pies.TRIANGLES)  # host order, host ids
    _, want = check(tune, g, g.positions, tris, 257, seed=13)
    assert len(set(want[0].tolist())) > 50


def test_skin_target(pies, tune):
    """Queries against a skin on the 3 x 3 x 3 lattice, at rest and with every node at A p + t (dyadic: the mapped nodes are
    exact); the yardstick runs on read_skin's positions, triangle indices are the skin's own."""
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    tets = lattice(g)
    lo, hi = F(T0) + 0.05, F(T0) + 1.95
    v0, tri0 = box_surface(lo + 0.5, hi - 0.5, 2)  # a first skin, so that the second one's triangles do not start at 0
    v, tri = box_surface(lo, hi, 5)                # 300 triangles: two tiles
    assert g.add_skin(v0, tets, tri0) == 0 and g.add_skin(v, tets, tri) == 1
    for skin, t in ((0, tri0), (1, tri)):
        x = g.read_skin(skin, normals=False)
        _, want = check(tune, g, x, t, 257, seed=17 + skin, target=pies.RAY_SKIN, skin=skin)
        assert want[0].max() < len(t) and len(set(want[0].tolist())) > 20
    A = np.float64([[1.5, 0.25, 0.0], [0.0, 1.25, 0.5], [0.25, 0.0, 1.0]])
    P1 = g.positions.astype(np.float64) @ A.T + np.float64([0.5, 2.0, 0.25])
    assert np.array_equal(P1.astype(F).astype(np.float64), P1)
    g.set_positions(P1.astype(F))
    x1 = g.read_skin(1, normals=False)
    assert np.abs(x1 - x).max() > 0.1
    check(tune, g, x1, tri, 257, seed=19, target=pies.RAY_SKIN, skin=1)
    # the scene target still sees the lattice's own 48 triangles
    check(tune, g, g.positions, g.ids(pies.TRIANGLES), 65, seed=23)


def winding_target(pies, name):
    """(handle, keyword arguments of the target, positions, triangles, query points) of the three closed targets"""
    if name == "lattice":  # the 48 surface triangles of the 3 x 3 x 3 lattice after 3 PD ticks
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        lattice(g)
        scenes.perturb(g, 3, 0.05)
        g.set_prev_positions(g.positions)
        g.tick(3)
        P, tris, kw = g.positions, g.ids(pies.TRIANGLES), {}
    elif name == "skin":  # the 300-triangle box skin, behind a first one
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        tets = lattice(g)
        lo, hi = F(T0) + 0.05, F(T0) + 1.95
        v0, tri0 = box_surface(lo + 0.5, hi - 0.5, 2)
        v, tris = box_surface(lo, hi, 5)
        assert g.add_skin(v0, tets, tri0) == 0 and g.add_skin(v, tets, tris) == 1
        P, kw = g.read_skin(1, normals=False), dict(target=pies.RAY_SKIN, skin=1)
    else:  # the turned box as loose nodes + triangles: 432 triangles, two tiles
        P0, tris = turned_box()
        g = pies.Solver(scenes.pbd_options(pies, 2))
        g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
        g.add_nodes_raw(P0, radius=0.05)
        g.add_triangles(tris)
        P, kw = g.positions, {}
        assert np.array_equal(P, P0)
    return g, kw, P, np.asarray(tris, np.int64), box_points(P, 600, seed=41, grow=WINDING_GROW)


@pytest.mark.parametrize("name", ["lattice", "skin", "turned box"])
def test_winding_on_closed_targets(pies, tune, name):
    g, kw, P, tris, p = winding_target(pies, name)
    w64 = winding64(p, P, tris)
    gate, err = gate_of(winding32(p, P, tris), w64, len(tris))
    first = None
    for variant, chunks in VARIANTS + ((None, None),):  # two calls alike, and every variant of the distance pass
        got = query(g, p, tune, variant, chunks, winding=True, **kw)
        assert got[4].dtype == np.float32
        if first is None:
            first = got
        assert np.array_equal(got[0], first[0]) and same_bits(got[1:], first[1:]), (variant, chunks)
    w = first[4]
    worst = float(np.abs(w.astype(np.float64) - w64).max())
    print("%s, %d triangles: device winding vs fp64 %.3g (restatement %.3g, gate %.3g)" % (name, len(tris), worst, err, gate))
    assert worst <= gate
    # the winding number alone: the same bits without a distance pass
    only = np.empty(len(p), F)
    fp = C.POINTER(C.c_float)
    assert pies.load().pies_closest_points(g._h, kw.get("target", 0), kw.get("skin", 0), len(p), p.ctypes.data_as(fp), float("inf"), None,
                                           None, None, None, only.ctypes.data_as(fp)) == pies.OK
    assert same_bits([only], [w])
    # inside and outside
    clear = np.abs(np.abs(w64) - 0.5) >= 0.05
    inside64 = np.abs(w64) > 0.5
    assert (~clear).mean() <= 0.02
    assert inside64.mean() >= 0.1 and (~inside64).mean() >= 0.1
    assert np.array_equal((np.abs(w) > F(0.5))[clear], inside64[clear])
    # the distance outputs of the same call are the restatement's
    want = nearest(p, P, tris)
    assert np.array_equal(first[0], want[0]) and same_bits(first[1:4], want[1:])


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_a_query_changes_nothing_else(pies, kind):
    """Ticks with a query between them end in the same node state, bit for bit, and the same launch counts as ticks without"""
    runs = []
    for asking in (False, True):
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
        p = points_for(g.positions, g.ids(pies.TRIANGLES), 257, 29)
        for _ in range(3):
            g.tick()
            launched = g.launch_counts()
            if asking:
                g.closest_points(p, winding=True)
                assert g.launch_counts() == launched
        runs.append(((counts, launched), g.positions.copy(), g.velocities.copy()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_a_query_behind_tick_async_sees_that_tick(pies):
    def make():
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        g.create_tet_box(4, 4, 6, translation=(0.25, 1.5, 0.5), w=1.0)
        scenes.perturb(g, 5, 0.05)
        g.set_prev_positions(g.positions)
        return g
    g, twin = make(), make()
    tris = g.ids(pies.TRIANGLES)
    p = points_for(g.positions, tris, 257, 31)
    before = nearest(p, g.positions, tris)
    g.tick_async()
    got = g.closest_points(p)  # queued behind the tick, no synchronisation in between
    twin.tick()
    P = twin.positions
    assert np.array_equal(g.positions, P)
    want = nearest(p, P, tris)
    assert np.array_equal(got[0], want[0]) and same_bits(got[1:], want[1:])
    assert not same_bits(want[1:2], before[1:2])  # the tick moved the surface


def test_empty_targets_give_no_candidates(pies):
    g = pies.Solver(pies.Options(solver=pies.PD))
    g.create_tet_box(3, 3, 3, translation=T0, triangles=False)
    p = np.random.default_rng(1).uniform(0, 3, (65, 3)).astype(F)
    for q in (p, p[:0]):
        got = g.closest_points(q, winding=True)
        assert (got[0] == NONE).all() and np.isposinf(got[1]).all() and not got[2].any() and np.array_equal(got[3], q) and not got[4].any()
        assert len(got[0]) == len(q)
    assert g.add_skin(F([[1.0, 2.0, 1.0]]), g.ids(pies.TET)) == 0  # a skin without triangles
    got = g.closest_points(p, target=pies.RAY_SKIN, skin=0, winding=True)
    assert (got[0] == NONE).all() and np.isposinf(got[1]).all() and not got[2].any() and np.array_equal(got[3], p) and not got[4].any()
