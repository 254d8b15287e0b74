"""GPU tests of the node renumbering of PD scenes (PIES_FLAG_RENUMBER_NODES): a shuffled unstructured mesh is solved in the
library's own numbering, and everything the host reads or writes stays in the host's.

The gate is the yardstick of tests/test_pd_parity_gpu.py, restated here: the device is no further from the oracle's fp64 solve
than max(2 x |oracle32 - fp64|, 1e-4 x spacing) (velocities: that / dt).  Runs with the flag on and off are held against
each other with the PD tolerance of that file (1e-5 x the bounding-box diagonal)."""
import numpy as np
import pytest

import scenes
from test_node_renumber import shuffled, shuffled_beam

pytestmark = pytest.mark.gpu
DT = 0.012


def pd_options(mod, iterations=10, **kw):
    return mod.Options(solver=mod.PD, iterations=iterations, **kw)


def tol_for(p):
    return 1e-5 * float(np.linalg.norm(p.max(0) - p.min(0))) + 2e-5


def yardstick(g, o32, o64, names=("positions", "velocities"), spacing=1.0):
    for name in names:
        a, b, c = getattr(g, name), getattr(o32, name), getattr(o64, name)
        assert np.isfinite(a).all(), name
        d_dev, d_ref = float(np.abs(a - c).max()), float(np.abs(b - c).max())
        gate = max(2.0 * d_ref, 1e-4 * spacing / (DT if name == "velocities" else 1.0))
        assert d_dev <= gate, (name, "device vs fp64 %.3g, oracle32 vs fp64 %.3g, gate %.3g" % (d_dev, d_ref, gate))


def oracles(oracle, **kw):
    o32, o64 = oracle.OracleSolver(pd_options(oracle, **kw)), oracle.OracleSolver(pd_options(oracle, **kw))
    o64.set_flag(oracle.FLAG_PD_SOLVE_FP64, 1)
    return o32, o64


def renumbered(pies, **kw):
    g = pies.Solver(pd_options(pies, **kw))
    g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    return g


def beam(s, mesh):
    scenes.build_unstructured_pd(s, mesh)
    scenes.perturb(s, 21, 0.02)
    s.set_prev_positions(s.positions)


def test_shuffled_beam_against_oracle(pies, oracle):
    """The shuffled Delaunay beam (strain + volume per element, surface triangles, the end cap pinned), flag on: host-order state
    after 1 and 3 ticks within the yardstick of the oracle built in host order."""
    mesh = shuffled_beam()
    g = renumbered(pies)
    o32, o64 = oracles(oracle)
    for s in (g, o32, o64):
        beam(s, mesh)
    g.finalize()
    assert g.count(pies.NODES_RENUMBERED) == 1 and g.count(pies.PD_TILES) > 0
    for ticks in (1, 2):
        for s in (g, o32, o64):
            s.tick(ticks)
        yardstick(g, o32, o64)
    assert g.pcg_health()["short_solves"] == 0 and not g.failed


def contact_scene(seed=3):
    """Two shuffled unstructured boxes, one resting just above the floor, the other falling onto it: point-triangle contacts in the
    first substep.  Returns (positions, velocities, tets, triangles) with the node ids of both bodies shuffled together."""
    pos, tets, _ = scenes.delaunay_beam((7, 6, 8), seed=seed)
    pos = pos - [0.0, pos[:, 1].min() - 0.02, 0.0]
    top = pos + np.float32([0.4, pos[:, 1].max() - pos[:, 1].min() + 0.06, 0.3])
    n = len(pos)
    p = np.concatenate([pos, top]).astype(np.float32)
    t = np.concatenate([tets, tets + n]).astype(np.uint32)
    v = np.zeros_like(p)
    v[n:, 1] = -2.0
    edges = np.zeros((0, 2), np.uint32)
    p2, t2, _ = shuffled((p, t, edges), seed=seed)
    perm = np.random.default_rng(seed).permutation(len(p))  # the same permutation shuffled() applied
    return p2, v[perm], t2, scenes.boundary_triangles(p2, t2)


def build_contact(s, scene):
    p, v, t, tri = scene
    s.add_nodes_raw(p, vel=v, radius=0.5)
    s.add_tet(t, 1.0)
    s.add_volume(t, 1.0)
    s.add_triangles(tri)
    s.set_prev_positions(s.positions)


def test_contacts_and_positions_agree_with_the_flag_off(pies):
    scene = contact_scene()
    on, off = renumbered(pies, iterations=6), pies.Solver(pd_options(pies, 6))
    for s in (on, off):
        build_contact(s, scene)
    on.tick()
    off.tick()
    assert on.count(pies.NODES_RENUMBERED) == 1 and off.count(pies.NODES_RENUMBERED) == 0
    a, b = on.tri_collisions, off.tri_collisions
    assert len(b) > 0
    key = lambda c: sorted(map(tuple, c.tolist()))  # noqa: E731
    assert key(a) == key(b)  # the same contacts in host ids, as multisets (the list's order may differ)
    on.tick(2)
    off.tick(2)
    tol = tol_for(off.positions)
    assert np.abs(on.positions - off.positions).max() <= tol
    assert np.abs(on.velocities - off.velocities).max() <= tol / DT


def test_every_read_path_is_in_host_order(pies):
    mesh = shuffled_beam()
    g = renumbered(pies)
    beam(g, mesh)
    g.tick(2)
    assert g.count(pies.NODES_RENUMBERED) == 1
    p = g.positions
    assert np.array_equal(g.read_positions_strided(5)[:, :3], p)
    f = g.tick_begin()
    x = np.array(g.export_acquire(f))
    g.export_release(f)
    q = g.positions  # the same tick, read through pies_read_nodes
    assert np.array_equal(np.asarray(x)[:, :3], q)
    assert np.array_equal(g.read_positions_strided(3), q)
    # and host order it is: the same ticks with the flag off end there too
    off = pies.Solver(pd_options(pies))
    beam(off, mesh)
    off.tick(3)
    assert np.abs(q - off.positions).max() <= tol_for(off.positions)


def test_write_nodes_after_finalize(pies):
    mesh = shuffled_beam()
    on, off = renumbered(pies), pies.Solver(pd_options(pies))
    for s in (on, off):
        beam(s, mesh)
        s.tick()
    subset = np.arange(0, len(mesh[0]), 7)
    for s in (on, off):
        v = s.velocities
        v[subset] += np.float32([0.5, 1.0, -0.25])
        s.set_velocities(v)
        s.tick(2)
    assert on.count(pies.NODES_RENUMBERED) == 1
    tol = tol_for(off.positions)
    assert np.abs(on.positions - off.positions).max() <= tol
    assert np.abs(on.velocities - off.velocities).max() <= tol / DT


def test_second_body_keeps_the_first_bodys_state(pies):
    mesh = shuffled_beam()
    on, off = renumbered(pies), pies.Solver(pd_options(pies))
    for s in (on, off):
        beam(s, mesh)
        s.tick(2)
    before = on.positions.copy(), on.velocities.copy()
    second = shuffled(scenes.delaunay_beam((4, 4, 12), seed=9), seed=4)
    for s in (on, off):
        s.add_nodes_raw(second[0] + np.float32([12.0, 0.0, 0.0]), radius=0.5)
        n0 = len(mesh[0])
        s.add_tet(second[1] + n0, 1.0)
        s.add_volume(second[1] + n0, 1.0)
    n0 = len(mesh[0])
    assert np.array_equal(on.positions[:n0], before[0]) and np.array_equal(on.velocities[:n0], before[1])
    on.finalize()
    assert on.count(pies.NODES_RENUMBERED) == 1 and len(on.node_order()) == n0 + len(second[0])
    assert np.array_equal(on.positions[:n0], before[0]) and np.array_equal(on.velocities[:n0], before[1])
    for s in (on, off):
        s.tick(2)
    tol = tol_for(off.positions)
    assert np.abs(on.positions - off.positions).max() <= tol


def _region(center, half):
    m = np.zeros((4, 4), np.float32)  # column-major: m[col][row]
    m[0, 0], m[1, 1], m[2, 2], m[3, 3] = half[0], half[1], half[2], 1.0
    m[3, :3] = center
    return m.reshape(16)


def test_every_container_is_translated(pies, oracle):
    """A small shuffled scene with shape matching, a fixed region (goal), a linked region (shape), node-pair constraints, distance
    and position constraints besides the elements, flag on, against the oracle in host order."""
    pos, tets, edges = shuffled(scenes.delaunay_beam((4, 5, 14), seed=7), seed=2)
    lo, hi = pos.min(0), pos.max(0)
    mid = 0.5 * (lo + hi)
    fixed = _region((mid[0], mid[1], lo[2]), (3.0, 3.0, 1.2))
    linked = _region((mid[0], mid[1], hi[2]), (3.0, 3.0, 2.5))
    pairs = np.stack([np.arange(0, 40, 2), np.arange(1, 41, 2)], 1).astype(np.uint32)
    g = renumbered(pies, iterations=6)
    o32, o64 = oracles(oracle, iterations=6)
    for s in (g, o32, o64):
        s.add_nodes_raw(pos, radius=0.5)
        s.add_tet(tets, 1.0)
        s.add_volume(tets, 1.0)
        s.add_distance(edges[:200], 0.5)
        s.add_triangles(scenes.boundary_triangles(pos, tets))
        s.add_shape(np.nonzero(np.abs(pos[:, 2] - mid[2]) < 2.0)[0].astype(np.uint32)[::-1].copy(), 5.0)
        s.add_fixed_regions(fixed, 50.0)
        s.add_linked_regions(linked, 10.0)
        s.add_node_pairs(pairs)
        s.add_position(np.uint32([5, 17]), 2.0)
        scenes.perturb(s, 5, 0.02)
        s.set_prev_positions(s.positions)
    assert g.count(pies.GOAL) == 1 and g.count(pies.SHAPE) == 2 and g.count(pies.NODE_PAIRS) == len(pairs)
    for k in range(2):
        assert np.array_equal(g.group_ids(pies.SHAPE, k), o32.group_ids(oracle.SHAPE, k))
    assert np.array_equal(g.group_ids(pies.GOAL, 0), o32.group_ids(oracle.GOAL, 0))
    g.set_pcg(3e-7, 256)
    for s in (g, o32, o64):
        s.tick(2)
    assert g.count(pies.NODES_RENUMBERED) == 1
    yardstick(g, o32, o64)
    moved = _region((mid[0] + 0.3, mid[1] + 0.2, lo[2] + 0.1), (3.0, 3.0, 1.2))
    for s in (g, o32, o64):
        s.update_fixed_regions(moved)
        s.tick(2)
    yardstick(g, o32, o64)
    assert not g.failed
