"""CPU tests of the node renumbering of PD scenes (PIES_FLAG_RENUMBER_NODES) through host-only handles (PIES_DEVICE_NONE): the
decision pies_finalize makes, the permutation it reports, and the host's view of the scene, which must not change."""
import numpy as np

import scenes
from pies_amd import capi


def shuffled(mesh, seed=11):
    """The mesh with its node ids shuffled by a seeded permutation: new id k is old node perm[k]."""
    pos, tets, edges = mesh
    perm = np.random.default_rng(seed).permutation(len(pos))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return pos[perm], inv[tets].astype(np.uint32), np.sort(inv[edges], axis=1).astype(np.uint32)


def shuffled_beam(dims=(7, 6, 40), seed=11):
    return shuffled(scenes.delaunay_beam(dims), seed)


def halo_per_row(tets, n, order=None, rows=256):
    """Halo columns per row of the PD system matrix over chunks of `rows` rows (what PIES_PD_WINDOW_HALO counts), from the
    tetrahedra alone; order[internal] = host id (None: the host numbering)."""
    inv = np.arange(n) if order is None else np.argsort(order)
    t = inv[np.asarray(tets, dtype=np.int64)]
    r, c = np.repeat(t, 4, axis=1).ravel(), np.tile(t, (1, 4)).ravel()
    out = (c // rows) != (r // rows)
    return len(np.unique((r[out] // rows) * (n + 1) + c[out])) / n


def pd_handle(mesh, renumber, shape_goal=False, solver=capi.PD):
    g = capi.Solver(capi.Options(solver=solver, iterations=10), device=capi.DEVICE_NONE)
    scenes.build_unstructured_pd(g, mesh)
    if shape_goal:
        g.add_shape(np.arange(100, 160, dtype=np.uint32)[::-1].copy(), 3.0)
        g.add_goal(np.arange(300, 340, dtype=np.uint32), 20.0)
    g.set_flag(capi.FLAG_RENUMBER_NODES, 1 if renumber else 0)
    g.finalize()
    return g


def test_shuffled_pd_beam_is_renumbered():
    mesh = shuffled_beam()
    n = len(mesh[0])
    g = pd_handle(mesh, True)
    assert g.count(capi.NODES_RENUMBERED) == 1
    order = g.node_order()
    assert order.dtype == np.uint32 and len(order) == n
    assert np.array_equal(np.sort(order), np.arange(n))
    assert not np.array_equal(order, np.arange(n))
    # deterministic: the same scene built again gives the same permutation
    assert np.array_equal(pd_handle(mesh, True).node_order(), order)
    # the internal order has at most half the halo of the shuffled host order
    host, internal = halo_per_row(mesh[1], n), halo_per_row(mesh[1], n, order)
    assert internal <= 0.5 * host, (internal, host)


def test_host_view_does_not_change():
    mesh = shuffled_beam()
    off, on = pd_handle(mesh, False, shape_goal=True), pd_handle(mesh, True, shape_goal=True)
    assert on.count(capi.NODES_RENUMBERED) == 1 and off.count(capi.NODES_RENUMBERED) == 0
    for t in (capi.POSITION, capi.TET, capi.VOLUME, capi.TRIANGLES):
        assert np.array_equal(on.ids(t), off.ids(t)), t
    for t in (capi.POSITION, capi.TET):  # (constraint indices: the numbering of the nodes does not enter)
        assert np.array_equal(on.order(t), off.order(t)), t
    for t in (capi.TET, capi.VOLUME):
        assert np.array_equal(on.rest(t), off.rest(t)), t
    for t in (capi.SHAPE, capi.GOAL):
        assert np.array_equal(on.group_ids(t, 0), off.group_ids(t, 0)), t
    for name in ("positions", "prev_positions", "velocities", "radii", "inv_masses"):
        assert np.array_equal(getattr(on, name), getattr(off, name)), name


def test_tile_plan_names_host_ids():
    """pies_get_pd_tile_plan of a renumbered scene: the plan the device runs, its node array mapped back to host ids - every
    element of a tile has its four (host) nodes among the tile's nodes."""
    mesh = shuffled_beam()
    g = pd_handle(mesh, True)
    assert g.count(capi.NODES_RENUMBERED) == 1
    plan = g.pd_tile_plan()
    tets = g.ids(capi.TET)
    assert plan is not None
    for t in range(len(plan["info"])):
        nn, ne = plan["info"][t] & 0xFFFF, plan["info"][t] >> 16
        nodes = set(plan["node"][t, :nn].tolist())
        for e in plan["elem"][t, :ne]:
            assert set(tets[e].tolist()) <= nodes, (t, e)


def test_identity_is_kept():
    mesh = shuffled_beam()
    n = len(mesh[0])
    # flag off
    g = pd_handle(mesh, False)
    assert g.count(capi.NODES_RENUMBERED) == 0 and np.array_equal(g.node_order(), np.arange(n))
    # flag on under PBD: accepted, identity
    g = pd_handle(mesh, True, solver=capi.PBD)
    assert g.count(capi.NODES_RENUMBERED) == 0 and np.array_equal(g.node_order(), np.arange(n))
    # flag on, a createTetBox PD lattice: its order is the row dictionary's
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=capi.DEVICE_NONE)
    g.create_tet_box(6, 5, 20, translation=(0.0, 0.02, 0.0), w=1.0, volume=True, triangles=True)
    g.set_flag(capi.FLAG_RENUMBER_NODES, 1)
    g.finalize()
    assert g.count(capi.NODES_RENUMBERED) == 0 and np.array_equal(g.node_order(), np.arange(g.count(capi.NODES)))


def test_refinalize_recomputes_or_drops_the_order():
    mesh = shuffled_beam()
    g = pd_handle(mesh, True)
    first = g.node_order()
    assert g.count(capi.NODES_RENUMBERED) == 1
    g.set_solver(capi.PBD)
    g.finalize()
    assert g.count(capi.NODES_RENUMBERED) == 0
    g.set_solver(capi.PD)
    g.finalize()
    assert g.count(capi.NODES_RENUMBERED) == 1 and np.array_equal(g.node_order(), first)
    # a second body: the new order covers every node
    g.add_nodes_raw(mesh[0] + np.float32([20.0, 0.0, 0.0]), radius=0.5)
    g.add_tet(mesh[1] + len(mesh[0]), 1.0)
    g.finalize()
    order = g.node_order()
    assert g.count(capi.NODES_RENUMBERED) == 1 and np.array_equal(np.sort(order), np.arange(2 * len(mesh[0])))
    g.set_flag(capi.FLAG_RENUMBER_NODES, 0)
    g.finalize()
    assert g.count(capi.NODES_RENUMBERED) == 0
    g.clear()
    assert g.count(capi.NODES_RENUMBERED) == 0 and len(g.node_order()) == 0
