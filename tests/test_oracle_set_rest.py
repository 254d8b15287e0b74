"""CPU pin of the oracle's set_rest (ora_set_rest, the counterpart of pies_set_rest): the live-edit GPU tests hand the oracle the
rest data the device was given, so the call must (i) change nothing when it writes back what is there, and (ii) carry everything
a factory derives from the rest pose - a scene built on another lattice and given the first one's rest data and node state is the
first scene, bit for bit, under PBD and under PD (whose system matrix is built from A^T A of the replaced Qinv)."""
import numpy as np
import pytest

import oracle_api as ora
import scenes

CONTAINERS = (ora.DISTANCE, ora.TET, ora.VOLUME, ora.BEND)
NODE_ARRAYS = ("positions", "prev_positions", "velocities", "radii", "inv_masses")


def options(solver):
    return ora.Options(solver=solver, iterations=4)


def build(o, solver, scale):
    """A beam with strain, volume, distance and bend constraints on a lattice of spacing `scale`.  Node 0, the only node the two
    lattices share, is pinned: a position constraint's target is no rest data (pies_get_rest has none for it)."""
    scenes.build_beam(o, (3, 3, 5), w_tet=1.0 if solver == ora.PD else 0.05, translation=(0.0, 0.52, 0.0), scale=scale, volume=True, triangles=True)
    o.add_position(np.uint32([0]), 2.0)
    G = lambda i, j, k: k + 5 * (j + 3 * i)  # noqa: E731
    o.add_bend(np.uint32([[G(i, 1, k), G(i + 1, 1, k + 1), G(i + 1, 1, k), G(i, 2, k + 1)] for i in range(2) for k in range(4)]), 0.6)
    o.set_flag(ora.FLAG_NODE_COLLISIONS, 0)


def copy_nodes(dst, src):
    for name in NODE_ARRAYS:
        getattr(dst, "set_" + name)(getattr(src, name))


def same(a, b):
    for name in NODE_ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert np.isfinite(x).all(), name
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, float(np.abs(x - y).max()))


@pytest.mark.parametrize("solver", [ora.PBD, ora.PD], ids=["pbd", "pd"])
def test_writing_back_the_rest_data_changes_nothing(solver):
    a, b = ora.OracleSolver(options(solver)), ora.OracleSolver(options(solver))
    for o in (a, b):
        build(o, solver, 1.0)
        scenes.perturb(o, 9, 0.05)
        o.set_prev_positions(o.positions)
    for t in range(3):
        # PBD: before every tick.  PD: before the first one only - the call marks the system for a rebuild like every scene edit
        # of the oracle, and a rebuild orders the direct solve by the node positions of that moment (other roundings, by design)
        for c in CONTAINERS if solver == ora.PBD or t == 0 else ():
            assert b.count(c) > 0
            b.set_rest(c, b.rest(c))
        a.tick()
        b.tick()
        same(a, b)


@pytest.mark.parametrize("solver", [ora.PBD, ora.PD], ids=["pbd", "pd"])
def test_rest_data_of_another_lattice_carries_the_scene(solver):
    a, b = ora.OracleSolver(options(solver)), ora.OracleSolver(options(solver))
    build(a, solver, 1.0)
    build(b, solver, 1.1)
    scenes.perturb(a, 9, 0.05)
    a.set_prev_positions(a.positions)
    for c in CONTAINERS:
        assert not np.array_equal(a.rest(c), b.rest(c)) or c == ora.BEND  # (a flat sheet's angles do not see the scale)
    copy_nodes(b, a)
    for c in CONTAINERS:
        b.set_rest(c, a.rest(c))
        assert np.array_equal(a.rest(c), b.rest(c))
    for t in range(3):
        a.tick()
        b.tick()
        same(a, b)
    # the replaced rest data mattered: without it scene B goes elsewhere
    start = ora.OracleSolver(options(solver))
    build(start, solver, 1.0)
    scenes.perturb(start, 9, 0.05)
    start.set_prev_positions(start.positions)
    c = ora.OracleSolver(options(solver))
    build(c, solver, 1.1)
    copy_nodes(c, start)
    c.tick(3)
    assert not np.array_equal(c.positions, a.positions)


def test_partial_range_and_bounds():
    o = ora.OracleSolver(options(ora.PD))
    build(o, ora.PD, 1.0)
    before = o.rest(ora.TET)
    new = before[3:7] * np.float32(1.25)
    o.set_rest(ora.TET, new, first=3)
    after = o.rest(ora.TET)
    assert np.array_equal(after[3:7], new) and np.array_equal(after[:3], before[:3]) and np.array_equal(after[7:], before[7:])
    target = o.rest(ora.DISTANCE)
    o.set_rest(ora.DISTANCE, target[-2:] * np.float32(0.5), first=len(target) - 2)
    assert np.array_equal(o.rest(ora.DISTANCE)[-2:], target[-2:] * np.float32(0.5))
    with pytest.raises(ValueError):
        o.set_rest(ora.TET, before, first=1)
