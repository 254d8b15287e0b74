"""GPU tests of pies_voxelize_tri_mesh (k_winding) and pies_add_tri_mesh_volume.

Values: the device's w against numpy fp64 within max(2 x |fp32 restatement - fp64|, T x 2^-22) (tests/test_trimesh.py holds the
restatements, computes each reference once and checks on the CPU that the inputs are benign).  Classification: `inside` equals
|w64| > 0.5 at EVERY sample of the closed meshes - the lattices are placed so that no sample is within 0.05 of the threshold
(checked on the CPU).  Bodies: nodes, elements and the triangle set equal the numpy restatement of the rules of pies_hip.h fed
with the device's own inside mask.

Largest device-minus-fp64 values seen on an MI355X run of this file (every check prints its figures; run with -s): values
1.31e-06 at T = 1 025 (gate 2.44e-04), 3.6e-07 at T = 1 (gate 7.35e-07, the tightest), hemisphere 5.1e-07 (gate 3.62e-05);
classification lattices 1.55e-06 (torus); body skins after 10 ticks 2.55e-07 positions (gate 9.54e-07), 1.45e-06 normals
(gate 2.91e-06); smallest stored barycentric coordinate -2.38e-07 (thin plate)."""
import numpy as np
import pytest

import scenes
from test_skin import ulp32
from test_skin_gpu import check
from test_trimesh import (BODIES, CLOSED, LATTICES, TRIANGLE_COUNTS, body_of, closed_case, hemisphere_case, icosphere, lattice_of,
                          thin_plate, triangle_set, value_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pies):
    """One handle for the calls that leave the scene alone"""
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    yield g
    g.close()


def value_check(dev, v, tri, origin, cell, dims, w64, gate, what):
    w, inside = dev.voxelize_tri_mesh(v, tri, origin, cell, dims)
    assert w.shape == tuple(dims) and np.isfinite(w).all()
    d = float(np.abs(w.astype(np.float64) - w64).max())
    print("%s: device - fp64 = %.3g, gate %.3g" % (what, d, gate))
    assert d <= gate, (what, d, gate)
    assert np.array_equal(inside, np.abs(w) > np.float32(0.5))
    return w, inside


@pytest.mark.parametrize("dims", LATTICES)
@pytest.mark.parametrize("count", TRIANGLE_COUNTS)
def test_winding_value(dev, count, dims):
    v, tri, origin, cell, w64, gate, _ = value_case(count, dims)
    value_check(dev, v, tri, origin, cell, dims, w64, gate, "T %d lattice %s" % (count, dims))


def test_winding_value_at_negative_coordinates(dev):
    v, tri, origin, cell, w64, gate, _ = value_case(257, (3, 5, 7), True)
    assert v.max() < 0 and origin.max() < 0
    value_check(dev, v, tri, origin, cell, (3, 5, 7), w64, gate, "shifted")


def test_winding_value_of_an_open_surface(dev):
    v, tri, origin, cell, dims, w64, gate, _ = hemisphere_case()
    value_check(dev, v, tri, origin, cell, dims, w64, gate, "hemisphere")


def test_two_calls_are_bit_equal(dev, pies):
    v, tri, origin, cell, _, _, _ = value_case(1025, (9, 8, 7))
    a = dev.voxelize_tri_mesh(v, tri, origin, cell, (9, 8, 7))
    b = dev.voxelize_tri_mesh(v, tri, origin, cell, (9, 8, 7))
    other = pies.Solver(pies.Options(solver=pies.PBD))
    c = other.voxelize_tri_mesh(v, tri, origin, cell, (9, 8, 7))
    for x in (b, c):
        assert np.array_equal(a[0].view(np.uint32), x[0].view(np.uint32)) and np.array_equal(a[1], x[1])
    # either output may be left out
    n = np.zeros(3, np.uint32) + np.uint32([9, 8, 7])
    vv, tt, oo = pies._f32(v), pies._u32(tri), pies._f32(origin)
    assert dev._L.pies_voxelize_tri_mesh(dev._h, len(vv), pies._pf(vv), len(tt), pies._pu(tt), pies._pf(oo), cell, pies._pu(n), None, None) == pies.OK


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_classification(dev, name):
    v, tri, origin, cell, dims, w64 = closed_case(name)
    w, inside = dev.voxelize_tri_mesh(v, tri, origin, cell, dims)
    print("%s: %d of %d samples inside, device - fp64 = %.3g" % (name, inside.sum(), inside.size, np.abs(w - w64).max()))
    assert np.array_equal(inside, np.abs(w64) > 0.5)


def tet_volumes(p, tets):
    q = p.astype(np.float64)[tets]
    return np.abs(np.linalg.det(q[:, 1:] - q[:, :1])) / 6.0


def check_body(pies, g, v, tri, resolution, first_nodes=0, density=2.5, velocity=(0.0, -1.0, 0.5)):
    first, n_nodes, n_tets, skin = g.add_tri_mesh_volume(v, tri, resolution, velocity=velocity, density=density)
    origin, cell, dims = lattice_of(v, resolution)
    _, inside = g.voxelize_tri_mesh(v, tri, origin, cell, dims)
    r = body_of(inside, v, resolution)
    assert first == first_nodes and n_nodes == len(r["positions"]) and n_tets == len(r["tets"]) == 6 * r["keep"].sum()
    assert g.count(pies.NODES) == first + n_nodes
    assert np.array_equal(g.positions[first:], r["positions"])
    assert np.array_equal(g.ids(pies.TET)[-n_tets:], r["tets"] + first) and np.array_equal(g.ids(pies.VOLUME)[-n_tets:], r["tets"] + first)
    mine = g.ids(pies.TRIANGLES)[-len(r["triangles"]):]
    assert np.array_equal(triangle_set(mine), triangle_set(r["triangles"] + first))
    assert np.array_equal(g.radii[first:], np.full(n_nodes, min(np.float32(0.5), np.float32(0.95) * np.float32(0.5) * cell), np.float32))
    assert np.array_equal(g.inv_masses[first:], np.full(n_nodes, np.float32(1.0) / np.float32(density), np.float32))
    assert np.array_equal(g.velocities[first:], np.tile(np.float32(velocity), (n_nodes, 1)))
    tet, ids, w = g.skin_binding(skin)
    assert len(w) == len(v) and np.array_equal(ids, (r["tets"] + first)[tet])
    print("resolution %d: %d kept cells of %s, %d nodes, min barycentric %.3g" % (resolution, r["keep"].sum(), r["dims"], n_nodes, w.min()))
    assert w.min() >= -1e-5
    # summed element volume = kept cells x cell^3: every lattice coordinate is rounded to fp32 (half an ulp of the largest
    # coordinate, at both ends of each of a cell's three edges), the cell size itself once
    total, expect = tet_volumes(g.positions, g.ids(pies.TET)[-n_tets:]).sum(), r["keep"].sum() * float(cell) ** 3
    tol = expect * (3.0 * ulp32(np.abs(r["positions"]).max()) / float(cell) + 3.0 * 2.0 ** -24)
    assert abs(total - expect) <= tol, (total, expect, tol)
    return r, skin


@pytest.mark.parametrize("name", sorted(BODIES))
def test_body_follows_the_rules(pies, name):
    make, resolution = BODIES[name]
    v, tri = make()
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    r, skin = check_body(pies, g, v, tri, resolution)
    assert skin == 0 and g.count(pies.SKINS) == 1 and g.count(pies.SKIN_VERTICES) == len(v)
    if name == "box":
        assert r["dims"] == (4, 2, 2) and r["keep"].all()
    # reversed winding: the same body
    h = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    h.add_tri_mesh_volume(v, tri[:, ::-1], resolution)
    assert np.array_equal(h.positions, g.positions) and np.array_equal(h.ids(pies.TET), g.ids(pies.TET))
    # a second body behind existing nodes: global ids
    check_body(pies, h, v + np.float32([6.0, 0.0, 0.0]), tri, resolution, first_nodes=h.count(pies.NODES))
    assert h.count(pies.SKINS) == 2


def test_thin_plate_becomes_a_body(pies):
    v, tri = thin_plate()
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    r, _ = check_body(pies, g, v, tri, 4)
    origin, cell, dims = lattice_of(v, 4)
    _, inside = g.voxelize_tri_mesh(v, tri, origin, cell, dims)
    assert r["keep"].sum() > inside.sum()  # the vertex clause, not the winding number, makes most of it


def scene_counts(pies, g):
    return tuple(g.count(k) for k in (pies.NODES, pies.POSITION, pies.DISTANCE, pies.TET, pies.VOLUME, pies.BEND, pies.TRIANGLES,
                                      pies.SKINS, pies.SKIN_VERTICES))


def test_failure_is_atomic(pies):
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5), w=1.0)
    g.tick()
    before, p = scene_counts(pies, g), g.positions
    v, tri = icosphere(1, 1.0, (4.0, 2.0, 0.0))
    bad = tri.copy()
    bad[-1, 2] = len(v)
    with pytest.raises(pies.PiesError):
        g.add_tri_mesh_volume(v, bad, 4)
    with pytest.raises(pies.PiesError):
        g.add_tri_mesh_volume(v, tri, 0)
    assert scene_counts(pies, g) == before and np.array_equal(g.positions, p)
    g.tick()
    assert not g.failed and np.isfinite(g.positions).all() and np.abs(g.positions - p).max() > 0
    first = g.add_tri_mesh_volume(v, tri, 4)[0]  # and the call still works afterwards
    assert first == 27
    g.tick()
    assert not g.failed and np.isfinite(g.positions).all()


def drop(pies, kind, renumber=False):
    v, tri = BODIES["icosphere"][0]()
    if kind == "pd":
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        if renumber:
            g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    else:
        g = pies.Solver(scenes.pbd_options(pies, 4))
        g.set_schedule(pies.SCHEDULE_LAYERED)
        g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)  # tetrahedral bodies: as bench.py runs them
    _, _, _, skin = g.add_tri_mesh_volume(v, tri, 6, velocity=(0.0, -2.0, 0.0))
    ids = g.ids(pies.TET).copy()
    rest = g.read_skin(skin)[0]
    assert np.abs(rest - v).max() <= 1e-5
    for k in range(10):
        g.tick()
        if k in (0, 9):
            check(g, skin, tri, "%s tick %d" % (kind, k + 1))
    assert not g.failed
    for a in (g.positions, g.velocities, *g.read_skin(skin)):
        assert np.isfinite(a).all()
    assert g.read_skin(skin)[0][:, 1].mean() < rest[:, 1].mean() - 0.05  # it fell, and the skin with it
    return g, ids, v, tri


@pytest.mark.parametrize("kind", ["pd", "pbd", "pd-renumbered"])
def test_it_simulates(pies, kind):
    g, ids, v, tri = drop(pies, kind.split("-")[0], renumber=kind.endswith("renumbered"))
    if kind == "pd":
        g.clear()
        assert g.count(pies.SKINS) == 0 and g.count(pies.NODES) == 0
        _, _, _, skin = g.add_tri_mesh_volume(v, tri, 6, velocity=(0.0, -2.0, 0.0))
        assert skin == 0 and np.array_equal(g.ids(pies.TET), ids)
        g.tick()
        assert np.isfinite(g.positions).all()
