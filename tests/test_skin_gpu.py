"""GPU tests of the embedded surface meshes (pies_add_skin / pies_read_skin / pies_export_acquire_skin).

The yardstick follows the pattern of the PD tests: the device is compared with an fp64 numpy evaluation of the STORED binding on
the node positions read back from the device, and may be no further from it than
    max(2 x |numpy fp32 restatement in the kernels' operation order - fp64|, 4 ulp of the scene's largest coordinate)
for positions, and the same form with a floor of 2e-6 for normals (tests/test_skin.py holds the restatements and checks on the
CPU that they stay inside that gate for these inputs).  The skins are subdivided box surfaces: well-shaped triangles, no slivers.

Largest device-minus-fp64 values seen on an MI355X run of this file: NOT RECORDED YET (every check prints its figures;
run with -s)."""
import numpy as np
import pytest

import scenes
from test_node_renumber import shuffled_beam
from test_skin import T0, box_surface, gates, lattice, normal_sums, normalize_sums, skin64, skin_mesh, ulp32

pytestmark = pytest.mark.gpu

LO, HI = np.float32(T0) + 0.05, np.float32(T0) + 1.95  # the skins' box, just inside the 3 x 3 x 3 lattice


def pbd(pies):
    g = pies.Solver(scenes.pbd_options(pies, 4))
    g.set_schedule(pies.SCHEDULE_LAYERED)
    return g


def pbd_lattice(pies, g):
    """The PBD body of these tests: the 3 x 3 x 3 lattice held by distance constraints (createBox; the reference's PBD strain
    projection flattens a tetrahedral body within a tick, quirk Q2, which would turn the skin's triangles into slivers).  The skin
    binds to createTetBox's 48 elements over the same node numbering: listed tetrahedra need not be constraints of the scene."""
    g.create_box(3, 3, 3, translation=T0, w=0.5, triangles=False)
    return lattice(pies.Solver(pies.Options(solver=pies.PD), device=pies.DEVICE_NONE))


def body(pies, kind):
    g = pbd(pies) if kind == "pbd" else pd(pies)
    return g, (pbd_lattice(pies, g) if kind == "pbd" else lattice(g))


def pd(pies, **kw):
    return pies.Solver(pies.Options(solver=pies.PD, iterations=10, **kw))


def check(g, skin, tri, what=""):
    """read_skin against the yardstick on the positions the device holds; returns (positions, normals) as read"""
    _, ids, w = g.skin_binding(skin)
    x, nr = g.read_skin(skin)
    x64, n64, gx, gn, _ = gates(g.positions, ids, w, tri)
    assert np.isfinite(x).all() and np.isfinite(nr).all()
    dx, dn = float(np.abs(x - x64).max()), float(np.abs(nr - n64).max())
    print("%s skin %d: device vs fp64 positions %.3g (gate %.3g), normals %.3g (gate %.3g)" % (what, skin, dx, gx, dn, gn))
    assert dx <= gx, (what, dx, gx)
    assert dn <= gn, (what, dn, gn)
    return x, nr


@pytest.mark.parametrize("count", [1, 63, 65, 257, 1025])
def test_rest_state(pies, count):
    """Bound and read before any tick: the inputs come back, the normals are those of the input surface (lane tails: 1, 63, 65;
    more than one workgroup: 257, 1 025)."""
    g = pd(pies)
    tets = lattice(g)
    v, tri = skin_mesh(count, LO, HI)
    assert g.add_skin(v, tets, tri) == 0
    x, nr = check(g, 0, tri, "rest %d" % count)
    _, ids, w = g.skin_binding(0)
    gx = gates(g.positions, ids, w, tri)[2]
    assert np.abs(x - v).max() <= gx
    assert np.array_equal(g.read_skin(0, normals=False), x)
    assert g.count(pies.SKINS) == 1 and g.count(pies.SKIN_VERTICES) == count


def test_affine_map(pies):
    """Every node written to A p + t: the skin is A v + t and its normals normalize(A^-T sum) of the rest sums - exact properties of
    the formulas (w0 = 1 - (w1 + w2 + w3); cross(A u, A v) = det A A^-T cross(u, v), det A > 0).  A, t and the lattice are dyadic,
    so the mapped nodes are exact in fp32."""
    A = np.float64([[1.5, 0.25, 0.0], [0.0, 1.25, 0.5], [0.25, 0.0, 1.0]])
    t = np.float64([0.5, 2.0, 0.25])
    assert np.linalg.det(A) > 0
    g = pd(pies)
    tets = lattice(g)
    v, tri = skin_mesh(257, LO, HI)
    g.add_skin(v, tets, tri)
    _, ids, w = g.skin_binding(0)
    P0 = g.positions.astype(np.float64)
    x0 = skin64(P0, ids, w)
    P1 = P0 @ A.T + t
    assert np.array_equal(P1.astype(np.float32).astype(np.float64), P1)
    g.set_positions(P1.astype(np.float32))
    x, nr = check(g, 0, tri, "affine")
    _, _, gx, gn, _ = gates(P1, ids, w, tri)
    assert np.abs(x - (x0 @ A.T + t)).max() <= gx
    # against the inputs themselves: plus the binding's own error (4 ulp of the rest scene, tests/test_skin.py) through A
    assert np.abs(x - (v.astype(np.float64) @ A.T + t)).max() <= gx + np.abs(A).sum(1).max() * 4 * ulp32(np.abs(P0).max())
    expect = normalize_sums(normal_sums(x0, tri) @ np.linalg.inv(A))  # rows: (A^-T s)^T = s^T A^-1
    assert np.abs(nr - expect).max() <= gn


def dynamic_run(pies, kind):
    g, tets = body(pies, kind)
    v, tri = skin_mesh(257, LO, HI)
    g.add_skin(v, tets, tri)
    scenes.perturb(g, 3, 0.05)
    g.set_prev_positions(g.positions)
    out = []
    for k in range(3):
        g.tick()
        out.append(check(g, 0, tri, "%s tick %d" % (kind, k + 1)))
    assert not g.failed
    return out


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_dynamic_state_and_reproducibility(pies, kind):
    """3 ticks of PBD (schedule LAYERED) / PD on the perturbed lattice: after every tick read_skin is the yardstick on `positions`;
    a second fresh run gives the same positions and normals bit for bit."""
    a, b = dynamic_run(pies, kind), dynamic_run(pies, kind)
    moved = np.abs(a[2][0] - a[0][0]).max()
    assert moved > 1e-3  # the skin follows the body
    for (xa, na), (xb, nb) in zip(a, b):
        assert np.array_equal(xa, xb) and np.array_equal(na, nb)


def test_renumbered_pd_scene(pies):
    """The shuffled Delaunay beam with PIES_FLAG_RENUMBER_NODES: the binding stays in host ids, the device records are translated;
    the skin is the one of the flag-off run within the PD tolerance of tests/test_node_renumber_gpu.py, and inside the yardstick."""
    from test_node_renumber_gpu import beam, pd_options, tol_for
    mesh = shuffled_beam()
    pos, tets, _ = mesh
    v, tri = box_surface(pos.min(0) + 0.8, pos.max(0) - 0.8, 6)
    on, off = pies.Solver(pd_options(pies)), pies.Solver(pd_options(pies))
    on.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    res = []
    for s in (on, off):
        beam(s, mesh)
        s.add_skin(v, tets, tri, max_distance=0.5)
        s.tick(3)
        res.append(check(s, 0, tri, "renumber"))
    assert on.count(pies.NODES_RENUMBERED) == 1 and off.count(pies.NODES_RENUMBERED) == 0
    for a, b in zip(on.skin_binding(0), off.skin_binding(0)):
        assert np.array_equal(a, b)
    assert np.array_equal(on.skin_binding(0)[1], tets[on.skin_binding(0)[0]])
    assert np.abs(res[0][0] - res[1][0]).max() <= tol_for(off.positions)


def test_export_path(pies):
    """Two frames in flight: export_acquire_skin of each equals a read_skin taken at the same tick count on a twin handle, bit for
    bit; the views stay valid until release; a third tick_begin with the oldest frame held fails as it does without skins."""
    def make():
        g, tets = body(pies, "pbd")
        v, tri = skin_mesh(257, LO, HI)
        g.add_skin(v, tets, tri)
        g.add_skin(v[:65], tets)
        scenes.perturb(g, 4, 0.05)
        g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)  # (as tests/test_export_gpu.py compares the two tick paths)
        return g
    g, twin = make(), make()
    f1, f2 = g.tick_begin(), g.tick_begin()
    assert (f1, f2) == (1, 2)
    x1, n1 = g.export_acquire_skin(f1, 0)  # held
    assert x1.shape == (257, 3) and n1.shape == (257, 3)
    keep = x1.copy(), n1.copy()
    with pytest.raises(pies.PiesError):
        g.tick_begin()
    twin.tick()
    r1 = twin.read_skin(0), twin.read_skin(1)
    y1, m1 = g.export_acquire_skin(f1, 1)
    assert y1.shape == (65, 3) and not m1.any()
    assert np.array_equal(x1, r1[0][0]) and np.array_equal(n1, r1[0][1]) and np.array_equal(y1, r1[1][0])
    assert np.array_equal(g.export_acquire(f1)[:, :3], twin.positions)
    assert np.array_equal(x1, keep[0]) and np.array_equal(n1, keep[1])  # still the frame's, until release
    g.export_release(f1)
    twin.tick()
    x2, n2 = g.export_acquire_skin(f2, 0)
    r2 = twin.read_skin(0)
    assert np.array_equal(x2, r2[0]) and np.array_equal(n2, r2[1])
    assert np.abs(x2 - keep[0]).max() > 0
    g.export_release(f2)
    assert g.tick_begin() == 3
    with pytest.raises(pies.PiesError):
        g.export_acquire_skin(f1, 0)  # only the last two frames are kept


def test_two_skins_on_two_bodies(pies):
    """One skin with triangles, one without (positions only; all-zero normals when asked); a second body added after the first
    skin was bound leaves the first skin's output unchanged."""
    g = pd(pies)
    tets = lattice(g)
    v, tri = skin_mesh(257, LO, HI)
    g.add_skin(v, tets, tri)
    first = g.read_skin(0)
    t2 = np.float32([5.25, 1.5, 0.5])
    tets2 = lattice(g, translation=tuple(t2))
    assert tets2.min() == 27
    v2 = skin_mesh(63, t2 + 0.05, t2 + 1.95)[0]
    assert g.add_skin(v2, tets2) == 1
    assert g.count(pies.SKINS) == 2 and g.count(pies.SKIN_VERTICES) == 320
    again = g.read_skin(0)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    x2 = g.read_skin(1, normals=False)  # normals = NULL
    y2, n2 = g.read_skin(1)
    assert np.array_equal(x2, y2) and not n2.any()
    none = np.zeros((0, 3), np.uint32)
    check(g, 1, none, "second body, rest")
    scenes.perturb(g, 6, 0.04)
    g.set_prev_positions(g.positions)
    g.tick(2)
    check(g, 0, tri, "first body")
    check(g, 1, none, "second body")


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_a_skin_changes_nothing_else(pies, kind):
    """launch_counts() - after finalize and after 3 ticks - and the node state after 3 ticks are the same with and without a bound
    skin (read between the ticks)."""
    runs = []
    for skinned in (False, True):
        g, tets = body(pies, kind)
        if skinned:
            v, tri = skin_mesh(257, LO, HI)
            g.add_skin(v, tets, tri)
        scenes.perturb(g, 8, 0.05)
        g.set_prev_positions(g.positions)
        g.finalize()
        counts = g.launch_counts()
        for _ in range(3):
            g.tick()
            if skinned:
                g.read_skin(0)
        # (the PBD node-node pass adapts its captured level launches to the scene at every synchronisation: the counts move
        # over the ticks, the same way in both runs)
        runs.append(((counts, g.launch_counts()), g.positions.copy(), g.velocities.copy()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])


def test_isolated_vertex_gets_a_zero_normal(pies):
    g = pd(pies)
    tets = lattice(g)
    v, tri = skin_mesh(65, LO, HI)
    v = np.concatenate([v, np.float32([[1.0, 2.5, 1.5]])])  # inside the lattice, in no triangle
    g.add_skin(v, tets, tri)
    x, nr = check(g, 0, tri, "isolated")
    assert not nr[65].any() and np.abs(x[65] - v[65]).max() <= 4 * ulp32(3.5)
    named = np.zeros(66, bool)
    named[tri.reshape(-1)] = True
    assert np.abs(np.linalg.norm(nr[named], axis=1) - 1.0).max() <= 1e-6
