"""CPU tests of the embedded surface meshes (pies_add_skin) through host-only handles (PIES_DEVICE_NONE): the binding rule of
include/pies_hip.h restated in numpy, the error cases, and what the binding survives.  Also the helpers the GPU tests share:
a subdivided box surface, and the skinning formulas in numpy fp64 and - operation for operation as the kernels run them - fp32."""
import numpy as np
import pytest

from pies_amd import capi
from test_node_renumber import shuffled_beam
import scenes

T0 = (0.25, 1.5, 0.5)  # translation of the 3 x 3 x 3 lattice: every node coordinate a multiple of 0.25, the largest 3.5


# ---- helpers (shared with tests/test_skin_gpu.py) -------------------------------------------------------------------------------
def box_surface(lo, hi, n):
    """The surface of the box [lo, hi], every face cut into n x n squares of two triangles (right isosceles up to the box's
    aspect: no slivers), wound outward: (vertices (6 n^2 + 2) x 3 float32, triangles (12 n^2) x 3 uint32).  Vertices are numbered
    face by face in the order the faces first reach them."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    index, pts, tris = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(pts)
            pts.append(p)
        return index[p]

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def corner(a, b):
                        p = [0, 0, 0]
                        p[axis], p[u], p[v] = side, a, b
                        return vid(tuple(p))
                    q = [corner(i, j), corner(i + 1, j), corner(i + 1, j + 1), corner(i, j + 1)]
                    if side == 0:
                        q = q[::-1]  # e_u x e_v = +e_axis: outward on the far side, reversed on the near one
                    tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    x = lo + np.asarray(pts, np.float64) / n * (hi - lo)
    return x.astype(np.float32), np.asarray(tris, np.uint32)


def skin_mesh(count, lo, hi):
    """A box surface cut down to exactly `count` vertices: the first `count` vertices of the coarsest subdivision that has as many,
    and the triangles among them (a subset of well-shaped triangles; some vertices at the cut keep few or none)."""
    n = 1
    while 6 * n * n + 2 < count:
        n += 1
    v, t = box_surface(lo, hi, n)
    return v[:count].copy(), t[(t < count).all(axis=1)].copy()


def skin64(P, ids, w):
    """fp64 evaluation of a stored binding: x = p0 + w1 (p1 - p0) + w2 (p2 - p0) + w3 (p3 - p0)"""
    P, w = np.asarray(P, np.float64), np.asarray(w, np.float64)
    p = [P[ids[:, k]] for k in range(4)]
    return p[0] + w[:, 1:2] * (p[1] - p[0]) + w[:, 2:3] * (p[2] - p[0]) + w[:, 3:4] * (p[3] - p[0])


def skin32(P, ids, w):
    """The same in fp32 in the order k_skin_positions runs it (numpy rounds every operation: no fused multiply-add)"""
    P, w = np.asarray(P, np.float32), np.asarray(w, np.float32)
    p = [P[ids[:, k]] for k in range(4)]
    x = p[0] + w[:, 1:2] * (p[1] - p[0])
    x = x + w[:, 2:3] * (p[2] - p[0])
    x = x + w[:, 3:4] * (p[3] - p[0])
    assert x.dtype == np.float32
    return x


def normal_sums(x, tris):
    """Per vertex the sum of cross(x_b - x_a, x_c - x_a) over the triangles that name it, ascending triangle index, in x's
    precision with every product and sum rounded (the loop of k_skin_normals)."""
    S = np.zeros_like(x)
    if len(tris):
        a, b, c = x[tris[:, 0]], x[tris[:, 1]], x[tris[:, 2]]
        u, v = b - a, c - a
        cr = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        assert cr.dtype == x.dtype
        for t in range(len(tris)):
            for k in tris[t]:
                S[k] = S[k] + cr[t]
    return S


def normalize_sums(S):
    len2 = S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1] + S[:, 2] * S[:, 2]
    ok = (len2 > 0) & np.isfinite(len2)
    out = np.zeros_like(S)
    out[ok] = S[ok] / np.sqrt(len2[ok])[:, None]
    return out


def normals_of(x, tris):
    return normalize_sums(normal_sums(x, tris))


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def gates(P, ids, w, tris):
    """The yardstick of the GPU tests for one skin on node positions P: (x64, n64, position gate, normal gate, fp32-vs-fp64
    errors).  Position gate: max(2 |fp32 restatement - fp64|, 4 ulp of the scene's largest coordinate); normals: the same form
    with a floor of 2e-6."""
    x64, x32 = skin64(P, ids, w), skin32(P, ids, w)
    n64, n32 = normals_of(x64, tris), normals_of(x32, tris)
    ex, en = float(np.abs(x32 - x64).max()), float(np.abs(n32 - n64).max())
    return x64, n64, max(2.0 * ex, 4.0 * ulp32(np.abs(P).max())), max(2.0 * en, 2e-6), (ex, en)


def host_solver(solver=capi.PD):
    return capi.Solver(capi.Options(solver=solver, iterations=4), device=capi.DEVICE_NONE)


def lattice(g, translation=T0):
    """createTetBox 3 x 3 x 3 (48 elements); returns its elements (global node ids)"""
    first = g.count(capi.TET)
    g.create_tet_box(3, 3, 3, translation=translation, w=1.0, volume=True, triangles=True)
    return g.ids(capi.TET)[first:]


def brute_force(P, tets, v, max_distance=0.0):
    """The binding rule in fp64, every element against every vertex: (best min-barycentric per vertex, its element, the
    (vertices x elements) matrix of min-barycentric coordinates, -inf where an element is no candidate)."""
    P = np.asarray(P, np.float64)
    p = P[tets]  # (m, 4, 3)
    lo, hi = p.min(1) - max_distance, p.max(1) + max_distance
    M = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]], 2)  # columns e1, e2, e3
    det = np.linalg.det(M)
    good = np.abs(det) > 1e-30
    inv = np.zeros_like(M)
    inv[good] = np.linalg.inv(M[good])
    v = np.asarray(v, np.float64)
    w123 = np.einsum("mij,vmj->vmi", inv, v[:, None, :] - p[None, :, 0, :])
    w = np.concatenate([1.0 - w123.sum(2, keepdims=True), w123], 2)
    m = w.min(2)
    inside = ((v[:, None, :] >= lo[None]) & (v[:, None, :] <= hi[None])).all(2)
    m[~(inside & good[None, :])] = -np.inf
    return m.max(1), m.argmax(1), m


# ---- one tetrahedron -------------------------------------------------------------------------------------------------------------
TET = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) + np.float32([1.0, 2.0, 3.0])


def one_tet():
    g = host_solver()
    g.addNodes(TET)
    return g


def test_one_tetrahedron_binds_with_the_expected_weights():
    g = one_tet()
    W = np.float64([[0.25, 0.25, 0.25, 0.25],    # centroid
                    [0.0, 0.5, 0.25, 0.25],      # on the face opposite node 0
                    [0.5, 0.5, 0.0, 0.0],        # on the edge 0-1
                    [0.0, 0.0, 1.0, 0.0],        # exactly node 2
                    [1.0625, -0.0625, 0.0, 0.0]])  # outside (x below the box by 0.0625), within max_distance = 0.1
    v = (W @ TET.astype(np.float64)).astype(np.float32)
    k = g.add_skin(v, [[0, 1, 2, 3]], max_distance=0.1)
    assert k == 0 and g.count(capi.SKINS) == 1 and g.count(capi.SKIN_VERTICES) == 5
    tet, ids, w = g.skin_binding(0)
    assert np.array_equal(tet, np.zeros(5, np.uint32)) and np.array_equal(ids, np.tile(np.uint32([0, 1, 2, 3]), (5, 1)))
    assert np.abs(w - W).max() <= 1e-6, w
    assert np.abs(w[3] - [0, 0, 1, 0]).max() <= 1e-6  # the node: a unit vector


def test_vertex_beyond_max_distance_fails_and_adds_nothing():
    g = one_tet()
    v = np.float32([[1.25, 2.25, 3.25], [0.8, 2.1, 3.1], [1.25, 2.25, 3.25]])  # vertex 1: 0.2 below the box in x
    with pytest.raises(capi.PiesError) as e:
        g.add_skin(v, [[0, 1, 2, 3]], max_distance=0.1)
    assert "vertex 1" in str(e.value)
    assert g.count(capi.SKINS) == 0 and g.count(capi.SKIN_VERTICES) == 0
    assert g.add_skin(v, [[0, 1, 2, 3]], max_distance=0.25) == 0  # within reach now


# ---- the 3 x 3 x 3 lattice ---------------------------------------------------------------------------------------------------------
def test_lattice_binding_matches_the_rule_in_fp64():
    g = host_solver()
    tets = lattice(g)
    assert len(tets) == 48
    P = g.positions
    rng = np.random.default_rng(17)
    v = (P.min(0) + rng.uniform(0.02, 0.98, (257, 3)) * (P.max(0) - P.min(0))).astype(np.float32)
    g.add_skin(v, tets)
    tet, ids, w = g.skin_binding(0)
    assert np.array_equal(ids, tets[tet])
    best, _, m = brute_force(P, tets, v)
    chosen = m[np.arange(len(v)), tet]
    assert (chosen >= best - 1e-5).all(), float((best - chosen).max())
    # the weights reproduce the vertex (fp64 sum of the stored fp32 weights) to 4 ulp of the largest coordinate
    x = np.einsum("vk,vkj->vj", w.astype(np.float64), P.astype(np.float64)[ids])
    err = float(np.abs(x - v).max())
    print("lattice: max |sum w p - v| = %.3g (4 ulp = %.3g)" % (err, 4 * ulp32(np.abs(P).max())))
    assert err <= 4 * ulp32(np.abs(P).max())
    # and sum to 1 within 2 ulp
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 2 * ulp32(1.0)
    # w0 is exactly 1 - (w1 + w2 + w3) in fp32
    assert np.array_equal(w[:, 0], np.float32(1.0) - (w[:, 1] + w[:, 2] + w[:, 3]))


def test_tie_binds_to_the_lower_index():
    """Two elements that share the face x = 1: a vertex on it has min barycentric 0 in both, the lower index wins whichever way
    round they are listed."""
    g = host_solver()
    g.addNodes(np.float32([[1, 0, 0], [1, 1, 0], [1, 0, 1], [0, 0, 0], [2, 0, 0]]) + np.float32([0.5, 1.0, 0.5]))
    left, right = [3, 0, 1, 2], [4, 0, 2, 1]
    v = np.float32([[1.5, 1.25, 0.75]])
    g.add_skin(v, [left, right])
    g.add_skin(v, [right, left])
    for k, first in ((0, left), (1, right)):
        tet, ids, w = g.skin_binding(k)
        assert tet[0] == 0 and ids[0].tolist() == first and abs(float(w[0].min())) == 0.0


def test_flat_element_is_never_chosen():
    g = host_solver()
    g.addNodes(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0],      # a flat element in the plane z = 1.5
                           [0, 0, -1], [2, 0, -1], [0, 2, -1], [0, 0, 1]]) + np.float32([1.0, 1.0, 1.5]))
    v = np.float32([[1.25, 1.25, 1.5]])  # in the flat element's plane and box, inside the second element
    g.add_skin(v, [[0, 1, 2, 3], [4, 5, 6, 7]])
    tet, ids, w = g.skin_binding(0)
    assert tet[0] == 1 and w[0].min() > 0
    with pytest.raises(capi.PiesError):  # the flat element alone: no candidate
        g.add_skin(v, [[0, 1, 2, 3]])
    assert g.count(capi.SKINS) == 1


def test_error_cases():
    g = one_tet()
    v = np.float32([[1.25, 2.25, 3.25]])
    for kw in (dict(vertices=v, tets=[[0, 1, 2, 4]]),                       # node id out of range
               dict(vertices=v, tets=[[0, 1, 2, 3]], triangles=[[0, 0, 1]]),  # triangle index >= n_vertices
               dict(vertices=np.zeros((0, 3), np.float32), tets=[[0, 1, 2, 3]]),  # no vertices
               dict(vertices=v, tets=[[0, 1, 2, 3]], max_distance=-0.5),
               dict(vertices=v, tets=[[0, 1, 2, 3]], max_distance=float("nan")),
               dict(vertices=v, tets=[[0, 1, 2, 3]], max_distance=float("inf"))):
        with pytest.raises(capi.PiesError):
            g.add_skin(**kw)
        assert g.last_error() != ""
    assert g.count(capi.SKINS) == 0
    L = capi.load()
    import ctypes as C
    assert L.pies_get_skin_binding(g._h, 0, None, None, None, 0, None) == capi.ERR_INVALID  # no such skin
    g.add_skin(v, [[0, 1, 2, 3]])
    assert L.pies_read_skin(g._h, 0, C.cast(v.ctypes.data, C.POINTER(C.c_float)), None, 1) == capi.ERR_HIP  # host-only handle


def test_binding_survives_finalize_appends_and_renumbering():
    mesh = shuffled_beam()
    pos, tets, _ = mesh
    g = host_solver()
    scenes.build_unstructured_pd(g, mesh)
    lo, hi = pos.min(0), pos.max(0)
    v, tri = box_surface(lo + 0.8, hi - 0.8, 4)
    g.add_skin(v, tets, tri, max_distance=0.5)
    before = g.skin_binding(0)
    g.set_flag(capi.FLAG_RENUMBER_NODES, 1)
    g.finalize()
    assert g.count(capi.NODES_RENUMBERED) == 1
    g.add_nodes_raw(pos + np.float32([20.0, 0.0, 0.0]), radius=0.5)
    g.add_tet(tets + len(pos), 1.0)
    g.finalize()
    g.set_solver(capi.PBD)
    g.finalize()
    after = g.skin_binding(0)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    # host ids: the bound element's nodes are the element as the host listed it
    assert np.array_equal(after[1], tets[after[0]])
    assert np.abs(skin64(g.positions, after[1], after[2]) - v).max() <= 1e-5


def test_clear_drops_the_skins():
    g = host_solver()
    tets = lattice(g)
    v, tri = skin_mesh(63, np.float32(T0) + 0.05, np.float32(T0) + 1.95)
    g.add_skin(v, tets, tri)
    g.add_skin(v[:10], tets)
    assert g.count(capi.SKINS) == 2 and g.count(capi.SKIN_VERTICES) == 73
    g.clear()
    assert g.count(capi.SKINS) == 0 and g.count(capi.SKIN_VERTICES) == 0


# ---- the yardstick's own inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 65, 257, 1025])
def test_fp32_restatement_stays_inside_the_gate(count):
    """The skins of tests/test_skin_gpu.py on the rest lattice: the fp32 restatement of the kernels is inside the gate it defines
    (it is by construction - twice its own error -; what this pins is that the inputs are benign: the errors stay near the
    floors), and the restated rest state returns the input vertices within the position gate."""
    g = host_solver()
    tets = lattice(g)
    v, tri = skin_mesh(count, np.float32(T0) + 0.05, np.float32(T0) + 1.95)
    assert len(v) == count
    g.add_skin(v, tets, tri)
    _, ids, w = g.skin_binding(0)
    P = g.positions
    x64, n64, gx, gn, (ex, en) = gates(P, ids, w, tri)
    print("count %d: fp32 vs fp64 positions %.3g (gate %.3g), normals %.3g (gate %.3g)" % (count, ex, gx, en, gn))
    assert ex <= gx and en <= gn
    assert gx <= 8 * ulp32(np.abs(P).max()) and gn <= 2e-5
    assert np.abs(skin32(P, ids, w) - v).max() <= gx
    if count > 1:
        length = np.linalg.norm(n64, axis=1)
        assert ((np.abs(length - 1.0) < 1e-12) | (length == 0.0)).all()
