"""CPU side of pies_voxelize_tri_mesh / pies_add_tri_mesh_volume: the rules of include/pies_hip.h restated in numpy (the
generalised winding number in fp64 and - operation for operation as k_winding runs it - in fp32, the lattice, the kept cells, the
node numbering, the six-tetrahedra split, the boundary rule), the meshes and lattices tests/test_trimesh_gpu.py uses, the conditions
those tests rely on checked here without a device, and the error cases through host-only handles (PIES_DEVICE_NONE).

The gate of the GPU value tests follows the project's PD yardstick pattern: the device may be no further from fp64 than
    max(2 x |fp32 restatement - fp64|, T x 2^-22),   T = triangle count
(2^-22 is four ulp of the 0.5 that bounds each triangle's term Omega / 4 pi)."""
import ctypes as C
import functools

import numpy as np
import pytest

from pies_amd import capi
from test_skin import box_surface

TILE = 256  # kVoxelTile of pies_amd/csrc/voxel_kernels.h: triangles staged in LDS at a time
TRIANGLE_COUNTS = [1, 63, 65, 255, 256, 257, 1025]  # either side of the tile, of a wavefront, more than one tile
LATTICES = [(1, 1, 1), (3, 5, 7), (9, 8, 7)]  # 1, 105 and 504 samples: one lane, straddling a wavefront, straddling a workgroup
SHIFT = np.float32([-7.3, -5.1, -3.7])  # the translation to negative coordinates


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def box_triangles(count, lo=(0.13, 0.21, 0.34), hi=(1.9, 1.6, 2.1)):
    """The first `count` triangles of the coarsest subdivided box surface that has as many (open unless count = 12 n^2)"""
    n = 1
    while 12 * n * n < count:
        n += 1
    v, t = box_surface(lo, hi, n)
    return v, t[:count].copy()


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """20 x 4^level triangles on the sphere, wound outward"""
    f = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, f, 0), (1, f, 0), (-1, -f, 0), (1, -f, 0), (0, -1, f), (0, 1, f), (0, -1, -f), (0, 1, -f), (f, 0, -1), (f, 0, 1), (-f, 0, -1), (-f, 0, 1)]
    v = [np.float64(p) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return (np.float64(centre) + radius * np.asarray(v)).astype(np.float32), np.asarray(t, np.uint32)


def torus(nu=16, nv=12, R=1.0, r=0.4, centre=(0.0, 0.0, 0.0)):
    """A torus around the y axis (genus 1), 2 nu nv triangles, wound outward"""
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    p = np.stack([(R + r * np.cos(w)) * np.cos(u), r * np.sin(w), (R + r * np.cos(w)) * np.sin(u)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    q = [((i + di) % nu) * nv + (j + dj) % nv for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1))]
    t = np.concatenate([np.stack([q[0], q[2], q[1]], -1).reshape(-1, 3), np.stack([q[0], q[3], q[2]], -1).reshape(-1, 3)])
    return (np.float64(centre) + p).astype(np.float32), t.astype(np.uint32)


def hemisphere(level=2):
    """The icosphere's triangles whose centroid lies above its equator: an OPEN surface, so w is fractional"""
    v, t = icosphere(level, 1.0, (1.0, 1.0, 1.0))
    return v, t[v[t][:, :, 1].mean(1) > 1.0].copy()


def thin_plate():
    """A closed plate 1.6 x 0.02 x 1.2, turned 40 degrees about z: thinner than any cell of a resolution-4 lattice"""
    v, t = box_surface((-0.8, -0.01, -0.6), (0.8, 0.01, 0.6), 8)
    a = np.deg2rad(40.0)
    rot = np.float64([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return (v.astype(np.float64) @ rot.T + [0.3, 2.0, 0.1]).astype(np.float32), t


# ---- the winding number ------------------------------------------------------------------------------------------------------------
def centres(origin, cell, dims, dtype):
    """Cell centres origin + ((i, j, k) + 0.5) cell as (nx ny nz, 3), k fastest, every operation in `dtype`"""
    o, c = np.asarray(origin, dtype), dtype(cell)
    ax = [o[a] + (np.arange(dims[a]).astype(dtype) + dtype(0.5)) * c for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    assert g.dtype == dtype
    return g


def _terms(c, a, b, d):
    """Omega of every (sample, triangle) pair for corner arrays broadcast against the samples, in the operands' precision,
    every product and sum rounded in the order k_winding runs them"""
    A, B, D = a - c, b - c, d - c
    x, y, z = 0, 1, 2
    la = np.sqrt(A[..., x] * A[..., x] + A[..., y] * A[..., y] + A[..., z] * A[..., z])
    lb = np.sqrt(B[..., x] * B[..., x] + B[..., y] * B[..., y] + B[..., z] * B[..., z])
    ld = np.sqrt(D[..., x] * D[..., x] + D[..., y] * D[..., y] + D[..., z] * D[..., z])
    num = (A[..., x] * (B[..., y] * D[..., z] - D[..., y] * B[..., z]) - B[..., x] * (A[..., y] * D[..., z] - D[..., y] * A[..., z])
           + D[..., x] * (A[..., y] * B[..., z] - B[..., y] * A[..., z]))
    ab = A[..., x] * B[..., x] + A[..., y] * B[..., y] + A[..., z] * B[..., z]
    bd = B[..., x] * D[..., x] + B[..., y] * D[..., y] + B[..., z] * D[..., z]
    da = D[..., x] * A[..., x] + D[..., y] * A[..., y] + D[..., z] * A[..., z]
    den = la * lb * ld + ab * ld + bd * la + da * lb
    with np.errstate(invalid="ignore"):
        om = c.dtype.type(2.0) * np.arctan2(num, den)
    om[((num == 0) & (den == 0)) | ~np.isfinite(om)] = 0
    assert om.dtype == c.dtype
    return om


def winding64(v, tri, origin, cell, dims):
    """w at the cell centres in fp64, shaped dims"""
    c = centres(np.float32(origin), np.float32(cell), dims, np.float64)  # (the lattice itself is fp32 data)
    p = np.asarray(v, np.float32).astype(np.float64)[tri]  # (T, 3, 3)
    w = np.zeros(len(c))
    for k in range(0, len(tri), 512):
        q = p[k:k + 512]
        w += _terms(c[:, None, :], q[None, :, 0], q[None, :, 1], q[None, :, 2]).sum(1)
    return (w / (4.0 * np.pi)).reshape(dims)


def winding32(v, tri, origin, cell, dims):
    """The same in fp32 in the kernel's order: one running sum per sample over the triangles in ascending index"""
    c = centres(np.float32(origin), np.float32(cell), dims, np.float32)
    p = np.asarray(v, np.float32)[tri]
    s = np.zeros(len(c), np.float32)
    for t in range(len(tri)):
        s = s + _terms(c, p[t, 0][None], p[t, 1][None], p[t, 2][None])
    w = s / np.float32(12.566370614359172)
    assert w.dtype == np.float32
    return w.reshape(dims)


def gate_of(w32, w64, n_triangles):
    err = float(np.abs(w32.astype(np.float64) - w64).max())
    return max(2.0 * err, n_triangles * 2.0 ** -22), err


def value_lattice(dims, shift=None):
    """The lattice of the value tests over box_triangles' box: generic numbers, no cell centre in a face's plane"""
    origin = np.float32([-0.05, -0.07, -0.03]) + (0 if shift is None else shift)
    return origin.astype(np.float32), np.float32(2.4) / np.float32(max(dims))


@functools.lru_cache(maxsize=None)
def value_case(count, dims, shifted=False):
    """(vertices, triangles, origin, cell, w64, gate, fp32 error) of one value test; computed once per session, read-only"""
    v, tri = box_triangles(count)
    if shifted:
        v = (v + SHIFT).astype(np.float32)
    origin, cell = value_lattice(dims, SHIFT if shifted else None)
    w64 = winding64(v, tri, origin, cell, dims)
    gate, err = gate_of(winding32(v, tri, origin, cell, dims), w64, len(tri))
    for a in (v, tri, origin, w64):
        a.setflags(write=False)
    return v, tri, origin, cell, w64, gate, err


@functools.lru_cache(maxsize=None)
def hemisphere_case():
    v, tri = hemisphere()
    dims = (3, 5, 7)
    origin, cell = np.float32([-0.13, -0.21, -0.17]), np.float32(0.33)
    w64 = winding64(v, tri, origin, cell, dims)
    gate, err = gate_of(winding32(v, tri, origin, cell, dims), w64, len(tri))
    return v, tri, origin, cell, dims, w64, gate, err


CLOSED = {  # name -> (mesh, lattice dims <= 12 per axis, origin, cell): lattices placed so that no cell centre lies on a surface
    "box": (lambda: box_surface((0.13, 0.21, 0.34), (1.9, 1.6, 2.1), 2), (11, 9, 12), (-0.11, -0.02, 0.07), 0.193),
    "icosphere": (lambda: icosphere(2, 1.0, (0.2, 1.3, -0.1)), (12, 11, 12), (-0.93, 0.17, -1.21), 0.197),
    "torus": (lambda: torus(centre=(0.1, 0.9, 0.3)), (12, 5, 12), (-1.43, 0.41, -1.19), 0.251),
}


@functools.lru_cache(maxsize=None)
def closed_case(name):
    make, dims, origin, cell = CLOSED[name]
    v, tri = make()
    origin, cell = np.float32(origin), np.float32(cell)
    return v, tri, origin, cell, dims, winding64(v, tri, origin, cell, dims)


BODIES = {  # name -> (mesh, resolution) of the body tests
    "icosphere": (lambda: icosphere(2, 1.0, (0.2, 2.6, -0.1)), 6),
    "torus": (lambda: torus(centre=(0.1, 1.9, 0.3)), 6),
    "box": (lambda: box_surface((0.5, 1.0, 0.25), (2.5, 2.0, 1.25), 2), 4),
}


# ---- the body's rules ------------------------------------------------------------------------------------------------------------
def lattice_of(v, resolution):
    """(origin float32[3], cell float32, dims) of pies_add_tri_mesh_volume, every operation in fp32"""
    v = np.asarray(v, np.float32)
    lo, hi = v.min(0), v.max(0)
    extent = hi - lo
    cell = extent.max() / np.float32(resolution)
    n = np.maximum(np.float32(1.0), np.ceil(extent / cell))
    origin = lo - np.float32(0.5) * (n * cell - extent)
    assert origin.dtype == np.float32 and cell.dtype == np.float32
    return origin, cell, tuple(int(x) for x in n)


def kept_cells(inside, v, origin, cell, dims):
    """|w| > 0.5 (the mask given) or a cell that holds an input vertex, the vertex's cell being floor((v - origin) / cell) clamped
    to the lattice"""
    keep = np.array(inside, bool).reshape(dims)
    c = np.floor((np.asarray(v, np.float32) - origin) / cell)
    assert c.dtype == np.float32
    c = np.clip(c, 0, np.float32(dims) - 1).astype(np.int64)
    keep[c[:, 0], c[:, 1], c[:, 2]] = True
    return keep


def lattice_nodes(keep, origin, cell):
    """(positions (n, 3) float32, index grid (nx + 1, ny + 1, nz + 1) with -1 for unused points): the lattice points that are a
    corner of a kept cell, numbered in ascending (i, j, k), k fastest"""
    nx, ny, nz = keep.shape
    used = np.zeros((nx + 1, ny + 1, nz + 1), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                used[di:di + nx, dj:dj + ny, dk:dk + nz] |= keep
    index = np.full(used.shape, -1, np.int64)
    index[used] = np.arange(used.sum())  # boolean indexing runs in C order: k fastest
    ijk = np.argwhere(used).astype(np.float32)
    pos = origin[None, :] + ijk * cell
    assert pos.dtype == np.float32
    return pos, index


def six_tets(keep, index):
    """The six tetrahedra of pies_create_tet_box per kept cell, cells in ascending index"""
    out = []
    for i, j, k in np.argwhere(keep):
        n = {(a, b, c): index[i + a, j + b, k + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)}
        n000, n001, n010, n011, n100, n101, n110, n111 = (n[corner] for corner in sorted(n))
        out += [(n000, n001, n011, n111), (n000, n010, n011, n111), (n000, n001, n101, n111),
                (n000, n100, n101, n111), (n000, n010, n110, n111), (n000, n100, n110, n111)]
    return np.asarray(out, np.uint32).reshape(-1, 4)


def boundary(pos, tets):
    """Every element face that belongs to exactly one element, wound so that the normal points away from the element's fourth
    vertex; elements in order, faces opposite vertex 0, 1, 2, 3"""
    faces = np.int64([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])
    t = np.asarray(tets, np.int64)
    f = t[:, faces].reshape(-1, 3)                   # (4 m, 3), element-major
    opposite = t.reshape(-1)                         # vertex f of element e at 4 e + f
    _, inverse, counts = np.unique(np.sort(f, 1), axis=0, return_inverse=True, return_counts=True)
    once = counts[inverse.reshape(-1)] == 1
    f, opposite = f[once], opposite[once]
    p = np.asarray(pos, np.float64)
    normal = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    flip = (normal * (p[opposite] - p[f[:, 0]])).sum(1) > 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return f.astype(np.uint32)


def body_of(inside, v, resolution):
    """The whole restatement from an inside mask: dict of origin, cell, dims, keep, positions, tets, triangles (local ids)"""
    origin, cell, dims = lattice_of(v, resolution)
    keep = kept_cells(inside, v, origin, cell, dims)
    pos, index = lattice_nodes(keep, origin, cell)
    tets = six_tets(keep, index)
    return dict(origin=origin, cell=cell, dims=dims, keep=keep, positions=pos, tets=tets, triangles=boundary(pos, tets))


def triangle_set(tri):
    """Triangles as a sorted array of triples, each rotated (orientation kept) so that its smallest id comes first"""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    r = t.argmin(1)
    t = np.stack([t[np.arange(len(t)), (r + k) % 3] for k in range(3)], 1)
    return t[np.lexsort(t.T[::-1])]


# ---- the restatements against each other and against the library's own lattice ---------------------------------------------------------
def host_solver(solver=capi.PD):
    return capi.Solver(capi.Options(solver=solver, iterations=4), device=capi.DEVICE_NONE)


def test_split_and_boundary_match_create_tet_box():
    """A full 4 x 2 x 3-cell block through six_tets and boundary equals pies_create_tet_box's elements and surface triangles"""
    keep = np.ones((4, 2, 3), bool)
    pos, index = lattice_nodes(keep, np.float32([0.5, 1.0, 0.25]), np.float32(0.5))
    g = host_solver()
    g.create_tet_box(5, 3, 4, translation=(0.5, 1.0, 0.25), scale=0.5, volume=False, triangles=True)
    assert np.array_equal(g.positions, pos) and np.array_equal(index.reshape(-1), np.arange(60))
    tets = six_tets(keep, index)
    assert np.array_equal(g.ids(capi.TET), tets)
    assert np.array_equal(triangle_set(g.ids(capi.TRIANGLES)), triangle_set(boundary(pos, tets)))


def test_node_numbering_skips_unused_points():
    keep = np.zeros((2, 2, 2), bool)
    keep[0, 0, 0] = keep[1, 1, 1] = True  # two cells that share one lattice point
    pos, index = lattice_nodes(keep, np.float32([0, 0, 0]), np.float32(1.0))
    assert len(pos) == 15 and (index >= 0).sum() == 15 and index[1, 1, 1] == 7
    assert (np.diff(index[index >= 0]) == 1).all()
    tets = six_tets(keep, index)
    tri = boundary(pos, tets)
    assert len(tets) == 12 and len(tri) == 24  # two separate cubes' surfaces
    centre = pos[tets].astype(np.float64).mean(1)
    vol = np.abs(np.linalg.det(pos[tets[:, 1:]].astype(np.float64) - pos[tets[:, :1]].astype(np.float64))) / 6
    assert abs(vol.sum() - 2.0) < 1e-12 and len(centre) == 12


def test_vertex_clause_keeps_cells_the_winding_misses():
    v, _ = thin_plate()
    origin, cell, dims = lattice_of(v, 4)
    none = np.zeros(dims, bool)
    keep = kept_cells(none, v, origin, cell, dims)
    assert keep.any() and not none.any()
    c = np.floor((v - origin) / cell).astype(int)
    assert keep[tuple(np.clip(c, 0, np.array(dims) - 1).T)].all()


def test_lattice_rule():
    v, _ = BODIES["box"][0]()
    origin, cell, dims = lattice_of(v, 4)
    assert dims == (4, 2, 2) and cell == np.float32(0.5) and np.array_equal(origin, np.float32([0.5, 1.0, 0.25]))
    for name in ("icosphere", "torus"):
        v, _ = BODIES[name][0]()
        origin, cell, dims = lattice_of(v, BODIES[name][1])
        lo, hi = v.min(0), v.max(0)
        assert max(dims) in (6, 7) and (origin <= lo + 1e-6).all() and (origin + np.float32(dims) * cell >= hi - 1e-6).all()


# ---- the conditions the GPU tests rely on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", LATTICES)
@pytest.mark.parametrize("count", TRIANGLE_COUNTS)
def test_fp32_restatement_stays_inside_the_gate(count, dims):
    v, tri, origin, cell, w64, gate, err = value_case(count, dims)
    assert len(tri) == count
    print("T %d lattice %s: |w32 - w64| = %.3g, gate %.3g" % (count, dims, err, gate))
    assert err <= gate
    assert gate < 0.05  # fp32 rounding is far from moving a sample across a classification margin


def test_fp32_restatement_shifted_and_hemisphere():
    for err, gate in (value_case(257, (3, 5, 7), True)[5:][::-1], hemisphere_case()[6:][::-1]):
        assert err <= gate < 0.05
    w64 = hemisphere_case()[5]
    frac = np.abs(w64 - np.round(w64))
    assert (frac > 0.02).mean() > 0.5  # an open surface: w is fractional, the value is what is tested
    assert np.abs(value_case(257, (3, 5, 7), True)[4] - value_case(257, (3, 5, 7))[4]).max() < 1e-3  # the same samples, moved


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_meshes_have_no_sample_near_the_threshold(name):
    v, tri, origin, cell, dims, w64 = closed_case(name)
    assert max(dims) <= 12
    margin = float(np.abs(np.abs(w64) - 0.5).min())
    print("%s: %d triangles, %d of %d samples inside, min ||w| - 0.5| = %.3g" % (name, len(tri), (np.abs(w64) > 0.5).sum(), w64.size, margin))
    assert margin >= 0.05
    assert np.abs(w64 - np.round(w64)).max() < 1e-9  # closed: an integer away from the surface
    inside = np.abs(w64) > 0.5
    assert inside.any() and not inside.all()
    w32 = winding32(v, tri, origin, cell, dims)
    assert np.array_equal(np.abs(w32) > 0.5, inside)
    assert name != "torus" or not inside[:, dims[1] // 2, :][dims[0] // 2 - 1:dims[0] // 2 + 1, dims[2] // 2 - 1:dims[2] // 2 + 1].any()  # the hole


@pytest.mark.parametrize("name", sorted(BODIES))
def test_body_lattices_have_no_centre_near_the_threshold(name):
    v, tri = BODIES[name][0]()
    origin, cell, dims = lattice_of(v, BODIES[name][1])
    w64 = winding64(v, tri, origin, cell, dims)
    assert float(np.abs(np.abs(w64) - 0.5).min()) >= 0.05


# ---- host-only handles ---------------------------------------------------------------------------------------------------------------
def counts(g):
    return tuple(g.count(k) for k in (capi.NODES, capi.POSITION, capi.DISTANCE, capi.TET, capi.VOLUME, capi.BEND, capi.TRIANGLES,
                                      capi.SKINS, capi.SKIN_VERTICES))


def raw_voxelize(g, v, tri, origin, cell, dims, nv=None, nt=None, null=()):
    v, tri, o, d = capi._f32(v), capi._u32(tri), capi._f32(origin), capi._u32(dims)
    arg = dict(v=capi._pf(v), tri=capi._pu(tri), o=capi._pf(o), d=capi._pu(d))
    for k in null:
        arg[k] = None
    return g._L.pies_voxelize_tri_mesh(g._h, len(v) if nv is None else nv, arg["v"], len(tri) if nt is None else nt, arg["tri"], arg["o"],
                                       cell, arg["d"], None, None)  # (no output: none of these calls gets as far as writing one)


def raw_add(g, v, tri, resolution=4, density=1.0, null=()):
    v, tri, vel = capi._f32(v), capi._u32(tri), np.zeros(3, np.float32)
    arg = dict(v=capi._pf(v), tri=capi._pu(tri), vel=capi._pf(vel))
    for k in null:
        arg[k] = None
    return g._L.pies_add_tri_mesh_volume(g._h, len(v), arg["v"], len(tri), arg["tri"], arg["vel"], density, 1.0, 0.8, 1.0, 1.0, 1.0, 1.0,
                                         resolution, None, None, None, None)


def test_host_only_handle_and_invalid_arguments():
    g = host_solver()
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5), w=1.0)
    before = counts(g)
    v, tri = icosphere(1)
    origin, cell, dims = np.float32([-1.1, -1.1, -1.1]), 0.55, (4, 4, 4)
    assert raw_voxelize(g, v, tri, origin, cell, dims) == capi.ERR_HIP
    assert "host-only" in g.last_error()
    assert raw_add(g, v, tri) == capi.ERR_HIP
    bad_index, bad_vertex = tri.copy(), v.copy()
    bad_index[5, 1] = len(v)
    bad_vertex[3, 2] = np.nan
    inf_vertex = v.copy()
    inf_vertex[0, 0] = np.inf
    for rc in (raw_voxelize(g, v, tri, origin, cell, dims, null=("v",)), raw_voxelize(g, v, tri, origin, cell, dims, null=("tri",)),
               raw_voxelize(g, v, tri, origin, cell, dims, null=("o",)), raw_voxelize(g, v, tri, origin, cell, dims, null=("d",)),
               raw_voxelize(g, v, bad_index, origin, cell, dims), raw_voxelize(g, bad_vertex, tri, origin, cell, dims),
               raw_voxelize(g, v, tri, origin, 0.0, dims), raw_voxelize(g, v, tri, origin, float("nan"), dims),
               raw_voxelize(g, v, tri, origin, cell, (4, 0, 4)), raw_voxelize(g, v, tri, origin, cell, dims, nt=0),
               raw_add(g, v, tri, null=("v",)), raw_add(g, v, tri, null=("tri",)), raw_add(g, v, tri, null=("vel",)),
               raw_add(g, v, bad_index), raw_add(g, bad_vertex, tri), raw_add(g, inf_vertex, tri), raw_add(g, v, tri, resolution=0),
               raw_add(g, v, tri, density=0.0), raw_add(g, v, tri, density=-1.0), raw_add(g, v, tri, density=float("nan")),
               raw_add(g, np.tile(v[:1], (len(v), 1)), tri)):  # a zero extent
        assert rc == capi.ERR_INVALID, g.last_error()
        assert g.last_error() != ""
    # the limits are checked before the device
    assert raw_voxelize(g, v, tri, origin, cell, (1 << 9, 1 << 9, (1 << 8) + 1)) == capi.ERR_UNSUPPORTED
    assert raw_voxelize(g, v, tri, origin, cell, (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert raw_voxelize(g, v, tri, origin, cell, (1 << 9, 1 << 9, 1 << 8)) == capi.ERR_HIP  # exactly 2^26 samples
    assert raw_add(g, v, tri, resolution=4096) == capi.ERR_UNSUPPORTED
    assert g._L.pies_voxelize_tri_mesh(None, 0, None, 0, None, None, 1.0, None, None, None) == capi.ERR_INVALID
    assert counts(g) == before
    g.finalize()  # the scene still builds
    assert counts(g) == before


def test_triangle_counts_straddle_the_kernels_tile():
    import os
    import re
    header = open(os.path.join(os.path.dirname(capi.HERE), "pies_amd", "csrc", "voxel_kernels.h")).read()
    assert int(re.search(r"kVoxelTile = (\d+)", header).group(1)) == TILE
    assert {1, 63, 65, 257, 1025, TILE - 1, TILE, TILE + 1} <= set(TRIANGLE_COUNTS)


def test_binding_declares_both_entry_points():
    L = capi.load()
    assert L.pies_voxelize_tri_mesh.argtypes[-1] == C.POINTER(C.c_uint8) and len(L.pies_add_tri_mesh_volume.argtypes) == 18
    assert L.pies_abi_version() == 4
