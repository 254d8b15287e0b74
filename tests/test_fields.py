"""CPU tests of the signed distance fields and field props (pies_add_field, pies_add_field_tri_mesh, pies_get_field,
pies_collide_field_props): the numpy fp32 restatements of the rules of include/pies_hip.h - `build_field`, made of
test_nearest.nearest and winding32, and `collide_fields`, whose response is test_props.collide's -, the yardsticks the device has
to match bit for bit in tests/test_fields_gpu.py; known answers with exact binary values; the accuracy of the rule itself; and the
entry points on a host-only handle.

Accuracy of the rule (test_one_step_lands_on_the_level_set): the field of a unit icosphere (320 triangles) built by `build_field`
with cell = 0.125 and margin = 0.375, 4 096 nodes of radius 0.05 between 0.3 and 1.3 from the centre pushed by a prop of radius
0.1 (R = 0.15).  The largest | fp64 brute-force distance of q to the mesh - R | measured 0.2036 of a cell (MEASURED_CELLS); the gate
is four times that rounded up to a power of two: one cell (GATE_CELLS).  The figure is the one-step rule's on a trilinear interpolant of a faceted
sphere, not rounding (fp32 contributes 1e-6 of a cell): the deepest nodes, 0.3 from the centre where the field's curvature is
three cells, travel 0.85 along a gradient that is a difference over one cell."""
import ctypes as C
import functools

import numpy as np
import pytest

from pies_amd import capi
from test_nearest import distance64, nearest, winding32, winding64
from test_props import F, NONE, TILE, _cross, _dot, _fmaxf, _q16, _rotation, _vec
from test_raycast import turned_box

MEASURED_CELLS = 0.2036  # see the module docstring
GATE_CELLS = 1.0

# what a (node, prop) pair came to (collide_fields(..., trace=[])): what the GPU test asserts the coverage of
C_FIXED, C_OUTSIDE, C_NAN_CELL, C_UNTOUCHED, C_TOUCH, C_TOUCH_FLAT = 0, 1, 2, 3, 4, 5
C_AWAY = 8  # added to a touch with vn > 0
ALL_CASES = {C_FIXED, C_OUTSIDE, C_NAN_CELL, C_UNTOUCHED, C_TOUCH, C_TOUCH_FLAT, C_TOUCH + C_AWAY}


# ---- the restatements: fp32, no fused multiply-adds, the operation order of the header -------------------------------------------
def lattice_points(dims, origin, cell):
    """(n, 3) local positions of the samples in storage order (i fastest): origin + (float)index * cell, the product rounded first"""
    nx, ny, nz = (int(d) for d in dims)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    o, c = np.asarray(origin, F), F(cell)
    p = np.stack([o[0] + i.astype(F) * c, o[1] + j.astype(F) * c, o[2] + k.astype(F) * c], axis=-1).reshape(-1, 3)
    assert p.dtype == np.float32
    return p


def field_lattice(P, cell, margin):
    """(dims (nx, ny, nz), origin) of pies_add_field_tri_mesh's lattice, in fp32"""
    P, cell, margin = np.asarray(P, F), F(cell), F(margin)
    lo, hi = P.min(0), P.max(0)
    origin = lo - margin
    cells = np.ceil(((hi + margin) - origin) / cell)
    assert origin.dtype == np.float32 and cells.dtype == np.float32
    return tuple(max(2, int(c) + 1) for c in cells), origin


def build_field(P, tris, cell, margin, chunk=4096):
    """pies_add_field_tri_mesh in numpy fp32: (samples (nz, ny, nx), origin, cell, winding number per sample (nz, ny, nx)).
    |sample| = sqrtf(dd) of test_nearest.nearest, the sign from test_nearest.winding32."""
    dims, origin = field_lattice(P, cell, margin)
    pts = lattice_points(dims, origin, cell)
    dist = np.concatenate([nearest(pts[a:a + chunk], P, tris)[1] for a in range(0, len(pts), chunk)])
    w = winding32(pts, P, tris)
    samples = np.where(np.abs(w) > F(0.5), -dist, dist).astype(F)
    shape = dims[::-1]
    return samples.reshape(shape), origin, F(cell), w.reshape(shape)


def _lerp(a, b, f):
    return a + (b - a) * f


def _field_contact(P, field, p, r):
    """(touched, n, q, case) of field prop P, field = (samples (nz, ny, nx), origin, cell), for the nodes at p (m x 3), radii r"""
    samples, origin, cell = field
    samples, origin, cell = np.asarray(samples, F), np.asarray(origin, F), F(cell)
    nz, ny, nx = samples.shape
    dims = (nx, ny, nz)
    R = F(P.radius) + r
    ax = _vec(P.axes).reshape(3, 3)
    d = p - _vec(P.centre)[None]
    g = [(_dot(ax[j][None], d) - origin[j]) / cell for j in range(3)]
    inside = np.ones(len(p), bool)
    for j in range(3):
        inside &= (g[j] >= F(0)) & (g[j] < F(dims[j] - 1))
    i = [np.where(inside, g[j], F(0)).astype(np.uint32).astype(np.int64) for j in range(3)]
    f = [g[j] - i[j].astype(F) for j in range(3)]
    s = [[[samples[i[2] + c, i[1] + b, i[0] + a] for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]  # s[a][b][c]
    m = [[_lerp(s[0][b][c], s[1][b][c], f[0]) for c in (0, 1)] for b in (0, 1)]  # m[b][c]
    phi = _lerp(_lerp(m[0][0], m[1][0], f[1]), _lerp(m[0][1], m[1][1], f[1]), f[2])
    touched = inside & (phi < R)
    D = [[s[1][b][c] - s[0][b][c] for c in (0, 1)] for b in (0, 1)]  # over b by f_1, then over c by f_2
    G0 = _lerp(_lerp(D[0][0], D[1][0], f[1]), _lerp(D[0][1], D[1][1], f[1]), f[2])
    E = [[s[a][1][c] - s[a][0][c] for c in (0, 1)] for a in (0, 1)]  # over a by f_0, then over c by f_2
    G1 = _lerp(_lerp(E[0][0], E[1][0], f[0]), _lerp(E[0][1], E[1][1], f[0]), f[2])
    H = [[s[a][b][1] - s[a][b][0] for b in (0, 1)] for a in (0, 1)]  # over a by f_0, then over b by f_1
    G2 = _lerp(_lerp(H[0][0], H[1][0], f[0]), _lerp(H[0][1], H[1][1], f[0]), f[1])
    G = np.stack([G0, G1, G2], axis=1)
    GG = _dot(G, G)
    steep = GG > 0
    nl = np.where(steep[:, None], G / np.sqrt(np.where(steep, GG, F(1)))[:, None], F([0.0, 1.0, 0.0])[None]).astype(F)
    n = (ax[0][None] * nl[:, 0:1] + ax[1][None] * nl[:, 1:2]) + ax[2][None] * nl[:, 2:3]
    q = p + n * (R - phi)[:, None]
    for x in (phi, GG, n, q):
        assert x.dtype == np.float32
    nan_cell = inside & np.isnan(sum(s[a][b][c] for a in (0, 1) for b in (0, 1) for c in (0, 1)))
    case = np.where(~inside, C_OUTSIDE, np.where(nan_cell, C_NAN_CELL, np.where(~touched, C_UNTOUCHED, np.where(steep, C_TOUCH, C_TOUCH_FLAT))))
    return touched, n, q, case


def collide_fields(pos, prev, vel, radius, inv_mass, props, fields, trace=None):
    """The rule of pies_collide_field_props in numpy fp32; fields[id] = (samples (nz, ny, nx), origin, cell).  Returns what
    test_props.collide returns: (pos, prev, vel, impulse, torque, hits, node_prop), the response and the two-level sums being its.
    trace: a list that receives (prop, case codes of all nodes) per prop."""
    with np.errstate(all="ignore"):
        pos, prev, vel = (np.array(a, F).reshape(-1, 3).copy() for a in (pos, prev, vel))
        radius, inv_mass = np.asarray(radius, F).reshape(-1), np.asarray(inv_mass, F).reshape(-1)
        n, k = len(pos), len(props)
        J, T = np.zeros((k, n, 3), F), np.zeros((k, n, 3), F)
        touched_by = np.zeros((k, n), bool)
        node_prop = np.full(n, NONE, np.uint32)
        movable = ~(inv_mass == 0)
        for i, P in enumerate(props):
            t, nn, q, case = _field_contact(P, fields[P.field], pos, radius)
            t = t & movable
            arm = q - _vec(P.pivot)[None]
            u = _vec(P.velocity)[None] + _cross(_vec(P.angular)[None], arm)
            rel = vel - u
            vn = _dot(rel, nn)
            tang = rel - nn * vn[:, None]
            v1 = u + (tang * (F(1) - F(P.friction)) + nn * _fmaxf(vn, F(0))[:, None])
            j = (vel - v1) * (F(1) / np.where(movable, inv_mass, F(1)))[:, None]
            tq = _cross(arm, j)
            J[i][t], T[i][t] = j[t], tq[t]
            pos[t], prev[t], vel[t] = q[t], q[t], v1[t]
            node_prop[t] = i
            touched_by[i] = t
            if trace is not None:
                trace.append((i, np.where(movable, case + C_AWAY * (t & (vn > 0)), C_FIXED)))
        impulse, torque = np.zeros((k, 3), F), np.zeros((k, 3), F)
        for first in range(0, n, TILE):
            si, st = np.zeros((k, 3), F), np.zeros((k, 3), F)
            for node in range(first, min(first + TILE, n)):
                si, st = si + J[:, node], st + T[:, node]  # (an untouched node adds 0)
            impulse, torque = impulse + si, torque + st
        return pos, prev, vel, impulse, torque, touched_by.sum(axis=1).astype(np.uint32), node_prop


def cases_of(trace):
    """(the set of case codes seen, the most props that touched one node)"""
    codes = np.stack([c for _, c in trace])
    touches = ((codes & 7) >= C_TOUCH).sum(0)
    return {int(c) for c in np.unique(codes)}, int(touches.max())


# ---- fields and scenes (shared with tests/test_fields_gpu.py) ---------------------------------------------------------------------
def box_mesh():
    """test_raycast.turned_box() with y scaled by 0.8: 432 triangles, so that the winding sum crosses a 256-triangle tile"""
    P, tri = turned_box()
    return (P * F([1.0, 0.8, 1.0])).astype(F), tri


@functools.lru_cache(maxsize=None)
def box_field(cell=0.37, margin=0.6):
    return build_field(*box_mesh(), cell, margin)


def sphere_field(n=12, cell=0.25, radius=0.8):
    """a host-sampled sphere about the local origin: (samples (n, n, n), origin, cell)"""
    origin = F([-0.5 * (n - 1) * cell] * 3)
    p = lattice_points((n, n, n), origin, cell).astype(np.float64)
    return (np.linalg.norm(p, axis=1) - radius).astype(F).reshape(n, n, n), origin, F(cell)


PLATEAU_CELL, NAN_SAMPLE = (1, 1, 1), (4, 3, 2)


def crafted_field():
    """a 6 x 5 x 4 lattice of a tilted plane with ripples; the eight corners of cell PLATEAU_CELL are all -0.25 (GG == 0 inside it)
    and sample NAN_SAMPLE is a NaN (the eight cells around it touch nothing)"""
    dims, origin, cell = (6, 5, 4), F([-1.25, -1.0, -0.75]), F(0.5)
    p = lattice_points(dims, origin, cell).astype(np.float64)
    v = (0.8 * p[:, 1] + 0.3 * p[:, 0] - 0.2 * p[:, 2] + 0.05 * np.sin(3.0 * p[:, 0] + 1.0) - 0.1).astype(F).reshape(dims[::-1])
    i, j, k = PLATEAU_CELL
    v[k:k + 2, j:j + 2, i:i + 2] = F(-0.25)
    i, j, k = NAN_SAMPLE
    v[k, j, i] = F(np.nan)
    return v, origin, cell


def host_fields():
    """the fields of the shared scenes that the host samples: ids 1 and 2 (id 0 is the mesh-built box)"""
    return [sphere_field(), crafted_field()]


def _extent(field):
    samples, origin, cell = field
    return np.asarray(origin, np.float64), (np.array(samples.shape[::-1], np.float64) - 1) * float(cell)


def make_field_props(n_props, fields, seed=0):
    """prop k places field k % 3 in a turned, moving frame; prop 2 m + 1 overlaps prop 2 m"""
    rng = np.random.default_rng(2000 + seed)
    props, place = [], None
    for k in range(n_props):
        field = k % len(fields)
        o, ext = _extent(fields[field])
        axes = np.eye(3, dtype=F) if k == 2 else _rotation(rng)
        place = _q16(rng.uniform(-5, 5, 3)) if k % 2 == 0 else place + np.array([0.5, 0.25, 0.0])
        centre = place - axes.astype(np.float64).T @ (o + 0.5 * ext)  # the lattice's middle comes to `place`
        props.append(capi.FieldProp.make(field, centre, axes=axes, radius=float(_q16(rng.uniform(0.0, 0.4))),
                                         velocity=rng.normal(size=3) * 2, angular=rng.normal(size=3),
                                         pivot=place + rng.normal(size=3) * 0.5, friction=[0.0, 0.25, 1.0, float(F(rng.uniform()))][k % 4]))
    return props


def _world(P, local):
    return np.array(list(P.centre), np.float64) + np.array(list(P.axes), np.float64).reshape(3, 3).T @ np.asarray(local, np.float64)


def make_field_scene(n_nodes, n_props, fields, seed=0):
    """(pos, vel, radius, inv_mass, props): every node is thrown into the lattice box of one prop grown by 15 % (most inside it,
    some outside), with random velocity, radius in {0, 0.1, 0.5}, invMass in {0, 0.5, 1}; one node in seven is placed by
    construction with a non-zero invMass - in the plateau cell and beside the NaN sample of a prop of the crafted field"""
    rng = np.random.default_rng(seed * 7919 + n_nodes * 31 + n_props)
    props = make_field_props(n_props, fields, seed)
    pos = np.zeros((n_nodes, 3), F)
    for i in range(n_nodes):
        P = props[int(rng.integers(n_props))]
        o, ext = _extent(fields[P.field])
        pos[i] = _world(P, o + ext * rng.uniform(-0.15, 1.15, 3)).astype(F)
    vel = (rng.normal(size=(n_nodes, 3)) * 3).astype(F)
    radius = rng.choice(np.array([0.0, 0.1, 0.5], F), n_nodes)
    inv_mass = rng.choice(np.array([0.0, 0.5, 1.0], F), n_nodes)
    special = []
    for P in props:
        if P.field == 2:
            _, origin, cell = fields[2]
            for cell_index, r in ((PLATEAU_CELL, 0.0), (NAN_SAMPLE, 0.5)):
                special.append((_world(P, np.asarray(origin, np.float64) + (np.array(cell_index) + [0.5, 0.375, 0.25]) * float(cell)), r))
    for m, i in enumerate(range(0, n_nodes, 7)):
        if special:
            p, r = special[m % len(special)]
            pos[i], radius[i], inv_mass[i] = p.astype(F), F(r), F(1.0 if m % 2 else 0.5)
    return pos, vel, radius, inv_mass, props


def test_every_case_occurs_in_the_shared_scenes():
    fields = [box_field()[:3]] + host_fields()
    for n_nodes in (255, 257, 600):
        for n_props in (3, 64):
            pos, vel, radius, inv_mass, props = make_field_scene(n_nodes, n_props, fields)
            trace = []
            out = collide_fields(pos, pos, vel, radius, inv_mass, props, fields, trace=trace)
            seen, most = cases_of(trace)
            assert ALL_CASES <= seen and most >= 2, (n_nodes, n_props, sorted(ALL_CASES - seen), most)
            assert (out[6] == NONE).any() and (out[6] != NONE).any()
            assert np.isfinite(out[0]).all() and np.isfinite(out[2]).all()


# ---- the build ------------------------------------------------------------------------------------------------------------------------
def test_the_build_lattices_of_the_gpu_test():
    """19 x 16 x 13 and 18 x 15 x 12: pairwise distinct dims; the fp32 signs equal the fp64 signs on every sample and no sample
    lies in the band 0.25 < |w| < 0.75 that the GPU test leaves out of the sign comparison"""
    P, tri = box_mesh()
    assert len(tri) == 432
    for (cell, margin), dims, inside in (((0.37, 0.6), (19, 16, 13), 380), ((0.41, 0.7), (18, 15, 12), None)):
        got, origin = field_lattice(P, cell, margin)
        assert got == dims and np.array_equal(origin, P.min(0) - F(margin))
        samples, o, c, w32 = box_field(cell, margin)
        assert samples.shape == dims[::-1] and samples.dtype == np.float32 and np.isfinite(samples).all()
        w64 = winding64(lattice_points(dims, origin, cell), P, tri).reshape(samples.shape)
        assert not ((np.abs(w64) > 0.25) & (np.abs(w64) < 0.75)).any()
        assert np.array_equal(np.signbit(samples), np.abs(w64) > 0.5)
        if inside is not None:
            assert int(np.signbit(samples).sum()) == inside
        # the last sample of every axis lies at or beyond the mesh's bounds grown by the margin
        top = origin + (np.array(dims, F) - F(1)) * F(cell)
        assert (top >= P.max(0) + F(margin)).all()


def test_the_built_field_is_the_distance_to_the_box():
    samples, origin, cell, _ = box_field()
    P, tri = box_mesh()
    pts = lattice_points(samples.shape[::-1], origin, cell)
    d64 = distance64(pts, P, tri).min(1)
    ulp = float(np.spacing(F(np.abs(P).max())))
    assert np.abs(np.abs(samples.reshape(-1)).astype(np.float64) - d64).max() <= 8.0 * ulp  # test_nearest's gate


# ---- known answers --------------------------------------------------------------------------------------------------------------------
def plane_field(n=5, cell=0.5):
    """phi = y on an n^3 lattice from (-1, -1, -1): exact binary samples"""
    origin = F([-1.0, -1.0, -1.0])
    return lattice_points((n, n, n), origin, cell)[:, 1].reshape(n, n, n).copy(), origin, F(cell)


def _one(p, v, P, field, r=0.0, w=1.0):
    return collide_fields(F([p]), F([p]), F([v]), F([r]), F([w]), P if isinstance(P, list) else [P], [field])


def test_one_step_onto_a_plane_is_exact():
    P = capi.FieldProp.make(0, (0.0, 0.0, 0.0), radius=0.25)
    pos, prev, vel, imp, tor, hits, who = _one((0.125, -0.375, 0.25), (0.0, -1.0, 0.5), P, plane_field(), r=0.125)
    assert np.array_equal(pos, F([[0.125, 0.375, 0.25]])) and np.array_equal(prev, pos)  # y = R = 0.375
    assert np.array_equal(vel, F([[0.0, 0.0, 0.5]])) and np.array_equal(imp, F([[0.0, -1.0, 0.0]]))
    assert hits.tolist() == [1] and who.tolist() == [0]
    # exactly on the level set: untouched; 2^-20 below (every step of the rule is still exact): touched
    on = _one((0.125, 0.375, 0.25), (0.0, -1.0, 0.0), P, plane_field(), r=0.125)
    assert on[5].tolist() == [0] and np.array_equal(on[0], F([[0.125, 0.375, 0.25]])) and on[6].tolist() == [NONE]
    below = _one((0.125, 0.375 - 2.0 ** -20, 0.25), (0.0, -1.0, 0.0), P, plane_field(), r=0.125)
    assert below[5].tolist() == [1] and np.array_equal(below[0], F([[0.125, 0.375, 0.25]]))


def test_a_turned_frame_turns_the_push():
    axes = F([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # local y is world x
    P = capi.FieldProp.make(0, (1.0, 2.0, 3.0), axes=axes, radius=0.5, velocity=(1.0, 0.0, 0.0), friction=1.0)
    pos, prev, vel, imp, tor, hits, who = _one((0.75, 2.25, 3.5), (0.0, 0.0, 0.0), P, plane_field())
    assert np.array_equal(pos, F([[1.5, 2.25, 3.5]])) and hits.tolist() == [1]  # world x = centre.x + R
    assert np.array_equal(vel, F([[1.0, 0.0, 0.0]])) and np.array_equal(imp, F([[-1.0, 0.0, 0.0]]))


def test_a_sampled_sphere_pushes_radially():
    field = sphere_field(n=17, cell=0.125, radius=0.5)
    P = capi.FieldProp.make(0, (0.0, 0.0, 0.0), radius=0.25)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * rng.uniform(0.45, 0.9, (64, 1))).astype(F)
    out = collide_fields(p, p, np.zeros_like(p), np.zeros(64, F), np.ones(64, F), [P], [field])
    inside = np.linalg.norm(p.astype(np.float64), axis=1) < 0.74
    assert out[5][0] >= inside.sum() > 8
    touched = out[6] == 0
    assert np.abs(np.linalg.norm(out[0][touched].astype(np.float64), axis=1) - 0.75).max() < 0.02  # a sixth of a cell
    cosine = (out[0][touched] * p[touched]).sum(1) / np.linalg.norm(out[0][touched], axis=1) / np.linalg.norm(p[touched], axis=1)
    assert cosine.min() > 0.99  # the interpolant's gradient is a difference over one cell: off by about cell / (4 r) = 0.07 rad at r = 0.45


def test_outside_the_lattice_and_on_its_last_edge():
    P = capi.FieldProp.make(0, (0.0, 0.0, 0.0), radius=4.0)  # every point of the lattice is below the level set
    field = plane_field()  # the lattice spans [-1, 1]^3: g_j == dims_j - 1 at local 1.0
    v = (0.0, 0.0, 0.0)
    assert _one((0.5, 0.5, 0.5), v, P, field)[5].tolist() == [1]
    assert _one((-1.0, -1.0, -1.0), v, P, field)[5].tolist() == [1]  # g == 0 is inside
    for p in ((1.0, 0.5, 0.5), (0.5, 1.0, 0.5), (0.5, 0.5, 1.0), (1.5, 0.0, 0.0), (np.nextafter(F(-1.0), F(-2.0)), 0.0, 0.0)):
        out = _one(p, v, P, field)
        assert out[5].tolist() == [0] and out[6].tolist() == [NONE] and np.array_equal(out[0], F([p])), p
    assert _one((1.0 - 2.0 ** -20, 0.5, 0.5), v, P, field)[5].tolist() == [1]  # g = 4 - 2^-19, exactly
    assert _one((float("nan"), 0.5, 0.5), v, P, field)[5].tolist() == [0]


def test_a_nan_sample_in_the_cell_means_not_touched():
    samples, origin, cell = plane_field()
    samples[2, 2, 2] = F(np.nan)  # the sample at local (0, 0, 0): the eight cells around it
    P = capi.FieldProp.make(0, (0.0, 0.0, 0.0), radius=4.0)
    for p in ((0.25, 0.25, 0.25), (-0.25, -0.25, -0.25), (0.0, 0.0, 0.0), (-0.5, 0.25, 0.0)):
        assert _one(p, (0, 0, 0), P, (samples, origin, cell))[5].tolist() == [0], p
    assert _one((0.75, 0.25, 0.25), (0, 0, 0), P, (samples, origin, cell))[5].tolist() == [1]


def test_a_plateau_leaves_along_the_frames_second_axis():
    flat = np.full((3, 3, 3), -0.5, F)
    axes = F([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    P = capi.FieldProp.make(0, (0.0, 0.0, 0.0), axes=axes, radius=0.25)
    trace = []
    out = collide_fields(F([[0.5, 0.25, 0.75]]), F([[0.5, 0.25, 0.75]]), F([[0, 0, 0]]), F([0.0]), F([1.0]), [P],
                         [(flat, F([0.0, 0.0, 0.0]), F(1.0))], trace=trace)
    assert cases_of(trace)[0] == {C_TOUCH_FLAT}
    assert np.array_equal(out[0], F([[1.25, 0.25, 0.75]]))  # axis 1 = world x, by R - phi = 0.75


def test_a_fixed_node_is_untouched_and_two_props_apply_in_order():
    field = plane_field()
    a = capi.FieldProp.make(0, (0.0, 0.0, 0.0), radius=0.25, velocity=(1.0, 0.0, 0.0), friction=0.5)
    b = capi.FieldProp.make(0, (0.0, 0.25, 0.0), radius=0.125, velocity=(0.0, 0.0, 2.0), friction=0.25)
    p, v = (0.25, -0.5, 0.0), (0.0, -1.0, 0.5)
    fixed = _one(p, v, [a, b], field, w=0.0)
    assert fixed[5].tolist() == [0, 0] and fixed[6].tolist() == [NONE] and np.array_equal(fixed[0], F([p]))
    both, first = _one(p, v, [a, b], field), _one(p, v, a, field)
    second = collide_fields(first[0], first[1], first[2], F([0.0]), F([1.0]), [b], [field])
    assert both[5].tolist() == [1, 1] and both[6].tolist() == [1]
    for x, y in ((both[0], second[0]), (both[2], second[2]), (both[3][0], first[3][0]), (both[3][1], second[3][0]), (both[4][1], second[4][0])):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- accuracy of the rule itself ------------------------------------------------------------------------------------------------------
def icosphere(level=2):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v).astype(F), np.array(f, np.int64)


def test_one_step_lands_on_the_level_set():
    P, tri = icosphere()
    assert len(tri) == 320
    cell, R = 0.125, 0.15
    samples, origin, c, _ = build_field(P, tri, cell, 0.375)
    rng = np.random.default_rng(9)
    d = rng.normal(size=(4096, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (d * rng.uniform(0.3, 1.3, (4096, 1))).astype(F)
    prop = capi.FieldProp.make(0, (0.0, 0.0, 0.0), radius=0.1)
    out = collide_fields(p, p, np.zeros_like(p), np.full(4096, 0.05, F), np.ones(4096, F), [prop], [(samples, origin, c)])
    touched = out[6] == 0
    assert touched.sum() > 2048 and (~touched).sum() > 256
    d64 = np.concatenate([distance64(out[0][touched][a:a + 1024], P, tri).min(1) for a in range(0, int(touched.sum()), 1024)])
    assert (np.abs(winding64(out[0][touched], P, tri)) < 0.5).all()  # every pushed node is outside the mesh
    err = float(np.abs(d64 - R).max()) / cell
    print("one step on a 0.125 lattice of a unit icosphere: largest |distance64(q) - R| = %.4g of a cell (gate %g)" % (err, GATE_CELLS))
    assert err <= GATE_CELLS


# ---- the entry points on a host-only handle ------------------------------------------------------------------------------------------
def _host_handle():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def test_add_field_and_get_field_round_trip():
    g = _host_handle()
    samples, origin, cell = crafted_field()
    assert g.add_field(samples, origin, cell) == 0 and g.add_field(*sphere_field()) == 1
    got, o, c = g.get_field(0)
    assert np.array_equal(got.view(np.uint32), samples.view(np.uint32)) and np.array_equal(o, origin) and c == float(cell)  # the NaN too
    assert g.get_field(1)[0].shape == (12, 12, 12)
    L, h = capi.load(), g._h
    dims = np.zeros(3, np.uint32)
    assert L.pies_get_field(h, 0, dims.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, 0) == capi.OK and dims.tolist() == [6, 5, 4]
    small = np.zeros(119, F)
    assert L.pies_get_field(h, 0, None, None, None, small.ctypes.data_as(C.POINTER(C.c_float)), 119) == capi.ERR_INVALID
    assert L.pies_get_field(h, 2, None, None, None, None, 0) == capi.ERR_INVALID and "unknown field" in g.last_error()
    assert L.pies_get_field(None, 0, None, None, None, None, 0) == capi.ERR_INVALID


def test_fields_survive_finalize_and_end_with_clear():
    g = _host_handle()
    assert g.add_field(*sphere_field()) == 0
    g.finalize()
    g.create_tet_box(2, 2, 2, translation=(5.0, 1.5, 0.5))
    g.finalize()
    assert g.get_field(0)[0].shape == (12, 12, 12) and g.add_field(*crafted_field()) == 1
    g.clear()
    with pytest.raises(capi.PiesError):
        g.get_field(0)
    L = capi.load()
    prop = capi.FieldProp.make(0, (0, 0, 0))
    assert L.pies_collide_field_props(g._h, 1, C.byref(prop), None, None, None, None) == capi.ERR_INVALID
    assert g.add_field(*crafted_field()) == 0  # the ids count from 0 again
    assert L.pies_collide_field_props(g._h, 1, C.byref(prop), None, None, None, None) == capi.ERR_HIP


def test_argument_checks_come_before_the_device_check():
    g = _host_handle()
    L, h = capi.load(), g._h
    inf, nan = float("inf"), float("nan")
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    def add(dims=(3, 3, 3), origin=(0, 0, 0), cell=1.0, samples=True, null=()):
        d, o, v = np.array(dims, np.uint32), np.array(origin, F), np.zeros(27, F)
        return L.pies_add_field(h, None if "dims" in null else d.ctypes.data_as(pu), None if "origin" in null else o.ctypes.data_as(pf), cell,
                                None if "samples" in null else v.ctypes.data_as(pf), None)

    for name in ("dims", "origin", "samples"):
        assert add(null=(name,)) == capi.ERR_INVALID and "NULL" in g.last_error()
    for dims in ((1, 3, 3), (3, 0, 3), (3, 3, 1)):
        assert add(dims=dims) == capi.ERR_INVALID
    for cell in (0.0, -1.0, nan, inf):
        assert add(cell=cell) == capi.ERR_INVALID
    for bad in (nan, inf, -inf):
        assert add(origin=(0, bad, 0)) == capi.ERR_INVALID
    assert add(dims=(4097, 4096, 2)) == capi.ERR_UNSUPPORTED and add(dims=(65536, 65536, 65536)) == capi.ERR_UNSUPPORTED  # checked before the samples are read
    assert L.pies_add_field(None, None, None, 1.0, None, None) == capi.ERR_INVALID
    assert g.count(capi.NODES) == 27  # nothing above touched the scene
    assert add() == capi.OK and add() == capi.OK  # fields 0 and 1

    # ---- the mesh build ----
    P, tri = box_mesh()
    tri = tri.astype(np.uint32)

    def mesh(P_=P, tri_=tri, cell=0.37, margin=0.6, nv=None, nt=None):
        P_, tri_ = np.ascontiguousarray(P_, F), np.ascontiguousarray(tri_, np.uint32)
        return L.pies_add_field_tri_mesh(h, len(P_) if nv is None else nv, P_.ctypes.data_as(pf), len(tri_) if nt is None else nt,
                                         tri_.ctypes.data_as(pu), cell, margin, None)

    assert mesh(nv=0) == capi.ERR_INVALID and mesh(nt=0) == capi.ERR_INVALID
    bad = P.copy()
    bad[7, 1] = nan
    assert mesh(P_=bad) == capi.ERR_INVALID and "non-finite" in g.last_error()
    worse = tri.copy()
    worse[5, 2] = len(P)
    assert mesh(tri_=worse) == capi.ERR_INVALID and "out of range" in g.last_error()
    for cell in (0.0, -0.37, nan, inf):
        assert mesh(cell=cell) == capi.ERR_INVALID
    for margin in (-0.1, nan, inf):
        assert mesh(margin=margin) == capi.ERR_INVALID
    assert mesh(cell=0.01) == capi.ERR_UNSUPPORTED  # 650 x 528 x 414 samples
    assert mesh(cell=1e-30) == capi.ERR_UNSUPPORTED
    assert mesh() == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert mesh(margin=0.0) == capi.ERR_HIP
    with pytest.raises(capi.PiesError):
        g.add_field_tri_mesh(P, tri, 0.37, 0.6)

    # ---- colliding ----
    def call(*props, n=None, null=False):
        arr = (capi.FieldProp * max(len(props), 1))(*props)
        return L.pies_collide_field_props(h, len(props) if n is None else n, None if null else arr, None, None, None, None)

    good = capi.FieldProp.make(1, (0.5, 1.0, 0.0), radius=0.25, velocity=(1, 0, 0), friction=0.5)

    def broken(**kw):
        p = capi.FieldProp.from_buffer_copy(good)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(p, name)[value[0]] = value[1]
            else:
                setattr(p, name, value)
        return p

    assert call(n=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()
    assert call(broken(field=2)) == capi.ERR_INVALID and "unknown field" in g.last_error()
    assert call(broken(field=0xFFFFFFFF)) == capi.ERR_INVALID
    for value in (-0.5, nan, inf):
        assert call(broken(radius=value)) == capi.ERR_INVALID, value
    for value in (-0.01, 1.5, nan):
        assert call(broken(friction=value)) == capi.ERR_INVALID, value
    for name, length in (("centre", 3), ("axes", 9), ("velocity", 3), ("angular", 3), ("pivot", 3)):
        for value in (nan, inf, -inf):
            assert call(broken(**{name: (length - 1, value)})) == capi.ERR_INVALID, (name, value)
    assert call(good, broken(radius=-1.0)) == capi.ERR_INVALID and "prop 1" in g.last_error()
    assert call(*([good] * 65)) == capi.ERR_UNSUPPORTED
    assert call(good) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert call(*([good] * 64)) == capi.ERR_HIP
    assert call() == capi.OK and call(n=0, null=True) == capi.OK
    who = np.zeros(g.count(capi.NODES), np.uint32)
    assert L.pies_collide_field_props(h, 0, None, None, None, None, who.ctypes.data_as(pu)) == capi.OK
    assert (who == NONE).all()
    with pytest.raises(capi.PiesError):
        g.collide_field_props([good])
    assert g.collide_field_props([], reaction=False) is None
    assert L.pies_collide_field_props(None, 0, None, None, None, None, None) == capi.ERR_INVALID


def test_a_handle_holds_at_most_field_max_fields():
    g = _host_handle()
    field = (np.zeros((2, 2, 2), F), (0, 0, 0), 1.0)
    assert [g.add_field(*field) for _ in range(capi.FIELD_MAX)] == list(range(capi.FIELD_MAX))
    with pytest.raises(capi.PiesError):
        g.add_field(*field)


def test_binding_declares_the_entry_points():
    for name in ("pies_add_field", "pies_add_field_tri_mesh", "pies_get_field", "pies_collide_field_props"):
        assert name in capi.SYMBOLS
    assert capi.FIELD_MAX == 64 and capi.FIELD_PROP_MAX == 64 and C.sizeof(capi.FieldProp) == 96
    L = capi.load()
    assert len(L.pies_add_field.argtypes) == 6 and len(L.pies_add_field_tri_mesh.argtypes) == 8
    assert len(L.pies_get_field.argtypes) == 7 and len(L.pies_collide_field_props.argtypes) == 7
    assert L.pies_collide_field_props.restype is C.c_int
    assert L.pies_abi_version() == 4
