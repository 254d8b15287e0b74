"""CPU tests of pies_closest_points: the numpy fp32 restatement of the pair rule of include/pies_hip.h (the yardstick of
tests/test_nearest_gpu.py, which asks the device for the same bits), held against an independent fp64 brute force, known answers,
the winding number in its two-level order, and the argument checks on a host-only handle.

Restatement against fp64 on the scene of test_restatement_stays_inside_the_gate (a turned 6 x 6 box surface, 432 triangles, 2 048
uniform points in its bounding box grown by 1.5): largest |sqrt(dd32) - d64| measured 1.24 ulp of the scene's largest coordinate,
the gate is four times that rounded up to a power of two: 8 ulp.  The fp32 winner's own fp64 distance stayed within 0.38 ulp of the
fp64 minimum (the same gate holds it).  Triangle indices are not compared with fp64: ties between the
triangles of a shared edge or corner are the normal case (the fp32 winner was the fp64 argmin on about 90 % of the points)."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi
from test_raycast import turned_box
from test_trimesh import _terms, gate_of

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
NONE = 0xFFFFFFFF
TILE = 256  # kNearTile of pies_amd/csrc/near_kernels.h: the first level of the winding sum
D_GAP_ULPS = 8.0  # see the module docstring
WINDING_GROW = 1.2  # the winding tests' box margin: more than 10 % of the points inside the turned box, more than 10 % outside
REGIONS = ("corner a", "corner b", "edge ab", "corner c", "edge ac", "edge bc", "interior")


# ---- the restatement (shared with tests/test_nearest_gpu.py) ---------------------------------------------------------------------
def pair_rule(p, a, b, c, max_distance=np.inf):
    """The rule for (point, triangle) pairs, operation for operation in fp32 (numpy rounds every product and sum: no fused
    multiply-add).  p: (N, 3); a, b, c: (T, 3).  Returns (candidate (N, T) bool, dd, u, v (N, T) float32, q (N, T, 3),
    region (N, T) index into REGIONS)."""
    p, a, b, c = (np.asarray(x, F) for x in (p, a, b, c))
    px, py, pz = (p[:, None, k] for k in range(3))
    ax, ay, az = (a[None, :, k] for k in range(3))
    e1x, e1y, e1z = (b[None, :, k] - a[None, :, k] for k in range(3))
    e2x, e2y, e2z = (c[None, :, k] - a[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        e11 = e1x * e1x + e1y * e1y + e1z * e1z
        e12 = e1x * e2x + e1y * e2y + e1z * e2z
        e22 = e2x * e2x + e2y * e2y + e2z * e2z
        apx, apy, apz = px - ax, py - ay, pz - az
        d1 = e1x * apx + e1y * apy + e1z * apz
        d2 = e2x * apx + e2y * apy + e2z * apz
        d3, d4, d5, d6 = d1 - e11, d2 - e12, d1 - e12, d2 - e22
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        zero, one = F(0.0), F(1.0)
        tests = [(d1 <= zero) & (d2 <= zero),
                 (d3 >= zero) & (d4 <= d3),
                 (vc <= zero) & (d1 >= zero) & (d3 <= zero),
                 (d6 >= zero) & (d5 <= d6),
                 (vb <= zero) & (d2 >= zero) & (d6 <= zero),
                 (va <= zero) & (d43 >= zero) & (d56 >= zero)]
        region = np.full(d1.shape, 6, np.int64)
        for k in reversed(range(6)):  # the first that holds
            region[tests[k]] = k
        tab = d1 / (d1 - d3)
        tac = d2 / (d2 - d6)
        tbc = d43 / (d43 + d56)
        inv = one / ((va + vb) + vc)
        z, o = np.zeros_like(d1), np.ones_like(d1)
        u = np.choose(region, [z, o, tab, z, z, one - tbc, vb * inv])
        v = np.choose(region, [z, z, z, o, tac, tbc, vc * inv])
        qx = (ax + e1x * u) + e2x * v
        qy = (ay + e1y * u) + e2y * v
        qz = (az + e1z * u) + e2z * v
        rx, ry, rz = px - qx, py - qy, pz - qz
        dd = rx * rx + ry * ry + rz * rz
        cand = (dd <= FLT_MAX) & (dd <= F(max_distance) * F(max_distance))
    for x in (d1, va, u, v, qx, dd):
        assert x.dtype == np.float32
    return cand, dd, u, v, np.stack([qx, qy, qz], -1), region


def nearest(points, P, tris, max_distance=np.inf, with_region=False):
    """The answers for the points on triangles `tris` (T, 3) over positions P, by the rule: (triangle uint32, distance, uv (N, 2),
    point (N, 3)[, region of the winner, -1 without one]); the smallest dd wins, the lowest index on equal dd - the minimum of the
    key bits(dd) << 32 | index.  No candidate is (NONE, +inf, 0, the point itself)."""
    p = np.asarray(points, F).reshape(-1, 3)
    P, tris = np.asarray(P, F), np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(p)
    tri, dist, uv, q = np.full(n, NONE, np.uint32), np.full(n, np.inf, F), np.zeros((n, 2), F), p.copy()
    reg = np.full(n, -1, np.int64)
    if len(tris) and n:
        cand, dd, u, v, qq, region = pair_rule(p, P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]], max_distance)
        key = dd.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.arange(len(tris), dtype=np.uint64)[None, :]
        key[~cand] = np.uint64(0xFFFFFFFFFFFFFFFF)
        best = key.argmin(1)  # (the keys of a row are distinct wherever they are candidates)
        rows = np.arange(n)
        won = cand[rows, best]
        tri[won] = best[won]
        dist[won] = np.sqrt(dd[rows, best][won])
        uv[won, 0], uv[won, 1] = u[rows, best][won], v[rows, best][won]
        q[won] = qq[rows, best][won]
        reg[won] = region[rows, best][won]
        assert dist.dtype == np.float32
    return (tri, dist, uv, q, reg) if with_region else (tri, dist, uv, q)


def winding32(points, P, tris):
    """The winding number in fp32 in the order of pies_hip.h: per tile of 256 triangles a sum in ascending index from 0, the tile
    sums in ascending tile index from 0, divided by 4 pi; the pair term is test_trimesh._terms (k_winding's)"""
    c = np.asarray(points, F).reshape(-1, 3)
    T = np.asarray(P, F)[np.asarray(tris, np.int64).reshape(-1, 3)]
    total = np.zeros(len(c), F)
    for base in range(0, len(T), TILE):
        s = np.zeros(len(c), F)
        for t in range(base, min(base + TILE, len(T))):
            s = s + _terms(c, T[t, 0][None], T[t, 1][None], T[t, 2][None])
        total = total + s
    w = total / F(12.566370614359172)
    assert w.dtype == np.float32
    return w


def winding64(points, P, tris):
    c = np.asarray(points, F).astype(np.float64).reshape(-1, 3)
    T = np.asarray(P, F).astype(np.float64)[np.asarray(tris, np.int64).reshape(-1, 3)]
    w = np.zeros(len(c))
    for k in range(0, len(T), 512):
        q = T[k:k + 512]
        w += _terms(c[:, None, :], q[None, :, 0], q[None, :, 1], q[None, :, 2]).sum(1)
    return w / (4.0 * np.pi)


# ---- an independent fp64 brute force ---------------------------------------------------------------------------------------------
def distance64(points, P, tris):
    """(N, T) distances in fp64, not by the region walk: the distance to the triangle's plane where the projection falls inside
    the triangle, and the distances to the three edge segments; the minimum of the four"""
    p = np.asarray(points, F).astype(np.float64)[:, None, :]
    P = np.asarray(P, F).astype(np.float64)
    a, b, c = (P[tris[:, k]][None, :, :] for k in range(3))

    def segment(s, e):
        d = e - s
        t = np.clip(((p - s) * d).sum(2) / (d * d).sum(2), 0.0, 1.0)
        return np.linalg.norm(p - (s + t[..., None] * d), axis=2)

    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n, axis=2, keepdims=True)
    h = ((p - a) * n).sum(2)
    foot = p - h[..., None] * n
    inside = np.ones(h.shape, bool)
    for s, e in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(e - s, foot - s) * n).sum(2) >= 0.0
    plane = np.where(inside, np.abs(h), np.inf)
    return np.minimum(np.minimum(plane, segment(a, b)), np.minimum(segment(b, c), segment(c, a)))


def box_points(P, count, seed, grow=1.5):
    """Uniform points in the bounding box of P grown about its centre by `grow`"""
    rng = np.random.default_rng(seed)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * grow
    return rng.uniform(mid - half, mid + half, (count, 3)).astype(F)


def test_restatement_stays_inside_the_gate():
    P, tri = turned_box()
    pts = box_points(P, 2048, seed=5)
    d64 = distance64(pts, P, tri)
    best64 = d64.min(1)
    got, d32, uv, q, region = nearest(pts, P, tri, with_region=True)
    assert (got != NONE).all() and set(region) == set(range(7))
    ulp = float(np.spacing(F(np.abs(P).max())))
    gap = float(np.abs(d32.astype(np.float64) - best64).max()) / ulp
    own = float(np.abs(d64[np.arange(len(pts)), got] - best64).max()) / ulp
    same = float((got == d64.argmin(1)).mean())
    print("restatement vs fp64: max |sqrt(dd32) - d64| = %.3g ulp of the largest coordinate, the winner's own fp64 distance within "
          "%.3g ulp of the minimum (gate %g); the fp64 argmin triangle on %.1f %% of the points" % (gap, own, D_GAP_ULPS, 100 * same))
    assert gap <= D_GAP_ULPS
    assert own <= D_GAP_ULPS
    # q is the point the weights give, at the distance reported
    a, b, c = (P[tri[got, k]].astype(np.float64) for k in range(3))
    u, v = uv[:, :1].astype(np.float64), uv[:, 1:].astype(np.float64)
    assert np.abs(a + (b - a) * u + (c - a) * v - q).max() <= D_GAP_ULPS * ulp
    assert np.abs(np.linalg.norm(pts.astype(np.float64) - q, axis=1) - d32).max() <= D_GAP_ULPS * ulp
    assert (uv >= 0).all() and (uv.sum(1) <= 1 + 2.0 ** -22).all()


# ---- known answers ---------------------------------------------------------------------------------------------------------------
RIGHT = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])  # unit right triangle in z = 0
ONE = [[0, 1, 2]]


def answer(p, P=RIGHT, tris=ONE, **kw):
    tri, dist, uv, q, region = nearest([p], P, tris, with_region=True, **kw)
    return int(tri[0]), float(dist[0]), tuple(float(x) for x in uv[0]), tuple(float(x) for x in q[0]), int(region[0])


def test_a_point_above_the_interior():
    assert answer([0.25, 0.25, 2.0]) == (0, 2.0, (0.25, 0.25), (0.25, 0.25, 0.0), 6)
    assert answer([0.25, 0.5, -0.5]) == (0, 0.5, (0.25, 0.5), (0.25, 0.5, 0.0), 6)


def test_a_point_beyond_each_edge():
    assert answer([0.5, -1.0, 0.0]) == (0, 1.0, (0.5, 0.0), (0.5, 0.0, 0.0), 2)
    assert answer([-1.0, 0.5, 0.0]) == (0, 1.0, (0.0, 0.5), (0.0, 0.5, 0.0), 4)
    assert answer([1.0, 1.0, 0.0]) == (0, float(np.sqrt(F(0.5))), (0.5, 0.5), (0.5, 0.5, 0.0), 5)
    assert answer([0.5, -1.0, 1.0])[1:] == (float(np.sqrt(F(2.0))), (0.5, 0.0), (0.5, 0.0, 0.0), 2)


def test_a_point_beyond_each_corner():
    assert answer([-1.0, -1.0, 0.0]) == (0, float(np.sqrt(F(2.0))), (0.0, 0.0), (0.0, 0.0, 0.0), 0)
    assert answer([2.0, -0.5, 0.0]) == (0, float(np.sqrt(F(1.25))), (1.0, 0.0), (1.0, 0.0, 0.0), 1)
    assert answer([-0.5, 2.0, 0.0]) == (0, float(np.sqrt(F(1.25))), (0.0, 1.0), (0.0, 1.0, 0.0), 3)


def test_a_point_on_a_shared_edge_reports_the_lower_index():
    P = F([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    mid = [0.5, 0.5, 0.0]
    tri, dist, uv, q, _ = answer(mid, P, [[0, 1, 2], [1, 3, 2]])
    assert (tri, dist, uv, q) == (0, 0.0, (0.5, 0.5), (0.5, 0.5, 0.0))
    tri, dist, uv, q, _ = answer(mid, P, [[1, 3, 2], [0, 1, 2]])  # the same pair of triangles in the other order
    assert (tri, dist, uv, q) == (0, 0.0, (0.0, 0.5), (0.5, 0.5, 0.0))  # the midpoint of that triangle's edge a c
    tri, dist, _, _, _ = answer([1.0, 0.0, 0.0], P, [[1, 3, 2], [0, 1, 2], [0, 1, 2]])  # a shared corner
    assert (tri, dist) == (0, 0.0)
    assert not np.signbit(nearest([mid], P, [[0, 1, 2]])[1][0])


def test_max_distance_cuts():
    p = [0.25, 0.25, 2.0]
    assert answer(p, max_distance=2.0)[:2] == (0, 2.0)  # dd <= max_distance^2: the rim is in
    tri, dist, uv, q, region = answer(p, max_distance=1.5)
    assert tri == NONE and dist == np.inf and uv == (0.0, 0.0) and q == (0.25, 0.25, 2.0) and region == -1
    # a nearer triangle out of reach does not hide a farther one within reach: there is none within reach at all
    P = np.concatenate([RIGHT, RIGHT + F([0, 0, 5])])
    assert answer(p, P, [[0, 1, 2], [3, 4, 5]], max_distance=1.0)[0] == NONE
    assert answer([0.25, 0.25, 4.5], P, [[0, 1, 2], [3, 4, 5]], max_distance=1.0)[:2] == (1, 0.5)


def test_max_distance_zero_finds_only_points_on_the_surface():
    assert answer([0.25, 0.25, 0.0], max_distance=0.0)[:2] == (0, 0.0)
    assert answer([1.0, 0.0, 0.0], max_distance=0.0)[:2] == (0, 0.0)
    assert answer([0.25, 0.25, 2.0 ** -20], max_distance=0.0)[0] == NONE
    assert answer([0.25, 0.25, 0.0], tris=np.zeros((0, 3), np.uint32))[0] == NONE


def test_a_degenerate_triangle_beside_a_good_one():
    line = F([[0, 0, 0], [1, 0, 0], [2, 0, 0]])  # collinear
    dot3 = F([[3, 3, 3]] * 3)  # three equal corners
    P = np.concatenate([line, dot3, RIGHT + F([0, 0, 1])])
    tris = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    for p in ([0.25, 0.25, 1.5], [0.5, 0.0, 0.0], [1.5, 0.0, 0.25], [3.0, 3.0, 3.0], [2.9, 3.2, 3.0], [-4.0, 7.0, 0.5]):
        cand, dd, u, v, q, _ = pair_rule([p], P[[0, 3, 6]], P[[1, 4, 7]], P[[2, 5, 8]])
        assert cand[0, 2] and (np.isfinite(dd[0][cand[0]])).all()  # finite candidates or none
        tri, dist, uv, q = nearest([p], P, tris)
        d64 = distance64(F([p]), P, np.int64([[6, 7, 8]]))[0, 0]
        assert tri[0] != NONE and np.isfinite(dist[0]) and np.isfinite(uv).all() and np.isfinite(q).all()
        assert dist[0] <= F(d64) + F(1e-6)  # no farther than the good triangle
    assert nearest([[0.25, 0.25, 1.5]], P, tris)[0][0] == 2
    assert nearest([[3.0, 3.0, 3.0]], P, tris)[:2] == (np.uint32(1), F(0.0))
    nan = F(np.nan)
    tri, dist, uv, q = nearest([[nan, 0.25, 1.0]], RIGHT, ONE)
    assert tri[0] == NONE and np.isposinf(dist[0]) and not uv.any() and np.isnan(q[0, 0]) and q[0, 1] == F(0.25)
    bad = RIGHT.copy()
    bad[2, 1] = nan
    assert nearest([[0.25, 0.25, 1.0]], np.concatenate([bad, RIGHT]), [[0, 1, 2], [3, 4, 5]])[0][0] == 1


# ---- the winding number in its two-level order -----------------------------------------------------------------------------------
def test_winding_restatement_stays_inside_the_trimesh_gate():
    P, tri = turned_box()
    pts = box_points(P, 2048, seed=5, grow=WINDING_GROW)
    w64 = winding64(pts, P, tri)
    w32 = winding32(pts, P, tri)
    gate, err = gate_of(w32, w64, len(tri))
    print("winding, two-level order vs fp64: max error %.3g (floor of the gate %.3g)" % (err, len(tri) * 2.0 ** -22))
    assert err <= len(tri) * 2.0 ** -22
    near = np.abs(np.abs(w64) - 0.5) < 0.05
    assert near.sum() == 0  # no point of this set is left out by the threshold clause of the GPU test
    inside = np.abs(w64) > 0.5
    assert inside.mean() > 0.1 and (~inside).mean() > 0.1
    assert np.array_equal(np.abs(w32) > F(0.5), inside)
    assert np.abs(w64[inside] - 1.0).max() < 1e-9 and np.abs(w64[~inside]).max() < 1e-9  # a closed surface wound outwards
    # one tile: the order is k_winding's single running sum
    assert np.array_equal(winding32(pts[:64], P, tri[:200]), _one_sum(pts[:64], P, tri[:200]))


def _one_sum(points, P, tris):
    T = P[tris]
    s = np.zeros(len(points), F)
    for t in range(len(T)):
        s = s + _terms(points, T[t, 0][None], T[t, 1][None], T[t, 2][None])
    return s / F(12.566370614359172)


# ---- the entry point on a host-only handle -----------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device_check():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    L, h = capi.load(), g._h
    p = np.zeros((4, 3), F)
    pp = p.ctypes.data_as(C.POINTER(C.c_float))
    inf = float("inf")

    def call(target=capi.RAY_SCENE_TRIANGLES, skin=0, n=4, p_=pp, max_distance=inf):
        return L.pies_closest_points(h, target, skin, n, p_, max_distance, None, None, None, None, None)

    assert call(p_=None) == capi.ERR_INVALID and "NULL" in g.last_error()
    assert call(target=2) == capi.ERR_INVALID and call(target=-1) == capi.ERR_INVALID
    assert call(target=capi.RAY_SKIN, skin=0) == capi.ERR_INVALID  # no skin yet
    assert g.add_skin(F([[1.0, 2.0, 1.0]]), g.ids(capi.TET)) == 0
    assert call(target=capi.RAY_SKIN, skin=1) == capi.ERR_INVALID
    assert call(max_distance=-1.0) == capi.ERR_INVALID and call(max_distance=float("nan")) == capi.ERR_INVALID
    assert call(max_distance=-inf) == capi.ERR_INVALID
    assert call(n=(1 << 26) + 1) == capi.ERR_UNSUPPORTED
    assert call(n=0) == capi.OK and call(n=0, p_=None) == capi.OK
    assert call() == capi.ERR_HIP and call(target=capi.RAY_SKIN) == capi.ERR_HIP and call(max_distance=0.0) == capi.ERR_HIP
    assert "PIES_DEVICE_NONE" in g.last_error()
    with pytest.raises(capi.PiesError):
        g.closest_points(p)
    assert L.pies_closest_points(None, 0, 0, 0, None, inf, None, None, None, None, None) == capi.ERR_INVALID


def test_binding_declares_the_entry_point():
    assert "pies_closest_points" in capi.SYMBOLS and capi.NEAR_NONE == NONE
    L = capi.load()
    assert L.pies_closest_points.restype is C.c_int and len(L.pies_closest_points.argtypes) == 11
    assert L.pies_abi_version() == 4
