"""CPU tests of pies_raycast: the numpy fp32 restatement of the pair rule of include/pies_hip.h (the yardstick of
tests/test_raycast_gpu.py, which asks the device for the same bits), held against an fp64 brute force, known answers, and the
argument checks on a host-only handle.

Restatement against fp64 on the scene of test_restatement_picks_the_fp64_triangle (a turned 6 x 6 box surface, 432 triangles,
2 048 rays aimed at interior points): the same triangle on every ray; largest |t32 - t64| measured 3.65 ulp of the scene's
largest coordinate, the gate is four times that rounded up to a power of two: 16 ulp."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi
from test_skin import box_surface

F = np.float32
FLT_MIN = F(np.finfo(np.float32).tiny)
MISS = 0xFFFFFFFF
T_GAP_ULPS = 16.0  # see the module docstring


# ---- the restatement (shared with tests/test_raycast_gpu.py) ---------------------------------------------------------------------
def pair_rule(o, d, a, b, c, t_max, cull_back=False):
    """The rule for (ray, triangle) pairs, operation for operation in fp32 (numpy rounds every product and sum: no fused
    multiply-add).  o, d: (R, 3); a, b, c: (T, 3).  Returns (hit (R, T) bool, t, u, v (R, T) float32; garbage where not hit)."""
    o, d, a, b, c = (np.asarray(x, F) for x in (o, d, a, b, c))
    ox, oy, oz = (o[:, None, k] for k in range(3))
    dx, dy, dz = (d[:, None, k] for k in range(3))
    ax, ay, az = (a[None, :, k] for k in range(3))
    e1x, e1y, e1z = (b[None, :, k] - a[None, :, k] for k in range(3))
    e2x, e2y, e2z = (c[None, :, k] - a[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        px = dy * e2z - dz * e2y
        py = dz * e2x - dx * e2z
        pz = dx * e2y - dy * e2x
        det = e1x * px + e1y * py + e1z * pz
        hit = (det >= FLT_MIN) if cull_back else (np.abs(det) >= FLT_MIN)
        inv = F(1.0) / det
        hit &= np.isfinite(inv)
        sx, sy, sz = ox - ax, oy - ay, oz - az
        u = (sx * px + sy * py + sz * pz) * inv
        hit &= (u >= F(0.0)) & (u <= F(1.0))
        qx = sy * e1z - sz * e1y
        qy = sz * e1x - sx * e1z
        qz = sx * e1y - sy * e1x
        v = (dx * qx + dy * qy + dz * qz) * inv
        hit &= (v >= F(0.0)) & (u + v <= F(1.0))
        t = (e2x * qx + e2y * qy + e2z * qz) * inv + F(0.0)
        hit &= (t >= F(0.0)) & (t <= F(t_max))
    for x in (det, inv, u, v, t):
        assert x.dtype == np.float32
    return hit, t, u, v


def cast(o, d, P, tris, t_max=np.inf, cull_back=False):
    """Nearest hits of the rays on triangles `tris` (T, 3) over positions P, by the rule: (triangle uint32, t, uv (R, 2)); the
    smallest t wins, the lowest index on equal t - the minimum of the key bits(t) << 32 | index.  A miss is (MISS, +inf, 0)."""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    P, tris = np.asarray(P, F), np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(o)
    tri, t, uv = np.full(n, MISS, np.uint32), np.full(n, np.inf, F), np.zeros((n, 2), F)
    if len(tris) == 0 or n == 0:
        return tri, t, uv
    hit, tt, u, v = pair_rule(o, d, P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]], t_max, cull_back)
    key = tt.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.arange(len(tris), dtype=np.uint64)[None, :]
    key[~hit] = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = key.argmin(1)  # (the keys of a row are distinct wherever they are not the miss key)
    rows = np.arange(n)
    won = hit[rows, best]
    tri[won] = best[won]
    t[won] = tt[rows, best][won]
    uv[won, 0], uv[won, 1] = u[rows, best][won], v[rows, best][won]
    return tri, t, uv


def cast64(o, d, P, tris):
    """fp64 brute force (Moeller-Trumbore with numpy's own products): per ray the (R, T) matrix of t, +inf where there is no hit"""
    o, d, P = np.asarray(o, np.float64)[:, None, :], np.asarray(d, np.float64)[:, None, :], np.asarray(P, np.float64)
    a, b, c = (P[tris[:, k]][None, :, :] for k in range(3))
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = (e1 * p).sum(2)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        s = o - a
        u = (s * p).sum(2) * inv
        q = np.cross(s, e1)
        v = (d * q).sum(2) * inv
        t = (e2 * q).sum(2) * inv
    ok = (np.abs(det) > 1e-300) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0)
    return np.where(ok, t, np.inf)


def turned_box(n=6):
    """A box surface of well-shaped triangles, turned out of the axes and moved off the origin so that no coordinate is round:
    (positions float32, triangles)"""
    v, tri = box_surface((-2.0, -1.5, -1.0), (2.0, 1.5, 1.0), n)
    a, b = 0.6, 0.35
    Rz = np.float64([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.float64([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (v.astype(np.float64) @ (Rz @ Rx).T + [3.0, 5.0, 2.0]).astype(F), tri


def aimed_rays(P, tri, count, seed):
    """Rays aimed at interior points of random triangles - every barycentric weight at least 0.05 -, from outside, within 60
    degrees of the normal, |d| in [0.5, 2]"""
    rng = np.random.default_rng(seed)
    P64 = P.astype(np.float64)
    k = rng.integers(0, len(tri), count)
    w = 0.05 + 0.85 * rng.dirichlet([1.0, 1.0, 1.0], count)  # each >= 0.05, sum 1
    a, b, c = (P64[tri[k, j]] for j in range(3))
    target = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)  # outward
    t1 = np.cross(nrm, rng.normal(size=(count, 3)))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    tilt = np.radians(rng.uniform(0.0, 59.0, count))[:, None]
    back = np.cos(tilt) * nrm + np.sin(tilt) * t1  # from the target towards the origin of the ray
    dist = rng.uniform(0.5, 6.0, (count, 1))
    length = rng.uniform(0.5, 2.0, (count, 1))
    return (target + dist * back).astype(F), (-back * length).astype(F), k


def test_restatement_picks_the_fp64_triangle():
    P, tri = turned_box()
    size = float(np.linalg.norm(P.max(0) - P.min(0)))
    o, d, aimed = aimed_rays(P, tri, 2048, seed=5)
    t64 = cast64(o, d, P, tri)
    order = np.sort(t64, axis=1)
    assert np.isfinite(order[:, 0]).all()  # every ray hits
    # the conditions the rays were made for hold for every one of them: none is left out below
    assert (order[:, 1] - order[:, 0] > 1e-3 * size).all()
    assert np.array_equal(t64.argmin(1), aimed)
    got, t32, uv = cast(o, d, P, tri)
    assert np.array_equal(got, aimed.astype(np.uint32))
    ulp = float(np.spacing(F(np.abs(P).max())))
    gap = float(np.abs(t32.astype(np.float64) - order[:, 0]).max()) / ulp
    print("restatement vs fp64: max |t32 - t64| = %.3g ulp of the largest coordinate (gate %g)" % (gap, T_GAP_ULPS))
    assert gap <= T_GAP_ULPS
    assert (uv >= 0).all() and (uv.sum(1) <= 1).all() and uv.min() > 0.04 and (1 - uv.sum(1)).min() > 0.04


# ---- known answers ---------------------------------------------------------------------------------------------------------------
RIGHT = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])  # unit right triangle in z = 0, normal +z


def test_axis_aligned_ray_through_the_centre():
    tri, t, uv = cast([[0.25, 0.25, 2.0]], [[0, 0, -1]], RIGHT, [[0, 1, 2]])
    assert tri[0] == 0 and t[0] == 2.0 and np.array_equal(uv[0], F([0.25, 0.25]))
    tri, t, uv = cast([[0.25, 0.5, 2.0]], [[0, 0, -4]], RIGHT, [[0, 1, 2]])  # t in units of |d|; u, v the weights of b and c
    assert tri[0] == 0 and t[0] == 0.5 and np.array_equal(uv[0], F([0.25, 0.5]))
    assert cast([[0.25, 0.25, 2.0]], [[0, 0, -1]], RIGHT, [[0, 1, 2]], t_max=1.5)[0][0] == MISS
    assert cast([[0.25, 0.25, 2.0]], [[0, 0, 1]], RIGHT, [[0, 1, 2]])[0][0] == MISS  # behind the origin
    assert cast([[0.75, 0.75, 2.0]], [[0, 0, -1]], RIGHT, [[0, 1, 2]])[0][0] == MISS  # u + v > 1


def test_back_face_culling_turns_a_hit_into_a_miss():
    below, up = [[0.25, 0.25, -1.0]], [[0, 0, 1]]
    # d x e2 . e1 > 0 for a ray against the normal: from above the front face is seen
    assert cast([[0.25, 0.25, 1.0]], [[0, 0, -1]], RIGHT, [[0, 1, 2]], cull_back=True)[0][0] == 0
    assert cast(below, up, RIGHT, [[0, 1, 2]])[0][0] == 0
    tri, t, uv = cast(below, up, RIGHT, [[0, 1, 2]], cull_back=True)
    assert tri[0] == MISS and np.isinf(t[0]) and not uv.any()


def test_degenerate_triangle_zero_direction_and_nan_miss():
    flat = F([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    o, d = [[0.25, 0.25, 1.0]], [[0, 0, -1]]
    assert cast(o, d, flat, [[0, 1, 2]])[0][0] == MISS
    assert cast(o, d, RIGHT, [[0, 1, 1]])[0][0] == MISS
    assert cast(o, [[0, 0, 0]], RIGHT, [[0, 1, 2]])[0][0] == MISS
    assert cast([[0.25, 0.25, 0.0]], [[1, 0, 0]], RIGHT, [[0, 1, 2]])[0][0] == MISS  # in the triangle's plane: det = 0
    nan = F(np.nan)
    assert cast([[nan, 0.25, 1.0]], d, RIGHT, [[0, 1, 2]])[0][0] == MISS
    assert cast(o, [[0, nan, -1]], RIGHT, [[0, 1, 2]])[0][0] == MISS
    bad = RIGHT.copy()
    bad[2, 1] = nan
    tri, t, uv = cast(o, d, bad, [[0, 1, 2]])
    assert tri[0] == MISS and np.isinf(t[0]) and t[0] > 0 and not uv.any()
    assert cast(o, d, RIGHT, np.zeros((0, 3), np.uint32))[0][0] == MISS


def test_coincident_triangles_report_the_lower_index():
    P = np.concatenate([RIGHT + F([0, 0, 1]), RIGHT, RIGHT])  # triangle 0 further away, 1 and 2 coincide
    tris = [[3, 4, 5], [0, 1, 2], [6, 7, 8], [3, 4, 5]]
    tri, t, _ = cast([[0.25, 0.25, -1.0]], [[0, 0, 1]], P, tris)
    assert tri[0] == 0 and t[0] == 1.0  # (0 and 2 and 3 coincide at t = 1; 1 is at t = 2)
    tri, t, _ = cast([[0.25, 0.25, 3.0]], [[0, 0, -1]], P, tris)
    assert tri[0] == 1 and t[0] == 2.0
    tri, _, _ = cast([[0.25, 0.25, -1.0]], [[0, 0, 1]], P, tris[1:])
    assert tri[0] == 1  # the nearest pair is (1, 2) of this list: the lower one


def test_minus_zero_t_becomes_plus_zero():
    tri, t, _ = cast([[0.25, 0.25, 0.0]], [[0, 0, -1]], RIGHT, [[0, 1, 2]])  # the origin lies in the triangle
    assert tri[0] == 0 and t[0] == 0.0 and not np.signbit(t[0])
    tri, t, _ = cast([[0.25, 0.25, 0.0]], [[0, 0, 1]], RIGHT, [[0, 1, 2]])
    assert tri[0] == 0 and t[0] == 0.0 and not np.signbit(t[0])


# ---- the entry point on a host-only handle -----------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device_check():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    L, h = capi.load(), g._h
    o, d = np.zeros((4, 3), F), np.ones((4, 3), F)
    po, pd = o.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.POINTER(C.c_float))
    inf = float("inf")

    def call(target=capi.RAY_SCENE_TRIANGLES, skin=0, n=4, o_=po, d_=pd, t_max=inf, flags=0):
        return L.pies_raycast(h, target, skin, n, o_, d_, t_max, flags, None, None, None)

    assert call(o_=None) == capi.ERR_INVALID and "NULL" in g.last_error()
    assert call(d_=None) == capi.ERR_INVALID
    assert call(target=2) == capi.ERR_INVALID and call(target=-1) == capi.ERR_INVALID
    assert call(target=capi.RAY_SKIN, skin=0) == capi.ERR_INVALID  # no skin yet
    assert g.add_skin(F([[1.0, 2.0, 1.0]]), g.ids(capi.TET)) == 0
    assert call(target=capi.RAY_SKIN, skin=1) == capi.ERR_INVALID
    assert call(t_max=-1.0) == capi.ERR_INVALID and call(t_max=float("nan")) == capi.ERR_INVALID
    assert call(n=(1 << 26) + 1) == capi.ERR_UNSUPPORTED
    assert call(n=0) == capi.OK and call(n=0, o_=None, d_=None) == capi.OK
    assert call() == capi.ERR_HIP and call(target=capi.RAY_SKIN) == capi.ERR_HIP and call(t_max=0.0) == capi.ERR_HIP
    assert "PIES_DEVICE_NONE" in g.last_error()
    with pytest.raises(capi.PiesError):
        g.raycast(o, d)
    with pytest.raises(ValueError):
        g.raycast(o, d[:3])
    assert L.pies_raycast(None, 0, 0, 0, None, None, inf, 0, None, None, None) == capi.ERR_INVALID
