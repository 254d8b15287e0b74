"""CPU tests of pies_apply_surface_loads: the numpy fp32 restatement of the rule of include/pies_hip.h (`apply_surface_loads`, the
yardstick the device has to match bit for bit in tests/test_loads_gpu.py), an independent fp64 formulation it is held to, physics
checks on that formulation, and the argument checks of the entry point on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi

F = np.float32
TILE = 256
DT = F(0.0125)
TO_END = capi.LOAD_TO_END

# branch codes of one (triangle, load) pair of the load's range (apply_surface_loads(..., trace=[])) ...
T_DEGENERATE, T_ABOVE, T_IN, T_IDLE = 0, 1, 2, 3  # nn > 0 fails; a fluid's depth > 0 fails; contributes; a gas with V <= 0
# ... and of one (node, load) pair
N_OUT, N_FIXED, N_HIT = 0, 1, 2  # named by no contributing triangle; by one, but invMass == 0; affected


# ---- the restatement: fp32, no fused multiply-adds, the operation order of the header -------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _vec(a):
    return np.array(list(a), F)


def resolve(load, n_tris):
    """(first, count) of a load's range in a container of n_tris triangles"""
    first = int(load.first)
    return first, (n_tris - first if load.count == TO_END else int(load.count))


def _corners(load, tris):
    """the range's triangles as the load reads them: (a, b, c), with LOAD_INWARD (a, c, b)"""
    return tris[:, [0, 2, 1]] if load.flags & capi.LOAD_INWARD else tris


def _tiled_sum(values, first):
    """values of the container indices first, first + 1, ...: per tile of 256 indices of the global tiling in ascending index from
    0, then the tiles in ascending index from 0"""
    total, i, end = F(0), first, first + len(values)
    while i < end:
        stop = min(end, (i // TILE + 1) * TILE)
        total = total + np.cumsum(np.concatenate([[F(0)], values[i - first:stop - first]]), dtype=F)[-1]
        i = stop
    return F(total)


def apply_surface_loads(pos, vel, inv_mass, triangles, loads, dt, trace=None):
    """The rule of pies_apply_surface_loads in numpy fp32.  Returns (vel, impulse, torque, nodes, volume, area).  Every load reads
    pos and vel as they are given; a node's changes are added in ascending load index from 0 and the sum to its velocity; the
    reaction sums are taken per tile of 256 node ids in ascending id from 0, then over the tiles in ascending index from 0.
    trace: a list that receives (load, branch code per node, branch code per triangle of the range, the range's first index)."""
    with np.errstate(all="ignore"):
        pos, vel = (np.array(a, F).reshape(-1, 3).copy() for a in (pos, vel))
        w = np.asarray(inv_mass, F).reshape(-1)
        all_tris = np.asarray(triangles, np.int64).reshape(-1, 3)
        dt = F(dt)
        n, k = len(pos), len(loads)
        movable = ~(w == 0)
        safe_w = np.where(movable, w, F(1))
        J, T = np.zeros((k, n, 3), F), np.zeros((k, n, 3), F)
        affected = np.zeros((k, n), bool)
        total = np.zeros((n, 3), F)
        volume, area = np.zeros(k, F), np.zeros(k, F)
        for i, L in enumerate(loads):
            first, count = resolve(L, len(all_tris))
            tris = _corners(L, all_tris[first:first + count])
            dv, hit, named = np.zeros((n, 3), F), np.zeros(n, bool), np.zeros(n, bool)
            tri_codes = np.zeros(count, np.int64)
            if count:
                a, b, c = pos[tris[:, 0]], pos[tris[:, 1]], pos[tris[:, 2]]
                o = pos[all_tris[first, 0]][None]
                six = _dot(a - o, _cross(b - o, c - o))
                N = _cross(b - a, c - a)
                nn = _dot(N, N)
                area_t = F(0.5) * np.sqrt(nn)
                volume[i] = _tiled_sum(six.astype(F), first) / F(6)
                area[i] = _tiled_sum(area_t.astype(F), first)
                acts, use = True, nn > 0
                if L.type == capi.LOAD_PRESSURE:
                    p = np.full(count, F(L.strength), F)
                elif L.type == capi.LOAD_GAS:
                    acts = bool(volume[i] > 0)
                    p = np.full(count, F(L.strength) * (F(L.rest_volume) / volume[i] - F(1)), F)
                else:
                    x = ((a + b) + c) / F(3)
                    depth = _dot(_vec(L.point)[None] - x, np.broadcast_to(_vec(L.up)[None], x.shape))
                    below = depth > 0
                    p = -(F(L.strength) * depth)
                    tri_codes = np.where(below, T_IN, T_ABOVE)
                    use = use & below
                force = N * (F(0.5) * p)[:, None]
                if L.type == capi.LOAD_FLUID and L.drag != 0:
                    rel = _vec(L.velocity)[None] - ((vel[tris[:, 0]] + vel[tris[:, 1]]) + vel[tris[:, 2]]) / F(3)
                    force = force + rel * (F(L.drag) * area_t)[:, None]
                third = (force / F(3)).astype(F)
                if L.type != capi.LOAD_FLUID:
                    tri_codes = np.full(count, T_IN)
                tri_codes = np.where(nn > 0, tri_codes, T_DEGENERATE)
                if not acts:
                    tri_codes = np.full(count, T_IDLE)
                    use = np.zeros(count, bool)
                for t in np.nonzero(use)[0]:
                    for node in tris[t]:
                        named[node] = True
                        if w[node] != 0:
                            dv[node] = dv[node] + third[t] * (dt * w[node])
                            hit[node] = True
            total[hit] = total[hit] + dv[hit]
            j = dv * (F(1) / safe_w)[:, None]
            tq = _cross(pos - _vec(L.point)[None], j)
            J[i][hit], T[i][hit] = j[hit], tq[hit]
            affected[i] = hit
            if trace is not None:
                trace.append((i, np.where(hit, N_HIT, np.where(named, N_FIXED, N_OUT)), tri_codes, first))
        out = vel.copy()
        any_hit = affected.any(axis=0)
        out[any_hit] = vel[any_hit] + total[any_hit]
        impulse, torque = np.zeros((k, 3), F), np.zeros((k, 3), F)
        for first in range(0, n, TILE):
            si, st = np.zeros((k, 3), F), np.zeros((k, 3), F)
            for node in range(first, min(first + TILE, n)):
                si, st = si + J[:, node], st + T[:, node]  # (a node not affected adds 0)
            impulse, torque = impulse + si, torque + st
        return out, impulse, torque, affected.sum(axis=1).astype(np.uint32), volume, area


def affected_of(trace, n):
    return np.array([codes == N_HIT for _, codes, _, _ in trace]).reshape(len(trace), n)


# ---- an independent fp64 formulation: the divergence theorem about the range's centroid, a scattered gather -------------------------
def apply_surface_loads_f64(pos, vel, inv_mass, triangles, loads, dt):
    """Returns (vel, impulse, torque, affected (k x n), volume, area, contributing triangles per load [bool per triangle of the
    range], the sum of |volume terms| per load)."""
    x, v = np.array(pos, np.float64).reshape(-1, 3), np.array(vel, np.float64).reshape(-1, 3)
    w = np.asarray(inv_mass, np.float64).reshape(-1)
    all_tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    dt = float(dt)
    n, k = len(x), len(loads)
    movable = w != 0
    mass = np.where(movable, 1.0 / np.where(movable, w, 1.0), 0.0)
    change = np.zeros((k, n, 3))
    affected = np.zeros((k, n), bool)
    volume, area, terms, faces = np.zeros(k), np.zeros(k), np.zeros(k), []
    for i, L in enumerate(loads):
        first, count = resolve(L, len(all_tris))
        tris = all_tris[first:first + count]
        if L.flags & capi.LOAD_INWARD:
            tris = tris[:, ::-1]  # (any reversal mirrors the normal)
        if not count:
            faces.append(np.zeros(0, bool))
            continue
        corners, speeds = x[tris], v[tris]  # t x 3 x 3
        centroid = corners.mean(axis=1)
        normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])  # twice the area vector
        twice = np.linalg.norm(normal, axis=1)
        middle = centroid.mean(axis=0)
        flux = np.einsum("ij,ij->i", centroid - middle, normal) / 6.0  # the divergence theorem: V = 1/3 sum of x . n dA
        # ... about the range's centroid; a range that is not closed has an area vector left over, and its volume depends on the
        # point it is taken about: the rule's is o, corner a of the range's first triangle
        o = x[all_tris[first, 0]]
        volume[i], area[i] = flux.sum() + (middle - o) @ normal.sum(axis=0) / 6.0, 0.5 * twice.sum()
        terms[i] = np.abs(np.einsum("ij,ij->i", centroid - o, normal)).sum() / 6.0
        use = twice > 0
        if L.type == capi.LOAD_PRESSURE:
            p = np.full(count, float(L.strength))
        elif L.type == capi.LOAD_GAS:
            p = np.full(count, float(L.strength) * (float(L.rest_volume) / volume[i] - 1.0))
            if not volume[i] > 0:
                use = np.zeros(count, bool)
        else:
            depth = (np.array(list(L.point), np.float64) - centroid) @ np.array(list(L.up), np.float64)
            p = -float(L.strength) * depth
            use = use & (depth > 0)
        push = 0.5 * normal * p[:, None]
        if L.type == capi.LOAD_FLUID and L.drag != 0:
            push = push + (np.array(list(L.velocity), np.float64) - speeds.mean(axis=1)) * (float(L.drag) * 0.5 * twice)[:, None]
        faces.append(use)
        count_at = np.zeros(n)
        for corner in range(3):
            ids = tris[use][:, corner]
            np.add.at(change[i], ids, push[use] / 3.0 * (dt * w[ids])[:, None])
            np.add.at(count_at, ids, 1.0)
        affected[i] = (count_at > 0) & movable
        change[i][~affected[i]] = 0.0
    out = v + change.sum(axis=0)
    momentum = change * mass[None, :, None]
    impulse = momentum.sum(axis=1)
    arms = x[None] - np.array([list(L.point) for L in loads], np.float64).reshape(k, 1, 3)
    torque = np.cross(arms, momentum).sum(axis=1)
    return out, impulse, torque, affected, volume, area, faces, terms


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def cube_mesh(m, size=1.0, corner=(0.0, 0.0, 0.0)):
    """(positions float64, triangles): the surface of a cube of edge `size` with its low corner at `corner`, every face an m x m
    grid of quads cut in two, wound outward: 6 m^2 + 2 nodes, 12 m^2 triangles"""
    ids, pos, tris = {}, [], []

    def node(p):
        if p not in ids:
            ids[p] = len(pos)
            pos.append(p)
        return ids[p]

    for d in range(3):
        u, v = (d + 1) % 3, (d + 2) % 3
        for side in (0, m):
            for i in range(m):
                for j in range(m):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[d], p[u], p[v] = side, i + di, j + dj
                        return node(tuple(p))
                    p00, p10, p11, p01 = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    tris += [[p00, p10, p11], [p00, p11, p01]] if side else [[p00, p11, p10], [p00, p01, p11]]
    return np.array(pos, np.float64) * (size / m) + np.array(corner, np.float64), np.array(tris, np.uint32)


def _rotation(axis, angle):
    axis = np.array(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


MARGIN = 1e-3  # of the scene's size: no centroid lies closer to a fluid's surface, no gas volume closer to 0 (of size^3)
HUB_FAN = 40
UP = (0.125, 1.0, -0.0625)  # used as given: not a unit vector


def single_triangle():
    pos = F([[0.0, 1.0, 0.0], [1.0, 1.25, 0.0], [0.25, 1.5, 1.0]])
    vel = F([[0.5, 0.0, -1.0], [0.0, 0.25, 0.0], [-0.5, 1.0, 0.5]])
    loads = [capi.SurfaceLoad.fluid(9.8125, (0.0, 2.0, 0.0), up=UP).with_drag(0.75, (0.25, 0.0, -0.5))]
    return pos, vel, F([1.0, 0.5, 2.0]), np.array([[0, 1, 2]], np.uint32), loads


def small_cube():
    """the 12-triangle cube, a gas inside it and a fluid around its lower part"""
    pos, tris = cube_mesh(1, 1.0, (0.25, -0.625, 0.5))
    pos = pos.astype(F)
    vel = (np.random.default_rng(11).normal(size=pos.shape)).astype(F)
    loads = [capi.SurfaceLoad.gas(1.5, 1.25, about=(0.75, -0.125, 1.0)), capi.SurfaceLoad.fluid(9.8125, (0.0, 0.03125, 0.0), up=UP),
             capi.SurfaceLoad.pressure(-2.0, about=(0.75, -0.125, 1.0))]
    return pos, vel, np.full(len(pos), F(2)), tris, loads


def make_body_scene(m, seed=0):
    """(pos, vel, inv_mass, triangles, marks).  The container holds, in this order: body A, a closed cube of 12 m^2 triangles, turned
    out of the axes, which the fluid's surface cuts; body B, a 12-triangle cube wound INWARD, below the surface; a cone of 40
    triangles around a hub node; a zero-area triangle on three nodes of a line.  Node 0 (a corner of A) is pinned.  marks: the
    ranges and ids the tests look up."""
    rng = np.random.default_rng(5000 + seed + m)
    a_pos, a_tris = cube_mesh(m, 1.5)
    a_pos = (a_pos - 0.75) @ _rotation((1.0, 2.0, 0.5), 0.4).T + [0.25, 0.125, -0.125]
    b_pos, b_tris = cube_mesh(1, 0.75, (2.5, -1.5, 0.25))
    b_tris = b_tris[:, [0, 2, 1]]
    angle = np.arange(HUB_FAN) * (2 * np.pi / HUB_FAN)
    ring = np.stack([-3.0 + np.cos(angle), -0.75 + 0.05 * np.sin(3 * angle), 0.5 + np.sin(angle)], axis=-1)
    hub = len(a_pos) + len(b_pos) + HUB_FAN
    ring0 = len(a_pos) + len(b_pos)
    fan = [[ring0 + j, ring0 + (j + 1) % HUB_FAN, hub] for j in range(HUB_FAN)]
    line0 = hub + 1
    line = np.array([[1.0, -1.0, 1.0], [1.25, -0.5, 1.125], [1.5, 0.0, 1.25]]) - [0.0, 1.0, 0.0]  # exact in fp32: the cross product is 0
    pos = np.concatenate([a_pos, b_pos, ring, [[-3.0, -0.25, 0.5]], line]).astype(F)
    tris = np.concatenate([a_tris, b_tris + len(a_pos), np.array(fan, np.uint32), [[line0, line0 + 1, line0 + 2]]]).astype(np.uint32)
    n = len(pos)
    vel = (rng.normal(size=(n, 3)) * 2).astype(F)
    inv_mass = rng.choice(np.array([0.5, 1.0, 2.0], F), n)
    inv_mass[0] = F(0)
    nA, nB = len(a_tris), len(b_tris)
    marks = dict(A=(0, nA), B=(nA, nB), fan=(nA + nB, HUB_FAN), degenerate=nA + nB + HUB_FAN, hub=hub, pinned=0, size=6.0)
    # the fluid's surface: through a point near A's middle, clear of every centroid
    centroids = pos.astype(np.float64)[tris.astype(np.int64)].mean(axis=1)
    for attempt in range(100):
        point = (0.0, 0.0625 + 0.03125 * attempt, 0.0)
        depth = (np.array(point) - centroids) @ np.array(UP)
        if np.abs(depth).min() > MARGIN * marks["size"]:
            break
    assert np.abs(depth).min() > MARGIN * marks["size"]
    marks["surface"] = point
    return pos, vel, inv_mass, tris, marks


def make_loads(n_loads, scene, n_range, seed=0):
    """The type cycles fluid, gas, pressure; every three loads the range moves on through: the first n_range triangles of body A,
    a range that starts mid-tile (first = 100) and runs to the container's end, body B, the cone with the zero-area triangle,
    everything (count = UINT32_MAX from 0), an empty range; every 18 loads the INWARD flag changes; the drag is on for every other
    (range, flag) setting.  So 64 loads take every type with both flag settings and the fluid with and without drag on every
    range; one load is a fluid with drag on A's first n_range triangles."""
    pos, vel, inv_mass, tris, marks = scene
    rng = np.random.default_rng(6000 + seed)
    nT = len(tris)
    ranges = [(0, n_range), (100, TO_END), marks["B"], (marks["fan"][0], HUB_FAN + 1), (0, TO_END), (nT, 0)]
    out = []
    for k in range(n_loads):
        j = k // 3
        first, count = ranges[j % 6]
        phase = j // 6
        about = np.round(rng.uniform(-1, 1, 3) * 16) / 16
        if k % 3 == 0:
            L = capi.SurfaceLoad.fluid(float(F(9.8125 * (1 + 0.125 * phase))), marks["surface"], up=UP, first=first, count=count)
            if (j + phase) % 2 == 0:
                L.with_drag(float(F(0.75 + 0.25 * phase)), np.round(rng.normal(size=3) * 8) / 8)
        elif k % 3 == 1:
            L = capi.SurfaceLoad.gas(1.5, 1.0, first=first, count=count, about=about)
        else:
            L = capi.SurfaceLoad.pressure(float(F(rng.normal() * 2)), first=first, count=count, about=about)
        if phase % 2:
            L.inward()
        if L.type == capi.LOAD_GAS:  # the rest volume: above and below the magnitude of the volume the range has now
            v64 = apply_surface_loads_f64(pos, vel, inv_mass, tris, [L], 0.0)[4][0]
            assert count == 0 or abs(v64) > MARGIN * marks["size"] ** 3, (k, v64)
            L.rest_volume = float(F(max(abs(v64), 0.5) * (0.75, 1.25)[phase // 2 % 2]))
        out.append(L)
    return out


RANGES = (255, 256, 257, 513)  # one tile, the tile edge, two and three tiles of the summation order
LOADS = (1, 3, 64)


def body_m(n_range):
    return 5 if n_range <= 300 else 7  # 300 triangles and 204 nodes, 588 triangles and 348 nodes


_scenes = {}


def shared_scene(n_range, n_loads):
    """(pos, vel, inv_mass, triangles, loads, marks) of one (range, loads) case; built once"""
    key = (n_range, n_loads)
    if key not in _scenes:
        scene = make_body_scene(body_m(n_range))
        _scenes[key] = scene[:4] + (make_loads(n_loads, scene, n_range), scene[4])
    return _scenes[key]


def two_bodies():
    """two closed cubes behind one another in the container, a gas in each; a fluid and a pressure on ranges that overlap"""
    a_pos, a_tris = cube_mesh(3, 1.0, (0.0, -0.5, 0.0))
    b_pos, b_tris = cube_mesh(4, 1.25, (2.0, -1.0, 0.5))
    pos = np.concatenate([a_pos, b_pos]).astype(F)
    tris = np.concatenate([a_tris, b_tris + len(a_pos)]).astype(np.uint32)
    rng = np.random.default_rng(21)
    vel = rng.normal(size=pos.shape).astype(F)
    inv_mass = rng.choice(np.array([0.5, 1.0, 2.0], F), len(pos))
    nA = len(a_tris)
    loads = [capi.SurfaceLoad.gas(2.0, 1.25, first=0, count=nA, about=(0.5, 0.0, 0.5)),
             capi.SurfaceLoad.gas(2.0, 1.5, first=nA, count=None, about=(2.625, -0.375, 1.125)),
             capi.SurfaceLoad.fluid(9.8125, (0.0, 0.03125 + 1.0 / 128, 0.0), up=UP, first=50, count=nA).with_drag(0.5),
             capi.SurfaceLoad.pressure(0.75, first=100, count=150)]
    return pos, vel, inv_mass, tris, loads


def all_cases():
    """every (pos, vel, inv_mass, triangles, loads) the GPU tests use"""
    cases = [single_triangle(), small_cube(), two_bodies()]
    for n_range in RANGES:
        for n_loads in LOADS:
            cases.append(shared_scene(n_range, n_loads)[:5])
    return cases


# ---- restatement against fp64 ---------------------------------------------------------------------------------------------------
# Measured on all_cases() (see test_restatement_against_fp64).  Each gate is 4 x the measured figure rounded up to a power of two.
GATE_VEL_ULP = 4.0         # measured 0.654 ulp
GATE_SUM = 2.0 ** -24      # measured 8.02e-9
GATE_VOLUME = 2.0 ** -18   # measured 8.91e-7
GATE_AREA = 2.0 ** -17     # measured 1.60e-6


def _deviation(pos, vel, inv_mass, tris, loads):
    trace = []
    v32, imp32, tor32, nodes32, vol32, area32 = apply_surface_loads(pos, vel, inv_mass, tris, loads, DT, trace=trace)
    v64, imp64, tor64, affected64, vol64, area64, faces64, terms64 = apply_surface_loads_f64(pos, vel, inv_mass, tris, loads, DT)
    differing = int((affected_of(trace, len(pos)) != affected64).sum())
    for k, _, tri_codes, _ in trace:
        differing += int(((tri_codes == T_IN) != faces64[k]).sum())
    speed = max(np.abs(v64).max(), np.abs(np.asarray(vel, np.float64)).max())
    ulp = float(np.spacing(F(speed)))
    scale = max(np.abs(imp64).max(), np.abs(tor64).max()) * max(1, int(nodes32.max()))
    some = terms64 > 0
    dev_volume = (np.abs(vol32 - vol64)[some] / terms64[some]).max() if some.any() else 0.0
    dev_area = (np.abs(area32 - area64)[some] / area64[some]).max() if some.any() else 0.0
    return (differing, np.abs(v32 - v64).max() / ulp, max(np.abs(imp32 - imp64).max(), np.abs(tor32 - tor64).max()) / scale,
            dev_volume, dev_area)


def test_restatement_against_fp64():
    """The fp32 restatement against the fp64 form on every scene the GPU tests use.  The builders keep every centroid 1e-3 of the
    scene's size away from the fluid's surface and every gas volume 1e-3 of size^3 away from 0, so no depth > 0 and no V > 0
    decision differs: the count is asserted to be 0 and nothing is left out of the comparison.  Velocities are compared in ulp of
    the scene's largest speed, impulse and torque relative to (largest |sum| x most nodes affected), a volume relative to the sum
    of the magnitudes of its terms, an area relative to itself.  Measured: see DESIGN.md 8i; the gates are four times the measured
    figures rounded up to a power of two."""
    worst = np.zeros(4)
    for case in all_cases():
        out = _deviation(*case)
        assert out[0] == 0
        worst = np.maximum(worst, out[1:])
    print("restatement vs fp64: velocities %.3g ulp of the largest speed; sums %.3g relative; volume %.3g; area %.3g" % tuple(worst))
    assert worst[0] <= GATE_VEL_ULP and worst[1] <= GATE_SUM and worst[2] <= GATE_VOLUME and worst[3] <= GATE_AREA


def branches_of(trace):
    """{(type-independent) triangle codes} and {node codes} a trace holds"""
    tri = {int(c) for _, _, codes, _ in trace for c in np.unique(codes)}
    node = {int(c) for _, codes, _, _ in trace for c in np.unique(codes)}
    return tri, node


def test_the_body_scenes_hold_what_they_promise():
    for n_range in (257, 513):
        pos, vel, inv_mass, tris, loads, marks = shared_scene(n_range, 64)
        assert len(tris) == 12 * body_m(n_range) ** 2 + 12 + HUB_FAN + 1 and (len(pos) > TILE) == (n_range == 513)
        assert (tris == marks["hub"]).sum() == HUB_FAN and inv_mass[marks["pinned"]] == 0
        trace = []
        out = apply_surface_loads(pos, vel, inv_mass, tris, loads, DT, trace=trace)
        assert branches_of(trace) == ({T_DEGENERATE, T_ABOVE, T_IN, T_IDLE}, {N_OUT, N_FIXED, N_HIT})
        kinds = {(L.type, L.flags, L.type == capi.LOAD_FLUID and L.drag != 0) for L in loads}
        assert kinds == {(capi.LOAD_PRESSURE, 0, False), (capi.LOAD_PRESSURE, 1, False), (capi.LOAD_GAS, 0, False),
                         (capi.LOAD_GAS, 1, False), (capi.LOAD_FLUID, 0, False), (capi.LOAD_FLUID, 0, True),
                         (capi.LOAD_FLUID, 1, False), (capi.LOAD_FLUID, 1, True)}
        # the first load: a fluid with drag whose surface cuts body A - triangles above and below
        _, node_codes, tri_codes, _ = trace[0]
        assert (tri_codes == T_IN).sum() > 20 and (tri_codes == T_ABOVE).sum() > 20 and node_codes[marks["pinned"]] == N_FIXED
        # a gas in body B: idle without the flag (the body is wound inward: V < 0), acting with it
        gases = [(L, t) for L, t in zip(loads, trace) if L.type == capi.LOAD_GAS and (L.first, L.count) == marks["B"]]
        assert {bool(L.flags): set(np.unique(t[2])) for L, t in gases} == {False: {T_IDLE}, True: {T_IN}}
        for L, t in gases:
            assert (out[4][t[0]] > 0) == bool(L.flags) and abs(abs(out[4][t[0]]) - 0.75 ** 3) < 1e-5
        # the hub's 40-entry row is walked, the zero-area triangle is passed over, an empty range gives zeros
        on_fan = [t for L, t in zip(loads, trace) if L.first == marks["fan"][0] and L.type == capi.LOAD_PRESSURE]
        assert on_fan and all(t[1][marks["hub"]] == N_HIT and t[2][-1] == T_DEGENERATE for t in on_fan)
        empty = [t[0] for L, t in zip(loads, trace) if L.count == 0]
        assert len(empty) >= 3 and not out[3][empty].any() and not out[4][empty].any() and not out[5][empty].any()
        untouched = ~affected_of(trace, len(pos)).any(axis=0)
        assert untouched[marks["pinned"]] and np.array_equal(out[0][untouched].view(np.uint32), vel[untouched].view(np.uint32))


# ---- physics on the fp64 form ----------------------------------------------------------------------------------------------------
def _turned_cube(m=3, size=1.25, centre=(0.5, -3.0, 1.0), angle=0.7):
    pos, tris = cube_mesh(m, size)
    return (pos - size / 2) @ _rotation((0.3, 1.0, -0.6), angle).T + centre, tris


def test_unit_cube_has_volume_1_and_area_6():
    for m in (1, 4):
        pos, tris = cube_mesh(m)
        zero = [capi.SurfaceLoad.pressure(0.0)]
        out = apply_surface_loads_f64(pos, np.zeros_like(pos), np.ones(len(pos)), tris, zero, 0.01)
        assert abs(out[4][0] - 1.0) < 1e-14 and abs(out[5][0] - 6.0) < 1e-14 and out[3].all()
        r = apply_surface_loads(pos, np.zeros_like(pos), np.ones(len(pos)), tris, zero, DT)
        assert r[4][0] == F(1) and r[5][0] == F(6) and not r[1].any() and np.array_equal(r[0], np.zeros_like(r[0]))


def test_shifted_cube_keeps_its_fp32_volume():
    """the 588-triangle cube 1000 units from the origin: the shift by o keeps the volume within the gate"""
    pos, tris = cube_mesh(7, 1.0, (1000.0, -1000.0, 1000.0))
    r = apply_surface_loads(pos, np.zeros_like(pos), np.ones(len(pos)), tris, [capi.SurfaceLoad.pressure(0.0)], DT)
    exact = apply_surface_loads_f64(pos.astype(F), np.zeros_like(pos), np.ones(len(pos)), tris, [capi.SurfaceLoad.pressure(0.0)], DT)
    print("shifted cube: fp32 volume off by %.3g relative" % (abs(float(r[4][0]) - exact[4][0]) / exact[7][0]))
    assert abs(float(r[4][0]) - exact[4][0]) <= GATE_VOLUME * exact[7][0] and abs(float(r[4][0]) - 1.0) < 1e-4


def test_constant_pressure_on_a_closed_surface_sums_to_zero():
    pos, tris = _turned_cube()
    L = capi.SurfaceLoad.pressure(3.0, about=(0.25, -2.5, 1.5))
    v, imp, tor, affected, vol, area, _, _ = apply_surface_loads_f64(pos, np.zeros_like(pos), np.ones(len(pos)), tris, [L], 0.01)
    per_node = 3.0 * area[0] * 0.01
    assert affected.all() and np.abs(imp).max() < 1e-13 * per_node and np.abs(tor).max() < 1e-12 * per_node
    assert np.linalg.norm(v, axis=1).max() > 1e-3 * per_node  # (the nodes do move: outward)


@pytest.mark.parametrize("angle,depth", [(0.0, 1.0), (0.7, 1.0), (2.1, 40.0)])
def test_a_submerged_body_receives_archimedes_force(angle, depth):
    size = 1.25
    pos, tris = _turned_cube(angle=angle, centre=(0.5, -depth - 1.5, 1.0))
    up = np.array([0.0, 1.0, 0.0])
    centre = pos.mean(axis=0)  # (the centre of volume of a cube)
    L = capi.SurfaceLoad.fluid(9.8125, (0.0, 0.0, 0.0), up=up)
    L.point[:] = [0.0, 0.0, 0.0]
    v, imp, tor, affected, vol, _, faces, _ = apply_surface_loads_f64(pos, np.zeros_like(pos), np.ones(len(pos)), tris, [L], 0.01)
    want = 9.8125 * size ** 3 * 0.01 * up
    assert faces[0].all() and np.allclose(imp[0], want, rtol=1e-11, atol=1e-13 * depth)
    arm = np.cross(centre, want)  # the torque about the origin is that of the force at the centre of volume
    assert np.allclose(tor[0], arm, rtol=1e-10, atol=1e-11 * depth)
    # a tilted `up` that is not a unit vector: the force follows it as given
    tilted = capi.SurfaceLoad.fluid(2.0, (0.0, 100.0, 0.0), up=(0.5, 2.0, 0.0))
    imp = apply_surface_loads_f64(pos, np.zeros_like(pos), np.ones(len(pos)), tris, [tilted], 0.01)[1]
    assert np.allclose(imp[0], 2.0 * size ** 3 * 0.01 * np.array([0.5, 2.0, 0.0]), rtol=1e-10)


def test_a_body_above_the_surface_is_not_affected():
    pos, tris = _turned_cube(centre=(0.5, 3.0, 1.0))
    vel = np.random.default_rng(3).normal(size=pos.shape)
    L = capi.SurfaceLoad.fluid(9.81, (0.0, 0.0, 0.0)).with_drag(2.0)
    v, imp, tor, affected, vol, area, faces, _ = apply_surface_loads_f64(pos, vel, np.ones(len(pos)), tris, [L], 0.01)
    assert not affected.any() and not faces[0].any() and np.array_equal(v, vel) and not imp.any() and abs(vol[0] - 1.25 ** 3) < 1e-12
    r = apply_surface_loads(pos.astype(F), vel.astype(F), np.ones(len(pos), F), tris, [L], DT)
    assert r[3].tolist() == [0] and np.array_equal(r[0], vel.astype(F))


def test_gas_at_its_rest_volume_does_nothing_and_changes_sign_across_it():
    pos, tris = cube_mesh(2, 2.0)  # volume 8, exact in both precisions
    n = len(pos)
    outward = pos - pos.mean(axis=0)
    for rest, sign in ((8.0, 0), (10.0, 1), (6.0, -1)):
        L = capi.SurfaceLoad.gas(1.5, rest)
        v = apply_surface_loads_f64(pos, np.zeros_like(pos), np.ones(n), tris, [L], 0.01)[0]
        r = apply_surface_loads(pos.astype(F), np.zeros((n, 3), F), np.ones(n, F), tris, [L], DT)
        for got in (v, r[0].astype(np.float64)):
            along = np.einsum("ij,ij->i", got, outward)
            assert (np.sign(np.where(np.abs(along) < 1e-12, 0.0, along)) == sign).all(), rest
        assert r[3].tolist() == [n] and r[4][0] == F(8)  # (at the rest volume the nodes are affected by a change of zero)
    # the pressure: p0 (V0 / V - 1)
    L = capi.SurfaceLoad.gas(1.5, 10.0)
    top = np.nonzero(pos[:, 1] == 2.0)[0]
    imp = apply_surface_loads_f64(pos, np.zeros_like(pos), np.ones(n), tris, [L], 0.01)[0][top].sum(axis=0)
    assert np.allclose(imp, [0.0, 1.5 * 0.25 * 4.0 * 0.01, 0.0], rtol=1e-12, atol=1e-15)


def test_a_mirrored_mesh_with_the_flag_gives_the_originals_result():
    pos, tris = _turned_cube()
    vel = np.random.default_rng(4).normal(size=pos.shape)
    w = np.random.default_rng(5).choice([0.5, 1.0, 2.0], len(pos))
    loads = [capi.SurfaceLoad.gas(1.5, 3.0), capi.SurfaceLoad.fluid(9.81, (0.0, -3.0, 0.0)).with_drag(0.5), capi.SurfaceLoad.pressure(2.0)]
    flagged = [capi.SurfaceLoad.from_buffer_copy(L).inward() for L in loads]
    a = apply_surface_loads_f64(pos, vel, w, tris, loads, 0.01)
    b = apply_surface_loads_f64(pos, vel, w, tris[:, [0, 2, 1]], flagged, 0.01)
    for x, y in zip(a[:6], b[:6]):
        assert np.allclose(x, y, rtol=1e-12, atol=1e-14)
    assert np.abs(a[1]).max() > 1e-3
    # ... in fp32 to the bit: (a, c, b) of the mirrored triangle are the original's (a, b, c)
    r = apply_surface_loads(pos.astype(F), vel.astype(F), w.astype(F), tris, loads, DT)
    s = apply_surface_loads(pos.astype(F), vel.astype(F), w.astype(F), tris[:, [0, 2, 1]], flagged, DT)
    for x, y in zip(r, s):
        assert np.array_equal(x, y)
    # without the flag the mirrored body's volume is negative and its gas idle
    t = apply_surface_loads(pos.astype(F), vel.astype(F), w.astype(F), tris[:, [0, 2, 1]], loads[:1], DT)
    assert t[4][0] == -r[4][0] and t[3].tolist() == [0]


def test_loads_read_the_state_the_call_found():
    pos, vel, w, tris, loads = small_cube()
    both = apply_surface_loads(pos, vel, w, tris, loads, DT)
    swapped = apply_surface_loads(pos, vel, w, tris, loads[::-1], DT)
    for x, y in zip(both[1:], swapped[1:]):
        assert np.array_equal(x, y[::-1])
    assert np.abs(both[0] - swapped[0]).max() <= 4 * np.spacing(np.abs(both[0]).max())  # (the order of a node's three terms)


# ---- the entry point on a host-only handle ------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device_check():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    L, h = capi.load(), g._h
    n_tris = g.count(capi.TRIANGLES)
    assert n_tris > 8
    inf, nan = float("inf"), float("nan")

    def call(*loads, n=None, null=False, dt=0.01):
        arr = (capi.SurfaceLoad * max(len(loads), 1))(*loads)
        return L.pies_apply_surface_loads(h, len(loads) if n is None else n, None if null else arr, dt, None, None, None, None, None)

    good = [capi.SurfaceLoad.pressure(2.0), capi.SurfaceLoad.gas(1.5, 2.0, first=2, count=n_tris - 2),
            capi.SurfaceLoad.fluid(9.81, (0, 1, 0)).with_drag(0.5, (1, 0, 0)).inward()]
    assert call(n=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()

    def broken(base, **kw):
        f = capi.SurfaceLoad.from_buffer_copy(base)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(f, name)[value[0]] = value[1]
            else:
                setattr(f, name, value)
        return f

    for k in range(3):
        for bad in (3, -1):
            assert call(broken(good[k], type=bad)) == capi.ERR_INVALID, (k, bad)
        for bad in (2, 3, 0x80000000):
            assert call(broken(good[k], flags=bad)) == capi.ERR_INVALID, (k, bad)
        for first, count in ((n_tris + 1, 0), (n_tris + 1, TO_END), (0, n_tris + 1), (n_tris - 1, 2), (5, TO_END - 1), (TO_END, 1)):
            assert call(broken(good[k], first=first, count=count)) == capi.ERR_INVALID and "range" in g.last_error(), (k, first, count)
        for first, count in ((n_tris, 0), (n_tris, TO_END), (0, n_tris), (n_tris - 1, 1), (3, 0)):
            assert call(broken(good[k], first=first, count=count)) == capi.ERR_HIP, (k, first, count)
        for name in ("point", "up", "velocity"):
            for bad in (nan, inf, -inf):
                assert call(broken(good[k], **{name: (2, bad)})) == capi.ERR_INVALID, (k, name, bad)
        for name in ("strength", "rest_volume", "drag"):
            for bad in (nan, inf, -inf):
                assert call(broken(good[k], **{name: bad})) == capi.ERR_INVALID, (k, name, bad)
        assert call(broken(good[k], drag=-0.5)) == capi.ERR_INVALID and "drag" in g.last_error()
    for bad in (0.0, -1.0):
        assert call(broken(good[1], rest_volume=bad)) == capi.ERR_INVALID and "rest_volume" in g.last_error(), bad
        assert call(broken(good[0], rest_volume=bad)) == capi.ERR_HIP  # (only a gas reads it)
    for bad in (-0.01, nan, inf, -inf):
        assert call(*good, dt=bad) == capi.ERR_INVALID and "dt" in g.last_error(), bad
    assert call(good[0], broken(good[0], drag=-1.0)) == capi.ERR_INVALID and "load 1" in g.last_error()
    assert call(*([good[0]] * 65)) == capi.ERR_UNSUPPORTED
    assert call(*good) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert call(*([good[2]] * 64)) == capi.ERR_HIP and call(*good, dt=0.0) == capi.ERR_HIP
    assert call() == capi.OK and call(n=0, null=True) == capi.OK
    with pytest.raises(capi.PiesError):
        g.apply_surface_loads(good, 0.01)
    assert g.apply_surface_loads([], 0.01, reaction=False) is None
    assert L.pies_apply_surface_loads(None, 0, None, 0.01, None, None, None, None, None) == capi.ERR_INVALID


def test_binding_declares_the_entry_point():
    assert "pies_apply_surface_loads" in capi.SYMBOLS and capi.LOAD_MAX == 64 and C.sizeof(capi.SurfaceLoad) == 64
    L = capi.load()
    assert L.pies_apply_surface_loads.restype is C.c_int and len(L.pies_apply_surface_loads.argtypes) == 9
    assert L.pies_abi_version() == 4
    f = capi.SurfaceLoad.fluid(9.81, (1, 2, 3), up=(0, 0, 1), first=4, count=5).with_drag(0.5, (1, 0, 0)).inward()
    assert (f.type, f.flags, f.first, f.count, list(f.point), list(f.up), f.drag) == (capi.LOAD_FLUID, 1, 4, 5, [1.0, 2.0, 3.0], [0.0, 0.0, 1.0], 0.5)
    assert capi.SurfaceLoad.gas(1.0, 2.0).count == TO_END and capi.SurfaceLoad.pressure(1.0).rest_volume == 0.0
