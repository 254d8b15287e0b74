"""CPU tests of pies_apply_forces: the numpy fp32 restatement of the rule of include/pies_hip.h (`apply_forces`, the yardstick the
device has to match bit for bit in tests/test_forces_gpu.py), an independent fp64 formulation it is held to, physics checks on
that formulation, and the argument checks of the entry point on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi

F = np.float32
TILE = 256
DT = F(0.0125)

# branch codes of one (node, force) pair (apply_forces(..., trace=[])): what the GPU test asserts the coverage of
B_OUT, B_FIXED, B_DD0, B_HIT = 0, 1, 2, 64  # an affected pair: B_HIT + type + 8 * falloff + 32 * (IS_FORCE of the three types that read it)
# ... and of one (triangle, wind) pair
T_DEGENERATE, T_OUT, T_IN = 0, 1, 2


def hit_code(type, falloff, is_force=0):
    return B_HIT + type + 8 * falloff + 32 * is_force


POINT_TYPES = (capi.FORCE_DIRECTIONAL, capi.FORCE_RADIAL, capi.FORCE_VORTEX, capi.FORCE_DRAG)
FALLOFFS = (capi.FALLOFF_NONE, capi.FALLOFF_LINEAR, capi.FALLOFF_SMOOTH)
# every (type, falloff, flag) a list of point forces can take
ALL_HITS = {hit_code(t, f, i) for t in POINT_TYPES[:3] for f in FALLOFFS for i in (0, 1)} | {hit_code(capi.FORCE_DRAG, f) for f in FALLOFFS}


# ---- the restatement: fp32, no fused multiply-adds, the operation order of the header -------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _fminf(a, b):
    """fminf: the other operand when one is a NaN"""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    return np.where(np.isnan(b) | (a < b) | ((a == b) & np.signbit(a)), a, b).astype(F)


def _vec(a):
    return np.array(list(a), F)


def _region(f, x):
    """(inside, d, dd, fall) of force f's region at the points x (m x 3)"""
    r = F(f.radius)
    d = x - _vec(f.centre)[None]
    dd = _dot(d, d)
    rr = r * r
    if f.falloff == capi.FALLOFF_LINEAR:
        fall = F(1) - np.sqrt(dd) / r
    elif f.falloff == capi.FALLOFF_SMOOTH:
        u = F(1) - dd / rr
        fall = u * u
    else:
        fall = np.ones(len(x), F)
    return dd < rr, d, dd, fall.astype(F)


def _is_force(f):
    return int(bool(f.flags & capi.FORCE_IS_FORCE)) if f.type != capi.FORCE_DRAG else 0


def _point(f, dt, pos, vel, w):
    """(affected, dv, codes) of a point force for all nodes (the caller masks invMass == 0)"""
    inside, d, dd, fall = _region(f, pos)
    vector = _vec(f.vector)
    ok = inside.copy()
    if f.type == capi.FORCE_DRAG:
        k = _fminf(F(f.strength) * dt, F(1))
        dv = (vector[None] - vel) * (k * fall)[:, None]
    else:
        a = np.broadcast_to(vector[None], pos.shape)
        if f.type == capi.FORCE_RADIAL:
            ok &= dd > 0
            a = (d / np.sqrt(np.where(dd > 0, dd, F(1)))[:, None]) * F(f.strength)
        elif f.type == capi.FORCE_VORTEX:
            a = _cross(vector[None], d) * F(f.strength)
        if f.flags & capi.FORCE_IS_FORCE:
            a = a * w[:, None]
        dv = a * (fall * dt)[:, None]
    codes = np.where(inside, np.where(ok, hit_code(f.type, f.falloff, _is_force(f)), B_DD0), B_OUT)
    return ok, dv.astype(F), codes


def _wind(f, dt, pos, vel, w, tris):
    """(affected, dv, node codes, triangle codes) of a wind: per node the sum over its (triangle, corner) entries in ascending
    triangle index from 0"""
    n = len(pos)
    dv, hit, named = np.zeros((n, 3), F), np.zeros(n, bool), np.zeros(n, bool)
    tri_codes = np.zeros(len(tris), np.int64)
    if len(tris):
        a, b, c = pos[tris[:, 0]], pos[tris[:, 1]], pos[tris[:, 2]]
        N = _cross(b - a, c - a)
        nn = _dot(N, N)
        solid = nn > 0
        length = np.sqrt(np.where(solid, nn, F(1)))
        unit = N / length[:, None]
        area = F(0.5) * length
        inside, _, _, fall = _region(f, ((a + b) + c) / F(3))
        rel = _vec(f.vector)[None] - ((vel[tris[:, 0]] + vel[tris[:, 1]]) + vel[tris[:, 2]]) / F(3)
        vn = _dot(rel, unit)
        force = (unit * (F(f.strength) * vn)[:, None] + (rel - unit * vn[:, None]) * F(f.shear)) * (area * fall)[:, None]
        third = (force / F(3)).astype(F)
        tri_codes = np.where(solid, np.where(inside, T_IN, T_OUT), T_DEGENERATE)
        for t in np.nonzero(solid & inside)[0]:
            for node in tris[t]:
                named[node] = True
                if w[node] != 0:
                    dv[node] = dv[node] + third[t] * (dt * w[node])
                    hit[node] = True
    codes = np.where(hit, hit_code(f.type, f.falloff), np.where(named, B_FIXED, B_OUT))
    return hit, dv, codes, tri_codes


def apply_forces(pos, vel, inv_mass, forces, dt, triangles=None, trace=None):
    """The rule of pies_apply_forces in numpy fp32.  Returns (vel, impulse, torque, nodes).  Every force reads pos and vel as they
    are given; a node's changes are added in ascending force index from 0 and the sum to its velocity; the reaction sums are taken
    per tile of 256 node ids in ascending id from 0, then over the tiles in ascending index from 0.  trace: a list that receives
    (force, branch code per node, branch code per triangle or None) of every force."""
    with np.errstate(all="ignore"):
        pos, vel = (np.array(a, F).reshape(-1, 3).copy() for a in (pos, vel))
        w = np.asarray(inv_mass, F).reshape(-1)
        tris = np.zeros((0, 3), np.int64) if triangles is None else np.asarray(triangles, np.int64).reshape(-1, 3)
        dt = F(dt)
        n, k = len(pos), len(forces)
        movable = ~(w == 0)
        safe_w = np.where(movable, w, F(1))
        J, T = np.zeros((k, n, 3), F), np.zeros((k, n, 3), F)
        affected = np.zeros((k, n), bool)
        total = np.zeros((n, 3), F)
        for i, f in enumerate(forces):
            if f.type == capi.FORCE_WIND:
                hit, dv, codes, tri_codes = _wind(f, dt, pos, vel, w, tris)
            else:
                hit, dv, codes = _point(f, dt, pos, vel, w)
                tri_codes = None
                codes = np.where(~movable & (codes != B_OUT), B_FIXED, codes)
            hit = hit & movable
            total[hit] = total[hit] + dv[hit]
            j = dv * (F(1) / safe_w)[:, None]
            tq = _cross(pos - _vec(f.centre)[None], j)
            J[i][hit], T[i][hit] = j[hit], tq[hit]
            affected[i] = hit
            if trace is not None:
                trace.append((i, codes, tri_codes))
        out = vel.copy()
        any_hit = affected.any(axis=0)
        out[any_hit] = vel[any_hit] + total[any_hit]
        impulse, torque = np.zeros((k, 3), F), np.zeros((k, 3), F)
        for first in range(0, n, TILE):
            si, st = np.zeros((k, 3), F), np.zeros((k, 3), F)
            for node in range(first, min(first + TILE, n)):
                si, st = si + J[:, node], st + T[:, node]  # (a node not affected adds 0)
            impulse, torque = impulse + si, torque + st
        return out, impulse, torque, affected.sum(axis=1).astype(np.uint32)


def affected_of(trace, n):
    return np.array([codes >= B_HIT for _, codes, _ in trace]).reshape(len(trace), n)


# ---- an independent fp64 formulation: plain vector geometry -----------------------------------------------------------------------
def _weight64(f, x):
    """inside and falloff of f's sphere at the points x, from distances (not squared ones)"""
    c, r = np.array(list(f.centre), np.float64), float(f.radius)
    dist = np.linalg.norm(x - c, axis=-1)
    s = dist / r if np.isfinite(r) else np.zeros_like(dist)
    fall = {capi.FALLOFF_NONE: np.ones_like(s), capi.FALLOFF_LINEAR: 1.0 - s, capi.FALLOFF_SMOOTH: (1.0 - s * s) ** 2}[f.falloff]
    return dist < r, fall, dist


def apply_forces_f64(pos, vel, inv_mass, forces, dt, triangles=None):
    """Returns (vel, impulse, torque, affected (k x n), triangle decisions per wind {force: inside (t)})."""
    x, v = np.array(pos, np.float64).reshape(-1, 3), np.array(vel, np.float64).reshape(-1, 3)
    w = np.asarray(inv_mass, np.float64).reshape(-1)
    tris = np.zeros((0, 3), np.int64) if triangles is None else np.asarray(triangles, np.int64).reshape(-1, 3)
    dt = float(dt)
    n, k = len(x), len(forces)
    movable = w != 0
    mass = np.where(movable, 1.0 / np.where(movable, w, 1.0), 0.0)
    change = np.zeros((k, n, 3))
    affected = np.zeros((k, n), bool)
    faces = {}
    for i, f in enumerate(forces):
        c, u = np.array(list(f.centre), np.float64), np.array(list(f.vector), np.float64)
        if f.type == capi.FORCE_WIND:
            corners, speeds = x[tris], v[tris]  # t x 3 x 3
            normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
            twice = np.linalg.norm(normal, axis=1)
            inside, fall, _ = _weight64(f, corners.mean(axis=1))
            use = (twice > 0) & inside
            faces[i] = use
            unit = normal[use] / twice[use][:, None]
            rel = u - speeds[use].mean(axis=1)
            along = np.einsum("ij,ij->i", rel, unit)[:, None] * unit
            push = (float(f.strength) * along + float(f.shear) * (rel - along)) * (0.5 * twice[use] * fall[use])[:, None]
            count = np.zeros(n)
            for corner in range(3):
                ids = tris[use][:, corner]
                np.add.at(change[i], ids, push / 3.0 * (dt * w[ids])[:, None])
                np.add.at(count, ids, 1.0)
            affected[i] = (count > 0) & movable
        else:
            inside, fall, dist = _weight64(f, x)
            if f.type == capi.FORCE_DRAG:
                change[i] = (u - v) * (min(float(f.strength) * dt, 1.0) * fall)[:, None]
            else:
                if f.type == capi.FORCE_RADIAL:
                    inside = inside & (dist > 0)
                    acc = float(f.strength) * (x - c) / np.where(dist > 0, dist, 1.0)[:, None]
                elif f.type == capi.FORCE_VORTEX:
                    acc = float(f.strength) * np.cross(u, x - c)
                else:
                    acc = np.broadcast_to(u, x.shape)
                if f.flags & capi.FORCE_IS_FORCE:
                    acc = acc * w[:, None]
                change[i] = acc * (fall * dt)[:, None]
            affected[i] = inside & movable
        change[i][~affected[i]] = 0.0
    out = v + change.sum(axis=0)
    momentum = change * mass[None, :, None]
    impulse = momentum.sum(axis=1)
    arms = x[None] - np.array([list(f.centre) for f in forces], np.float64).reshape(k, 1, 3)
    torque = np.cross(arms, momentum).sum(axis=1)
    return out, impulse, torque, affected, faces


# ---- test scenes (shared with tests/test_forces_gpu.py) ---------------------------------------------------------------------------
MARGIN = 1e-3  # of a region's radius: nothing the regions are asked about lies closer to a region's surface


def _near_a_surface(points, forces):
    """per point: within MARGIN * radius of some force's region surface (fp64)"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    near = np.zeros(len(points), bool)
    for f in forces:
        if np.isfinite(f.radius):
            dist = np.linalg.norm(points - np.array(list(f.centre), np.float64), axis=1)
            near |= np.abs(dist - float(f.radius)) < MARGIN * float(f.radius)
    return near


def make_forces(n_forces, seed=0):
    """point forces: the type cycles radial, vortex, drag, directional, the falloff none, linear, smooth, the IS_FORCE flag
    alternates and changes phase every 12 - so 24 forces take every (type, falloff, flag); one region in five is everywhere"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for k in range(n_forces):
        centre = np.round(rng.uniform(-5, 5, 3) * 16) / 16
        is_force = bool((k // 12 + k) % 2)
        kind = (capi.FORCE_RADIAL, capi.FORCE_VORTEX, capi.FORCE_DRAG, capi.FORCE_DIRECTIONAL)[k % 4]
        if kind == capi.FORCE_RADIAL:
            f = capi.Force.radial(centre, float(F(rng.normal() * 4)), is_force=is_force)
        elif kind == capi.FORCE_VORTEX:
            f = capi.Force.vortex(centre, rng.normal(size=3), float(F(rng.normal() * 2)), is_force=is_force)
        elif kind == capi.FORCE_DRAG:
            f = capi.Force.drag(float(F(rng.uniform(0.5, 120.0))), velocity=rng.normal(size=3))  # (some reach the cap at dt = 1 / 80)
        else:
            f = capi.Force.directional(rng.normal(size=3) * 5, is_force=is_force)
        f.within(centre, float("inf") if k % 5 == 4 else float(F(rng.uniform(3.0, 6.0))), FALLOFFS[k % 3])
        out.append(f)
    return out


def make_scene(n_nodes, n_forces, seed=0):
    """(pos, vel, inv_mass, forces): loose nodes with random velocity, invMass in {0, 0.25, 0.5, 1, 2}; node 0 sits exactly at the
    centre of force 0 (a radial one) with invMass 1; every node keeps MARGIN from every region's surface"""
    rng = np.random.default_rng(seed * 7919 + n_nodes * 31 + n_forces)
    forces = make_forces(n_forces, seed)
    pos = rng.uniform(-6, 6, (n_nodes, 3)).astype(F)
    vel = (rng.normal(size=(n_nodes, 3)) * 3).astype(F)
    inv_mass = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], F), n_nodes)
    pos[0], inv_mass[0] = _vec(forces[0].centre), F(1)
    for _ in range(100):
        near = _near_a_surface(pos, forces)
        if not near.any():
            break
        pos[near] = rng.uniform(-6, 6, (int(near.sum()), 3)).astype(F)
    assert not _near_a_surface(pos, forces).any()
    return pos, vel, inv_mass, forces


GRID_W, GRID_H, HUB_FAN = 17, 16, 40


def make_cloth(seed=0):
    """(pos, vel, inv_mass, triangles, forces, marks): a 17 x 16 grid of nodes, triangulated (272 nodes, 480 triangles), gently
    waved; a hub node with a fan of 40 triangles around it; three nodes on a line and the zero-area triangle on them; five nodes
    in no triangle; the grid's first corner pinned (invMass 0).  Forces: a wind whose region cuts the sheet (linear falloff), a
    wind everywhere with shear, a drag.  marks: the ids the GPU test looks up in the trace."""
    rng = np.random.default_rng(3000 + seed)
    gx, gy = np.meshgrid(np.arange(GRID_W), np.arange(GRID_H), indexing="ij")
    grid = np.stack([gx * 0.25, 2.0 + 0.15 * np.sin(gx * 0.7) * np.cos(gy * 0.5), gy * 0.25], axis=-1).reshape(-1, 3)
    node = lambda i, j: i * GRID_H + j
    tris = []
    for i in range(GRID_W - 1):
        for j in range(GRID_H - 1):
            tris += [[node(i, j), node(i + 1, j), node(i + 1, j + 1)], [node(i, j), node(i + 1, j + 1), node(i, j + 1)]]
    hub = len(grid)
    angle = np.arange(HUB_FAN) * (2 * np.pi / HUB_FAN)
    ring = np.stack([6.0 + np.cos(angle), 2.0 + 0.2 * np.sin(3 * angle), 1.0 + np.sin(angle)], axis=-1)
    fan = [[hub, hub + 1 + j, hub + 1 + (j + 1) % HUB_FAN] for j in range(HUB_FAN)]
    line0 = hub + 1 + HUB_FAN
    line = np.array([[1.0, 3.0, 1.0], [1.25, 3.5, 1.125], [1.5, 4.0, 1.25]])  # exact in fp32: the cross product is 0, not tiny
    loose0 = line0 + 3
    loose = rng.uniform(0, 4, (5, 3))
    pos = np.concatenate([grid, [[6.0, 2.5, 1.0]], ring, line, loose]).astype(F)
    degenerate = len(tris) + len(fan)
    tris = np.array(tris + fan + [[line0, line0 + 1, line0 + 2]], np.uint32)
    n = len(pos)
    vel = (rng.normal(size=(n, 3)) * 2).astype(F)
    inv_mass = rng.choice(np.array([0.5, 1.0, 2.0], F), n)
    inv_mass[0] = F(0)
    centroids = pos.astype(np.float64)[tris.astype(np.int64)].mean(axis=1)
    asked = np.concatenate([centroids, pos.astype(np.float64)])  # what the regions are asked about

    def clear_of_all(build):
        """the first of a family of regions that keeps MARGIN from every centroid and every node"""
        for attempt in range(100):
            f = build(0.03125 * attempt)
            if not _near_a_surface(asked, [f]).any():
                return f

    cut = clear_of_all(lambda s: capi.Force.wind((6.0, 1.0, -2.0), 1.5, shear=0.25).within((2.0 + s, 2.0, 1.75), 1.625, capi.FALLOFF_LINEAR))
    brake = clear_of_all(lambda s: capi.Force.drag(4.0, velocity=(0.5, 0.0, 0.0)).within((6.0, 2.0, 1.0), 2.5 + s, capi.FALLOFF_SMOOTH))
    forces = [cut, capi.Force.wind((-1.0, 0.5, 4.0), 0.75, shear=0.5), brake]
    assert not _near_a_surface(centroids, forces).any() and not _near_a_surface(pos, forces).any()
    marks = dict(hub=hub, degenerate=degenerate, pinned=0, loose=list(range(loose0, n)), grid=len(grid))
    return pos, vel, inv_mass, tris, forces, marks


def single_triangle():
    pos = F([[0.0, 1.0, 0.0], [1.0, 1.25, 0.0], [0.25, 1.5, 1.0]])
    vel = F([[0.5, 0.0, -1.0], [0.0, 0.25, 0.0], [-0.5, 1.0, 0.5]])
    return pos, vel, F([1.0, 0.5, 2.0]), np.array([[0, 1, 2]], np.uint32), [capi.Force.wind((3.0, -1.0, 2.0), 1.25, shear=0.5)]


# ---- restatement against fp64 ---------------------------------------------------------------------------------------------------
# Measured on the scenes below (the GPU tests' scenes): see test_restatement_against_fp64.  Each gate is 4 x the measured figure
# rounded up to a power of two.
GATE_VEL_ULP = 16.0
GATE_SUM = 2.0 ** -23


def _deviation(pos, vel, inv_mass, forces, triangles=None):
    trace = []
    v32, imp32, tor32, nodes32 = apply_forces(pos, vel, inv_mass, forces, DT, triangles, trace=trace)
    v64, imp64, tor64, affected64, faces64 = apply_forces_f64(pos, vel, inv_mass, forces, DT, triangles)
    differing = int((affected_of(trace, len(pos)) != affected64).sum())
    for k, _, tri_codes in trace:
        if tri_codes is not None:
            differing += int(((tri_codes == T_IN) != faces64[k]).sum())
    speed = max(np.abs(v64).max(), np.abs(np.asarray(vel, np.float64)).max())
    ulp = float(np.spacing(F(speed)))
    scale = max(np.abs(imp64).max(), np.abs(tor64).max()) * max(1, int(nodes32.max()))
    return differing, np.abs(v32 - v64).max() / ulp, max(np.abs(imp32 - imp64).max(), np.abs(tor32 - tor64).max()) / scale


def test_restatement_against_fp64():
    """The fp32 restatement against the plain fp64 geometry on the scenes the GPU tests use (600 loose nodes with 3 and 64 point
    forces, the cloth, the single triangle).  With the builders' margin of 1e-3 of a radius around every region's surface no
    inside / outside decision differs, for any (node, force) or (triangle, wind) pair: the count is asserted to be 0 and nothing is
    left out of the comparison.  Velocities deviate by at most 2.8 ulp of the scene's largest speed (the 64-force scene: a node's
    change is a sum of up to 64 terms, each with the conditioning of d / |d| or of the triangle normal), the sums of impulse and
    torque by at most 2.53e-8 of (largest |sum| x most nodes affected); the gates are 16 ulp and 2^-23, four times the measured
    figures rounded up to a power of two."""
    worst_vel, worst_sum = 0.0, 0.0
    cases = [make_scene(600, 3) + (None,), make_scene(600, 64) + (None,)]
    cloth = make_cloth()
    cases.append((cloth[0], cloth[1], cloth[2], cloth[4], cloth[3]))
    tri = single_triangle()
    cases.append((tri[0], tri[1], tri[2], tri[4], tri[3]))
    for pos, vel, inv_mass, forces, triangles in cases:
        differing, dev_vel, dev_sum = _deviation(pos, vel, inv_mass, forces, triangles)
        assert differing == 0
        worst_vel, worst_sum = max(worst_vel, dev_vel), max(worst_sum, dev_sum)
    print("restatement vs fp64: velocities %.3g ulp of the largest speed; sums %.3g relative" % (worst_vel, worst_sum))
    assert worst_vel <= GATE_VEL_ULP and worst_sum <= GATE_SUM


def branches_of(trace):
    return {int(c) for _, codes, _ in trace for c in np.unique(codes)}


def required_branches(n_forces):
    """what a list of make_forces(n_forces) can reach: three forces hold three of the four point types (radial, vortex, drag),
    all three falloffs and both IS_FORCE settings; 24 and more hold every (type, falloff, flag)"""
    hits = ALL_HITS if n_forces >= 24 else {hit_code(f.type, f.falloff, _is_force(f)) for f in make_forces(n_forces)}
    return hits | {B_OUT, B_FIXED, B_DD0}


def test_every_branch_occurs_in_the_shared_scenes():
    three = required_branches(3)
    assert {(c - B_HIT) & 7 for c in three if c >= B_HIT} == {capi.FORCE_RADIAL, capi.FORCE_VORTEX, capi.FORCE_DRAG}
    assert {((c - B_HIT) >> 3) & 3 for c in three if c >= B_HIT} == set(FALLOFFS) and {(c - B_HIT) >> 5 for c in three if c >= B_HIT} == {0, 1}
    assert required_branches(64) == ALL_HITS | {B_OUT, B_FIXED, B_DD0}
    for n_nodes in (255, 257, 600):
        for n_forces in (3, 64):
            pos, vel, inv_mass, forces = make_scene(n_nodes, n_forces)
            trace = []
            out = apply_forces(pos, vel, inv_mass, forces, DT, trace=trace)
            assert branches_of(trace) == required_branches(n_forces), (n_nodes, n_forces)
            assert (out[3] > 0).all() and (out[3] < n_nodes).all()
            untouched = ~affected_of(trace, n_nodes).any(axis=0)
            assert np.array_equal(out[0][untouched].view(np.uint32), vel[untouched].view(np.uint32))
    capped = [f for f in make_forces(64) if f.type == capi.FORCE_DRAG and F(f.strength) * DT >= 1]
    assert capped and len(capped) < 16  # the drag's cap is reached by some and not by all


def test_the_cloth_scene_holds_what_it_promises():
    pos, vel, inv_mass, tris, forces, marks = make_cloth()
    assert marks["grid"] == 272 and len(pos) > TILE and (tris == marks["hub"]).sum() == HUB_FAN
    trace = []
    out = apply_forces(pos, vel, inv_mass, forces, DT, tris, trace=trace)
    (_, cut_nodes, cut_tris), (_, all_nodes, all_tris), (_, drag_nodes, _) = trace
    assert cut_tris[marks["degenerate"]] == T_DEGENERATE and all_tris[marks["degenerate"]] == T_DEGENERATE
    assert (cut_tris == T_IN).sum() > 20 and (cut_tris == T_OUT).sum() > 20  # the region cuts the sheet
    assert (all_tris == T_IN).sum() == len(tris) - 1
    assert all_nodes[marks["hub"]] >= B_HIT and all_nodes[marks["pinned"]] == B_FIXED and inv_mass[marks["pinned"]] == 0
    assert (all_nodes[marks["loose"]] == B_OUT).all() and (all_nodes[-8:-5] == B_OUT).all()  # no triangle; a degenerate one only
    assert np.array_equal(out[0][marks["pinned"]], vel[marks["pinned"]])
    assert out[3][1] == marks["grid"] - 1 + 1 + HUB_FAN and 0 < out[3][0] < out[3][1] and out[3][2] > 0


# ---- physics on the fp64 form ----------------------------------------------------------------------------------------------------
def _sheet64(n=6):
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([gx * 0.5, np.full_like(gx, 1.0, dtype=np.float64), gy * 0.5], axis=-1).reshape(-1, 3)
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            tris += [[a, b, c], [a, c, d]]
    return pos, np.array(tris)


def test_flat_sheet_facing_a_uniform_wind():
    pos, tris = _sheet64()
    area = (0.5 * 5) ** 2
    wind = capi.Force.wind((0.0, -3.0, 0.0), 1.75, shear=0.5)
    v, imp, tor, affected, _ = apply_forces_f64(pos, np.zeros_like(pos), np.full(len(pos), 2.0), [wind], 0.01, tris)
    assert np.allclose(imp[0], [0.0, -1.75 * area * 3.0 * 0.01, 0.0], rtol=1e-12, atol=1e-15) and affected.all()
    # wind along the sheet: only the shear term acts
    along = capi.Force.wind((2.0, 0.0, 0.0), 1.75, shear=0.5)
    imp = apply_forces_f64(pos, np.zeros_like(pos), np.ones(len(pos)), [along], 0.01, tris)[1]
    assert np.allclose(imp[0], [0.5 * area * 2.0 * 0.01, 0.0, 0.0], rtol=1e-12, atol=1e-15)


def test_a_triangle_moving_with_the_wind_receives_nothing():
    pos, vel, w, tris, _ = single_triangle()
    u = (3.0, -1.0, 2.0)
    moving = np.tile(np.array(u), (3, 1))
    v, imp, tor, affected, _ = apply_forces_f64(pos, moving, w, [capi.Force.wind(u, 2.0, shear=1.0)], 0.01, tris)
    assert np.array_equal(v, moving) and not imp.any() and affected.all()


def test_winding_does_not_matter_to_the_wind():
    pos, vel, w, tris, forces = single_triangle()
    a = apply_forces_f64(pos, vel, w, forces, 0.01, tris)
    b = apply_forces_f64(pos, vel, w, forces, 0.01, tris[:, ::-1])
    assert np.abs(a[1]).max() > 1e-3 and np.allclose(a[1], b[1], rtol=1e-13) and np.allclose(a[0], b[0], rtol=1e-13)
    r = apply_forces(pos, vel, w, forces, DT, tris)  # ... and in fp32 within rounding
    s = apply_forces(pos, vel, w, forces, DT, tris[:, ::-1])
    assert np.allclose(r[1], s[1], rtol=1e-5)


def test_radial_force_on_a_symmetric_cloud_sums_to_zero():
    rng = np.random.default_rng(7)
    half = rng.uniform(-1, 1, (200, 3))
    centre = np.array([0.5, -0.25, 1.0])
    pos = np.concatenate([centre + half, centre - half])
    blast = capi.Force.radial(centre, 5.0, is_force=True).within(centre, 4.0, capi.FALLOFF_SMOOTH)
    v, imp, tor, affected, _ = apply_forces_f64(pos, np.zeros_like(pos), np.ones(len(pos)), [blast], 0.01)
    per_node = 5.0 * 0.01
    assert affected.all() and np.abs(imp).max() < 1e-12 * per_node * len(pos) and np.abs(tor).max() < 1e-12 * per_node * len(pos)
    assert np.linalg.norm(v, axis=1).max() > 0.1 * per_node


def test_drag_at_its_cap_brings_the_velocity_to_the_mediums():
    rng = np.random.default_rng(8)
    pos, vel = rng.uniform(-1, 1, (50, 3)), rng.normal(size=(50, 3))
    for strength in (80.0, 1000.0):
        out = apply_forces_f64(pos, vel, np.ones(50), [capi.Force.drag(strength, velocity=(0.5, -1.0, 0.25))], 0.0125)[0]
        assert np.allclose(out, [0.5, -1.0, 0.25], rtol=0, atol=1e-14)
    r = apply_forces(pos.astype(F), vel.astype(F), np.ones(50, F), [capi.Force.drag(80.0, velocity=(0.5, -1.0, 0.25))], DT)[0]
    assert np.abs(r - F([0.5, -1.0, 0.25])).max() <= 4 * np.spacing(F(4.0))
    half = apply_forces_f64(pos, vel, np.ones(50), [capi.Force.drag(40.0)], 0.0125)[0]
    assert np.allclose(half, 0.5 * vel)


# ---- known answers of the restatement ---------------------------------------------------------------------------------------------
def test_forces_read_the_state_the_call_found():
    pos, vel, w, dt = F([[0.0, 0.0, 0.0]]), F([[1.0, 0.0, 0.0]]), F([0.5]), F(1.0 / 64)
    push, brake = capi.Force.directional((0.0, 8.0, 0.0)), capi.Force.drag(32.0)
    both = apply_forces(pos, vel, w, [push, brake], dt)
    swapped = apply_forces(pos, vel, w, [brake, push], dt)
    assert np.array_equal(both[0], F([[0.5, 0.125, 0.0]])) and np.array_equal(both[0], swapped[0])  # the drag brakes (1, 0, 0), not the pushed velocity
    assert np.array_equal(both[1][0], F([0.0, 0.25, 0.0])) and np.array_equal(both[1][1], F([-1.0, 0.0, 0.0]))
    force = apply_forces(pos, vel, w, [capi.Force.directional((0.0, 8.0, 0.0), is_force=True)], dt)
    assert np.array_equal(force[0], F([[1.0, 0.0625, 0.0]])) and force[3].tolist() == [1]


def test_a_node_on_the_surface_is_outside():
    f = capi.Force.directional((1.0, 0.0, 0.0)).within((0.0, 0.0, 0.0), 2.0)
    pos = F([[2.0, 0.0, 0.0], [np.nextafter(F(2.0), F(0.0)), 0.0, 0.0]])
    out = apply_forces(pos, np.zeros((2, 3), F), np.ones(2, F), [f], DT)
    assert out[3].tolist() == [1] and not out[0][0].any() and out[0][1][0] == DT


# ---- the entry point on a host-only handle ------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device_check():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    L, h = capi.load(), g._h
    inf, nan = float("inf"), float("nan")

    def call(*forces, n=None, null=False, dt=0.01):
        arr = (capi.Force * max(len(forces), 1))(*forces)
        return L.pies_apply_forces(h, len(forces) if n is None else n, None if null else arr, dt, None, None, None)

    good = [capi.Force.directional((0, -1, 0)), capi.Force.radial((0, 0, 0), 2.0).within((0, 0, 0), 3.0, capi.FALLOFF_LINEAR),
            capi.Force.vortex((0, 0, 0), (0, 1, 0)), capi.Force.drag(2.0), capi.Force.wind((1, 0, 0), 1.0, shear=0.5)]
    assert call(n=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()

    def broken(base, **kw):
        f = capi.Force.from_buffer_copy(base)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(f, name)[value[0]] = value[1]
            else:
                setattr(f, name, value)
        return f

    for k in range(5):
        for bad in (5, -1):
            assert call(broken(good[k], type=bad)) == capi.ERR_INVALID, (k, bad)
        for bad in (3, -1):
            assert call(broken(good[k], falloff=bad)) == capi.ERR_INVALID, (k, bad)
        for bad in (-0.5, nan, -inf):
            assert call(broken(good[k], radius=bad)) == capi.ERR_INVALID, (k, bad)
        for name in ("centre", "vector"):
            for bad in (nan, inf, -inf):
                assert call(broken(good[k], **{name: (1, bad)})) == capi.ERR_INVALID, (k, name, bad)
        for name in ("strength", "shear"):
            for bad in (nan, inf, -inf):
                assert call(broken(good[k], **{name: bad})) == capi.ERR_INVALID, (k, name, bad)
        assert call(broken(good[k], radius=inf)) == capi.ERR_HIP and call(broken(good[k], radius=0.0)) == capi.ERR_HIP
    for bad in (-0.01, nan, inf, -inf):
        assert call(*good, dt=bad) == capi.ERR_INVALID and "dt" in g.last_error(), bad
    assert call(good[0], broken(good[0], radius=-1.0)) == capi.ERR_INVALID and "force 1" in g.last_error()
    assert call(*([good[0]] * 65)) == capi.ERR_UNSUPPORTED
    assert call(*good) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert call(*([good[4]] * 64)) == capi.ERR_HIP and call(*good, dt=0.0) == capi.ERR_HIP
    assert call() == capi.OK and call(n=0, null=True) == capi.OK
    with pytest.raises(capi.PiesError):
        g.apply_forces(good, 0.01)
    assert g.apply_forces([], 0.01, reaction=False) is None
    assert L.pies_apply_forces(None, 0, None, 0.01, None, None, None) == capi.ERR_INVALID


def test_binding_declares_the_entry_point():
    assert "pies_apply_forces" in capi.SYMBOLS and capi.FORCE_MAX == 64 and C.sizeof(capi.Force) == 48
    L = capi.load()
    assert L.pies_apply_forces.restype is C.c_int and len(L.pies_apply_forces.argtypes) == 7
    assert L.pies_abi_version() == 4
    f = capi.Force.radial((1, 2, 3), -2.0, is_force=True).within((1, 2, 3), 4.0, capi.FALLOFF_SMOOTH)
    assert (f.type, f.flags, f.falloff, f.radius, f.strength, list(f.centre)) == (capi.FORCE_RADIAL, 1, 2, 4.0, -2.0, [1.0, 2.0, 3.0])
    assert capi.Force.wind((1, 0, 0), 1.0).radius == float("inf")
