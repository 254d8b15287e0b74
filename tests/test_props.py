"""CPU tests of pies_collide_props: the numpy fp32 restatement of the rule of include/pies_hip.h (`collide`, the yardstick the
device has to match bit for bit in tests/test_props_gpu.py), an independent fp64 formulation it is held to, known answers with exact
binary values, and the argument checks of the entry point on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi

F = np.float32
TILE = 256
NONE = 0xFFFFFFFF
UP = np.array([0.0, 1.0, 0.0], F)

# branch codes of a touch (collide(..., trace=[])): what the GPU test asserts the coverage of
B_SPHERE, B_CAP_T0, B_CAP_T1, B_CAP_MID, B_BOX_IN, B_BOX_OUT, B_DD0 = 0, 1, 2, 3, 4, 10, 16  # B_BOX_IN + 2 j + (l_j < 0)
ALL_BRANCHES = {B_SPHERE, B_CAP_T0, B_CAP_T1, B_CAP_MID, B_BOX_OUT} | {B_BOX_IN + k for k in range(6)}


# ---- the restatement: fp32, no fused multiply-adds, the operation order of the header -------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _fmaxf(a, b):
    """fmaxf: the other operand when one is a NaN; +0 above -0"""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    return np.where(np.isnan(b) | (a > b) | ((a == b) & ~np.signbit(a)), a, b).astype(F)


def _fminf(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    return np.where(np.isnan(b) | (a < b) | ((a == b) & np.signbit(a)), a, b).astype(F)


def _sphere_rule(p, c, R):
    d = p - c
    dd = _dot(d, d)
    touched = dd < R * R
    safe = np.where(dd > 0, dd, F(1))
    n = np.where((dd > 0)[:, None], d / np.sqrt(safe)[:, None], UP[None])
    return touched, n.astype(F), (c + n * R[:, None]).astype(F), dd


def _vec(a):
    return np.array(list(a), F)


def _contact(P, p, r):
    """(touched, n, q, branch) of prop P for the nodes at p (m x 3) with radii r"""
    R = F(P.radius) + r
    centre = _vec(P.centre)
    m = len(p)
    if P.shape == capi.PROP_SPHERE:
        t, n, q, dd = _sphere_rule(p, centre[None], R)
        return t, n, q, np.full(m, B_SPHERE) + B_DD0 * (dd == 0)
    if P.shape == capi.PROP_CAPSULE:
        ab = _vec(P.end) - centre
        ap = p - centre[None]
        den = _dot(ab, ab)
        tt = _fminf(_fmaxf(_dot(ap, ab[None]) / den, F(0)), F(1)) if den > 0 else np.zeros(m, F)
        t, n, q, dd = _sphere_rule(p, (centre[None] + ab[None] * tt[:, None]).astype(F), R)
        return t, n, q, np.where(tt == 0, B_CAP_T0, np.where(tt == 1, B_CAP_T1, B_CAP_MID)) + B_DD0 * (dd == 0)
    ax = _vec(P.axes).reshape(3, 3)
    half = _vec(P.half)
    d = p - centre[None]
    l = np.stack([_dot(ax[j][None], d) for j in range(3)], axis=1)
    inside = (np.abs(l[:, 0]) <= half[0]) & (np.abs(l[:, 1]) <= half[1]) & (np.abs(l[:, 2]) <= half[2])
    e = half[None] - np.abs(l)
    js = np.zeros(m, np.int64)
    js = np.where(e[:, 1] < e[np.arange(m), js], 1, js)
    js = np.where(e[:, 2] < e[np.arange(m), js], 2, js)
    es, ls = e[np.arange(m), js], l[np.arange(m), js]
    n_in = np.where((ls >= 0)[:, None], ax[js], -ax[js]).astype(F)
    q_in = (p + n_in * (es + R)[:, None]).astype(F)
    k = np.stack([_fminf(_fmaxf(l[:, j], -half[j]), half[j]) for j in range(3)], axis=1)
    c = ((centre[None] + ax[0][None] * k[:, 0:1]) + ax[1][None] * k[:, 1:2]) + ax[2][None] * k[:, 2:3]
    t, n, q, dd = _sphere_rule(p, c.astype(F), R)
    branch = np.where(inside, B_BOX_IN + 2 * js + (ls < 0), B_BOX_OUT + B_DD0 * (dd == 0))
    return np.where(inside, True, t), np.where(inside[:, None], n_in, n), np.where(inside[:, None], q_in, q), branch


def collide(pos, prev, vel, radius, inv_mass, props, trace=None):
    """The rule of pies_collide_props in numpy fp32.  Returns (pos, prev, vel, impulse, torque, hits, node_prop).  A node meets the
    props one after the other (the nodes are independent of each other, so a prop is applied to all of them at once); the sums
    are taken per tile of 256 node ids in ascending id from 0, then over the tiles in ascending index from 0.  trace: a list that
    receives (prop, node ids, branch codes) of every prop's touches."""
    with np.errstate(all="ignore"):
        pos, prev, vel = (np.array(a, F).reshape(-1, 3).copy() for a in (pos, prev, vel))
        radius, inv_mass = np.asarray(radius, F).reshape(-1), np.asarray(inv_mass, F).reshape(-1)
        n, k = len(pos), len(props)
        J, T = np.zeros((k, n, 3), F), np.zeros((k, n, 3), F)
        touched_by = np.zeros((k, n), bool)
        node_prop = np.full(n, NONE, np.uint32)
        movable = ~(inv_mass == 0)
        for i, P in enumerate(props):
            t, nn, q, branch = _contact(P, pos, radius)
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
                trace.append((i, np.nonzero(t)[0], branch[t]))
        impulse, torque = np.zeros((k, 3), F), np.zeros((k, 3), F)
        for first in range(0, n, TILE):
            si, st = np.zeros((k, 3), F), np.zeros((k, 3), F)
            for node in range(first, min(first + TILE, n)):
                si, st = si + J[:, node], st + T[:, node]  # (an untouched node adds 0)
            impulse, torque = impulse + si, torque + st
        return pos, prev, vel, impulse, torque, touched_by.sum(axis=1).astype(np.uint32), node_prop


# ---- an independent fp64 formulation: closest point of the prop's core, then a rounded surface ---------------------------------
def collide64(pos, vel, radius, inv_mass, props):
    """Plain geometry in fp64: every prop is a core (a point, a segment, a box) inflated by its radius plus the node's.  Returns
    (pos, vel, impulse, torque, touched (k x n))."""
    pos, vel = np.array(pos, np.float64).reshape(-1, 3), np.array(vel, np.float64).reshape(-1, 3)
    n, k = len(pos), len(props)
    impulse, torque, touched = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, n), bool)
    for node in range(n):
        if inv_mass[node] == 0:
            continue
        x, v = pos[node].copy(), vel[node].copy()
        for i, P in enumerate(props):
            R = float(P.radius) + float(radius[node])
            c = np.array(list(P.centre), np.float64)
            normal = None
            if P.shape == capi.PROP_BOX:
                A = np.array(list(P.axes), np.float64).reshape(3, 3)
                h = np.array(list(P.half), np.float64)
                local = A @ (x - c)
                if np.all(np.abs(local) <= h):  # in the core: out through the nearest face
                    depth = h - np.abs(local)
                    j = int(np.argmin(depth))
                    normal = A[j] * (1.0 if local[j] >= 0 else -1.0)
                    target = x + normal * (depth[j] + R)
                else:
                    core = c + A.T @ np.clip(local, -h, h)
            elif P.shape == capi.PROP_CAPSULE:
                b = np.array(list(P.end), np.float64)
                seg = b - c
                s = np.clip(np.dot(x - c, seg) / np.dot(seg, seg), 0.0, 1.0) if np.dot(seg, seg) > 0 else 0.0
                core = c + s * seg
            else:
                core = c
            if normal is None:
                off = x - core
                dist = np.linalg.norm(off)
                if not dist < R:
                    continue
                normal = off / dist if dist > 0 else np.array([0.0, 1.0, 0.0])
                target = core + R * normal
            arm = target - np.array(list(P.pivot), np.float64)
            u = np.array(list(P.velocity), np.float64) + np.cross(np.array(list(P.angular), np.float64), arm)
            rel = v - u
            vn = np.dot(rel, normal)
            v_new = u + (1.0 - float(P.friction)) * (rel - vn * normal) + max(vn, 0.0) * normal
            j = (v - v_new) / float(inv_mass[node])
            impulse[i] += j
            torque[i] += np.cross(arm, j)
            touched[i, node] = True
            x, v = target, v_new
        pos[node], vel[node] = x, v
    return pos, vel, impulse, torque, touched


# ---- test scenes (shared with tests/test_props_gpu.py) ----------------------------------------------------------------------------
def _q16(a):
    return np.round(np.asarray(a, np.float64) * 16) / 16  # multiples of 1/16: sums with a radius of 0 or 0.5 are exact


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).astype(F)


def make_props(n_props, seed):
    """shapes cycle sphere, capsule, box; from prop 3 on, prop 2 m + 1 overlaps prop 2 m (the first three, one per shape, stand
    apart so that the nodes placed for their branches meet them first); every prop moves and turns about a pivot of its own"""
    rng = np.random.default_rng(1000 + seed)
    props, centre = [], None
    for k in range(n_props):
        centre = _q16(rng.uniform(-5, 5, 3)) if k < 3 or k % 2 == 0 else centre + np.array([0.5, 0.25, 0.0])
        motion = dict(velocity=rng.normal(size=3) * 2, angular=rng.normal(size=3), pivot=centre + rng.normal(size=3) * 0.5,
                      friction=[0.0, 0.25, 1.0, float(F(rng.uniform()))][k % 4])
        if k % 3 == 0:
            props.append(capi.Prop.sphere(centre, float(_q16(rng.uniform(0.4, 1.0))), **motion))
        elif k % 3 == 1:
            props.append(capi.Prop.capsule(centre, centre + _q16(rng.normal(size=3)) + np.array([0.0625, 0, 0]),
                                           float(_q16(rng.uniform(0.3, 0.8))), **motion))
        else:
            props.append(capi.Prop.box(centre, _q16(rng.uniform(0.4, 1.0, 3)), axes=np.eye(3, dtype=F) if k == 2 else _rotation(rng),
                                       rounding=float(_q16(rng.uniform(0.0, 0.4))), **motion))
    return props


def _specials(props):
    """(position, radius) of nodes placed by construction: at a prop's centre, exactly on a surface, inside two props, and one per
    branch of the rule; the first three props (one per shape) come first so that a few dozen nodes cover every branch"""
    out = []
    for k, P in enumerate(props):
        c = np.array(list(P.centre), np.float64)
        if P.shape == capi.PROP_SPHERE:
            out += [(c, 0.5), (c + np.array([P.radius + 0.5, 0, 0]), 0.5), (c + np.array([0.3, 0.4, -0.2]), 0.1)]
        elif P.shape == capi.PROP_CAPSULE:
            ab = np.array(list(P.end), np.float64) - c
            side = np.cross(ab, [0.3, 0.5, 0.7])
            side = side / np.linalg.norm(side) * 0.5 * P.radius
            out += [(c, 0.0), (c - 0.05 * ab + 0.2 * side, 0.1), (c + 1.05 * ab + 0.2 * side, 0.1), (c + 0.5 * ab + side, 0.1)]
        else:
            A, h = np.array(list(P.axes), np.float64).reshape(3, 3), np.array(list(P.half), np.float64)
            out.append((c, 0.5))
            for j in range(3):
                for sign in (1.0, -1.0):
                    out.append((c + A.T @ (h * (np.array([0.1, -0.15, 0.2]) * (np.arange(3) != j) + 0.9 * sign * (np.arange(3) == j))), 0.1))
            out.append((c + A.T @ (h * np.array([1.0, 1.0, 0.5])) + A[0] * 0.3, 0.5))
        if k >= 3 and k % 2 == 1:  # inside two props
            out.append((c - np.array([0.25, 0.125, 0.0]), 0.5))
    return out


def make_scene(n_nodes, n_props, seed=0):
    """(pos, vel, radius, inv_mass, props): loose nodes with random velocity, radius in {0, 0.1, 0.5}, invMass in {0, 0.5, 1}; one
    node in seven is placed by construction (with a non-zero invMass)"""
    rng = np.random.default_rng(seed * 7919 + n_nodes * 31 + n_props)
    props = make_props(n_props, seed)
    pos = rng.uniform(-6, 6, (n_nodes, 3)).astype(F)
    vel = (rng.normal(size=(n_nodes, 3)) * 3).astype(F)
    radius = rng.choice(np.array([0.0, 0.1, 0.5], F), n_nodes)
    inv_mass = rng.choice(np.array([0.0, 0.5, 1.0], F), n_nodes)
    special = _specials(props)
    for m, i in enumerate(range(0, n_nodes, 7)):
        p, r = special[m % len(special)]
        pos[i], radius[i], inv_mass[i] = p.astype(F), F(r), F(1.0 if m % 2 else 0.5)
    return pos, vel, radius, inv_mass, props


def branches_of(trace):
    return {int(b) & 15 for _, _, codes in trace for b in codes}, any(int(b) & B_DD0 for _, _, codes in trace for b in codes)


# ---- restatement against fp64 ---------------------------------------------------------------------------------------------------
GATE_POS_ULP, GATE_VEL_ULP = 32.0, 128.0


def test_restatement_against_fp64():
    """The fp32 restatement against the plain fp64 geometry on the scenes the GPU test uses (600 nodes; 3 and 64 props): position
    and velocity of every node whose touches are the same in both, in ulp of the scene's extent (the largest coordinate or velocity
    component of the scene, 10.7 here: 2^-20).  Measured here: positions 6.26 ulp, velocities 24.6 ulp, under gates of 32 and 128.
    The figure is the conditioning of the rule, not of its restatement: the normal of a node near a
    prop's core is d / |d|, so one ulp of error in d = p - c (c itself a rounded sum for a capsule and a box, p a rounded push of
    the prop before) becomes R / |d| ulp in q and |rel| R / |d| in the velocity, and among 600 random nodes in 64 props a few lie
    within a tenth of R of a core.  The sums of impulse and torque deviate by 8.1e-9 of (largest |sum| x most hits) at most,
    under a gate of 2^-24.  Nodes whose touched / untouched decision differs sit within rounding of a surface; they may be at most
    1 % of the nodes and are left out of the comparison (none here: the nodes placed exactly on a surface are untouched in both)."""
    worst = {"pos": 0.0, "vel": 0.0, "sum": 0.0}
    for n_props in (3, 64):
        pos, vel, radius, inv_mass, props = make_scene(600, n_props)
        p32, prev32, v32, imp32, tor32, hits32, who = collide(pos, pos, vel, radius, inv_mass, props)
        p64, v64, imp64, tor64, touched64 = collide64(pos, vel, radius, inv_mass, props)
        trace = []
        collide(pos, pos, vel, radius, inv_mass, props, trace=trace)
        touched32 = np.zeros_like(touched64)
        for k, ids, _ in trace:
            touched32[k, ids] = True
        same = (touched32 == touched64).all(axis=0)
        assert (~same).mean() <= 0.01, (~same).sum()
        assert touched32.any(axis=0).mean() > 0.05 and (~touched32.any(axis=0)).mean() > 0.05
        extent = max(np.abs(p64).max(), np.abs(v64).max(), np.abs(pos).max(), np.abs(vel).max())
        ulp = float(np.spacing(F(extent)))
        worst["pos"] = max(worst["pos"], np.abs(p32[same] - p64[same]).max() / ulp)
        worst["vel"] = max(worst["vel"], np.abs(v32[same] - v64[same]).max() / ulp)
        assert np.array_equal(prev32[touched32.any(axis=0)], p32[touched32.any(axis=0)])
        # the sums: over the nodes both agree on, in fp64 from the restatement's own touches
        clean = same.all()
        if clean:
            scale = max(np.abs(imp64).max(), np.abs(tor64).max()) * max(1, int(hits32.max()))
            worst["sum"] = max(worst["sum"], max(np.abs(imp32 - imp64).max(), np.abs(tor32 - tor64).max()) / scale)
    print("restatement vs fp64: positions %.3g ulp, velocities %.3g ulp of the extent; sums %.3g relative" %
          (worst["pos"], worst["vel"], worst["sum"]))
    assert worst["pos"] <= GATE_POS_ULP and worst["vel"] <= GATE_VEL_ULP
    assert worst["sum"] <= 2.0 ** -24


def test_every_branch_occurs_in_the_shared_scenes():
    for n_nodes in (255, 257, 600):
        for n_props in (3, 64):
            pos, vel, radius, inv_mass, props = make_scene(n_nodes, n_props)
            trace = []
            out = collide(pos, pos, vel, radius, inv_mass, props, trace=trace)
            seen, dd0 = branches_of(trace)
            assert seen == ALL_BRANCHES and dd0, (n_nodes, n_props, sorted(ALL_BRANCHES - seen), dd0)
            assert (out[6] == NONE).any() and (out[6] != NONE).any()


# ---- known answers ----------------------------------------------------------------------------------------------------------------
def _one(p, v, P, r=0.0, w=1.0):
    out = collide(F([p]), F([p]), F([v]), F([r]), F([w]), P if isinstance(P, list) else [P])
    return out


def test_node_at_a_spheres_centre_leaves_upwards():
    P = capi.Prop.sphere((1.0, 2.0, 3.0), 0.5)
    pos, prev, vel, imp, tor, hits, who = _one((1.0, 2.0, 3.0), (0.0, -1.0, 0.0), P, r=0.25)
    assert np.array_equal(pos, F([[1.0, 2.75, 3.0]])) and np.array_equal(prev, pos)
    assert np.array_equal(vel, F([[0.0, 0.0, 0.0]])) and np.array_equal(imp, F([[0.0, -1.0, 0.0]]))
    assert hits.tolist() == [1] and who.tolist() == [0]


def test_node_exactly_on_the_surface_is_untouched():
    P = capi.Prop.sphere((1.0, 2.0, 3.0), 0.5)
    pos, prev, vel, imp, tor, hits, who = _one((1.75, 2.0, 3.0), (-1.0, 0.0, 0.0), P, r=0.25)  # dd == R * R == 0.5625
    assert np.array_equal(pos, F([[1.75, 2.0, 3.0]])) and np.array_equal(vel, F([[-1.0, 0.0, 0.0]]))
    assert hits.tolist() == [0] and who.tolist() == [NONE] and not imp.any() and not tor.any()
    inside = _one((np.nextafter(F(1.75), F(0)), 2.0, 3.0), (-1.0, 0.0, 0.0), P, r=0.25)
    assert inside[5].tolist() == [1] and np.array_equal(inside[0], F([[1.75, 2.0, 3.0]]))


def test_capsule_with_equal_ends_is_a_sphere():
    rng = np.random.default_rng(5)
    p, v = rng.uniform(-1, 1, (64, 3)).astype(F), rng.normal(size=(64, 3)).astype(F)
    r, w = np.full(64, 0.1, F), np.ones(64, F)
    kw = dict(velocity=(0.5, -1.0, 0.25), angular=(0.1, 0.2, 0.3), pivot=(0.3, 0.1, 0.2), friction=0.5)
    a = collide(p, p, v, r, w, [capi.Prop.capsule((0.1, 0.2, 0.3), (0.1, 0.2, 0.3), 0.7, **kw)])
    b = collide(p, p, v, r, w, [capi.Prop.sphere((0.1, 0.2, 0.3), 0.7, **kw)])
    assert 0 < a[5][0] < 64
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_node_at_a_boxs_centre_leaves_along_the_first_axis():
    axes = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F)
    P = capi.Prop.box((1.0, 1.0, 1.0), (0.5, 0.5, 0.5), axes=axes, rounding=0.25)
    pos, prev, vel, imp, tor, hits, who = _one((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), P, r=0.125)
    assert np.array_equal(pos, F([[1.0, 1.0, 1.875]])) and np.array_equal(prev, pos) and hits.tolist() == [1]  # 0.5 + (0.25 + 0.125)
    # a shorter third half extent wins, and a negative side leaves along -axis
    P = capi.Prop.box((1.0, 1.0, 1.0), (0.5, 0.5, 0.25), axes=axes)
    assert np.array_equal(_one((1.0, 0.875, 1.0), (0, 0, 0), P)[0], F([[1.0, 0.75, 1.0]]))


def test_friction_zero_and_one():
    v = (F(0.3), F(-0.7), F(0.11))
    u = (0.5, 0.0, -0.25)
    still = _one((1.0, 2.0, 3.0), v, capi.Prop.sphere((1.0, 2.0, 3.0), 0.5, friction=0.0))
    assert np.array_equal(still[2].view(np.uint32), F([[v[0], 0.0, v[2]]]).view(np.uint32))  # the tangential bits of v, no normal part
    free = _one((1.0, 2.0, 3.0), v, capi.Prop.sphere((1.0, 2.0, 3.0), 0.5, velocity=u, friction=0.0))
    # n = (0, 1, 0), u = (0.5, 0, -0.25): rel = v - u, vn < 0 -> v' = u + tang: the tangential components are (u + (v - u))
    rel = F(v) - F(u)
    tang = rel - UP * rel[1]
    assert np.array_equal(free[2][0].view(np.uint32), (F(u) + (tang * F(1.0) + UP * F(0.0))).view(np.uint32))
    stick = _one((1.0, 2.0, 3.0), v, capi.Prop.sphere((1.0, 2.0, 3.0), 0.5, velocity=u, friction=1.0))
    assert np.array_equal(stick[2], F([[0.5, 0.0, -0.25]]))  # the prop's velocity, no outward part (vn < 0)
    away = _one((1.0, 2.0, 3.0), (0.3, 2.0, 0.11), capi.Prop.sphere((1.0, 2.0, 3.0), 0.5, velocity=u, friction=1.0))
    assert np.array_equal(away[2], F([[0.5, 2.0, -0.25]]))  # ... plus the outward normal part


def test_a_prop_moving_away_leaves_the_normal_velocity_alone():
    # the prop retreats downwards faster than the node falls: vn > 0, the normal part of v survives, nothing is taken from it
    out = _one((1.0, 2.0, 3.0), (0.0, -1.0, 0.0), capi.Prop.sphere((1.0, 2.0, 3.0), 0.5, velocity=(0.0, -4.0, 0.0)))
    assert np.array_equal(out[2], F([[0.0, -1.0, 0.0]])) and not out[3].any() and out[5].tolist() == [1]


def test_a_fixed_node_is_untouched_and_uncounted():
    out = _one((1.0, 2.0, 3.0), (0.0, -1.0, 0.0), capi.Prop.sphere((1.0, 2.0, 3.0), 0.5), w=0.0)
    assert np.array_equal(out[0], F([[1.0, 2.0, 3.0]])) and np.array_equal(out[2], F([[0.0, -1.0, 0.0]]))
    assert out[5].tolist() == [0] and out[6].tolist() == [NONE] and not out[3].any()


def test_two_props_are_applied_one_after_the_other():
    a = capi.Prop.sphere((0.0, 0.0, 0.0), 1.0, velocity=(1.0, 0.0, 0.0), friction=0.5)
    b = capi.Prop.box((0.5, 1.0, 0.0), (1.0, 0.5, 1.0), velocity=(0.0, 0.0, 2.0), friction=0.25)
    p, v = (0.25, 0.5, 0.0), (0.0, -1.0, 0.5)
    both = _one(p, v, [a, b])
    first = _one(p, v, a)
    second = collide(first[0], first[1], first[2], F([0.0]), F([1.0]), [b])
    assert both[5].tolist() == [1, 1] and both[6].tolist() == [1]
    for x, y in ((both[0], second[0]), (both[1], second[1]), (both[2], second[2]), (both[3][0], first[3][0]), (both[3][1], second[3][0]),
                 (both[4][1], second[4][0])):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    other = _one(p, v, [b, a])
    assert not np.array_equal(other[0], both[0])  # the order matters


def test_the_sums_follow_the_two_level_order():
    rng = np.random.default_rng(11)
    n = 600
    p = rng.uniform(-1, 1, (n, 3)).astype(F)
    v = (rng.normal(size=(n, 3)) * 100).astype(F)
    P = capi.Prop.sphere((0.0, 0.0, 0.0), 3.0, friction=0.37)
    out = collide(p, p, v, np.zeros(n, F), np.ones(n, F), [P])
    assert out[5].tolist() == [n]
    j = v - out[2]  # invMass 1
    tiles = []
    for first in range(0, n, TILE):
        s = np.zeros(3, F)
        for i in range(first, min(first + TILE, n)):
            s = s + j[i]
        tiles.append(s)
    assert np.array_equal(out[3][0], (np.zeros(3, F) + tiles[0]) + tiles[1] + tiles[2])
    one = np.zeros(3, F)
    for i in range(n):
        one = one + j[i]
    assert not np.array_equal(out[3][0], one)  # (a single running sum gives other bits on this input)


# ---- the entry point on a host-only handle ------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device_check():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    L, h = capi.load(), g._h
    inf, nan = float("inf"), float("nan")

    def call(*props, n=None, null=False):
        arr = (capi.Prop * max(len(props), 1))(*props)
        return L.pies_collide_props(h, len(props) if n is None else n, None if null else arr, None, None, None, None)

    good = [capi.Prop.sphere((0, 0, 0), 1.0), capi.Prop.capsule((0, 0, 0), (1, 0, 0), 0.5), capi.Prop.box((0, 0, 0), (1, 1, 1))]
    assert call(n=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()

    def broken(base, **kw):
        p = capi.Prop.from_buffer_copy(base)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(p, name)[value[0]] = value[1]
            else:
                setattr(p, name, value)
        return p

    assert call(broken(good[0], shape=3)) == capi.ERR_INVALID and call(broken(good[0], shape=-1)) == capi.ERR_INVALID
    for k in range(3):
        for bad in (-0.5, nan, inf):
            assert call(broken(good[k], radius=bad)) == capi.ERR_INVALID, (k, bad)
        for bad in (-0.01, 1.5, nan):
            assert call(broken(good[k], friction=bad)) == capi.ERR_INVALID, (k, bad)
        for name in ("centre", "velocity", "angular", "pivot"):
            for bad in (nan, inf, -inf):
                assert call(broken(good[k], **{name: (1, bad)})) == capi.ERR_INVALID, (k, name, bad)
    assert call(broken(good[1], end=(2, nan))) == capi.ERR_INVALID
    assert call(broken(good[2], axes=(7, inf))) == capi.ERR_INVALID
    for bad in (-1.0, nan, inf):
        assert call(broken(good[2], half=(0, bad))) == capi.ERR_INVALID
    assert call(good[0], broken(good[0], radius=-1.0)) == capi.ERR_INVALID and "prop 1" in g.last_error()
    assert call(*([good[0]] * 65)) == capi.ERR_UNSUPPORTED
    # fields a shape ignores may hold anything
    for p in (broken(good[0], end=(0, nan), axes=(3, nan), half=(1, -1.0)), broken(good[1], axes=(0, inf), half=(2, nan)),
              broken(good[2], end=(1, nan))):
        assert call(p) == capi.ERR_HIP
    assert call(*good) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert call(*([good[1]] * 64)) == capi.ERR_HIP
    assert call() == capi.OK and call(n=0, null=True) == capi.OK
    who = np.zeros(g.count(capi.NODES), np.uint32)
    assert L.pies_collide_props(h, 0, None, None, None, None, who.ctypes.data_as(C.POINTER(C.c_uint32))) == capi.OK
    assert (who == NONE).all()
    with pytest.raises(capi.PiesError):
        g.collide_props(good)
    assert g.collide_props([], reaction=False) is None
    assert L.pies_collide_props(None, 0, None, None, None, None, None) == capi.ERR_INVALID


def test_binding_declares_the_entry_point():
    assert "pies_collide_props" in capi.SYMBOLS and capi.PROP_NONE == NONE and capi.PROP_MAX == 64
    assert C.sizeof(capi.Prop) == 120
    L = capi.load()
    assert L.pies_collide_props.restype is C.c_int and len(L.pies_collide_props.argtypes) == 7
    assert L.pies_abi_version() == 4
