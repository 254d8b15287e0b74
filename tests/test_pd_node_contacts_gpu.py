"""GPU tests of the PD node-node contacts (PIES_FLAG_PD_NODE_CONTACTS): detection against a brute-force enumeration, the solve and
the friction loop against the oracle fed the device's contact list, what the contacts do to colliding bodies, renumbering,
determinism, the capacity latch, and that the flag off (or under PBD) changes nothing.

One tick is one substep (timeSubsteps = 1) and one detection, on the predicted positions p + h v."""
import numpy as np
import pytest

import scenes
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu
DT = 0.012
H = np.float32(DT)


def pd_options(mod, iterations=6, **kw):
    return mod.Options(solver=mod.PD, iterations=iterations, **kw)


def contact_solver(pies, on=True, **kw):
    g = pies.Solver(pd_options(pies, **kw))
    if on is not None:
        g.set_flag(pies.FLAG_PD_NODE_CONTACTS, 1 if on else 0)
    return g


def pair_mix(i, j):
    """The friction pass's order: murmur3's 64-bit finaliser over (min << 32 | max) (pd_contact_kernels.h pair_mix)."""
    m = (1 << 64) - 1
    k = (min(i, j) << 32) | max(i, j)
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & m
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & m
    k ^= k >> 33
    return k


def joined_pairs(g, pies):
    """Node pairs joined by an element (distance, tet, volume, bend, triangle, listed node pair)."""
    out = set()
    for ctype in (pies.DISTANCE, pies.TET, pies.VOLUME, pies.BEND, pies.TRIANGLES, pies.NODE_PAIRS):
        ids = g.ids(ctype)
        if ids.size == 0:
            continue
        ids = ids.reshape(len(ids), -1)
        for a in range(ids.shape[1]):
            for b in range(a + 1, ids.shape[1]):
                for i, j in zip(ids[:, a].tolist(), ids[:, b].tolist()):
                    if i != j:
                        out.add((min(i, j), max(i, j)))
    return out


def brute_force(p, v, r, im, joined):
    """The contact rule on the predicted positions p + h v in fp32: (definite contacts, pairs within 1e-5 of touching)."""
    q = (p + H * v).astype(np.float32)
    d = q[None, :, :] - q[:, None, :]
    dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    rr = (r[:, None] + r[None, :]).astype(np.float32)
    hit = dist2 < rr * rr
    near = np.abs(np.sqrt(dist2.astype(np.float64)) - rr) <= 1e-5 * rr
    ok = (im[:, None] + im[None, :]) > 0
    sure, edge = set(), set()
    for i, j in zip(*np.nonzero(np.triu(hit & ok, 1))):
        if (i, j) not in joined:
            (edge if near[i, j] else sure).add((int(i), int(j)))
    for i, j in zip(*np.nonzero(np.triu(near & ok, 1))):
        if (i, j) not in joined:
            edge.add((int(i), int(j)))
    return sure, edge


NODES = 9  # PIES_NODES / the oracle's node count


def two_boxes(s, gap=0.9, speed=2.0, y=3.0, dims=(3, 3, 3)):
    """Two createTetBox lattices moving into each other along x, box B's lowest x `gap` beyond box A's highest."""
    s.create_tet_box(*dims, translation=(0, y, 0), velocity=(speed, 0, 0))
    s.create_tet_box(*dims, translation=(20, y, 0), velocity=(-speed, 0, 0))
    place_boxes(s, gap, s.count(NODES) // 2)


def place_boxes(s, gap, per_box):
    p = s.positions.copy()
    a, b = p[:per_box], p[per_box:2 * per_box]
    p[per_box:2 * per_box, 0] += (a[:, 0].max() + gap) - b[:, 0].min()
    s.set_positions(p)
    s.set_prev_positions(p)


SPHERES = np.float32([[0, 8, 0], [0.8, 8, 0], [3, 8, 0], [4, 8, 0], [6, 8, 0], [6.9, 8, 0], [9, 8, 0], [9, 8.9, 0],
                      [12, 8, 0], [12.5, 8, 0], [15, 8, 0], [15.6, 8, 0], [18, 8, 0], [18.3, 8.2, 0.1]])
SPHERE_R = np.float32([0.5, 0.5, 0.5, 0.5, 0.4, 0.4, 0.6, 0.35, 0.5, 0.5, 0.5, 0.5, 0.3, 0.3])
SPHERE_IM = np.float32([1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 0.5])
SPHERE_V = np.float32([[1, 0, 0], [-1, 0, 0]] + [[0, 0, 0]] * 12)


def detection_scene(s):
    """Two tet boxes driven into each other, spheres that overlap, touch and miss, a pinned-pinned overlapping pair (8, 9) and an
    overlapping pair joined by a distance constraint (10, 11)."""
    two_boxes(s, 0.9)
    first = s.add_nodes_raw(SPHERES, vel=SPHERE_V, radius=SPHERE_R, invMass=SPHERE_IM)
    s.add_distance(np.uint32([[first + 10, first + 11]]), 1.0)  # an overlapping pair joined by a distance constraint
    return first


def test_detection_equals_brute_force(pies):
    g = contact_solver(pies)
    detection_scene(g)
    p, v, r, im = g.positions, g.velocities, g.radii, g.inv_masses
    joined = joined_pairs(g, pies)
    g.tick()
    got = g.node_contacts()
    assert g.count(pies.NODE_CONTACTS) == len(got)
    pairs = {(int(min(a, b)), int(max(a, b))) for a, b in got}
    assert len(pairs) == len(got)  # each unordered pair once
    sure, edge = brute_force(p, v, r, im, joined)
    assert sure - pairs == set(), sorted(sure - pairs)
    assert pairs - sure - edge == set(), sorted(pairs - sure - edge)
    n = len(p) - len(SPHERES)
    # the scene has what it claims: box-box contacts, overlapping spheres, and the excluded pairs are not listed
    assert any(a < n // 2 <= b < n for a, b in pairs)
    assert (n + 0, n + 1) in pairs and (n + 6, n + 7) in pairs and (n + 12, n + 13) in pairs
    assert (n + 4, n + 5) not in pairs and (n + 8, n + 9) not in pairs and (n + 10, n + 11) not in pairs
    # friction order: ascending pair key
    keys = [pair_mix(int(a), int(b)) for a, b in got]
    assert keys == sorted(keys)


def yardstick(g, o32, o64, spacing=1.0):
    for name in ("positions", "velocities"):
        a, b, c = getattr(g, name), getattr(o32, name), getattr(o64, name)
        assert np.isfinite(a).all(), name
        d_dev, d_ref = float(np.abs(a - c).max()), float(np.abs(b - c).max())
        gate = max(2.0 * d_ref, 1e-4 * spacing / (DT if name == "velocities" else 1.0))
        assert d_dev <= gate, (name, "device vs fp64 %.3g, oracle32 vs fp64 %.3g, gate %.3g" % (d_dev, d_ref, gate))


def replay_scene(s):
    """A tet box sliding on the floor (friction 0.3), spheres resting on it and on each other, one sliding beside it."""
    s.create_tet_box(3, 2, 3, translation=(0, 1.0, 0), velocity=(1.5, 0, 0))
    nb = s.count(NODES)
    p = s.positions.copy()
    p[:, 1] += 0.02 - p[:, 1].min()
    s.set_positions(p)
    s.set_prev_positions(p)
    top = p[:, 1].max()
    lo, hi = p.min(0), p.max(0)
    sph = np.float32([[lo[0] + 0.3, top + 0.95, lo[2] + 0.2], [lo[0] + 1.2, top + 0.97, lo[2] + 0.5],
                      [lo[0] + 0.7, top + 1.8, lo[2] + 0.3], [hi[0] + 0.5, p[:, 1].min() + 0.4, lo[2] + 1.0]])
    vel = np.float32([[0.5, 0, 0], [0, 0, 0.3], [0, -0.5, 0], [-1.0, 0, 0]])
    s.add_nodes_raw(sph, vel=vel, radius=0.5)
    return nb


def test_oracle_replay(pies, oracle):
    g = contact_solver(pies, friction=0.3)
    replay_scene(g)
    g.finalize()
    seen = 0
    for _ in range(6):
        pos, prev, vel = g.positions, g.prev_positions, g.velocities
        g.tick()
        pairs = g.node_contacts()
        seen = max(seen, len(pairs))
        o32, o64 = oracle.OracleSolver(pd_options(oracle, friction=0.3)), oracle.OracleSolver(pd_options(oracle, friction=0.3))
        o64.set_flag(oracle.FLAG_PD_SOLVE_FP64, 1)
        for o in (o32, o64):
            replay_scene(o)
            o.set_positions(pos)
            o.set_prev_positions(prev)
            o.set_velocities(vel)
            if len(pairs):
                o.add_node_pairs(pairs)
            o.tick()
        yardstick(g, o32, o64)
    assert seen >= 3
    assert g.pcg_health()["short_solves"] == 0 and not g.failed


def colliding_blocks(s, speed=3.0):
    a, _ = scenes.loose_particles((3, 3, 3), spacing=1.05, jitter=0.0, y0=4.0)
    b = a + np.float32([a[:, 0].max() - a[:, 0].min() + 2.0, 0.0, 0.0])
    p = np.concatenate([a, b])
    v = np.zeros_like(p)
    v[: len(a), 0], v[len(a):, 0] = speed, -speed
    s.add_nodes_raw(p, vel=v, radius=0.5)


def rope_on_itself(s, n=40, spacing=0.4, r=0.25, lift=0.8):
    """A rope (distance chain) whose lower strand is held by position constraints and whose upper strand falls onto it."""
    half = n // 2
    lower = np.stack([np.arange(half) * spacing, np.full(half, 3.0), np.zeros(half)], 1)
    upper = np.stack([np.arange(half)[::-1] * spacing, np.full(half, 3.0 + lift), np.zeros(half)], 1)
    s.add_nodes_raw(np.concatenate([lower, upper]).astype(np.float32), radius=r)
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.uint32)
    s.add_distance(chain, 100.0)
    s.add_position(np.arange(half, dtype=np.uint32), 1000.0)
    return half


def closest_unjoined(p, r, joined, subset=None):
    """min over unjoined pairs of |p_i - p_j| / (r_i + r_j)."""
    d = np.linalg.norm(p[None, :, :] - p[:, None, :], axis=2) / (r[:, None] + r[None, :])
    np.fill_diagonal(d, np.inf)
    for i, j in joined:
        d[i, j] = d[j, i] = np.inf
    if subset is not None:
        d = d[np.ix_(*subset)]
    return float(d.min())


@pytest.mark.parametrize("scene", ["blocks", "rope"])
def test_contacts_keep_bodies_apart(pies, scene):
    out = {}
    for on in (True, False):
        g = contact_solver(pies, on, gravity=0.0 if scene == "blocks" else 10.0)
        half = colliding_blocks(g) if scene == "blocks" else rope_on_itself(g)
        joined = joined_pairs(g, pies)
        g.tick(30)
        p, r = g.positions, g.radii
        assert np.isfinite(p).all() and not g.failed, g.last_error()
        n = len(p)
        split = n // 2 if scene == "blocks" else half
        out[on] = (closest_unjoined(p, r, joined), closest_unjoined(p, r, joined, (np.arange(split), np.arange(split, n))))
        if on:
            assert g.pcg_health()["short_solves"] == 0
    assert out[True][0] >= 0.9, out  # no contacting pair ends closer than 0.9 (r_i + r_j)
    assert out[False][1] < 0.9, out   # without the flag the bodies pass into each other


def pile_under(mesh_pos, spacing=1.0):
    lo, hi = mesh_pos.min(0), mesh_pos.max(0)
    xs = np.arange(lo[0], hi[0] + 1e-3, spacing)
    zs = np.arange(lo[2] + 1.0, hi[2] + 1e-3, spacing)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    return np.stack([X.ravel(), np.full(X.size, lo[1] - 0.9), Z.ravel()], 1).astype(np.float32)


def test_renumbering_keeps_contacts_in_host_ids(pies):
    mesh = shuffled_beam()
    res = {}
    for renumber in (1, 0):
        g = contact_solver(pies, iterations=10)
        g.set_flag(pies.FLAG_RENUMBER_NODES, renumber)
        scenes.build_unstructured_pd(g, mesh)
        g.add_nodes_raw(pile_under(mesh[0]), radius=0.5)
        g.finalize()
        assert g.count(pies.NODES_RENUMBERED) == renumber
        g.tick()
        pairs = {(int(min(a, b)), int(max(a, b))) for a, b in g.node_contacts()}
        res[renumber] = (pairs, g.positions)
        assert not g.failed
    assert len(res[1][0]) > 20
    assert res[1][0] == res[0][0]
    p = res[0][1]
    tol = 1e-5 * float(np.linalg.norm(p.max(0) - p.min(0))) + 2e-5
    assert float(np.abs(res[1][1] - p).max()) <= tol


def motion_scene(s):
    """Every node free (no pinned pair: PD gives an inverse mass of 0 an infinite diagonal): the boxes, the free spheres of
    detection_scene, two colliding blocks of loose particles and an overlapping trio."""
    two_boxes(s, 0.9)
    keep = np.nonzero(SPHERE_IM > 0)[0]
    s.add_nodes_raw(SPHERES[keep], vel=SPHERE_V[keep], radius=SPHERE_R[keep])
    colliding_blocks(s)
    s.add_nodes_raw(np.float32([[0, 12, 0], [0.7, 12, 0], [0.3, 12.6, 0]]), radius=0.5)


def test_runs_are_bit_identical(pies):
    runs = []
    for _ in range(2):
        g = contact_solver(pies, friction=0.3)
        motion_scene(g)
        lists = []
        for _ in range(10):
            g.tick()
            lists.append(g.node_contacts())
        runs.append((g.positions, lists))
    assert sum(len(c) for c in runs[0][1]) > 0
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)


def test_partner_overflow_latches(pies, tune):
    tune("PIES_PD_NODE_CONTACT_PARTNERS", 4)
    g = contact_solver(pies)
    rng = np.random.default_rng(3)
    g.add_nodes_raw((np.float32([0, 5, 0]) + rng.uniform(-0.2, 0.2, (8, 3))).astype(np.float32), radius=0.5)
    g.tick()
    assert g.failed
    assert "node-node contact list" in g.last_error() and "(4)" in g.last_error(), g.last_error()
    p = g.positions
    g.tick()
    assert np.array_equal(g.positions, p)


@pytest.mark.parametrize("solver", ["pd", "pbd"])
def test_flag_off_changes_nothing(pies, solver):
    res = []
    for on in ((None, False) if solver == "pd" else (False, True)):
        if solver == "pd":
            g = contact_solver(pies, on)
        else:
            g = pies.Solver(scenes.pbd_options(pies, 4))
            g.set_flag(pies.FLAG_PD_NODE_CONTACTS, 1 if on else 0)
        motion_scene(g)
        g.tick(4)
        res.append((g.positions, g.velocities, g.launch_counts(), g.count(pies.NODE_CONTACTS)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]
    assert res[0][3] == res[1][3] == 0
