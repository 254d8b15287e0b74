"""Every global-step variant of the PD substep against the fp64 yardstick, and the friction order of the listed node pairs.

The kernels of a substep's global step are chosen by the scene's shape and by tuning switches: the one-launch CG
(pd_cg1_kernels.hip) or the two-launch form with its grid-barrier continuation (pd_cg_kernels.hip; also whenever a row has
several lanes), 1 / 2 / 4 / 8 lanes per SELL row, the right-hand side inside the residual kernel or in k_pd_rhs with one or four
lanes per node, and the CG partition over `nparts` / `npartsI` workgroups.  Each variant below is run on small scenes against
two oracle runs (fp32, and the same loop with its global solve in double) after every tick, positions and velocities, with the
yardstick of test_pd_parity_gpu as the gate.  Every case proves that the variant ran (counters, launch counts), and every case
runs twice: the two runs must agree bit for bit (a race on the partial sums or on a grid barrier shows up there first).

Scenes: A = two materials, an odd element count, floor contacts, pins (_two_boxes); B = an unstructured Delaunay beam (no row
dictionary: the windowed matrix); C = a single tetrahedron (4 rows) and a 105-node box (a partial last SELL slice and a partial
wavefront at every lane count; a slice holds 64 / lanes rows); D = two boxes in point-triangle contact in the contact-heavy
graph variant (PIES_TRI_FAST_ROWS=1: cg.useCAp), every tick started from the fp32 oracle's state."""
import numpy as np
import pytest

import scenes
from test_pd_parity_gpu import _two_boxes, build_pd_beam, pd_options, record, yardstick

pytestmark = pytest.mark.gpu
TICKS = 4
ITERS = 6
# every switch a variant may set; the ones a variant does not name are unset for its run
SWITCHES = ("PIES_PD_CG_SINGLE", "PIES_PD_CG_SINGLE_ROWS", "PIES_SELL_LANES", "PIES_PD_ROW_DICT", "PIES_PD_WINDOW", "PIES_PD_FUSE_RHS",
            "PIES_PD_TILE_ELEMS", "PIES_PD_RHS_LANES", "PIES_CG_BLOCKS", "PIES_CG_INIT_BLOCKS", "PIES_PCG_NEVER_EXIT", "PIES_TRI_FAST_ROWS")


def scene_a(s):
    _two_boxes(s)


_MESH_B = []


def scene_b(s):
    if not _MESH_B:
        _MESH_B.append(scenes.delaunay_beam((6, 5, 30), seed=11))
    scenes.build_unstructured_pd(s, _MESH_B[0])
    scenes.perturb(s, 5, 0.03)
    s.set_prev_positions(s.positions)


def scene_c_tet(s):
    """one tetrahedron (4 rows: one partial slice at every lane count) resting on the floor, sliding"""
    s.addNodes(np.float32([[0, 0.02, 0], [1.0, 0.02, 0.1], [0.2, 0.03, 1.1], [0.3, 1.0, 0.4]]))
    ids = np.uint32([[0, 1, 2, 3]])
    s.add_tet(ids, 1.0)
    s.add_volume(ids, 1.0)
    s.add_triangles(np.uint32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))
    scenes.perturb(s, 3, 0.05)
    v = s.velocities
    v[:, 0] = 0.8
    s.set_velocities(v)
    s.set_prev_positions(s.positions)


def scene_c_box(s):
    """a 5 x 3 x 7 box: 105 rows, not a multiple of 64 (a partial last slice and wavefront at every lane count), end cap pinned"""
    build_pd_beam(s, (5, 3, 7))
    scenes.perturb(s, 7, 0.04)
    s.set_prev_positions(s.positions)


def scene_d(s):
    """test_tri_collisions_gpu.two_boxes: a box falling onto one that sits on the floor"""
    s.create_tet_box(3, 3, 3, translation=(0, 0.02, 0), w=1.0)
    s.create_tet_box(3, 3, 3, translation=(0.4, 2.06, 0.3), w=1.0)
    v = s.velocities
    v[27:, 1] = -2.0
    s.set_velocities(v)
    s.set_prev_positions(s.positions)


SCENES = {"A": scene_a, "B": scene_b, "C_tet": scene_c_tet, "C_box": scene_c_box, "D": scene_d}
TEACHER_FORCED = {"D"}  # contact decisions are discontinuous: every tick starts from the fp32 oracle's state

# name: the switches of the variant (one axis at a time from the default, and a few combinations the library produces itself)
VARIANTS = {
    "default": {},
    "cg_single": {"PIES_PD_CG_SINGLE": "1"},
    "cg_two_launch": {"PIES_PD_CG_SINGLE": "0"},
    "cg_rows_single": {"PIES_PD_CG_SINGLE_ROWS": "1"},
    "cg_rows_two_launch": {"PIES_PD_CG_SINGLE_ROWS": "0"},
    "sell_lanes2": {"PIES_SELL_LANES": "2", "PIES_PD_ROW_DICT": "0", "PIES_PD_WINDOW": "0"},
    "sell_lanes4": {"PIES_SELL_LANES": "4", "PIES_PD_ROW_DICT": "0", "PIES_PD_WINDOW": "0"},
    "sell_lanes8": {"PIES_SELL_LANES": "8", "PIES_PD_ROW_DICT": "0", "PIES_PD_WINDOW": "0"},
    "rhs_fused": {"PIES_PD_FUSE_RHS": "1"},
    "rhs_kernel": {"PIES_PD_FUSE_RHS": "0"},
    "records_lanes1": {"PIES_PD_TILE_ELEMS": "0", "PIES_PD_RHS_LANES": "1"},
    "records_lanes4": {"PIES_PD_TILE_ELEMS": "0", "PIES_PD_RHS_LANES": "4"},
    "cg_blocks1": {"PIES_CG_BLOCKS": "1"},
    "cg_blocks3": {"PIES_CG_BLOCKS": "3"},
    # (the window caps the workgroups at its chunk count: the plain SELL arrays keep all 1 024, most of them without a row)
    "cg_blocks1024": {"PIES_CG_BLOCKS": "1024", "PIES_PD_WINDOW": "0"},
    "init_blocks1": {"PIES_CG_INIT_BLOCKS": "1"},
    "init_blocks4096": {"PIES_CG_INIT_BLOCKS": "4096", "PIES_PD_WINDOW": "0"},
    "never_exit": {"PIES_PCG_NEVER_EXIT": "1"},
    # what the library picks on its own: the two-launch form whenever a row has several lanes, per-element records (k_pd_rhs<4>)
    "two_launch_lanes4_records": {"PIES_PD_CG_SINGLE": "0", "PIES_SELL_LANES": "4", "PIES_PD_ROW_DICT": "0", "PIES_PD_WINDOW": "0",
                                  "PIES_PD_TILE_ELEMS": "0"},
    "lanes8_blocks1024_init1": {"PIES_SELL_LANES": "8", "PIES_PD_ROW_DICT": "0", "PIES_PD_WINDOW": "0", "PIES_CG_BLOCKS": "1024",
                                "PIES_CG_INIT_BLOCKS": "1"},
}
COMMON = ["cg_single", "cg_two_launch", "sell_lanes2", "sell_lanes4", "sell_lanes8", "cg_blocks1", "cg_blocks3", "cg_blocks1024",
          "init_blocks1", "init_blocks4096", "never_exit", "two_launch_lanes4_records"]
CASES = ([(sc, v) for sc in ("A", "B", "C_box") for v in COMMON + ["rhs_fused", "rhs_kernel", "records_lanes1", "records_lanes4"]]
         + [("C_tet", v) for v in COMMON + ["lanes8_blocks1024_init1"]]
         + [("C_box", "lanes8_blocks1024_init1")]
         + [("D", v) for v in ("cg_rows_single", "cg_rows_two_launch", "sell_lanes4", "cg_blocks1", "cg_blocks3", "init_blocks1")])
# Variants that add the same terms in the same order as another one: the two must agree bit for bit.
#   rhs_kernel vs rhs_fused: k_pd_rhs<1> and the residual kernel evaluate the same rhs_of_node<1> (pd_rhs_device.h) per node, and
#     the residual kernel then uses that value either way.
# (never_exit vs default is claimed to be such a pair as well, and is not: test_never_exit_changes_nothing)
BIT_EQUAL = {"rhs_kernel": "rhs_fused"}

_ORACLE = {}


def oracle_run(oracle, scene):
    """per tick: (state before the tick, fp32 oracle after it, fp64 oracle after it); cached per scene"""
    if scene in _ORACLE:
        return _ORACLE[scene]
    opts = dict(iterations=ITERS)
    o32, o64 = oracle.OracleSolver(pd_options(oracle, **opts)), oracle.OracleSolver(pd_options(oracle, **opts))
    o64.set_flag(oracle.FLAG_PD_SOLVE_FP64, 1)
    for o in (o32, o64):
        SCENES[scene](o)
    out = []
    for t in range(TICKS):
        before = (o32.positions, o32.prev_positions, o32.velocities)
        if scene in TEACHER_FORCED:
            o64.set_positions(before[0]); o64.set_prev_positions(before[1]); o64.set_velocities(before[2])
        o32.tick(); o64.tick()
        out.append((before, _State(o32), _State(o64)))
    _ORACLE[scene] = out
    return out


class _State:
    def __init__(self, s):
        self.positions, self.velocities = s.positions, s.velocities


def set_variant(tune, variant, scene):
    sw = dict(VARIANTS[variant])
    if scene == "D":
        sw["PIES_TRI_FAST_ROWS"] = "1"
    for name in SWITCHES:
        tune(name, sw.get(name))


def device_run(pies, scene, steps):
    """one device run of the scene; returns the solver (still open) and its states after each tick"""
    g = pies.Solver(pd_options(pies, ITERS))
    SCENES[scene](g)
    g.finalize()
    states = []
    for before, _, _ in steps:
        if scene in TEACHER_FORCED:
            g.set_positions(before[0]); g.set_prev_positions(before[1]); g.set_velocities(before[2])
        g.tick()
        states.append((g.positions, g.velocities))
    return g, states


def prove(pies, g, scene, variant):
    """the variant ran: counters and launch counts of the handle, not the switches"""
    sw = VARIANTS[variant]
    single, lc = g.count(pies.PD_CG_SINGLE), g.launch_counts()
    lanes = int(sw.get("PIES_SELL_LANES", "1"))
    two_launch = sw.get("PIES_PD_CG_SINGLE") == "0" or lanes != 1 or sw.get("PIES_PD_CG_SINGLE_ROWS") == "0"
    assert single == (0 if two_launch else 1), (variant, single)
    assert (lc["pd_cg_update"] > 0) == two_launch, (variant, lc)
    if lanes != 1 or sw.get("PIES_PD_WINDOW") == "0":
        assert g.count(pies.PD_WINDOW_ENTRIES) == 0 and g.count(pies.ROW_STENCILS) == 0, variant
    elif scene == "B":
        assert g.count(pies.PD_WINDOW_ENTRIES) > 0 and g.count(pies.ROW_STENCILS) == 0
    if sw.get("PIES_PD_TILE_ELEMS") == "0":
        assert g.count(pies.PD_TILES) == 0, variant
    elif scene != "C_tet":
        assert g.count(pies.PD_TILES) > 0, variant
    if variant in ("rhs_fused", "rhs_kernel"):
        # No counter says which form evaluated the right-hand side: the inputs of the rule in enqueue_pd_substep are asserted
        # instead - the one-launch CG, tile sums (a few records per node: rhsLanes = 1), no contact rows, no node contacts; then
        # PIES_PD_FUSE_RHS alone decides.
        assert single == 1 and g.count(pies.PD_TILES) > 0 and g.count(pies.PD_TILE_RECORDS) <= 6 * g.count(pies.NODES)
        assert not g.count(pies.NODE_CONTACTS) and lc["pd_cg_update"] == 0
    if scene == "D":
        assert len(g.tri_collisions) > 0


@pytest.mark.parametrize("scene,variant", CASES, ids=["%s-%s" % c for c in CASES])
def test_global_step_variant_against_fp64(pies, oracle, tune, scene, variant):
    steps = oracle_run(oracle, scene)
    set_variant(tune, variant, scene)
    runs = []
    for rep in range(2):
        g, states = device_run(pies, scene, steps)
        if rep == 0:
            prove(pies, g, scene, variant)
        assert not g.failed and g.pcg_health()["short_solves"] == 0, (scene, variant, g.pcg_health())
        g.close()
        runs.append(states)
    test = "variant_%s_%s" % (scene, variant)
    for t, ((_, o32, o64), (p, v), (p2, v2)) in enumerate(zip(steps, runs[0], runs[1])):
        assert np.isfinite(p).all() and np.isfinite(v).all(), (test, t)
        assert np.array_equal(p, p2) and np.array_equal(v, v2), (test, t, "two runs differ", float(np.abs(p - p2).max()))
        yardstick(test, _Arrays(p, v), o32, o64, names=("positions", "velocities"))
    if variant in BIT_EQUAL:
        set_variant(tune, BIT_EQUAL[variant], scene)
        g, states = device_run(pies, scene, steps)
        g.close()
        for t, ((p, v), (q, w)) in enumerate(zip(runs[0], states)):
            record(test, "vs_%s_positions" % BIT_EQUAL[variant], float(np.abs(p - q).max()), 0.0)
            assert np.array_equal(p, q) and np.array_equal(v, w), (test, t, float(np.abs(p - q).max()), float(np.abs(v - w).max()))


@pytest.mark.xfail(strict=True, reason="PIES_PCG_NEVER_EXIT=1 changes the results: a column below the tolerance goes on iterating")
@pytest.mark.parametrize("scene", ["A", "B", "C_box", "D"])
def test_never_exit_changes_nothing(pies, oracle, tune, scene):
    """PIES_PCG_NEVER_EXIT=1 (profiling: every captured CG launch does its full work) is meant to leave positions and velocities
    bit for bit as they are ("a converged column stands still", substep_graph.cpp).  It does not: cg1_scalars / k_cg_update
    freeze a column only when its gamma is exactly 0 or its denominator is not positive, so a column below the tolerance keeps
    taking the steps the early exit skips - positions move by up to 1.4e-5 on scene B, and on scene D (contact rows) 11 of 24
    solves end above the tolerance.  (The single tetrahedron converges exactly and is bit-equal.)  Strict: once the kernels
    freeze a converged solve, this passes and the marker has to go."""
    steps = oracle_run(oracle, scene)
    res = []
    for variant in ("default", "never_exit"):
        set_variant(tune, variant, scene)
        g, states = device_run(pies, scene, steps)
        health = g.pcg_health()
        g.close()
        assert health["short_solves"] == 0, (scene, variant, health)
        res.append(states)
    for t, ((p, v), (q, w)) in enumerate(zip(res[0], res[1])):
        record("never_exit_%s" % scene, "vs_default_positions", float(np.abs(p - q).max()), 0.0)
        assert np.array_equal(p, q) and np.array_equal(v, w), (scene, t, float(np.abs(p - q).max()), float(np.abs(v - w).max()))


class _Arrays:
    def __init__(self, p, v):
        self.positions, self.velocities = p, v


# ---------------------------------------------------------------------------------------------------------------------------
# Friction order of the listed node pairs (pies_add_node_pair_constraints).  The reference runs, after the velocity update, the
# node-node friction (Solver.cpp:398-428), the point-triangle friction (:431-471), then the floor friction (:473-484).  Scene:
# two tet boxes resting on the floor, side by side, sliding along z against each other; the bottom rows' overlapping node pairs
# are listed.  Their nodes are in floor contact, and both frictions change their velocities: the floor friction must come after
# the pairs'.  Every tick starts from the device's state (with the sliding drive re-imposed), so that the node contacts the
# device detects (PIES_FLAG_PD_NODE_CONTACTS) can be fed to the oracle after the listed pairs, as test_oracle_replay does.
FR, THR, DT = 0.3, 0.05, 0.012


def _friction_template(oracle):
    t = oracle.OracleSolver(pd_options(oracle, ITERS))
    t.create_tet_box(5, 2, 5, translation=(0.0, 0.02, 0.0), w=1.0)
    t.create_tet_box(3, 2, 6, translation=(4.95, 0.02, 0.2), w=1.0)
    return (t.positions, t.ids(oracle.TET), t.ids(oracle.VOLUME), t.ids(oracle.TRIANGLES), 50)


def _friction_scene(s, tpl, perm):
    """the template's scene with node k of the host numbering = template node perm[k]; returns the listed pairs (host ids)"""
    pos, tet, vol, tri, na = tpl
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    s.add_nodes_raw(pos[perm], radius=0.5)
    s.add_tet(inv[tet].astype(np.uint32), 1.0)
    s.add_volume(inv[vol].astype(np.uint32), 1.0)
    s.add_triangles(inv[tri].astype(np.uint32))
    a = [i for i in range(na) if pos[i, 1] < 0.05]
    b = [j for j in range(na, len(pos)) if pos[j, 1] < 0.05]
    pairs = np.uint32([(inv[i], inv[j]) for i in a for j in b if np.linalg.norm(pos[i] - pos[j]) < 1.0])
    s.add_node_pairs(pairs)
    return pairs


def _drive(v, first_body, speed=2.5):
    v = v.copy()
    v[first_body, 2], v[~first_body, 2] = speed, -speed
    v[first_body, 0] += 0.3
    v[~first_body, 0] -= 0.3
    return v


def _floor_friction(v, ns):
    v = v.copy()
    for i in np.nonzero(ns)[0]:
        for _ in range(int(ns[i])):
            perp = np.array([v[i, 0], 0.0, v[i, 2]])
            v[i] -= (FR if np.linalg.norm(perp) >= THR else 1.0) * perp
    return v


def _pair_friction(v, p, pairs):
    v = v.copy()
    for a, b in pairs:
        d = p[b] - p[a]
        dist = np.linalg.norm(d)
        if dist > 1.0:
            continue
        n = d / dist
        rv = v[b] - v[a]
        perp = rv - rv.dot(n) * n
        f = -FR if np.linalg.norm(perp) >= THR else 1.0
        v[a] += -f * perp * 0.5
        v[b] += f * perp * 0.5
    return v


@pytest.mark.parametrize("tri,contacts,renumber", [(1, 0, 0), (0, 0, 0), (1, 1, 0), (0, 1, 0), (1, 0, 1)])
def test_node_pair_floor_friction_order(pies, oracle, tune, tri, contacts, renumber):
    """The listed pairs' nodes on the floor, both branches of enqueue_pd_substep (triangle pipeline on / off), with and without
    the device's node-node contacts, and once with the nodes renumbered on the device (a shuffled host order and 64-row chunks,
    so that the Hilbert order is kept: the bitmap of the pairs' nodes is in device numbering).  Velocities against the fp64
    yardstick.  A numpy restatement of the friction tail (fp64, from the oracle's positions) shows that the scene exercises the
    order: it matches the oracle, and the other order (floor friction first) is several gates away from it."""
    tpl = _friction_template(oracle)
    n = len(tpl[0])
    perm = np.random.default_rng(3).permutation(n) if renumber else np.arange(n)
    if renumber:
        tune("PIES_CG_CHUNK_ROWS", "64")
    opts = dict(friction=FR, staticFrictionThreshold=THR)
    g = pies.Solver(pd_options(pies, ITERS, **opts))
    pairs = _friction_scene(g, tpl, perm)
    g.set_flag(pies.FLAG_TRIANGLE_COLLISIONS, tri)
    g.set_flag(pies.FLAG_PD_NODE_CONTACTS, contacts)
    g.set_flag(pies.FLAG_RENUMBER_NODES, renumber)
    g.set_pcg(3e-7, 256)  # (w = 1e5 on the diagonal: test_pd_node_pair_collision_constraints)
    first_body = perm < tpl[4]
    g.set_velocities(_drive(g.velocities, first_body))
    g.finalize()
    assert g.count(pies.NODES_RENUMBERED) == renumber and len(pairs) >= 4
    nodes = np.unique(pairs)
    tri_count = np.bincount(g.ids(pies.TRIANGLES).reshape(-1), minlength=n)
    test = "node_pair_floor_friction_tri%d_nc%d_renum%d" % (tri, contacts, renumber)
    worst, contacts_seen = 0.0, 0
    for t in range(TICKS):
        pos, prev, vel = g.positions, g.prev_positions, _drive(g.velocities, first_body)
        g.set_velocities(vel)
        g.tick()
        listed = pairs if not contacts else np.concatenate([pairs, g.node_contacts().astype(np.uint32).reshape(-1, 2)])
        contacts_seen += len(listed) - len(pairs)
        o32, o64 = oracle.OracleSolver(pd_options(oracle, ITERS, **opts)), oracle.OracleSolver(pd_options(oracle, ITERS, **opts))
        o64.set_flag(oracle.FLAG_PD_SOLVE_FP64, 1)
        for o in (o32, o64):
            _friction_scene(o, tpl, perm)
            o.set_flag(oracle.FLAG_TRIANGLE_COLLISIONS, tri)
            o.set_positions(pos); o.set_prev_positions(prev); o.set_velocities(vel)
            if contacts and len(listed) > len(pairs):
                o.add_node_pairs(listed[len(pairs):])
            o.tick()
        yardstick(test, g, o32, o64, names=("positions", "velocities"))
        # the scene exercises the order: the listed nodes are on the floor, and both frictions move their velocities
        p1 = o32.positions.astype(np.float64)
        v0 = (1.0 - 0.006) * (p1 - pos) / DT + DT * np.array([0.0, -10.0, 0.0])
        ns = np.where(pos[:, 1] + DT * vel[:, 1] < 0.05, tri_count, 0)
        assert (ns[nodes] > 0).all(), (t, ns[nodes])
        ref = _floor_friction(_pair_friction(v0, p1, pairs), ns)
        other = _pair_friction(_floor_friction(v0, ns), p1, pairs)
        if not tri and not contacts:
            assert np.abs(ref - o32.velocities)[nodes].max() < 1e-4, t  # (the restatement is the oracle's arithmetic)
        assert np.abs(_pair_friction(v0, p1, pairs) - v0)[nodes].max() > 0.1 and np.abs(_floor_friction(v0, ns) - v0)[nodes].max() > 0.1
        worst = max(worst, float(np.abs(ref - other)[nodes].max()))
    record(test, "order_effect[velocities]", worst, 1e-4 / DT)
    assert worst > 4 * 1e-4 / DT, worst  # the wrong order would be caught by the gate several times over
    if contacts:
        assert contacts_seen > 0
    assert g.pcg_health()["short_solves"] == 0 and not g.failed
