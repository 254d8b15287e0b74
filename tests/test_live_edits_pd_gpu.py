"""Edits of a live Projective-Dynamics scene (see live_edits.py for the pattern): node-array writes, rest data, goals, flags and
the CG ceiling, appended bodies - each applied to a handle that is finalized, captured and ticked, and held to
test_pd_parity_gpu.yardstick against an fp32 and an fp64 oracle that took the same edit at the same moment.

The one these were written for: pies_write_nodes(PIES_NODE_INV_MASS).  The system matrix K = diag(1 / (invMass h^2)) + sum w A^T A,
its preconditioner and its dictionaries are built from the masses in pies_finalize, k_pd_predict reads the mass from pos.w; a write
that only uploads pos.w leaves the two sides of the solve with different masses (positions off by the mass ratio, 100 to 1 000
gates on these scenes)."""
import numpy as np
import pytest

import scenes
from live_edits import node_edit, pd_edit_matters, pd_gate, put_state, state_of
from test_node_renumber import shuffled
from test_pd_parity_gpu import yardstick
from test_skin import gates, skin_mesh

pytestmark = pytest.mark.gpu

BOTH = ("positions", "velocities")
WRITES = ("positions", "prev_positions", "velocities", "radii", "inv_masses")
# (radii: neighbours 1.0 apart with r = 0.475 do not touch, with 1.3 r they do - the listed node pairs below)


def options(mod, **kw):
    o = dict(solver=mod.PD, iterations=6)
    o.update(kw)
    return mod.Options(**o)


def beam(s, pairs=False, goal=False):
    """The 3 x 3 x 6 beam (54 nodes): w = 20, volume and triangles, the k = 0 cap pinned"""
    s.create_tet_box(3, 3, 6, translation=(0.0, 0.52, 0.0), w=20.0, volume=True, triangles=True)
    s.add_position(np.uint32([6 * (j + 3 * i) for i in range(3) for j in range(3)]), 2.0)
    if pairs:  # lattice neighbours along z in the middle of the beam: the only place a PD radius acts without detected contacts
        s.add_node_pairs(np.uint32([[6 * (j + 3 * i) + k, 6 * (j + 3 * i) + k + 1] for i in range(3) for j in range(3) for k in (2, 3)]))
    if goal:
        s.add_goal(np.uint32([6 * (j + 3 * i) + 5 for i in range(3) for j in range(3)]), 20.0)
    scenes.perturb(s, 9, 0.08)
    s.set_prev_positions(s.positions)


SHUFFLED = shuffled(scenes.delaunay_beam((4, 5, 14), seed=7), seed=2)  # (280 nodes: the smallest the suite renumbers)


def shuffled_beam(s, pairs=False, goal=False):
    pos, tets, edges = SHUFFLED
    scenes.build_unstructured_pd(s, SHUFFLED, w=20.0)
    if pairs:
        near = edges[np.abs(np.linalg.norm(pos[edges[:, 0]] - pos[edges[:, 1]], axis=1) - 1.05) < 0.05]
        s.add_node_pairs(near[:20])
    if goal:
        s.add_goal(np.nonzero(pos[:, 2] > pos[:, 2].max() - 0.8)[0].astype(np.uint32), 20.0)
    scenes.perturb(s, 9, 0.08)
    s.set_prev_positions(s.positions)


CONFIGS = {"pd": (beam, False), "pd-renumbered": (shuffled_beam, True)}


def device(pies, renumber=False, pcg=False, **kw):
    g = pies.Solver(options(pies, **kw))
    if renumber:
        g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    if pcg:  # True: w = 1e5 of a listed node pair on the diagonal needs more CG iterations than the default ceiling
        g.set_pcg(*((3e-7, 256) if pcg is True else pcg))
    return g


def oracles(oracle, count=3, **kw):
    """fp32, fp64, and fp64 again for the run without the edit"""
    out = [oracle.OracleSolver(options(oracle, **kw)) for _ in range(count)]
    for o in out[1:]:
        o.set_flag(oracle.FLAG_PD_SOLVE_FP64, 1)
    return out


def run(test, pies, oracle, build, edit, renumber=False, pcg=False, names=BOTH, k=2, m=2, tick=None):
    """The pattern: returns (L, S, o64) after the m compared ticks.  edit(s, S) is applied to L and to the two oracles."""
    L, T = device(pies, renumber, pcg), device(pies, renumber, pcg)
    o32, o64, without = oracles(oracle)
    for s in (L, T, o32, o64, without):
        build(s)
        s.tick(k)
    assert L.count(pies.NODES_RENUMBERED) == (1 if renumber else 0)
    S = state_of(T)
    T.close()
    for s in (L, o32, o64):
        edit(s, S)
    for t in range(m):
        (tick or (lambda g: g.tick()))(L)
        for o in (o32, o64, without):
            o.tick()
        if t == 0:
            pd_edit_matters(test, o32, o64, without, names)
        yardstick(test, L, o32, o64, names=names)
    assert not L.failed and L.pcg_health()["short_solves"] == 0
    return L, S, o64


# ---- 1. node-array writes, each alone ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", WRITES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_node_write(pies, oracle, config, what):
    """The mass case runs with pies_set_pcg(1e-7, 256): the seeded masses spread 100 : 1, and at the default relative residual of
    3e-7 the CG ends three times as far from the fp64 solve as the oracle's direct fp32 solve does - on the renumbered beam 4.22e-4
    against a gate of 2.98e-4 at the second tick, the same to the digit on a fresh handle built with these masses as on the live
    one, so it is the tolerance and not the edit (at 1e-7: 5.1e-5).  INTEGRATION.md tells hosts with such masses to do the same."""
    build, renumber = CONFIGS[config]
    pairs = what == "radii"
    pcg = True if pairs else (1e-7, 256) if what == "inv_masses" else None
    new = {}

    def edit(s, S):
        new[0] = node_edit(what, S)
        getattr(s, "set_" + what)(new[0])
    L, S, o64 = run("live_%s_write_%s" % (config, what), pies, oracle, lambda s: build(s, pairs=pairs), edit, renumber, pcg=pcg)
    if what == "inv_masses":  # the host reads the new masses back, and the exported frame carries them
        assert np.array_equal(L.inv_masses, new[0])
        f = L.tick_begin()
        frame = np.array(L.export_acquire(f))
        L.export_release(f)
        assert np.array_equal(frame[:, 3], new[0])
    for name in ("radii", "inv_masses"):
        assert np.array_equal(getattr(L, name), new[0] if name == what else S[name])


def test_mass_write_back_keeps_the_scene(pies):
    """Only new masses cost the rebuild: a host that writes back the masses it read keeps its device scene (pies_get_pcg_health
    counts the solves since the buffers were built), and the twin that wrote nothing stays equal bit for bit."""
    L, T = device(pies), device(pies)
    for g in (L, T):
        beam(g)
        g.tick(2)
    L.set_inv_masses(L.inv_masses)
    for g in (L, T):
        g.tick()
    assert L.pcg_health()["solves"] == T.pcg_health()["solves"] == 18
    for name in ("positions", "velocities", "prev_positions"):
        assert np.array_equal(getattr(L, name).view(np.uint32), getattr(T, name).view(np.uint32)), name
    L.set_inv_masses(L.inv_masses * np.float32(2.0))
    L.tick()
    assert L.pcg_health()["solves"] == 6  # new masses: the scene was built again


def boxes(s):
    """A createTetBox lattice held by its bottom layer and a second one 0.9 above it (r = 0.475 each: in contact from the start),
    offset and pressed down by gravity - contacts in every tick; no triangles, so that node contacts are all that holds it; 54 nodes"""
    s.create_tet_box(3, 3, 3, translation=(0.0, 3.0, 0.0), w=1.0, triangles=False)
    s.add_position(np.uint32([3 * (0 + 3 * i) + k for i in range(3) for k in range(3)]), 20.0)
    s.create_tet_box(3, 3, 3, translation=(0.3, 5.9, 0.2), velocity=(0.0, -1.0, 0.0), w=1.0, triangles=False)
    s.set_prev_positions(s.positions)


def run_contacts(test, pies, oracle, build, edit, k=2, m=2, flag_before=1):
    """PIES_FLAG_PD_NODE_CONTACTS: the oracle has no detection of its own - like test_pd_node_contacts_gpu.test_oracle_replay,
    fresh oracles are given the state before each tick and the contact list the device detected in it.  edit(L, S) returns the
    state after the edit; the run without it is the twin's next tick replayed the same way."""
    L, T = device(pies, pcg=True, friction=0.3), device(pies, pcg=True, friction=0.3)
    for g in (L, T):
        g.set_flag(pies.FLAG_PD_NODE_CONTACTS, flag_before)
        build(g)
        g.tick(k)
    S = state_of(T)
    before = edit(L, S)

    def replay(state, pairs, fp64):
        o = oracle.OracleSolver(options(oracle, friction=0.3))
        o.set_flag(oracle.FLAG_PD_SOLVE_FP64, fp64)
        build(o)
        put_state(o, state)
        if len(pairs):
            o.add_node_pairs(pairs)
        o.tick()
        return o
    seen = 0
    for t in range(m):
        L.tick()
        pairs = L.node_contacts()
        seen += len(pairs)
        o32, o64 = replay(before, pairs, 0), replay(before, pairs, 1)
        if t == 0:
            T.tick()
            pd_edit_matters(test, o32, o64, replay(S, T.node_contacts(), 1), BOTH)
        yardstick(test, L, o32, o64, names=BOTH)
        before = state_of(L)
    assert seen > 0 and not L.failed and L.pcg_health()["short_solves"] == 0
    return L


@pytest.mark.parametrize("what", WRITES)
def test_node_write_with_node_contacts(pies, oracle, what):
    def edit(L, S):
        after = dict(S)
        after[what] = node_edit(what, S, radius_factor=1.1)
        getattr(L, "set_" + what)(after[what])
        return after
    run_contacts("live_pd-contacts_write_%s" % what, pies, oracle, boxes, edit)


# ---- 2. rest data on a live handle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("container", ["TET", "VOLUME"])
def test_set_rest_partial_range(pies, oracle, container):
    """Qinv of elements 7 .. 46 of 240 scaled by 1 / 1.15 (a pre-strain): K, the rest dictionary and the row dictionary follow"""
    def edit(s, S):
        t = getattr(pies, container)  # (the same number in the oracle's binding)
        s.set_rest(t, s.rest(t)[7:47] * np.float32(1.0 / 1.15), first=7)
    assert getattr(pies, container) == getattr(oracle, container)
    L, S, o64 = run("live_pd_set_rest_%s" % container.lower(), pies, oracle, beam, edit)
    t = getattr(pies, container)
    assert np.array_equal(L.rest(t), o64.rest(t))


# ---- 3. goals ---------------------------------------------------------------------------------------------------------------

def translation(x, y, z):
    m = np.eye(4, dtype=np.float32)
    m[3, :3] = (x, y, z)  # column-major: m[col][row]
    return m.reshape(16)


@pytest.mark.parametrize("through", ["tick", "tick_begin"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_goal_transform_set_twice_last_wins(pies, oracle, config, through):
    build, renumber = CONFIGS[config]
    first, last = translation(-0.6, 0.9, 0.3), translation(0.4, 0.3, -0.2)
    name = "live_%s_goal_%s" % (config, through)
    frames = []

    def edit(s, S):
        s.set_goal_transform(0, first)
        s.set_goal_transform(0, last)

    def tick_begin(g):
        f = g.tick_begin()
        frames.append(np.array(g.export_acquire(f)))
        g.export_release(f)
    L, S, o64 = run(name, pies, oracle, lambda s: build(s, goal=True), edit, renumber, tick=tick_begin if through == "tick_begin" else None)
    if frames:
        assert np.array_equal(frames[-1][:, :3], L.positions)
    # had the first transform won, the result would be elsewhere: an fp64 oracle given the first one only, same ticks
    o32, alt = oracles(oracle, 2)
    for o in (o32, alt):
        build(o, goal=True)
        o.tick(2)
        o.set_goal_transform(0, first)
        o.tick(2)
    assert float(np.abs(alt.positions - o64.positions).max()) >= 10.0 * pd_gate(o32, alt, "positions")


# ---- 4. flags and the CG ceiling flipped between ticks ------------------------------------------------------------------------

def dropped_box(s):
    """test_oracle_golden._two_boxes - a box on the floor, a second above it, offset and falling - with the second one 0.14 higher
    and twice as fast: it reaches the first in ticks 3 and 4, the ticks compared (checked with the oracle: 38 and 118 contacts,
    20 gates in the velocities at tick 3)"""
    s.create_tet_box(3, 3, 3, translation=(0, 0.02, 0), w=1.0)
    s.create_tet_box(3, 3, 3, translation=(0.4, 2.2, 0.3), w=1.0)
    v = s.velocities
    v[27:, 1] = -4.0
    s.set_velocities(v)
    s.set_prev_positions(s.positions)


def test_triangle_collisions_switched_on(pies, oracle):
    def build(s):
        dropped_box(s)
        s.set_flag(pies.FLAG_TRIANGLE_COLLISIONS if isinstance(s, pies.Solver) else oracle.FLAG_TRIANGLE_COLLISIONS, 0)

    def edit(s, S):
        s.set_flag(pies.FLAG_TRIANGLE_COLLISIONS if isinstance(s, pies.Solver) else oracle.FLAG_TRIANGLE_COLLISIONS, 1)
    L, S, o64 = run("live_pd_triangle_collisions_on", pies, oracle, build, edit, pcg=True)
    assert len(L.tri_collisions) > 0 and o64.count(oracle.TRI_CONTACTS) > 0


def test_node_contacts_switched_on(pies, oracle):
    def edit(L, S):
        L.set_flag(pies.FLAG_PD_NODE_CONTACTS, 1)
        return S
    run_contacts("live_pd_node_contacts_on", pies, oracle, boxes, edit, flag_before=0)


def test_pcg_ceiling_changed(pies, oracle):
    """pies_set_pcg on a live handle: the substep is captured again with another iteration budget (that is what shows the edit
    arrived - the oracle's direct solve has no such parameter), the result stays inside the yardstick and no solve runs short."""
    L = device(pies)
    o32, o64 = oracles(oracle, 2)
    for s in (L, o32, o64):
        beam(s)
        s.tick(2)
    assert L.pcg_stats()[0] <= 3e-7 * 1.0001  # the default tolerance
    L.set_pcg(1e-6, 24)
    assert L.pcg_health()["budget"] == 24  # pies_set_pcg starts the budget over at min(max_iters, 32)
    for t in range(2):
        for s in (L, o32, o64):
            s.tick()
        yardstick("live_pd_set_pcg", L, o32, o64, names=BOTH)
    h = L.pcg_health()
    res, iters_used, solves = L.pcg_stats()
    assert h["budget"] <= 24 and h["short_solves"] == 0 and res <= 1e-6 * 1.0001 and iters_used <= 24 and solves == 6


# ---- 5. topology appended to a live scene -----------------------------------------------------------------------------------

def second_body(s):
    s.create_tet_box(2, 2, 3, translation=(8.0, 0.6, 0.0), velocity=(0.0, -2.0, 0.5), w=20.0, volume=True, triangles=True)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_second_body_appended(pies, oracle, config):
    build, renumber = CONFIGS[config]
    name = "live_%s_append" % config
    L = device(pies, renumber)
    o32, o64, without = oracles(oracle)
    for s in (L, o32, o64, without):
        build(s)
        s.tick(2)
    n_old = L.count(pies.NODES)
    for s in (L, o32, o64):
        second_body(s)
    factory = o64.positions[n_old:].copy()
    for t in range(2):
        for s in (L, o32, o64, without):
            s.tick()
        yardstick(name, L, o32, o64, names=BOTH)
        gate = pd_gate(o32, o64, "positions")
        if t == 0:  # the appended body moves (oracle values on both sides)
            assert float(np.abs(o64.positions[n_old:] - factory).max()) >= 10.0 * gate
        # host ids keep their meaning: in the oracle the first body, far from the second, continues the trajectory it has without
        # it, and the yardstick above holds the device's first n_old nodes to that
        assert float(np.abs(o64.positions[:n_old] - without.positions).max()) <= gate
    assert L.count(pies.NODES) == n_old + 12 and L.count(pies.NODES_RENUMBERED) == (1 if renumber else 0)
    assert np.array_equal(np.sort(L.node_order()), np.arange(n_old + 12))
    assert not L.failed and L.pcg_health()["short_solves"] == 0


def test_second_body_appended_with_a_skin_bound_to_the_first(pies, oracle):
    L = device(pies)
    beam(L)
    tets = L.ids(pies.TET)
    p = L.positions
    v, tri = skin_mesh(60, p.min(0) + 0.15, p.max(0) - 0.15)
    assert L.add_skin(v, tets, tri) == 0
    L.tick(2)
    second_body(L)
    L.tick()
    _, ids, w = L.skin_binding(0)
    x, nr = L.read_skin(0)
    x64, n64, gx, gn, _ = gates(L.positions, ids, w, tri)
    assert ids.max() < 54 and np.isfinite(x).all()
    assert float(np.abs(x - x64).max()) <= gx and float(np.abs(nr - n64).max()) <= gn
    assert float(np.abs(x - v).max()) > 100 * gx  # (the skin moved with the body)
