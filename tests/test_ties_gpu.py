"""GPU tests of pies_apply_ties.  The yardstick is the numpy fp32 restatement of the rule (tests/test_ties.py: apply_ties): the
velocities read back after the call, the impulse, the torque and the live count per group, the per-tie array and the broken bytes
must be equal BIT FOR BIT - the rule uses only fp32 + - x / sqrt and comparisons, which the device and numpy round alike, and
every sum has one stated order.  Positions and previous positions must not change by a bit."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

import scenes
from test_node_renumber import shuffled_beam
from test_ties import DT, F, T_BROKEN, T_LIVE, apply_ties, check_marks, entries_of, make_groups, make_scene

pytestmark = pytest.mark.gpu

NODES = (5, 63, 65, 257, 600)   # dense rows on five nodes; the lane tail of a wavefront; 1, 2 and 3 workgroups of tied nodes
TIES = (1, 255, 257, 700)       # one tile, the tile's edge, a second and a third tile of the sum order and of the tie lanes
GROUPS = (1, 3, 64)
ITERATIONS = (1, 2, 8)
CASES = [(n, t, g, 2) for n in NODES for t in TIES for g in GROUPS] + [(600, 700, g, i) for g in GROUPS for i in (1, 8)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def loose(pies, pos, vel, inv_mass):
    g = pies.Solver(pies.Options(solver=pies.PBD))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=np.full(len(pos), 0.05, F), invMass=inv_mass)
    return g


def state(g):
    return g.positions, g.prev_positions, g.velocities


def assert_call(g, tie_set, groups, dt, iterations, before, want, what=""):
    """one call with every output against `want` = apply_ties(...) of the state `before` it"""
    impulse, torque, live, per_tie = g.apply_ties(tie_set, groups, dt, iterations, per_tie=True)
    after = state(g)
    assert same_bits(after[0], before[0]) and same_bits(after[1], before[1]), (what, "positions")
    assert same_bits(after[2], want[0]), (what, "velocities", int((after[2].view(np.uint32) != want[0].view(np.uint32)).any(axis=1).sum()))
    assert same_bits(per_tie, want[4]), (what, "per tie", int((per_tie.view(np.uint32) != want[4].view(np.uint32)).any(axis=1).sum()))
    assert same_bits(impulse, want[1]) and same_bits(torque, want[2]), (what, "sums")
    assert np.array_equal(live, want[3]), (what, live, want[3])
    assert np.array_equal(g.tie_state(tie_set), want[5]), (what, "broken")
    return impulse, torque, live, per_tie


@pytest.mark.parametrize("n_nodes,n_ties,n_groups,iterations", CASES)
def test_bits_equal_the_restatement(pies, n_nodes, n_ties, n_groups, iterations):
    pos, vel, inv_mass, ties, groups, marks = make_scene(n_nodes, n_ties, n_groups)
    g = loose(pies, pos, vel, inv_mass)
    tie_set = g.add_ties(ties, n_groups)
    before = state(g)
    assert same_bits(before[0], pos) and same_bits(before[2], vel)
    trace = []
    want = apply_ties(before[0], before[2], inv_mass, ties, groups, DT, iterations, trace=trace)
    assert_call(g, tie_set, groups, DT, iterations, before, want)
    live = np.array(trace) == T_LIVE
    touched = np.zeros(n_nodes, bool)
    for v, i, _ in entries_of(ties):
        touched[v] |= live[i]
    assert same_bits(state(g)[2][~touched], vel[~touched])
    if marks:  # every branch the rule has, and the rows the scene promises (0, 1, 2 and 70 entries on a node)
        check_marks(ties, groups, inv_mass, marks, trace)
        assert not same_bits(want[0], vel) and want[5].any() and not want[5].all()


def test_dt_zero_and_released_groups(pies):
    pos, vel, inv_mass, ties, groups, _ = make_scene(600, 700, 3)
    g = loose(pies, pos, vel, inv_mass)
    tie_set = g.add_ties(ties, 3)
    before = state(g)
    trace = []
    want = apply_ties(before[0], before[2], inv_mass, ties, groups, F(0), 4, trace=trace)
    out = assert_call(g, tie_set, groups, 0.0, 4, before, want, "dt == 0")
    assert same_bits(state(g)[2], vel) and not out[3][:, :3].any() and (out[3][:, 3] > 0).all()  # nothing is written ...
    assert g.tie_state(tie_set).sum() == trace.count(T_BROKEN) > 0 and out[2].sum() == trace.count(T_LIVE) > 0  # ... ties still break
    # every group released: nothing is written, nothing is live, the stretch is still given and long ties still break
    g2 = loose(pies, pos, vel, inv_mass)
    set2 = g2.add_ties(ties, 3)
    off = make_groups(3)
    for f in off:
        f.strength = 0.0
    want = apply_ties(pos, vel, inv_mass, ties, off, DT, 4)
    impulse, torque, live, per_tie = assert_call(g2, set2, off, DT, 4, before, want, "released")
    assert not impulse.any() and not torque.any() and not live.any() and not per_tie[:, :3].any() and (per_tie[:, 3] > 0).all()
    assert same_bits(state(g2)[2], vel) and g2.tie_state(set2).any()


def test_outputs_are_optional_and_calls_repeat(pies):
    pos, vel, inv_mass, ties, groups, _ = make_scene(600, 700, 64)
    full = loose(pies, pos, vel, inv_mass)
    out = full.apply_ties(full.add_ties(ties, 64), groups, DT, 4, per_tie=True)
    after = state(full)
    broken = full.tie_state(0)
    L, arr = pies.load(), (pies.TieGroup * 64)(*groups)
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for asked in itertools.product((False, True), repeat=4):  # every subset of the outputs
        g = loose(pies, pos, vel, inv_mass)
        tie_set = g.add_ties(ties, 64)
        bufs = (np.full((64, 3), 7, F), np.full((64, 3), 7, F), np.full(64, 7, np.uint32), np.full((700, 4), 7, F))
        args = [b.ctypes.data_as(pu if b.dtype == np.uint32 else pf) if a else None for a, b in zip(asked, bufs)]
        assert L.pies_apply_ties(g._h, tie_set, 64, arr, DT, 4, *args) == pies.OK, asked
        for a, b in zip(state(g), after):
            assert same_bits(a, b), asked
        assert np.array_equal(g.tie_state(tie_set), broken), asked
        for a, got, exp in zip(asked, bufs, out):
            assert same_bits(got, exp) if a else (got == 7).all(), asked
    bare = loose(pies, pos, vel, inv_mass)
    assert bare.apply_ties(bare.add_ties(ties, 64), groups, DT, 4, reaction=False) is None
    # a second call on the edited state is the restatement of the restatement, with the first call's broken ties
    want = apply_ties(after[0], after[2], inv_mass, ties, groups, DT, 4, broken=broken)
    assert_call(full, 0, groups, DT, 4, after, want, "second call")
    assert not same_bits(want[0], after[2]) and broken.any()


def test_broken_ties_stay_broken_until_reset(pies):
    """the broken bytes survive a pies_finalize forced by an appended body - the device copy is dropped and staged again from the
    host copy the call refreshed - and pies_reset_ties clears them"""
    pos, vel, inv_mass, ties, groups, _ = make_scene(257, 255, 3)
    g = loose(pies, pos, vel, inv_mass)
    tie_set = g.add_ties(ties, 3)
    before = state(g)
    first = apply_ties(before[0], before[2], inv_mass, ties, groups, DT, 2)
    assert_call(g, tie_set, groups, DT, 2, before, first, "first")
    assert first[5].any() and not first[5].all()
    slack = [pies.TieGroup.from_buffer_copy(x) for x in groups]
    for x in slack:
        x.break_stretch = 0.0  # no tie breaks in these calls: what is broken is what the set remembers
    extra = np.array([[9.0, 9.0, 9.0]], F)
    g.add_nodes_raw(extra, vel=np.zeros((1, 3), F), radius=np.full(1, 0.05, F), invMass=np.ones(1, F))
    before = state(g)
    assert len(before[0]) == len(pos) + 1
    masses = np.concatenate([inv_mass, np.ones(1, F)])
    second = apply_ties(before[0], before[2], masses, ties, slack, DT, 2, broken=first[5])
    out = assert_call(g, tie_set, slack, DT, 2, before, second, "after a finalize")
    assert np.array_equal(second[5], first[5]) and not out[3][first[5].astype(bool), :3].any()
    g.reset_ties(tie_set)
    assert not g.tie_state(tie_set).any()
    before = state(g)
    third = apply_ties(before[0], before[2], masses, ties, slack, DT, 2)
    out = assert_call(g, tie_set, slack, DT, 2, before, third, "after a reset")
    assert not third[5].any() and out[2].sum() > second[3].sum()


def two_boxes(pies, solver, schedule=None):
    g = pies.Solver(pies.Options(solver=solver))
    if schedule is not None:
        g.set_schedule(schedule)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    n = g.count(pies.NODES)
    g.create_tet_box(3, 3, 3, translation=(0.5, 2.75, 0.5))
    return g, n


def box_ties(pies, pos, n):
    """the lower face of the upper box sewn to triangles of node triples of the lower box's upper face; two groups, the second
    breaks"""
    top = np.nonzero(pos[:n, 1] == pos[:n, 1].max())[0]
    low = n + np.nonzero(pos[n:, 1] == pos[n:, 1].min())[0]
    ties = []
    for j, a in enumerate(low):
        corners = [int(top[(j + s) % len(top)]) for s in (0, 1, 5)]
        ties.append(pies.Tie.on_triangle(int(a), corners, 0.25, 0.125 * (j % 4), stiffness=400.0 + 25.0 * j, damping=1.0 + 0.5 * (j % 3), group=j % 2))
    ties.append(pies.Tie.make(int(low[0]), int(top[3]), stiffness=200.0))
    groups = [pies.TieGroup.make((0.5, 2.0, 0.5)), pies.TieGroup.make((0.0, 2.0, 0.0), strength=0.5, break_stretch=0.75)]
    return ties, groups


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_ticks_and_calls_alternate(pies, solver, schedule):
    """three rounds of tick -> read the state -> apply -> compare with the restatement of the state read, under PBD's three
    schedules and under PD: the call edits what the next substep starts from, and a broken tie stays broken over the ticks"""
    sched = None if schedule is None else getattr(pies, "SCHEDULE_" + schedule)
    g, n = two_boxes(pies, getattr(pies, solver), sched)
    ties, groups = box_ties(pies, g.positions, n)
    tie_set = g.add_ties(ties, 2)
    broken = np.zeros(len(ties), np.uint8)
    for round_ in range(3):
        g.tick()
        before = state(g)
        want = apply_ties(before[0], before[2], g.inv_masses, ties, groups, DT, 4, broken=broken)
        out = assert_call(g, tie_set, groups, DT, 4, before, want, "round %d" % round_)
        assert (broken <= want[5]).all() and out[2][0] >= 1 and not same_bits(want[0], before[2])
        broken = want[5]
    assert not g.failed and np.isfinite(g.positions).all()
    calm, _ = two_boxes(pies, getattr(pies, solver), sched)
    calm.tick(3)
    assert not same_bits(g.positions, calm.positions)


def test_renumbered_scene_gives_the_same_bits(pies):
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES: node state in host numbering, the sums (whose order is defined on
    tie indices) and the per-tie array are those of the same scene with the flag off, and the restatement's."""
    mesh = shuffled_beam()
    pos = np.asarray(mesh[0], F)
    n = len(pos)
    rng = np.random.default_rng(29)
    groups = [pies.TieGroup.make((0.5, 0.5, 0.5)), pies.TieGroup.make((1.0, 0.0, 0.0), strength=0.75), pies.TieGroup.make((0.0, 1.0, 0.0), strength=2.0)]
    ties = []
    for k in range(900):
        a, b, c, d = (int(i) for i in rng.choice(n, 4, replace=False))
        u, v = rng.uniform(0.05, 0.45, 2)
        spring = dict(stiffness=float(F(rng.uniform(50, 900))), damping=float(F(rng.uniform(0, 5))), group=k % 3)
        ties.append(pies.Tie.on_triangle(a, (b, c, d), u, v, **spring) if k % 4 else pies.Tie.make(a, [b, c], (0.25, 0.75), **spring))
    vel = (rng.normal(size=(n, 3)) * 2).astype(F)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        tie_set = g.add_ties(ties, 3)
        before = state(g)
        out = g.apply_ties(tie_set, groups, DT, 4, per_tie=True)
        assert g.count(pies.NODES_RENUMBERED) == flag
        got.append((state(g), out))
        if flag:
            want = apply_ties(before[0], before[2], g.inv_masses, ties, groups, DT, 4)
    (state_on, out_on), (state_off, out_off) = got
    for a, b in zip(state_on, state_off):
        assert same_bits(a, b)
    assert same_bits(state_on[2], want[0])
    for a, b, c in zip(out_on, out_off, (want[1], want[2], want[3], want[4])):
        assert same_bits(a, b) and same_bits(a, c)
    assert len(ties) > 3 * 256 and (out_on[2] > 0).all()


def test_resources_return_to_zero(pies):
    """what the calls allocate is counted (pies_resource_counts), held over repeated calls, and given back: after pies_destroy of a
    handle that staged two sets the counts are those from before pies_create"""
    gc.collect()
    live = lambda: pies.resource_counts()["live"]  # noqa: E731
    start = live()
    g, n = two_boxes(pies, pies.PBD)
    g.finalize()
    built = live()
    ties, groups = box_ties(pies, g.positions, n)
    sets = [g.add_ties(ties, 2), g.add_ties(ties[:3], 2)]
    counts = []
    for _ in range(3):
        for s in sets:
            g.apply_ties(s, groups, DT, 2, per_tie=True)
        counts.append(live())
    assert counts[0] == counts[1] == counts[2]
    assert counts[0]["device_allocations"] > built["device_allocations"]  # the calls do allocate
    g.close()
    assert live() == start


def test_the_substep_is_untouched(pies):
    for solver in (pies.PBD, pies.PD):
        g, n = two_boxes(pies, solver)
        ties, groups = box_ties(pies, g.positions, n)
        tie_set = g.add_ties(ties, 2)
        g.tick()
        before = g.launch_counts()
        out = g.apply_ties(tie_set, groups, DT, 8)
        assert out[2][0] >= 1 and g.launch_counts() == before
        g.tick()
        assert not g.failed
