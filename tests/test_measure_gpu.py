"""GPU tests of pies_measure_elements / pies_measure_nodes.  The yardsticks are the numpy fp32 restatements of the two rules
(tests/test_measure.py: measure_elements, measure_nodes - the singular values from the oracle's svd3): records, summaries and node
sums must be equal BIT FOR BIT, flags and counts exactly, and node state, launch counts and the next ticks must be what they would
have been without the calls."""
import numpy as np
import pytest

import scenes
from test_measure import (T_COLLAPSED, T_IDENTITY, T_INVERTED, T_NONFINITE, T_OVER, T_UNDER, F, build_elements,
                          make_element_scene, make_node_scene, make_ranges, measure_elements, measure_nodes, summary_words)
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 65, 255, 257, 600)  # the lane tail of a wavefront; 1, 2 and 3 tiles of the summation orders


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_records(got, want):
    """bit for bit; of a NONFINITE record only the flags are specified"""
    ok = want["flags"] != T_NONFINITE
    return len(got) == len(want) and same_bits(got["flags"], want["flags"]) and same_bits(got[ok], want[ok])


def state(g):
    return g.positions, g.prev_positions, g.velocities


def posed(pies, scene, solver):
    """the scene on a device handle: finalized in the rest pose, then the measured pose written"""
    g = build_elements(pies, scene, solver)
    g.finalize()
    g.set_positions(scene["pos1"])
    return g


def want_of(scene, **kw):
    return measure_elements(scene["pos1"], scene["ids"], scene["rest"], scene["lo"], scene["hi"], scene["volume"], **kw)


@pytest.mark.parametrize("n_elems", SIZES)
def test_elements_equal_the_restatement(pies, n_elems):
    scene = make_element_scene(n_elems)
    g = posed(pies, scene, pies.PBD)
    assert same_bits(g.rest(pies.TET), scene["rest"])
    trace = []
    want, want_summary = want_of(scene, trace=trace)
    before = state(g)
    got, summary = g.measure_elements(pies.TET)
    assert same_records(got, want), int((got["flags"] != want["flags"]).sum())
    assert summary_words(summary) == summary_words(want_summary)
    for a, b in zip(state(g), before):
        assert same_bits(a, b)
    # records alone, the summary alone, both again: the same bits
    alone, none = g.measure_elements(pies.TET, summary=False)
    assert none is None and same_records(alone, want)
    none, again = g.measure_elements(pies.TET, records=False)
    assert none is None and summary_words(again) == summary_words(want_summary)
    assert g.measure_elements(pies.TET, records=False, summary=False) == (None, None)
    if n_elems >= 63:  # every branch of the rule
        bits, marks = trace[0], scene["marks"]
        assert bits[marks["rest"]] == T_IDENTITY and not bits[marks["rotated"]] & (T_IDENTITY | 15)
        assert got["green"][marks["rotated"]] < 1e-6 and got["green"][marks["rest"]] < 1e-6
        assert bits[marks["over"]] & 15 == T_OVER and bits[marks["under"]] & 15 == T_UNDER and bits[marks["inverted"]] & 15 == T_INVERTED
        assert bits[marks["collapsed"]] & (T_COLLAPSED | T_INVERTED) == T_COLLAPSED and got["j"][marks["collapsed"]] == 0
        assert bits[marks["nan"]] == T_NONFINITE and summary.nonfinite == 1 and got["flags"][marks["nan"]] == T_NONFINITE
        assert summary.inverted >= 1 and summary.over >= 1 and summary.under >= 2 and summary.min_j < 0 < summary.max_j
    # sub-ranges: first > 0, inside one tile, across a tile boundary
    for first, n in ((n_elems // 2, n_elems - n_elems // 2), (3, 40), (200, 100), (255, 2), (256, 300), (n_elems, 0)):
        if first + n > n_elems:
            continue
        want, want_summary = want_of(scene, first=first, n=n)
        got, summary = g.measure_elements(pies.TET, first, n)
        assert same_records(got, want), (first, n)
        assert summary_words(summary) == summary_words(want_summary), (first, n)


@pytest.mark.parametrize("solver,volume", [("PD", True), ("PD", False)])
def test_volume_and_strain_on_a_pd_handle(pies, solver, volume):
    scene = make_element_scene(600, volume)
    g = posed(pies, scene, getattr(pies, solver))
    ctype = pies.VOLUME if volume else pies.TET
    want, want_summary = want_of(scene)
    got, summary = g.measure_elements(ctype)
    assert same_records(got, want) and summary_words(summary) == summary_words(want_summary)
    assert summary.over > 1 and summary.under > 1 and summary.nonfinite == 1
    assert g.count(pies.TET if volume else pies.VOLUME) == 0
    with pytest.raises(pies.PiesError):
        g.measure_elements(pies.TET if volume else pies.VOLUME, 0, 1)


def tet_box(pies, solver, schedule=None):
    g = pies.Solver(pies.Options(solver=solver))
    if schedule is not None:
        g.set_schedule(schedule)
    g.create_tet_box(6, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def restated(pies, g, ctype):
    """the restatement of the handle's own scene at the positions read back"""
    lo, hi = (F(0.8), F(1.0)) if ctype == pies.TET else (F(1.0), F(1.0))  # create_tet_box's limits
    return measure_elements(g.positions, g.ids(ctype), g.rest(ctype), lo, hi, ctype == pies.VOLUME)


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_a_box_after_three_ticks(pies, solver, schedule):
    g = tet_box(pies, getattr(pies, solver), None if schedule is None else getattr(pies, "SCHEDULE_" + schedule))
    g.tick(3)
    assert not g.failed
    for ctype in (pies.TET, pies.VOLUME):
        got, summary = g.measure_elements(ctype)
        want, want_summary = restated(pies, g, ctype)
        assert len(got) == g.count(ctype) > 64 and same_records(got, want)
        assert summary_words(summary) == summary_words(want_summary) and summary.nonfinite == 0
    assert summary.max_green > 0


def test_renumbered_scene_gives_the_same_bits(pies):
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES, its nodes moved off the rest pose: element records (in host order)
    and node sums (over host ids) are those of the same scene with the flag off, and the restatement's."""
    mesh = shuffled_beam()
    n = len(mesh[0])
    rng = np.random.default_rng(23)
    vel = (rng.normal(size=(n, 3)) * 0.5).astype(F)
    moved = (np.asarray(mesh[0], np.float64) * [1.0, 1.0, 1.25] + rng.normal(size=(n, 3)) * 0.05).astype(F)
    ranges, about = make_ranges(n, 8)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_positions(moved)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        g.finalize()
        assert g.count(pies.NODES_RENUMBERED) == flag
        got.append((g.measure_elements(pies.TET), g.measure_nodes(ranges, about)))
        if flag:
            ids, rest = g.ids(pies.TET), g.rest(pies.TET)
            want = measure_elements(g.positions, ids, rest, F(0.8), F(1.0))  # (add_tet's default limits)
            want_nodes = measure_nodes(g.positions, g.velocities, g.inv_masses, ranges, about)
    ((rec_on, sum_on), nodes_on), ((rec_off, sum_off), nodes_off) = got
    assert len(rec_on) > 3 * 256 and n > 3 * 256
    assert same_bits(rec_on, rec_off) and summary_words(sum_on) == summary_words(sum_off)
    assert same_records(rec_on, want[0]) and summary_words(sum_on) == summary_words(want[1])
    assert sum_on.over > 100 and sum_on.nonfinite == 0
    assert same_bits(nodes_on, nodes_off) and same_bits(nodes_on, want_nodes)


def test_the_calls_see_the_scene_as_it_is(pies):
    scene = make_element_scene(65)
    g = posed(pies, scene, pies.PBD)
    first, _ = g.measure_elements(pies.TET)
    # a pies_set_rest between two calls is seen by the second
    rest = scene["rest"].copy()
    rest[10:20] *= F(0.5)
    g.set_rest(pies.TET, rest[10:20], first=10)
    second, summary = g.measure_elements(pies.TET)
    want, want_summary = measure_elements(scene["pos1"], scene["ids"], rest, scene["lo"], scene["hi"])
    assert same_records(second, want) and summary_words(summary) == summary_words(want_summary)
    assert not same_bits(second[10:20], first[10:20]) and same_bits(second[20:], first[20:])
    # ... and so is a body appended between two calls
    box = tet_box(pies, pies.PBD)
    before = box.count(pies.TET), box.count(pies.NODES)
    a, _ = box.measure_elements(pies.TET)
    box.create_tet_box(2, 2, 2, translation=(9.0, 1.5, 0.5))
    b, summary = box.measure_elements(pies.TET)
    want, want_summary = restated(pies, box, pies.TET)
    assert len(b) == box.count(pies.TET) > before[0] and same_bits(b[:before[0]], a)
    assert same_records(b, want) and summary_words(summary) == summary_words(want_summary)
    sums = box.measure_nodes([(0, before[1]), (before[1], box.count(pies.NODES) - before[1])])
    assert same_bits(sums, measure_nodes(box.positions, box.velocities, box.inv_masses, [(0, before[1]), (before[1], box.count(pies.NODES) - before[1])]))
    assert sums["dynamic"][1] + sums["fixed"][1] == 8


def test_the_calls_run_behind_queued_work(pies):
    queued, plain, frames = (tet_box(pies, pies.PBD) for _ in range(3))
    n = plain.count(pies.NODES)
    plain.tick(2)
    queued.tick_async(2)
    a, b = queued.measure_elements(pies.TET), plain.measure_elements(pies.TET)
    assert same_bits(a[0], b[0]) and summary_words(a[1]) == summary_words(b[1])
    want, want_summary = restated(pies, plain, pies.TET)
    assert same_records(b[0], want) and summary_words(b[1]) == summary_words(want_summary)
    queued.tick_async(1)
    plain.tick(1)
    assert same_bits(queued.measure_nodes([(0, n)]), plain.measure_nodes([(0, n)]))
    # a frame begun before the call delivers that frame's positions, and the call answers for the state after it
    frame = frames.tick_begin()
    got, summary = frames.measure_elements(pies.TET)
    sums = frames.measure_nodes([(0, n)])
    exported = frames.export_acquire(frame)[:, :3].copy()
    frames.export_release(frame)
    once = tet_box(pies, pies.PBD)
    once.tick()
    assert same_bits(exported, once.positions)
    want, want_summary = restated(pies, once, pies.TET)
    assert same_records(got, want) and summary_words(summary) == summary_words(want_summary)
    assert same_bits(sums, measure_nodes(once.positions, once.velocities, once.inv_masses, [(0, n)]))


def loose_nodes(pies, pos, vel, inv_mass):
    g = pies.Solver(pies.Options(solver=pies.PBD))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=np.full(len(pos), 0.05, F), invMass=inv_mass)
    return g


@pytest.mark.parametrize("n_ranges", (1, 3, 64))
@pytest.mark.parametrize("n_nodes", SIZES)
def test_node_sums_equal_the_restatement(pies, n_nodes, n_ranges):
    pos, vel, inv_mass = make_node_scene(n_nodes)
    ranges, about = make_ranges(n_nodes, n_ranges)
    g = loose_nodes(pies, pos, vel, inv_mass)
    before = state(g)
    trace = []
    want = measure_nodes(pos, vel, inv_mass, ranges, about, trace=trace)
    got = g.measure_nodes(ranges, about)
    assert same_bits(got, want), [k for k in range(n_ranges) if got[k] != want[k]]
    assert same_bits(g.measure_nodes(ranges, about), got)  # two calls, the same bits
    assert same_bits(g.measure_nodes(ranges), measure_nodes(pos, vel, inv_mass, ranges))  # about NULL: the origin
    for a, b in zip(state(g), before):
        assert same_bits(a, b)
    for k in range(n_ranges):  # a range alone gives the bits it gives in the list
        if k < 8 or k % 9 == 0:
            assert same_bits(g.measure_nodes(ranges[k:k + 1], about[k:k + 1])[0], got[k]), k
    if n_nodes == 600 and n_ranges == 64:
        assert {t for t, _, _ in trace} == {0, 1, 2, 3} and trace[1][1:] == (0, 5) and trace[2] == (0, 0, 0)
        assert got["dynamic"][1] == 0 and got["fixed"][1] == 5 and not got["mass"][1] and got["mass"][0] > 0


def test_the_calls_are_read_only(pies):
    for solver in (pies.PBD, pies.PD):
        measured, twin = tet_box(pies, solver), tet_box(pies, solver)
        n = twin.count(pies.NODES)
        measured.tick()
        twin.tick()
        counts, before = measured.launch_counts(), state(measured)
        measured.measure_elements(pies.TET)
        measured.measure_elements(pies.VOLUME, 5, 100, records=False)
        sums = measured.measure_nodes([(0, n), (n // 2, 10)], [(0, 1, 0), (1, 1, 1)])
        assert sums["dynamic"][0] + sums["fixed"][0] == n and sums["kinetic"][0] > 0
        assert measured.launch_counts() == counts
        for a, b in zip(state(measured), before):
            assert same_bits(a, b)
        measured.tick(3)
        twin.tick(3)
        assert not measured.failed
        if solver == pies.PBD:
            for a, b in zip(state(measured), state(twin)):
                assert same_bits(a, b)
        assert np.isfinite(measured.positions).all()
