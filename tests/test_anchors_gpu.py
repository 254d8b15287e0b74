"""GPU tests of pies_apply_anchors.  The yardstick is the numpy fp32 restatement of the rule (tests/test_anchors.py: apply_anchors):
positions, previous positions and velocities read back after the call, the impulse, the torque and the live count per frame and
the per-anchor array must be equal BIT FOR BIT - the rule uses only fp32 + - x / sqrt and comparisons, which the device and numpy
round alike, and the sums have one stated order."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

import scenes
from test_anchors import (A_FIXED, A_PIN, A_RELEASED, A_SPRING, DT, F, apply_anchors, check_marks, make_frames, make_scene, rows_of)
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu

NODES = (1, 63, 65, 255, 257, 600)  # the lane tail of a wavefront; 1, 2 and 3 workgroups of anchored nodes
ANCHORS = (1, 255, 257, 700)        # one tile, the tile's edge, a second and a third tile of the sum order
FRAMES = (1, 3, 64)


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


def restated(before, inv_mass, anchors, frames, dt, trace=None):
    return apply_anchors(before[0], before[2], inv_mass, anchors, frames, dt, prev=before[1], trace=trace)


def assert_call(g, anchor_set, frames, dt, want, what=""):
    """one call with every output against `want` = apply_anchors(...) of the state before it"""
    impulse, torque, live, per_anchor = g.apply_anchors(anchor_set, frames, dt, per_anchor=True)
    for name, got, exp in zip(("positions", "previous positions", "velocities"), state(g), want[:3]):
        assert same_bits(got, exp), (what, name, int((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1).sum()))
    assert same_bits(per_anchor, want[6]), (what, "per anchor", int((per_anchor.view(np.uint32) != want[6].view(np.uint32)).any(axis=1).sum()))
    assert same_bits(impulse, want[3]) and same_bits(torque, want[4]), (what, "sums")
    assert np.array_equal(live, want[5]), (what, live, want[5])
    return impulse, torque, live, per_anchor


@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("n_anchors", ANCHORS)
@pytest.mark.parametrize("n_nodes", NODES)
def test_bits_equal_the_restatement(pies, n_nodes, n_anchors, n_frames):
    pos, vel, inv_mass, anchors, frames, marks = make_scene(n_nodes, n_anchors, n_frames)
    g = loose(pies, pos, vel, inv_mass)
    anchor_set = g.add_anchors(anchors, n_frames)
    before = state(g)
    assert same_bits(before[0], pos) and same_bits(before[2], vel)
    trace = []
    want = restated(before, inv_mass, anchors, frames, DT, trace=trace)
    assert_call(g, anchor_set, frames, DT, want)
    after = state(g)
    rows = rows_of(anchors, n_nodes)
    untouched = np.array([not any(trace[i] in (A_SPRING, A_PIN) for i in row) for row in rows])
    for a, b in zip(after, before):
        assert same_bits(a[untouched], b[untouched])
    pinned = np.array([any(trace[i] == A_PIN for i in row) for row in rows])
    moved = (after[0].view(np.uint32) != before[0].view(np.uint32)).any(axis=1)
    assert not moved[~pinned].any() and same_bits(after[1][~pinned], before[1][~pinned])
    if marks:  # every branch the rule has, and the rows the scene promises (0, 1, 2 and 40 anchors on a node)
        check_marks(anchors, frames, inv_mass, marks, trace)
        assert untouched.any() and moved.sum() == pinned.sum() >= 2 and not same_bits(after[2], before[2])


def test_dt_zero_and_released_frames(pies):
    pos, vel, inv_mass, anchors, frames, marks = make_scene(600, 700, 3)
    g = loose(pies, pos, vel, inv_mass)
    anchor_set = g.add_anchors(anchors, 3)
    before = state(g)
    trace = []
    want = restated(before, inv_mass, anchors, frames, F(0), trace=trace)
    out = assert_call(g, anchor_set, frames, 0.0, want, "dt == 0")
    after = state(g)
    rows = rows_of(anchors, 600)
    pinned = np.array([any(trace[i] == A_PIN for i in row) for row in rows])
    assert pinned.sum() == 2 and same_bits(after[2][~pinned], vel[~pinned])  # the springs do nothing ...
    spring = np.array([c == A_SPRING for c in trace])
    assert spring.any() and not out[3][spring, :3].any() and (out[3][:, 3] > 0).all()
    assert not same_bits(after[0][pinned], pos[pinned]) and same_bits(after[0][~pinned], pos[~pinned])  # ... and the pins hold
    released_pin = marks["pins"][1]
    assert trace[rows[released_pin][0]] == A_RELEASED and all(same_bits(a[released_pin], b[released_pin]) for a, b in zip(after, before))
    # every frame released: nothing is written, nothing is live, the stretch is still given
    g2 = loose(pies, pos, vel, inv_mass)
    set2 = g2.add_anchors(anchors, 3)
    off = make_frames(3)
    for f in off:
        f.strength = 0.0
    impulse, torque, live, per_anchor = g2.apply_anchors(set2, off, DT, per_anchor=True)
    assert not impulse.any() and not torque.any() and not live.any() and not per_anchor[:, :3].any() and (per_anchor[:, 3] > 0).all()
    for a, b in zip(state(g2), before):
        assert same_bits(a, b)


def test_outputs_are_optional_and_calls_repeat(pies):
    pos, vel, inv_mass, anchors, frames, _ = make_scene(600, 700, 64)
    full = loose(pies, pos, vel, inv_mass)
    out = full.apply_anchors(full.add_anchors(anchors, 64), frames, DT, per_anchor=True)
    after = state(full)
    L, arr = pies.load(), (pies.AnchorFrame * 64)(*frames)
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for asked in itertools.product((False, True), repeat=4):  # every subset of the outputs
        g = loose(pies, pos, vel, inv_mass)
        anchor_set = g.add_anchors(anchors, 64)
        bufs = (np.full((64, 3), 7, F), np.full((64, 3), 7, F), np.full(64, 7, np.uint32), np.full((700, 4), 7, F))
        args = [b.ctypes.data_as(pu if b.dtype == np.uint32 else pf) if a else None for a, b in zip(asked, bufs)]
        assert L.pies_apply_anchors(g._h, anchor_set, 64, arr, DT, *args) == pies.OK, asked
        for a, b in zip(state(g), after):
            assert same_bits(a, b), asked
        for a, got, exp in zip(asked, bufs, out):
            assert same_bits(got, exp) if a else (got == 7).all(), asked
    bare = loose(pies, pos, vel, inv_mass)
    assert bare.apply_anchors(bare.add_anchors(anchors, 64), frames, DT, reaction=False) is None
    # a second call on the edited state is the restatement of the restatement
    want = restated(after, inv_mass, anchors, frames, DT)
    assert_call(full, 0, frames, DT, want, "second call")
    assert not same_bits(want[2], after[2])


def tet_box(pies, solver, schedule=None):
    g = pies.Solver(pies.Options(solver=solver))
    if schedule is not None:
        g.set_schedule(schedule)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def box_anchors(pies, pos):
    """the top face of the tet box tied to a frame that moves up and turns, two of its corners pinned; a second frame holds one
    bottom node by two springs"""
    top = np.nonzero(pos[:, 1] == pos[:, 1].max())[0]
    centre = np.round(pos[top].astype(np.float64).mean(axis=0) * 16) / 16
    frames = [pies.AnchorFrame.make(centre, velocity=(0.5, 2.0, 0.0), angular=(0.0, 1.5, 0.0), strength=1.0),
              pies.AnchorFrame.make((0.0, 1.0, 0.0), velocity=(0.0, -1.0, 0.5), strength=0.5)]
    now = pies.AnchorFrame.make(centre + [0.0625, 0.125, 0.0])  # where the hub stands now: the springs are stretched
    corners = [top[0], top[-1]]
    anchors = [pies.Anchor.at(int(i), 0, now, pos[i], pin=True) if i in corners else
               pies.Anchor.at(int(i), 0, now, pos[i], stiffness=800.0 + 10.0 * k, damping=1.5) for k, i in enumerate(top)]
    low = int(np.nonzero(pos[:, 1] == pos[:, 1].min())[0][0])
    anchors += [pies.Anchor.make(low, 1, (0.5, 0.25, 0.5), stiffness=300.0), pies.Anchor.make(low, 1, (0.0, 0.5, 1.0), stiffness=150.0, damping=4.0)]
    return anchors, frames, corners


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_the_edit_reaches_the_next_substep(pies, solver, schedule):
    """apply_anchors on one handle, read + restatement + set_positions / set_prev_positions / set_velocities on the other, then one
    tick on both: the same bits, under PBD's three schedules and under PD."""
    sched = None if schedule is None else getattr(pies, "SCHEDULE_" + schedule)
    device, host = tet_box(pies, getattr(pies, solver), sched), tet_box(pies, getattr(pies, solver), sched)
    device.finalize()
    host.finalize()
    before = state(host)
    anchors, frames, corners = box_anchors(pies, before[0])
    anchor_set = device.add_anchors(anchors, 2)
    want = restated(before, host.inv_masses, anchors, frames, DT)
    out = assert_call(device, anchor_set, frames, DT, want, "after the call")
    assert out[2].tolist() == [len(anchors) - 2, 2] and not same_bits(want[0][corners], before[0][corners])
    host.set_positions(want[0])
    host.set_prev_positions(want[1])
    host.set_velocities(want[2])
    device.tick()
    host.tick()
    assert not device.failed and np.isfinite(device.positions).all()
    for a, b in zip(state(device), state(host)):
        assert same_bits(a, b)
    calm = tet_box(pies, getattr(pies, solver), sched)
    calm.tick()
    assert not same_bits(device.positions, calm.positions)


def test_renumbered_scene_gives_the_same_bits(pies):
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES: node state in host numbering, the sums (whose order is defined on
    anchor indices) and the per-anchor array are those of the same scene with the flag off, and the restatement's."""
    mesh = shuffled_beam()
    pos = np.asarray(mesh[0], F)
    n = len(pos)
    rng = np.random.default_rng(23)
    frames = make_frames(3, seed=5)
    frames[1].strength = 0.75  # (three live frames)
    now = [pies.AnchorFrame.from_buffer_copy(f) for f in frames]
    nodes = rng.permutation(n)[:900]
    anchors = []
    for k, i in enumerate(nodes):
        f = k % 3
        spot = pos[i] + rng.normal(size=3).astype(F) * F(0.05)
        anchors.append(pies.Anchor.at(int(i), f, now[f], spot, pin=True) if k % 97 == 0 else
                       pies.Anchor.at(int(i), f, now[f], spot, stiffness=float(F(rng.uniform(50, 900))), damping=float(F(rng.uniform(0, 5)))))
    anchors += [pies.Anchor.at(int(i), 2, now[2], pos[i], stiffness=250.0) for i in nodes[1:60]]  # second springs (none of them pinned)
    vel = (rng.normal(size=(n, 3)) * 2).astype(F)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        anchor_set = g.add_anchors(anchors, 3)
        before = state(g)
        out = g.apply_anchors(anchor_set, frames, DT, per_anchor=True)
        assert g.count(pies.NODES_RENUMBERED) == flag
        got.append((state(g), out))
        if flag:
            want = restated(before, g.inv_masses, anchors, frames, DT)
    (state_on, out_on), (state_off, out_off) = got
    for a, b, c in zip(state_on, state_off, want[:3]):
        assert same_bits(a, b) and same_bits(a, c)
    for a, b, c in zip(out_on, out_off, want[3:]):
        assert same_bits(a, b) and same_bits(a, c)
    assert len(anchors) > 3 * 256 and (out_on[2] > 0).all() and sum(a.flags for a in anchors) >= 5


def test_sets_are_assets(pies):
    """a set added before pies_finalize is applied after it, after a tick, and after nodes were appended and the scene finalized
    again - each time the bits of a fresh handle brought to the same state, which is what the restatement gives -; two sets on one
    handle are independent; after pies_clear the id is refused"""
    g = tet_box(pies, pies.PBD)
    anchors, frames, corners = box_anchors(pies, g.positions)
    first = g.add_anchors(anchors, 2)
    other_anchors = [pies.Anchor.make(1, 0, (0.5, 2.0, 0.5), stiffness=500.0, damping=1.0), pies.Anchor.make(2, 0, (1.0, 2.0, 0.5), pin=True)]
    other_frames = [pies.AnchorFrame.make((0.25, 0.0, 0.0), velocity=(1.0, 0.0, 0.0), strength=2.0)]
    other = g.add_anchors(other_anchors, 1)
    assert (first, other) == (0, 1)
    g.finalize()
    fresh = tet_box(pies, pies.PBD)
    fresh.finalize()
    before = state(g)
    want = restated(before, g.inv_masses, anchors, frames, DT)
    out = assert_call(g, first, frames, DT, want, "after finalize")
    got = fresh.apply_anchors(fresh.add_anchors(anchors, 2), frames, DT, per_anchor=True)  # (added after the finalize)
    for a, b in zip(out, got):
        assert same_bits(a, b)
    for a, b in zip(state(g), state(fresh)):
        assert same_bits(a, b)
    g.tick()
    before = state(g)
    assert_call(g, first, frames, DT, restated(before, g.inv_masses, anchors, frames, DT), "after a tick")
    before = state(g)
    assert_call(g, other, other_frames, DT, restated(before, g.inv_masses, other_anchors, other_frames, DT), "the second set")
    n = g.count(pies.NODES)
    g.create_tet_box(2, 2, 2, translation=(6.0, 1.5, 0.5))  # appended nodes: the device copy is dropped and staged again
    assert g.count(pies.NODES) > n
    before = state(g)
    want = restated(before, g.inv_masses, anchors, frames, DT)
    assert_call(g, first, frames, DT, want, "after appended nodes")
    assert same_bits(state(g)[2][n:], before[2][n:])
    assert [bytes(a) for a in g.get_anchors(first)[0]] == [bytes(a) for a in anchors]
    g.clear()
    with pytest.raises(pies.PiesError):
        g.apply_anchors(first, frames, DT)
    assert "unknown set" in g.last_error()


def test_the_call_runs_behind_queued_work(pies):
    queued, plain, frames_box = (tet_box(pies, pies.PBD) for _ in range(3))
    anchors, frames, _ = box_anchors(pies, plain.positions)
    sets = [g.add_anchors(anchors, 2) for g in (queued, plain, frames_box)]
    plain.tick(2)
    queued.tick_async(2)
    a = queued.apply_anchors(sets[0], frames, DT, per_anchor=True)
    b = plain.apply_anchors(sets[1], frames, DT, per_anchor=True)
    assert b[2].tolist() == [len(anchors) - 2, 2]
    for x, y in zip(state(queued), state(plain)):
        assert same_bits(x, y)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # a frame begun before the call delivers that frame's positions, and the call edits the state behind it
    frame = frames_box.tick_begin()
    frames_box.apply_anchors(sets[2], frames, DT, reaction=False)
    exported = frames_box.export_acquire(frame)[:, :3].copy()
    frames_box.export_release(frame)
    once = tet_box(pies, pies.PBD)
    once.tick()
    assert same_bits(exported, once.positions)
    before = state(once)
    want = restated(before, once.inv_masses, anchors, frames, DT)
    for x, y in zip(state(frames_box), want[:3]):
        assert same_bits(x, y)
    assert not same_bits(want[0], before[0]) and not same_bits(want[2], before[2])


def test_the_substep_is_untouched(pies):
    for solver in (pies.PBD, pies.PD):
        g = tet_box(pies, solver)
        anchors, frames, _ = box_anchors(pies, g.positions)
        anchor_set = g.add_anchors(anchors, 2)
        g.tick()
        before = g.launch_counts()
        out = g.apply_anchors(anchor_set, frames, DT)
        assert out[2][0] >= 1 and g.launch_counts() == before
        g.tick()
        assert not g.failed


def test_a_scene_without_nodes(pies):
    """no node, no set: every anchor names a node that does not exist, and a handle without sets refuses every id - before and after
    a finalize of the empty scene"""
    empty = pies.Solver(pies.Options(solver=pies.PBD))
    frames = [pies.AnchorFrame.make((0.0, 1.0, 0.0))]
    for _ in range(2):
        with pytest.raises(pies.PiesError):
            empty.add_anchors([pies.Anchor.make(0, 0, (0.0, 0.0, 0.0), stiffness=1.0)], 1)
        assert "node id" in empty.last_error()
        with pytest.raises(pies.PiesError):
            empty.apply_anchors(0, frames, DT)
        assert "unknown set" in empty.last_error()
        empty.finalize()
    assert empty.count(pies.NODES) == 0 and not empty.failed


def test_resources_return_to_zero(pies):
    """what the calls allocate is counted (pies_resource_counts), held over repeated calls, and given back: a handle that used
    anchors is left by pies_clear with what a handle that did not is left with, and by pies_destroy with nothing"""
    gc.collect()
    live = lambda: pies.resource_counts()["live"]  # noqa: E731
    start = live()

    def cycle(anchored):
        base = live()
        g = tet_box(pies, pies.PBD)
        g.finalize()
        built = live()
        if anchored:
            anchors, frames, _ = box_anchors(pies, g.positions)
            sets = [g.add_anchors(anchors, 2), g.add_anchors(anchors[:3], 2)]
            counts = []
            for _ in range(3):
                for s in sets:
                    g.apply_anchors(s, frames, DT, per_anchor=True)
                counts.append(live())
            assert counts[0] == counts[1] == counts[2]
            assert counts[0]["device_allocations"] > built["device_allocations"]  # the calls do allocate
        g.clear()
        cleared = {k: v - base[k] for k, v in live().items()}
        g.close()
        assert live() == base
        return cleared

    assert cycle(True) == cycle(False)
    assert live() == start
