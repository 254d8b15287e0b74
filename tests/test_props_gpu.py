"""GPU tests of pies_collide_props.  The yardstick is the numpy fp32 restatement of the rule (tests/test_props.py: collide): the
node state read back after the call, the impulse, the torque, the hits and node_prop must be equal BIT FOR BIT - the rule uses only
fp32 + - x / sqrt, fmin / fmax and comparisons, which the device and numpy round alike, and the sums have one stated order."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_node_renumber import shuffled_beam
from test_props import ALL_BRANCHES, F, NONE, branches_of, collide, make_props, make_scene

pytestmark = pytest.mark.gpu

NODES = (1, 63, 65, 255, 257, 600)  # the lane tail of a wavefront; 1, 2 and 3 tiles of the summation order
PROPS = (1, 3, 64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def loose(pies, scene):
    pos, vel, radius, inv_mass, _ = scene
    g = pies.Solver(pies.Options(solver=pies.PBD))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=radius, invMass=inv_mass)
    return g


def state(g):
    return g.positions, g.prev_positions, g.velocities


def assert_state(g, want, what=""):
    for name, got, ref in zip(("positions", "previous positions", "velocities"), state(g), want):
        assert same_bits(got, ref), (what, name, int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1).sum()))


@pytest.mark.parametrize("n_props", PROPS)
@pytest.mark.parametrize("n_nodes", NODES)
def test_bits_equal_the_restatement(pies, n_nodes, n_props):
    scene = make_scene(n_nodes, n_props)
    pos, vel, radius, inv_mass, props = scene
    g = loose(pies, scene)
    before = state(g)
    assert same_bits(before[0], pos) and same_bits(before[2], vel)
    trace = []
    want = collide(before[0], before[1], before[2], radius, inv_mass, props, trace=trace)
    impulse, torque, hits, who = g.collide_props(props, node_prop=True)
    assert_state(g, want[:3])
    assert same_bits(impulse, want[3]) and same_bits(torque, want[4])
    assert np.array_equal(hits, want[5]) and np.array_equal(who, want[6])
    untouched = who == NONE
    for got, was in zip(state(g), before):
        assert same_bits(got[untouched], was[untouched])
    assert not (who[inv_mass == 0] != NONE).any() and hits.sum() >= (who != NONE).sum() > 0
    if n_nodes >= 255 and n_props >= 3:  # every branch of the rule among the touched nodes (placed by construction: make_scene)
        seen, dd0 = branches_of(trace)
        assert seen == ALL_BRANCHES and dd0, (sorted(ALL_BRANCHES - seen), dd0)
        assert untouched.any() and (hits > 0).sum() >= 3


def test_outputs_are_optional_and_calls_repeat(pies):
    scene = make_scene(600, 64)
    props = scene[4]
    full, bare, again, some = (loose(pies, scene) for _ in range(4))
    out = full.collide_props(props, node_prop=True)
    assert bare.collide_props(props, reaction=False) is None  # all four outputs NULL
    assert_state(bare, state(full), "no outputs")
    out2 = again.collide_props(props, node_prop=True)
    assert_state(again, state(full), "second handle")
    for a, b in zip(out, out2):
        assert same_bits(a, b)
    hits = np.zeros(64, np.uint32)  # one output alone
    arr = (pies.Prop * 64)(*props)
    assert pies.load().pies_collide_props(some._h, 64, arr, None, None, hits.ctypes.data_as(C.POINTER(C.c_uint32)), None) == pies.OK
    assert np.array_equal(hits, out[2])
    assert_state(some, state(full), "hits only")
    # a second call on the edited state is the restatement of the restatement
    pos, prev, vel = state(full)
    want = collide(pos, prev, vel, scene[2], scene[3], props)
    got = full.collide_props(props, node_prop=True)
    assert_state(full, want[:3], "second call")
    assert same_bits(got[0], want[3]) and same_bits(got[1], want[4]) and np.array_equal(got[2], want[5]) and np.array_equal(got[3], want[6])


def test_a_scene_without_nodes(pies):
    """a finalised handle without nodes: OK, and every reaction output the host hands in is zeroed (no kernel runs)"""
    empty = pies.Solver(pies.Options(solver=pies.PBD))
    props = make_props(2, 0)
    impulse, torque, hits = np.full((2, 3), 7, F), np.full((2, 3), 7, F), np.full(2, 7, np.uint32)
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = pies.load().pies_collide_props(empty._h, 2, (pies.Prop * 2)(*props), impulse.ctypes.data_as(pf), torque.ctypes.data_as(pf),
                                        hits.ctypes.data_as(pu), None)
    assert rc == pies.OK and not impulse.any() and not torque.any() and not hits.any()
    out = empty.collide_props(props, node_prop=True)
    assert all(not x.any() for x in out[:3]) and out[3].shape == (0,)


def tet_box(pies, solver, schedule=None):
    g = pies.Solver(pies.Options(solver=solver))
    if schedule is not None:
        g.set_schedule(schedule)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def corner_sphere(g, pies):
    """a moving sphere over the lattice's first node, reaching its neighbours"""
    p0 = g.positions[0].astype(np.float64)
    return [pies.Prop.sphere(p0 + [-0.25, 0.5, -0.125], 1.25, velocity=(0.5, -1.0, 0.25), angular=(0.0, 0.5, 0.0), friction=0.5)]


def write_path(g, props):
    """the route the call replaces: read, the restatement on the host, pies_write_nodes"""
    pos, prev, vel = state(g)
    want = collide(pos, prev, vel, g.radii, g.inv_masses, props)
    g.set_positions(want[0])
    g.set_prev_positions(want[1])
    g.set_velocities(want[2])
    return want


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_the_edit_reaches_the_next_substep(pies, solver, schedule):
    """collide_props on one handle, read + restatement + pies_write_nodes on the other, then one tick on both: the same bits,
    under PBD's three schedules and under PD."""
    sched = None if schedule is None else getattr(pies, "SCHEDULE_" + schedule)
    device, host = tet_box(pies, getattr(pies, solver), sched), tet_box(pies, getattr(pies, solver), sched)
    props = corner_sphere(device, pies)
    device.finalize()
    host.finalize()
    impulse, torque, hits = device.collide_props(props)
    want = write_path(host, props)
    assert 1 <= hits[0] < device.count(pies.NODES) and hits[0] == want[5][0]
    assert same_bits(impulse, want[3]) and same_bits(torque, want[4])
    assert_state(device, want[:3], "after the call")
    device.tick()
    host.tick()
    assert not device.failed and np.isfinite(device.positions).all()
    assert_state(device, state(host), "after the tick")
    assert not same_bits(device.positions, tet_box(pies, getattr(pies, solver), sched).positions)


def test_renumbered_scene_gives_the_same_bits(pies):
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES: the state in host numbering, node_prop, and the impulse and torque
    (whose order is defined on host ids) are those of the same scene with the flag off, and the restatement's."""
    mesh = shuffled_beam()
    pos = np.asarray(mesh[0], np.float64)
    n = len(pos)
    lo, hi = pos.min(0), pos.max(0)
    props = make_props(6, 3)
    rng = np.random.default_rng(17)
    for k, P in enumerate(props):  # spread along the beam: the shuffled host ids of every tile meet some of them
        P.centre[:] = [float(x) for x in (lo + (hi - lo) * [0.5, 0.5, (k + 0.5) / 6] + rng.normal(size=3) * 0.3).astype(F)]
        P.end[:] = [P.centre[0] + 1.0, P.centre[1] + 0.5, P.centre[2] + 2.0]
        P.pivot[:] = [P.centre[0] + 0.5, P.centre[1], P.centre[2] - 0.25]
        P.radius = 1.5
    vel = (rng.normal(size=(n, 3)) * 2).astype(F)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        before = state(g)
        out = g.collide_props(props, node_prop=True)
        assert g.count(pies.NODES_RENUMBERED) == flag
        got.append((state(g), out))
        if flag:
            want = collide(before[0], before[1], before[2], g.radii, g.inv_masses, props)
    (state_on, out_on), (state_off, out_off) = got
    for a, b, c in zip(state_on, state_off, want[:3]):
        assert same_bits(a, b) and same_bits(a, c)
    for a, b, c in zip(out_on, out_off, want[3:]):
        assert same_bits(a, b) and same_bits(a, c)
    touched = np.nonzero(out_on[3] != NONE)[0]
    assert (out_on[2] > 0).sum() >= 4 and len(np.unique(touched // 256)) == (n + 255) // 256 and len(touched) < n


def test_the_call_runs_behind_queued_work(pies):
    queued, plain, frames = (tet_box(pies, pies.PBD) for _ in range(3))
    props = corner_sphere(queued, pies)
    queued.tick_async(2)
    a = queued.collide_props(props)
    plain.tick(2)
    b = plain.collide_props(props)
    assert b[2][0] >= 1
    assert_state(queued, state(plain), "two queued ticks")
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # a frame begun before the call delivers the positions from before the push
    frame = frames.tick_begin()
    frames.collide_props(props, reaction=False)
    exported = frames.export_acquire(frame)[:, :3].copy()
    frames.export_release(frame)
    once = tet_box(pies, pies.PBD)
    once.tick()
    assert same_bits(exported, once.positions)
    want = collide(*state(once), once.radii, once.inv_masses, props)
    assert not same_bits(want[0], exported)
    assert_state(frames, want[:3], "behind the frame")


def test_the_substep_is_untouched(pies):
    for solver in (pies.PBD, pies.PD):
        g = tet_box(pies, solver)
        g.tick()
        before = g.launch_counts()
        out = g.collide_props(corner_sphere(g, pies))
        assert out[2][0] >= 1 and g.launch_counts() == before
