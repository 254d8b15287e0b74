"""GPU tests of pies_apply_surface_loads.  The yardstick is the numpy fp32 restatement of the rule (tests/test_loads.py:
apply_surface_loads): the velocities read back after the call, the impulse, the torque, the node counts, the volumes and the areas
must be equal BIT FOR BIT - the rule uses only fp32 + - x / sqrt and comparisons, which the device and numpy round alike, and the
sums have one stated order - and positions and previous positions must be the bits they were."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_forces import apply_forces, make_forces
from test_loads import (DT, HUB_FAN, LOADS, N_FIXED, N_HIT, N_OUT, RANGES, T_ABOVE, T_DEGENERATE, T_IDLE, T_IN, TO_END, F, affected_of,
                        apply_surface_loads, branches_of, shared_scene, single_triangle, small_cube, two_bodies)
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def loose(pies, pos, vel, inv_mass, triangles=None):
    g = pies.Solver(pies.Options(solver=pies.PBD))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=np.full(len(pos), 0.05, F), invMass=inv_mass)
    if triangles is not None and len(triangles):
        g.add_triangles(triangles)
    return g


def state(g):
    return g.positions, g.prev_positions, g.velocities


def assert_call(g, loads, dt, want, before, what=""):
    """one call with every output against `want` = apply_surface_loads(...) of the state `before`"""
    got = g.apply_surface_loads(loads, dt)
    pos, prev, vel = state(g)
    assert same_bits(pos, before[0]) and same_bits(prev, before[1]), (what, "positions changed")
    assert same_bits(vel, want[0]), (what, "velocities", int((vel.view(np.uint32) != want[0].view(np.uint32)).any(axis=1).sum()))
    assert same_bits(got[3], want[4]) and same_bits(got[4], want[5]), (what, "volume, area", got[3], want[4], got[4], want[5])
    assert same_bits(got[0], want[1]) and same_bits(got[1], want[2]), (what, "sums")
    assert np.array_equal(got[2], want[3]), (what, got[2], want[3])
    return got


def check_case(pies, case, what=""):
    pos, vel, inv_mass, tris, loads = case
    g = loose(pies, pos, vel, inv_mass, tris)
    before = state(g)
    assert same_bits(before[0], pos) and same_bits(before[2], vel)
    trace = []
    want = apply_surface_loads(before[0], before[2], inv_mass, tris, loads, DT, trace=trace)
    got = assert_call(g, loads, DT, want, before, what)
    untouched = ~affected_of(trace, len(pos)).any(axis=0)
    assert same_bits(g.velocities[untouched], vel[untouched]) and untouched[inv_mass == 0].all()
    return g, want, got, trace


def test_single_triangle(pies):
    g, want, got, trace = check_case(pies, single_triangle())
    assert got[2].tolist() == [3] and np.abs(got[0]).max() > 0 and got[3][0] == 0 and got[4][0] > 0  # (one triangle about its own corner)
    # a scene without triangles: zeros, and nothing moves
    pos, vel, inv_mass, tris, loads = single_triangle()
    bare = loose(pies, pos, vel, inv_mass)
    free = [pies.SurfaceLoad.pressure(2.0, first=0, count=0)]
    out = bare.apply_surface_loads(free, DT)
    assert all(not np.asarray(x).any() for x in out) and same_bits(bare.velocities, vel)
    empty = pies.Solver(pies.Options(solver=pies.PBD))  # ... and one without nodes
    assert all(not np.asarray(x).any() for x in empty.apply_surface_loads(free, DT))


def test_the_12_triangle_cube(pies):
    g, want, got, trace = check_case(pies, small_cube())
    assert got[3][0] == F(1) and got[4][0] == F(6) and got[2].tolist() == [8, 8, 8]


def test_two_bodies_and_overlapping_ranges(pies):
    g, want, got, trace = check_case(pies, two_bodies())
    assert abs(got[3][0] - 1.0) < 1e-5 and abs(got[3][1] - 1.25 ** 3) < 1e-5 and (got[2] > 0).all()
    hit = affected_of(trace, len(g.positions))
    assert not (hit[0] & hit[1]).any() and (hit[2] & hit[3]).any() and (hit[2] & hit[0]).any() and (hit[2] & hit[1]).any()


@pytest.mark.parametrize("n_loads", LOADS)
@pytest.mark.parametrize("n_range", RANGES)
def test_bits_equal_the_restatement(pies, n_range, n_loads):
    pos, vel, inv_mass, tris, loads, marks = shared_scene(n_range, n_loads)
    g, want, got, trace = check_case(pies, (pos, vel, inv_mass, tris, loads), (n_range, n_loads))
    assert loads[0].count == n_range and not same_bits(g.velocities, vel)
    _, node_codes, tri_codes, _ = trace[0]  # a fluid with drag on body A's first n_range triangles: the surface cuts the body
    assert (tri_codes == T_IN).any() and (tri_codes == T_ABOVE).any() and node_codes[marks["pinned"]] == N_FIXED
    if n_range >= 257 and n_loads == 64:  # every branch: three loads do not hold every (type, range, flag) setting
        assert branches_of(trace) == ({T_DEGENERATE, T_ABOVE, T_IN, T_IDLE}, {N_OUT, N_FIXED, N_HIT})
        gases = {bool(L.flags): t for L, t in zip(loads, trace) if L.type == pies.LOAD_GAS and (L.first, L.count) == marks["B"]}
        assert set(np.unique(gases[False][2])) == {T_IDLE} and set(np.unique(gases[True][2])) == {T_IN}  # V <= 0, and PIES_LOAD_INWARD
        assert got[3][gases[False][0]] < 0 < got[3][gases[True][0]]
        assert (tris == marks["hub"]).sum() == HUB_FAN and any(t[1][marks["hub"]] == N_HIT for t in trace)  # the hub's 40-entry row
        assert any(L.count == TO_END and L.first == 100 for L in loads) and any(L.count == 0 for L in loads)
        assert any(L.type == pies.LOAD_FLUID and L.drag == 0 for L in loads)


def test_outputs_are_optional_and_calls_repeat(pies, tune):
    pos, vel, inv_mass, tris, loads, marks = shared_scene(513, 64)
    calm = [L for L in loads if not (L.type == pies.LOAD_FLUID and L.drag != 0)]  # a list without drag: either route
    full, bare, again, some, other = (loose(pies, pos, vel, inv_mass, tris) for _ in range(5))
    out = full.apply_surface_loads(loads, DT)
    assert bare.apply_surface_loads(loads, DT, reaction=False) is None  # every output NULL
    assert same_bits(bare.velocities, full.velocities)
    out2 = again.apply_surface_loads(loads, DT)  # two handles, the same bits
    assert same_bits(again.velocities, full.velocities)
    for a, b in zip(out, out2):
        assert same_bits(a, b)
    # each output alone through the raw ABI
    arr = (pies.SurfaceLoad * 64)(*loads)
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    shapes = [((64, 3), F), ((64, 3), F), ((64,), np.uint32), ((64,), F), ((64,), F)]
    for which, (shape, dtype) in enumerate(shapes):
        g = loose(pies, pos, vel, inv_mass, tris)
        buf = np.zeros(shape, dtype)
        args = [None] * 5
        args[which] = buf.ctypes.data_as(pu if dtype is np.uint32 else pf)
        assert pies.load().pies_apply_surface_loads(g._h, 64, arr, DT, *args) == pies.OK
        assert same_bits(buf, out[which]) and same_bits(g.velocities, full.velocities), which
    torque = np.zeros((64, 3), F)
    assert pies.load().pies_apply_surface_loads(some._h, 0, None, DT, None, torque.ctypes.data_as(pf), None, None, None) == pies.OK
    assert same_bits(some.velocities, vel)  # no load: nothing happens
    # a second call on the edited state is the restatement of the restatement
    before = state(full)
    want = apply_surface_loads(before[0], before[2], inv_mass, tris, loads, DT)
    assert_call(full, loads, DT, want, before, "second call")
    # both routes of a list without drag give the same bits
    reference = other.apply_surface_loads(calm, DT)
    for variant in ("scratch", "inplace"):
        tune("PIES_LOAD_VARIANT", variant)
        g = loose(pies, pos, vel, inv_mass, tris)
        got = g.apply_surface_loads(calm, DT)
        assert same_bits(g.velocities, other.velocities), variant
        for a, b in zip(got, reference):
            assert same_bits(a, b), variant
        quiet = loose(pies, pos, vel, inv_mass, tris)
        assert quiet.apply_surface_loads(calm, DT, reaction=False) is None and same_bits(quiet.velocities, other.velocities), variant
    want = apply_surface_loads(pos, vel, inv_mass, tris, calm, DT)
    assert same_bits(other.velocities, want[0]) and same_bits(reference[0], want[1])
    tune("PIES_LOAD_VARIANT", "sideways")
    with pytest.raises(pies.PiesError):
        loose(pies, pos, vel, inv_mass, tris).apply_surface_loads(calm, DT)
    # ... and a list with drag takes the scratch array whatever the switch says
    tune("PIES_LOAD_VARIANT", "inplace")
    g = loose(pies, pos, vel, inv_mass, tris)
    before = state(g)
    assert_call(g, loads, DT, apply_surface_loads(before[0], before[2], inv_mass, tris, loads, DT), before, "drag, inplace asked")


def tet_box(pies, solver, schedule=None):
    g = pies.Solver(pies.Options(solver=solver))
    if schedule is not None:
        g.set_schedule(schedule)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def box_loads(pies, height=2.0):
    """a gas in the box and a fluid with drag whose surface cuts it (height: a level within the body as it stands)"""
    return [pies.SurfaceLoad.gas(1.5, 40.0, about=(0.5, 2.0, 0.75)),
            pies.SurfaceLoad.fluid(9.8125, (0.0, float(height) + 1.0 / 256, 0.0), up=(0.0625, 1.0, 0.03125)).with_drag(0.5, (0.5, 0.0, 0.0))]


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_the_edit_reaches_the_next_substep(pies, solver, schedule):
    """apply_surface_loads on one handle, read + restatement + pies_write_nodes(velocities) on the other, then one tick on both:
    the same bits, under PBD's three schedules and under PD."""
    sched = None if schedule is None else getattr(pies, "SCHEDULE_" + schedule)
    device, host = tet_box(pies, getattr(pies, solver), sched), tet_box(pies, getattr(pies, solver), sched)
    device.finalize()
    host.finalize()
    before = state(host)
    loads = box_loads(pies, before[0][:, 1].mean())
    tris = host.ids(pies.TRIANGLES)
    assert len(tris) > 0
    want = apply_surface_loads(before[0], before[2], host.inv_masses, tris, loads, DT)
    assert want[3][0] > want[3][1] >= 1 and want[4][0] != 0
    assert_call(device, loads, DT, want, before, "after the call")
    host.set_velocities(want[0])
    device.tick()
    host.tick()
    assert not device.failed and np.isfinite(device.positions).all()
    for a, b in zip(state(device), state(host)):
        assert same_bits(a, b)
    calm = tet_box(pies, getattr(pies, solver), sched)
    calm.tick()
    assert not same_bits(device.positions, calm.positions)


def test_renumbered_scene_gives_the_same_bits(pies):
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES: the velocities in host numbering and every output (whose orders
    are defined on host ids and container indices) are those of the same scene with the flag off, and the restatement's."""
    mesh = shuffled_beam()
    pos = np.asarray(mesh[0], np.float64)
    n = len(pos)
    mid = (pos.min(0) + pos.max(0)) / 2
    level = float(np.round(mid[1] * 16) / 16) + 1.0 / 512
    loads = [pies.SurfaceLoad.gas(2.0, 1.0, about=np.round(mid * 16) / 16), pies.SurfaceLoad.pressure(-0.75, first=100, count=700),
             pies.SurfaceLoad.fluid(9.8125, (0.0, level, 0.0), up=(0.0625, 1.0, 0.03125)).with_drag(0.75, (0.0, 0.0, 1.0))]
    vel = (np.random.default_rng(17).normal(size=(n, 3)) * 2).astype(F)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        before = state(g)
        out = g.apply_surface_loads(loads, DT)
        assert g.count(pies.NODES_RENUMBERED) == flag
        after = state(g)
        assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])
        got.append((after[2], out))
        if flag:
            trace = []
            want = apply_surface_loads(before[0], before[2], g.inv_masses, g.ids(pies.TRIANGLES), loads, DT, trace=trace)
    (vel_on, out_on), (vel_off, out_off) = got
    assert same_bits(vel_on, vel_off) and same_bits(vel_on, want[0])
    for a, b, c in zip(out_on, out_off, (want[1], want[2], want[3], want[4], want[5])):
        assert same_bits(a, b) and same_bits(a, c)
    cut = trace[2][2]
    assert (cut == T_IN).any() and (cut == T_ABOVE).any() and (out_on[2] > 0).all() and n > 3 * 256 and out_on[3][0] != 0


def test_the_call_runs_behind_queued_work(pies):
    queued, plain, frames = (tet_box(pies, pies.PBD) for _ in range(3))
    plain.tick(2)
    loads = box_loads(pies, plain.positions[:, 1].mean())  # (two PBD ticks move this box a long way)
    queued.tick_async(2)
    a = queued.apply_surface_loads(loads, DT)
    b = plain.apply_surface_loads(loads, DT)
    assert 1 <= b[2][1] < b[2][0]
    for x, y in zip(state(queued), state(plain)):
        assert same_bits(x, y)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # a frame begun before the call delivers that frame's positions, and the call edits the velocities behind it
    frame = frames.tick_begin()
    once = tet_box(pies, pies.PBD)
    once.tick()
    loads = box_loads(pies, once.positions[:, 1].mean())
    frames.apply_surface_loads(loads, DT, reaction=False)
    exported = frames.export_acquire(frame)[:, :3].copy()
    frames.export_release(frame)
    assert same_bits(exported, once.positions)
    before = state(once)
    want = apply_surface_loads(before[0], before[2], once.inv_masses, once.ids(pies.TRIANGLES), loads, DT)
    assert same_bits(frames.velocities, want[0]) and same_bits(frames.positions, before[0]) and not same_bits(want[0], before[2])


def test_appended_triangles_reach_the_loads(pies):
    pos, vel, inv_mass, tris, loads, marks = shared_scene(257, 3)
    fan_first = marks["fan"][0]
    g = loose(pies, pos, vel, inv_mass, tris[:fan_first])
    everything = [pies.SurfaceLoad.pressure(1.25), pies.SurfaceLoad.fluid(9.8125, marks["surface"], up=(0.125, 1.0, -0.0625)).with_drag(0.5)]
    before = state(g)
    first = assert_call(g, everything, DT, apply_surface_loads(before[0], before[2], inv_mass, tris[:fan_first], everything, DT), before, "without the cone")
    assert same_bits(g.velocities[marks["hub"]], vel[marks["hub"]])
    g.add_triangles(tris[fan_first:])  # the cone and the zero-area triangle: the incidence is built again
    before = state(g)
    second = assert_call(g, everything, DT, apply_surface_loads(before[0], before[2], inv_mass, tris, everything, DT), before, "with the cone")
    assert second[2][0] == first[2][0] + HUB_FAN + 1 and not same_bits(g.velocities[marks["hub"]], vel[marks["hub"]])
    assert second[4][0] > first[4][0]


def test_the_substep_and_the_forces_are_untouched(pies):
    for solver in (pies.PBD, pies.PD):
        g = tet_box(pies, solver)
        g.tick()
        before = g.launch_counts()
        out = g.apply_surface_loads(box_loads(pies, g.positions[:, 1].mean()), DT)
        assert out[2][0] >= 1 and g.launch_counts() == before
        g.tick()
        assert not g.failed
    # pies_apply_forces before and after a call gives the bits it gave without the call in between (the scratch array is shared)
    pos, vel, inv_mass, tris, loads, marks = shared_scene(257, 3)
    forces = make_forces(3) + [pies.Force.wind((3.0, -1.0, 0.5), 1.5, shear=0.5)]
    with_loads, without = loose(pies, pos, vel, inv_mass, tris), loose(pies, pos, vel, inv_mass, tris)
    first = [g.apply_forces(forces, DT) for g in (with_loads, without)]
    mid = state(with_loads)
    with_loads.apply_surface_loads(loads, DT)
    after_loads = apply_surface_loads(mid[0], mid[2], inv_mass, tris, loads, DT)[0]
    assert same_bits(with_loads.velocities, after_loads)
    without.set_velocities(after_loads)
    second = [g.apply_forces(forces, DT) for g in (with_loads, without)]
    for a, b in zip(first[0] + second[0], first[1] + second[1]):
        assert same_bits(a, b)
    assert same_bits(with_loads.velocities, without.velocities)
    want = apply_forces(mid[0], after_loads, inv_mass, forces, DT, tris)
    assert same_bits(with_loads.velocities, want[0])
