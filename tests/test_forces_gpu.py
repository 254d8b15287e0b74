"""GPU tests of pies_apply_forces.  The yardstick is the numpy fp32 restatement of the rule (tests/test_forces.py: apply_forces):
the velocities read back after the call, the impulse, the torque and the node counts must be equal BIT FOR BIT - the rule uses
only fp32 + - x / sqrt, fmin and comparisons, which the device and numpy round alike, and the sums have one stated order - and
positions and previous positions must be the bits they were."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_forces import (B_DD0, B_FIXED, B_HIT, B_OUT, DT, HUB_FAN, T_DEGENERATE, T_IN, T_OUT, F, affected_of, apply_forces,
                         branches_of, make_cloth, make_forces, make_scene, required_branches, single_triangle)
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu

NODES = (1, 63, 65, 255, 257, 600)  # the lane tail of a wavefront; 1, 2 and 3 tiles of the summation order
FORCES = (1, 3, 64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def loose(pies, pos, vel, inv_mass, triangles=None):
    g = pies.Solver(pies.Options(solver=pies.PBD))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=np.full(len(pos), 0.05, F), invMass=inv_mass)
    if triangles is not None:
        g.add_triangles(triangles)
    return g


def state(g):
    return g.positions, g.prev_positions, g.velocities


def assert_call(g, forces, dt, want, before, what=""):
    """one call with the reaction against `want` = apply_forces(...) of the state `before`"""
    impulse, torque, nodes = g.apply_forces(forces, dt)
    pos, prev, vel = state(g)
    assert same_bits(pos, before[0]) and same_bits(prev, before[1]), (what, "positions changed")
    assert same_bits(vel, want[0]), (what, "velocities", int((vel.view(np.uint32) != want[0].view(np.uint32)).any(axis=1).sum()))
    assert same_bits(impulse, want[1]) and same_bits(torque, want[2]), (what, "sums")
    assert np.array_equal(nodes, want[3]), (what, nodes, want[3])
    return impulse, torque, nodes


@pytest.mark.parametrize("n_forces", FORCES)
@pytest.mark.parametrize("n_nodes", NODES)
def test_bits_equal_the_restatement(pies, n_nodes, n_forces):
    pos, vel, inv_mass, forces = make_scene(n_nodes, n_forces)
    g = loose(pies, pos, vel, inv_mass)
    before = state(g)
    assert same_bits(before[0], pos) and same_bits(before[2], vel)
    trace = []
    want = apply_forces(before[0], before[2], inv_mass, forces, DT, trace=trace)
    assert_call(g, forces, DT, want, before)
    untouched = ~affected_of(trace, n_nodes).any(axis=0)
    assert same_bits(g.velocities[untouched], vel[untouched]) and untouched[inv_mass == 0].all()
    if n_nodes >= 255 and n_forces >= 3:  # every branch the list can reach (four point types do not fit into three forces)
        assert branches_of(trace) == required_branches(n_forces)
        assert {B_OUT, B_FIXED, B_DD0} <= branches_of(trace) and (want[3] > 0).all() and untouched.any()
        assert not same_bits(g.velocities, vel)


def cloth(pies):
    pos, vel, inv_mass, tris, forces, marks = make_cloth()
    return loose(pies, pos, vel, inv_mass, tris), (pos, vel, inv_mass, tris, forces, marks)


def test_cloth_in_two_winds_and_a_drag(pies):
    g, (pos, vel, inv_mass, tris, forces, marks) = cloth(pies)
    before = state(g)
    trace = []
    want = apply_forces(before[0], before[2], inv_mass, forces, DT, tris, trace=trace)
    assert_call(g, forces, DT, want, before)
    (_, cut_nodes, cut_tris), (_, all_nodes, all_tris), _ = trace
    assert (tris == marks["hub"]).sum() == HUB_FAN and all_nodes[marks["hub"]] >= B_HIT  # the hub's 40-entry row
    assert cut_tris[marks["degenerate"]] == T_DEGENERATE and all_tris[marks["degenerate"]] == T_DEGENERATE
    assert all_nodes[marks["pinned"]] == B_FIXED and same_bits(g.velocities[marks["pinned"]], vel[marks["pinned"]])
    assert (cut_tris == T_IN).any() and (cut_tris == T_OUT).any() and (all_nodes[marks["loose"]] == B_OUT).all()
    # the winds alone and in the other order: the per-force sums are the same bits, each force reads the state the call found
    other = loose(pies, pos, vel, inv_mass, tris)
    got = other.apply_forces(forces[::-1], DT)
    for a, b in zip(got, want[1:]):
        assert same_bits(a, b[::-1])


def test_single_triangle(pies):
    pos, vel, inv_mass, tris, forces = single_triangle()
    g = loose(pies, pos, vel, inv_mass, tris)
    before = state(g)
    want = apply_forces(before[0], before[2], inv_mass, forces, DT, tris)
    out = assert_call(g, forces, DT, want, before)
    assert out[2].tolist() == [3] and np.abs(out[0]).max() > 0
    # a wind in a scene without triangles affects nothing
    bare = loose(pies, pos, vel, inv_mass)
    out = bare.apply_forces(forces, DT)
    assert out[2].tolist() == [0] and not out[0].any() and same_bits(bare.velocities, vel)


def test_a_scene_without_nodes(pies):
    """a finalised handle without nodes: OK, and every reaction output the host hands in is zeroed (no kernel runs)"""
    empty = pies.Solver(pies.Options(solver=pies.PBD))
    forces = [pies.Force.radial((0.0, 1.0, 0.0), 2.0), pies.Force.directional((0.0, 0.0, 3.0))]
    impulse, torque, nodes = np.full((2, 3), 7, F), np.full((2, 3), 7, F), np.full(2, 7, np.uint32)
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = pies.load().pies_apply_forces(empty._h, 2, (pies.Force * 2)(*forces), DT, impulse.ctypes.data_as(pf), torque.ctypes.data_as(pf),
                                       nodes.ctypes.data_as(pu))
    assert rc == pies.OK and not impulse.any() and not torque.any() and not nodes.any()
    assert all(not x.any() for x in empty.apply_forces(forces, DT))


def test_outputs_are_optional_and_calls_repeat(pies, tune):
    pos, vel, inv_mass, forces = make_scene(600, 64)
    full, bare, again, some = (loose(pies, pos, vel, inv_mass) for _ in range(4))
    out = full.apply_forces(forces, DT)
    assert bare.apply_forces(forces, DT, reaction=False) is None  # all three outputs NULL
    assert same_bits(bare.velocities, full.velocities)
    out2 = again.apply_forces(forces, DT)
    assert same_bits(again.velocities, full.velocities)
    for a, b in zip(out, out2):
        assert same_bits(a, b)
    nodes = np.zeros(64, np.uint32)  # one output alone
    arr = (pies.Force * 64)(*forces)
    assert pies.load().pies_apply_forces(some._h, 64, arr, DT, None, None, nodes.ctypes.data_as(C.POINTER(C.c_uint32))) == pies.OK
    assert np.array_equal(nodes, out[2]) and same_bits(some.velocities, full.velocities)
    torque = np.zeros((64, 3), F)
    assert pies.load().pies_apply_forces(some._h, 0, None, DT, None, torque.ctypes.data_as(C.POINTER(C.c_float)), None) == pies.OK
    assert same_bits(some.velocities, full.velocities)  # no force: nothing happens
    # a second call on the edited state is the restatement of the restatement
    before = state(full)
    want = apply_forces(before[0], before[2], inv_mass, forces, DT)
    assert_call(full, forces, DT, want, before, "second call")
    # both variants of a list without a wind give the same bits
    for variant in ("scratch", "inplace"):
        tune("PIES_FORCE_VARIANT", variant)
        g = loose(pies, pos, vel, inv_mass)
        got = g.apply_forces(forces, DT)
        assert same_bits(g.velocities, again.velocities), variant
        for a, b in zip(got, out):
            assert same_bits(a, b), variant
        quiet = loose(pies, pos, vel, inv_mass)
        assert quiet.apply_forces(forces, DT, reaction=False) is None and same_bits(quiet.velocities, again.velocities), variant
    tune("PIES_FORCE_VARIANT", "sideways")
    with pytest.raises(pies.PiesError):
        loose(pies, pos, vel, inv_mass).apply_forces(forces, DT)
    # ... and a list with a wind takes the scratch array whatever the switch says
    tune("PIES_FORCE_VARIANT", "inplace")
    g, (cpos, cvel, cw, tris, cforces, _) = cloth(pies)
    before = state(g)
    assert_call(g, cforces, DT, apply_forces(before[0], before[2], cw, cforces, DT, tris), before, "wind, inplace asked")


def tet_box(pies, solver, schedule=None):
    g = pies.Solver(pies.Options(solver=solver))
    if schedule is not None:
        g.set_schedule(schedule)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def box_forces(pies, around=(0.5, 2.0, 0.75)):
    """a push in a sphere that holds a part of the box (around: a point of the body as it stands) and a wind everywhere"""
    return [pies.Force.directional((1.5, 0.0, -0.5)).within(around, 1.3125, pies.FALLOFF_SMOOTH),
            pies.Force.wind((0.0, 2.0, 6.0), 1.25, shear=0.25)]


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_the_edit_reaches_the_next_substep(pies, solver, schedule):
    """apply_forces on one handle, read + restatement + pies_write_nodes(velocities) on the other, then one tick on both: the same
    bits, under PBD's three schedules and under PD."""
    sched = None if schedule is None else getattr(pies, "SCHEDULE_" + schedule)
    device, host = tet_box(pies, getattr(pies, solver), sched), tet_box(pies, getattr(pies, solver), sched)
    forces = box_forces(pies)
    device.finalize()
    host.finalize()
    before = state(host)
    tris = host.ids(pies.TRIANGLES)
    assert len(tris) > 0
    want = apply_forces(before[0], before[2], host.inv_masses, forces, DT, tris)
    assert 1 <= want[3][0] < device.count(pies.NODES) and want[3][1] > want[3][0]
    assert_call(device, forces, DT, want, before, "after the call")
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
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES: the velocities in host numbering and the impulse, torque and counts
    (whose order is defined on host ids) are those of the same scene with the flag off, and the restatement's."""
    mesh = shuffled_beam()
    pos = np.asarray(mesh[0], np.float64)
    n = len(pos)
    lo, hi = pos.min(0), pos.max(0)
    mid = (lo + hi) / 2
    forces = make_forces(6, 3)
    for k, f in enumerate(forces):  # spread along the beam
        centre = np.round((lo + (hi - lo) * [0.5, 0.5, (k + 0.5) / 6]) * 16) / 16
        f.within(centre, float("inf") if k == 4 else 4.03125, f.falloff)
    forces += [pies.Force.wind((3.0, -1.0, 0.5), 1.5, shear=0.5),
               pies.Force.wind((0.0, 2.0, 0.0), 0.75).within(np.round(mid * 16) / 16 + [0.0, 0.0, 3.0], 9.03125, pies.FALLOFF_LINEAR)]
    vel = (np.random.default_rng(17).normal(size=(n, 3)) * 2).astype(F)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        before = state(g)
        out = g.apply_forces(forces, DT)
        assert g.count(pies.NODES_RENUMBERED) == flag
        after = state(g)
        assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])
        got.append((after[2], out))
        if flag:
            trace = []
            want = apply_forces(before[0], before[2], g.inv_masses, forces, DT, g.ids(pies.TRIANGLES), trace=trace)
    (vel_on, out_on), (vel_off, out_off) = got
    assert same_bits(vel_on, vel_off) and same_bits(vel_on, want[0])
    for a, b, c in zip(out_on, out_off, want[1:]):
        assert same_bits(a, b) and same_bits(a, c)
    cut = trace[7][2]
    assert (cut == T_IN).any() and (cut == T_OUT).any() and (out_on[2] > 0).all() and n > 3 * 256


def test_the_call_runs_behind_queued_work(pies):
    queued, plain, frames = (tet_box(pies, pies.PBD) for _ in range(3))
    plain.tick(2)
    forces = box_forces(pies, plain.positions[0])  # (two PBD ticks move this box a long way)
    queued.tick_async(2)
    a = queued.apply_forces(forces, DT)
    b = plain.apply_forces(forces, DT)
    assert 1 <= b[2][0] < b[2][1]
    for x, y in zip(state(queued), state(plain)):
        assert same_bits(x, y)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # a frame begun before the call delivers that frame's positions, and the call edits the velocities behind it
    frame = frames.tick_begin()
    forces = box_forces(pies)
    frames.apply_forces(forces, DT, reaction=False)
    exported = frames.export_acquire(frame)[:, :3].copy()
    frames.export_release(frame)
    once = tet_box(pies, pies.PBD)
    once.tick()
    assert same_bits(exported, once.positions)
    before = state(once)
    want = apply_forces(before[0], before[2], once.inv_masses, forces, DT, once.ids(pies.TRIANGLES))
    assert same_bits(frames.velocities, want[0]) and same_bits(frames.positions, before[0]) and not same_bits(want[0], before[2])


def test_appended_triangles_reach_the_wind(pies):
    pos, vel, inv_mass, tris, forces, marks = make_cloth()
    fan_first = marks["degenerate"] - HUB_FAN
    g = loose(pies, pos, vel, inv_mass, tris[:fan_first])
    wind = forces[1:2]  # everywhere
    before = state(g)
    first = assert_call(g, wind, DT, apply_forces(before[0], before[2], inv_mass, wind, DT, tris[:fan_first]), before, "the grid alone")
    assert first[2].tolist() == [marks["grid"] - 1] and same_bits(g.velocities[marks["hub"]], vel[marks["hub"]])
    g.add_triangles(tris[fan_first:])  # the fan and the degenerate triangle: the incidence is built again
    before = state(g)
    second = assert_call(g, wind, DT, apply_forces(before[0], before[2], inv_mass, wind, DT, tris), before, "with the fan")
    assert second[2].tolist() == [marks["grid"] - 1 + 1 + HUB_FAN] and not same_bits(g.velocities[marks["hub"]], vel[marks["hub"]])


def test_the_substep_is_untouched(pies):
    for solver in (pies.PBD, pies.PD):
        g = tet_box(pies, solver)
        g.tick()
        before = g.launch_counts()
        out = g.apply_forces(box_forces(pies, g.positions[0]), DT)
        assert out[2][0] >= 1 and g.launch_counts() == before
        g.tick()
        assert not g.failed
