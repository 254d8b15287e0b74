"""GPU tests of the signed distance fields and field props.  The yardsticks are the numpy fp32 restatements of tests/test_fields.py:
`build_field` for pies_add_field_tri_mesh - dims, origin and the bits of |sample|; the sign goes through atan2f, which the device
and numpy need not round alike, and is compared on every sample whose fp64 winding number is not near the threshold - and
`collide_fields` for pies_collide_field_props, on the samples read back with pies_get_field: the node state, the impulse, the
torque, the hits and node_prop must be equal BIT FOR BIT."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_fields import (ALL_CASES, box_field, box_mesh, cases_of, collide_fields, crafted_field, field_lattice, host_fields,
                         lattice_points, make_field_props, make_field_scene, sphere_field)
from test_nearest import winding64
from test_node_renumber import shuffled_beam
from test_props import F, NONE
from test_props_gpu import assert_state, same_bits, state, tet_box

pytestmark = pytest.mark.gpu

NODES = (1, 63, 64, 65, 255, 256, 257, 600)  # the lane tail of a wavefront; 1, 2 and 3 tiles of the summation order
PROPS = (1, 3, 64)


@pytest.fixture(scope="module")
def built(pies):
    """the mesh-built box field, built once on the device: (samples, origin, cell) as pies_get_field returns it"""
    g = pies.Solver(pies.Options(solver=pies.PBD))
    P, tri = box_mesh()
    assert g.add_field_tri_mesh(P, tri, 0.37, 0.6) == 0
    return g.get_field(0)


def fields_of(built):
    return [built] + host_fields()


def add_fields(g, fields):
    for k, (samples, origin, cell) in enumerate(fields):
        assert g.add_field(samples, origin, float(cell)) == k


def loose(pies, scene, fields):
    pos, vel, radius, inv_mass, _ = scene
    g = pies.Solver(pies.Options(solver=pies.PBD))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=radius, invMass=inv_mass)
    add_fields(g, fields)
    return g


# ---- 1. the build --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell,margin,dims", [(0.37, 0.6, (19, 16, 13)), (0.41, 0.7, (18, 15, 12))])
def test_the_build_equals_the_restatement(pies, cell, margin, dims):
    P, tri = box_mesh()
    g = pies.Solver(pies.Options(solver=pies.PBD))
    first, second = g.add_field_tri_mesh(P, tri, cell, margin), g.add_field_tri_mesh(P, tri, cell, margin)
    assert (first, second) == (0, 1)
    samples, origin, got_cell = g.get_field(0)
    want, want_origin, want_cell, _ = box_field(cell, margin)
    assert samples.shape == dims[::-1] and field_lattice(P, cell, margin)[0] == dims
    assert same_bits(origin, want_origin) and F(got_cell) == want_cell
    assert same_bits(np.abs(samples), np.abs(want))
    w64 = winding64(lattice_points(dims, origin, cell), P, tri).reshape(samples.shape)
    clear = ~((np.abs(w64) > 0.25) & (np.abs(w64) < 0.75))
    assert (~clear).mean() <= 0.01
    assert np.array_equal(np.signbit(samples)[clear], (np.abs(w64) > 0.5)[clear])
    assert 0.05 < np.signbit(samples).mean() < 0.5
    assert same_bits(g.get_field(1)[0], samples)  # two builds agree bit for bit


# ---- 2. colliding --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_props", PROPS)
@pytest.mark.parametrize("n_nodes", NODES)
def test_bits_equal_the_restatement(pies, built, n_nodes, n_props):
    fields = fields_of(built)
    scene = make_field_scene(n_nodes, n_props, fields)
    pos, vel, radius, inv_mass, props = scene
    g = loose(pies, scene, fields)
    before = state(g)
    assert same_bits(before[0], pos) and same_bits(before[2], vel)
    trace = []
    want = collide_fields(before[0], before[1], before[2], radius, inv_mass, props, fields, trace=trace)
    impulse, torque, hits, who = g.collide_field_props(props, node_prop=True)
    assert_state(g, want[:3])
    assert same_bits(impulse, want[3]) and same_bits(torque, want[4])
    assert np.array_equal(hits, want[5]) and np.array_equal(who, want[6])
    untouched = who == NONE
    for got, was in zip(state(g), before):
        assert same_bits(got[untouched], was[untouched])
    assert not (who[inv_mass == 0] != NONE).any() and hits.sum() >= (who != NONE).sum()
    if n_nodes >= 255 and n_props >= 3:  # every case of the rule (placed by construction: make_field_scene)
        seen, most = cases_of(trace)
        assert ALL_CASES <= seen and most >= 2, (sorted(ALL_CASES - seen), most)
        assert untouched.any() and (hits > 0).sum() >= 3


# ---- 3. optional outputs -------------------------------------------------------------------------------------------------------------
def test_outputs_are_optional_and_calls_repeat(pies, built):
    fields = fields_of(built)
    scene = make_field_scene(600, 64, fields)
    props = scene[4]
    full, bare, again, some = (loose(pies, scene, fields) for _ in range(4))
    out = full.collide_field_props(props, node_prop=True)
    assert bare.collide_field_props(props, reaction=False) is None  # all four outputs NULL
    assert_state(bare, state(full), "no outputs")
    out2 = again.collide_field_props(props, node_prop=True)
    assert_state(again, state(full), "second handle")
    for a, b in zip(out, out2):
        assert same_bits(a, b)
    hits = np.zeros(64, np.uint32)  # one output alone
    arr = (pies.FieldProp * 64)(*props)
    assert pies.load().pies_collide_field_props(some._h, 64, arr, None, None, hits.ctypes.data_as(C.POINTER(C.c_uint32)), None) == pies.OK
    assert np.array_equal(hits, out[2])
    assert_state(some, state(full), "hits only")
    # a second call on the edited state is the restatement of the restatement
    pos, prev, vel = state(full)
    want = collide_fields(pos, prev, vel, scene[2], scene[3], props, fields)
    got = full.collide_field_props(props, node_prop=True)
    assert_state(full, want[:3], "second call")
    assert same_bits(got[0], want[3]) and same_bits(got[1], want[4]) and np.array_equal(got[2], want[5]) and np.array_equal(got[3], want[6])


def test_a_scene_without_nodes(pies):
    """a finalised handle without nodes: OK, and every reaction output the host hands in is zeroed (no kernel runs)"""
    empty = pies.Solver(pies.Options(solver=pies.PBD))
    add_fields(empty, host_fields())
    props = [pies.FieldProp.make(0, (0.0, 1.0, 0.0), radius=0.25), pies.FieldProp.make(1, (1.0, 0.0, 0.5), velocity=(0.5, 0.0, 0.0))]
    impulse, torque, hits = np.full((2, 3), 7, F), np.full((2, 3), 7, F), np.full(2, 7, np.uint32)
    pf, pu = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = pies.load().pies_collide_field_props(empty._h, 2, (pies.FieldProp * 2)(*props), impulse.ctypes.data_as(pf),
                                              torque.ctypes.data_as(pf), hits.ctypes.data_as(pu), None)
    assert rc == pies.OK and not impulse.any() and not torque.any() and not hits.any()
    out = empty.collide_field_props(props, node_prop=True)
    assert all(not x.any() for x in out[:3]) and out[3].shape == (0,)


# ---- 4. the edit reaches the next substep ---------------------------------------------------------------------------------------------
def corner_ball(g, pies, field=0):
    """the sampled sphere (radius 0.8, inflated to 1.25), moving, over the lattice's first node, reaching its neighbours"""
    p0 = g.positions[0].astype(np.float64)
    return [pies.FieldProp.make(field, p0 + [-0.25, 0.5, -0.125], radius=0.45, velocity=(0.5, -1.0, 0.25), angular=(0.0, 0.5, 0.0), friction=0.5)]


def write_path(g, props, fields):
    """the route the call replaces: read, the restatement on the host, pies_write_nodes"""
    pos, prev, vel = state(g)
    want = collide_fields(pos, prev, vel, g.radii, g.inv_masses, props, fields)
    g.set_positions(want[0])
    g.set_prev_positions(want[1])
    g.set_velocities(want[2])
    return want


@pytest.mark.parametrize("solver,schedule", [("PBD", "LAYERED"), ("PBD", "COLOURED"), ("PBD", "EXACT"), ("PD", None)])
def test_the_edit_reaches_the_next_substep(pies, solver, schedule):
    sched = None if schedule is None else getattr(pies, "SCHEDULE_" + schedule)
    device, host = tet_box(pies, getattr(pies, solver), sched), tet_box(pies, getattr(pies, solver), sched)
    fields = [sphere_field()]
    add_fields(device, fields)
    props = corner_ball(device, pies)
    device.finalize()
    host.finalize()
    impulse, torque, hits = device.collide_field_props(props)
    want = write_path(host, props, fields)
    assert 1 <= hits[0] < device.count(pies.NODES) and hits[0] == want[5][0]
    assert same_bits(impulse, want[3]) and same_bits(torque, want[4])
    assert_state(device, want[:3], "after the call")
    device.tick()
    host.tick()
    assert not device.failed and np.isfinite(device.positions).all()
    assert_state(device, state(host), "after the tick")
    assert not same_bits(device.positions, tet_box(pies, getattr(pies, solver), sched).positions)


# ---- 5. queued work and numbering -------------------------------------------------------------------------------------------------------
def test_renumbered_scene_gives_the_same_bits(pies, built):
    """The shuffled beam under PD with PIES_FLAG_RENUMBER_NODES: the state in host numbering, node_prop, and the impulse and torque
    (whose order is defined on host ids) are those of the same scene with the flag off, and the restatement's."""
    fields = fields_of(built)
    mesh = shuffled_beam()
    pos = np.asarray(mesh[0], np.float64)
    n = len(pos)
    lo, hi = pos.min(0), pos.max(0)
    props = make_field_props(6, fields, 3)
    rng = np.random.default_rng(17)
    for k, P in enumerate(props):  # spread along the beam: the shuffled host ids of every tile meet some of them
        samples, origin, cell = fields[P.field]
        middle = np.asarray(origin, np.float64) + 0.5 * (np.array(samples.shape[::-1]) - 1) * float(cell)
        place = lo + (hi - lo) * [0.5, 0.5, (k + 0.5) / 6] + rng.normal(size=3) * 0.3
        centre = place - np.array(list(P.axes), np.float64).reshape(3, 3).T @ middle
        P.centre[:] = [float(x) for x in centre.astype(F)]
        P.pivot[:] = [float(x) for x in (place + [0.5, 0.0, -0.25]).astype(F)]
        P.radius = 0.75
    vel = (rng.normal(size=(n, 3)) * 2).astype(F)
    got = []
    for flag in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        scenes.build_unstructured_pd(g, mesh)
        g.set_velocities(vel)
        g.set_flag(pies.FLAG_RENUMBER_NODES, flag)
        add_fields(g, fields)
        before = state(g)
        out = g.collide_field_props(props, node_prop=True)
        assert g.count(pies.NODES_RENUMBERED) == flag
        got.append((state(g), out))
        if flag:
            want = collide_fields(before[0], before[1], before[2], g.radii, g.inv_masses, props, fields)
    (state_on, out_on), (state_off, out_off) = got
    for a, b, c in zip(state_on, state_off, want[:3]):
        assert same_bits(a, b) and same_bits(a, c)
    for a, b, c in zip(out_on, out_off, want[3:]):
        assert same_bits(a, b) and same_bits(a, c)
    touched = np.nonzero(out_on[3] != NONE)[0]
    assert (out_on[2] > 0).sum() >= 4 and len(np.unique(touched // 256)) == (n + 255) // 256 and len(touched) < n


def test_the_call_runs_behind_queued_work(pies):
    fields = [sphere_field()]
    queued, plain, frames, once = (tet_box(pies, pies.PBD) for _ in range(4))
    for g in (queued, plain, frames):
        add_fields(g, fields)
    props = corner_ball(queued, pies)
    queued.tick_async(2)
    a = queued.collide_field_props(props)
    plain.tick(2)
    b = plain.collide_field_props(props)
    assert b[2][0] >= 1
    assert_state(queued, state(plain), "two queued ticks")
    for x, y in zip(a, b):
        assert same_bits(x, y)
    # a frame begun before the call delivers the positions from before the push
    frame = frames.tick_begin()
    frames.collide_field_props(props, reaction=False)
    exported = frames.export_acquire(frame)[:, :3].copy()
    frames.export_release(frame)
    once.tick()
    assert same_bits(exported, once.positions)
    want = collide_fields(*state(once), once.radii, once.inv_masses, props, fields)
    assert not same_bits(want[0], exported)
    assert_state(frames, want[:3], "behind the frame")


# ---- 6. the substep is untouched ------------------------------------------------------------------------------------------------------
def test_the_substep_is_untouched(pies):
    for solver in (pies.PBD, pies.PD):
        g, twin = tet_box(pies, solver), tet_box(pies, solver)
        add_fields(g, [sphere_field()])
        g.tick()
        twin.tick()
        before = g.launch_counts()
        hit = g.collide_field_props(corner_ball(g, pies))
        assert hit[2][0] >= 1 and g.launch_counts() == before
        g2 = tet_box(pies, solver)
        add_fields(g2, [sphere_field()])
        g2.tick()
        far = pies.FieldProp.make(0, (100.0, 100.0, 100.0), radius=0.5)
        miss = g2.collide_field_props([far], node_prop=True)
        assert miss[2][0] == 0 and (miss[3] == NONE).all() and not miss[0].any() and g2.launch_counts() == before
        g2.tick()
        twin.tick()
        assert_state(g2, state(twin), "a tick after a call that touched nothing")


# ---- 7. lifetime on a live handle ------------------------------------------------------------------------------------------------------
def test_a_field_survives_finalize_and_an_appended_body(pies, built):
    P, tri = box_mesh()
    g, fresh = tet_box(pies, pies.PBD), tet_box(pies, pies.PBD)
    assert g.add_field_tri_mesh(P, tri, 0.37, 0.6) == 0 and g.add_field(*sphere_field()) == 1
    g.finalize()  # drops the device copies: the host copies are staged again at the next use
    g.create_tet_box(2, 2, 2, translation=(6.0, 1.5, 0.5))
    g.tick()
    assert same_bits(g.get_field(0)[0], built[0])
    fresh.create_tet_box(2, 2, 2, translation=(6.0, 1.5, 0.5))
    fresh.tick()
    fields = [built, sphere_field()]
    p0 = g.positions[0].astype(np.float64)
    middle = np.asarray(built[1], np.float64) + 0.5 * (np.array(built[0].shape[::-1]) - 1) * float(built[2])
    props = [pies.FieldProp.make(0, p0 - middle, radius=0.25, velocity=(0.0, 1.0, 0.0), friction=0.25), corner_ball(g, pies, field=1)[0]]
    want = collide_fields(*state(fresh), fresh.radii, fresh.inv_masses, props, fields)
    got = g.collide_field_props(props)
    assert got[2][0] >= 1 and got[2][1] >= 1 and np.array_equal(got[2], want[5])
    assert_state(g, want[:3], "after finalize and an appended body")
    assert same_bits(got[0], want[3]) and same_bits(got[1], want[4])
    g.clear()
    with pytest.raises(pies.PiesError):
        g.get_field(0)
    g.create_tet_box(2, 2, 2, translation=(0.0, 1.5, 0.0))
    arr = (pies.FieldProp * 1)(props[0])
    assert pies.load().pies_collide_field_props(g._h, 1, arr, None, None, None, None) == pies.ERR_INVALID
    assert g.add_field(*crafted_field()) == 0
