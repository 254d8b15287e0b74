"""GPU tests of pies_drive_actuators / pies_drive_actuators_device.  The device against the numpy restatement of the rule
(tests/test_actuators.py) bit for bit; a driven handle against the rebuild path - pies_set_rest with the restatement's rests - and
against the oracle given the same rests, through tests/live_edits.py's comparison as test_live_edits_gpu.py uses it; the closed
loop; rebuilds behind a drive; a renumbered scene; the device-pointer form (tests/device_buffers.py, and the torch bridge in a child
process, tests/actuators_child.py); optional outputs, repeats, launch counts and the resource ledger."""
import ctypes as C
import gc
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from device_buffers import DevBuf, Hip
from live_edits import NODE_ARRAYS, any_bit_differs, put_state, same_bits, state_of
from test_actuators import B_NOT_LIVE, F, U, bits, containers, drive_actuators, lattice_and_sheet, random_set
from test_live_edits_gpu import Case
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "actuators_child.py")


@pytest.fixture(scope="module")
def hip():
    return Hip()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def body(pies, schedule="LAYERED", copies=1):
    """the lattice and the sheet of tests/test_actuators.py on a device handle (copies=2: 472 constraints, for sets of two tiles)"""
    g = pies.Solver(scenes.pbd_options(pies, 4))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.set_schedule(getattr(pies, "SCHEDULE_" + schedule))
    lattice_and_sheet(g, copies=copies)
    return g


def add_random_set(g, seed, n, channels, bends=None):
    ids, rest = containers(g)
    k = g.add_actuators(random_set(np.random.default_rng(seed), {t: len(r) for t, r in rest.items()}, n, channels, bends), channels)
    return k, g.get_actuators(k)[0]


def activations(seed, channels, first=1.4):
    a = np.random.default_rng(seed).uniform(-1.5, 1.5, channels).astype(F)
    a[0] = first
    return a


def check_against_restatement(g, k, acts, activation, before=None):
    """one host-pointer drive of set k against the restatement on the state and the rest data the call finds"""
    ids, rest = containers(g)
    state = state_of(g) if before is None else before
    want_rest, want_per, want_sums, want_live = drive_actuators(state["positions"], ids, rest, acts, activation)
    sums, live, per = g.drive_actuators(k, activation, per_actuator=True)
    assert same(per, want_per), float(np.abs(per - want_per).max())
    assert same(sums, want_sums), (sums, want_sums)
    assert np.array_equal(live, want_live)
    for t in rest:
        assert same(g.rest(t), want_rest[t])  # (constraints outside the set keep their bits: the restatement copies them)
    for name in NODE_ARRAYS:
        assert same(getattr(g, name), state[name]), name  # node state is unchanged by a bit
    return want_rest


# ---- 1. bits equal the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 63, 65, 255, 257, 700])
def test_bits_equal_the_restatement(pies, n, channels):
    """n: a lane tail, the tile's edge, a second and a third tile of the sum order.  700 actuators need more constraints than one
    lattice and one sheet have: the scene then carries four of each."""
    g = pies.Solver(scenes.pbd_options(pies, 4))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    lattice_and_sheet(g, seed=n, copies=4 if n > 236 else 1)
    k, acts = add_random_set(g, 100 * n + channels, n, channels)
    g.finalize()
    rest1 = check_against_restatement(g, k, acts, activations(n + channels, channels))
    g.tick()
    # a second drive on the moved state: base stays the rest at pies_add_actuators, the values follow the nodes
    rest2 = check_against_restatement(g, k, acts, activations(n + channels + 1, channels, first=-1.1))
    assert any(not same(rest1[t], rest2[t]) for t in rest1)
    g.close()


# ---- 2. the same bits as the rebuild path, and as the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("schedule,dims", [("EXACT", (4, 4, 8)), ("COLOURED", (4, 4, 8)), ("LAYERED", (4, 4, 15))])
def test_drive_equals_set_rest_and_the_oracle(pies, oracle, schedule, dims):
    c = Case(pies, oracle, schedule, dims, bend=True)
    A = c.handle()
    A.finalize()
    k, acts = add_random_set(A, 7, 60, 3, bends=12)
    ids, rest = containers(A)
    S = state_of(A)
    activation = activations(7, 3)
    new = drive_actuators(S["positions"], ids, rest, acts, activation)[0]
    assert all(not same(new[t], rest[t]) for t in new)

    def build(s):
        c.scene(s)
        for t in new:
            s.set_rest(t, new[t])
    A.drive_actuators(k, activation)
    B = c.handle(build)
    B.finalize()
    for t in new:
        assert same(A.rest(t), B.rest(t))
    c.compare(("drive", schedule), A, B, c.fresh_oracle(S, B, build), c.handle(), m=3)
    for name in NODE_ARRAYS:
        assert same(getattr(A, name), getattr(B, name)), name
    A.close()
    B.close()


def pd_body(pies, s):
    """distance, bend and tetrahedral (strain + volume) constraints, no shape constraints: the 3 x 3 x 6 beam with createBox's
    distance constraints over the same lattice and a few bend quadruples"""
    s.create_tet_box(3, 3, 6, translation=(0.0, 0.52, 0.0), w=20.0, volume=True, triangles=True)
    s.create_box(3, 3, 6, w=5.0, existing_offset=0, triangles=False)
    G = lambda i, j, k: k + 6 * (j + 3 * i)  # noqa: E731
    s.add_bend(U([[G(i, 1, k), G(i + 1, 1, k + 1), G(i + 1, 1, k), G(i, 2, k + 1)] for i in range(2) for k in range(0, 5, 2)]), 3.0)
    s.add_position(U([6 * (j + 3 * i) for i in range(3) for j in range(3)]), 2.0)
    scenes.perturb(s, 9, 0.08)
    s.set_prev_positions(s.positions)


def test_drive_equals_set_rest_under_pd(pies):
    """A and B are fresh builds with the same records and the same matrix: neither datum enters the system"""
    A, B, W = (pies.Solver(pies.Options(solver=pies.PD, iterations=6)) for _ in range(3))
    for s in (A, B, W):
        pd_body(pies, s)
    A.finalize()
    k, acts = add_random_set(A, 11, 40, 2, bends=4)
    ids, rest = containers(A)
    activation = activations(11, 2)
    new = check_against_restatement(A, k, acts, activation)
    assert {a.type for a in acts} == {pies.DISTANCE, pies.BEND}
    for t in new:
        B.set_rest(t, new[t])
    B.finalize()
    for t in range(3):
        for s in (A, B, W):
            s.tick()
        same_bits(("pd", "drive against set_rest, tick %d" % t), A, B)
    assert any_bit_differs(A, W) and not A.failed  # the drive matters
    for s in (A, B, W):
        s.close()


# ---- 3. the closed loop ----------------------------------------------------------------------------------------------------------
def test_closed_loop_equals_set_rest_every_tick(pies):
    """Ten ticks under PBD LAYERED with another activation vector before each: a drive on the live handle A; the rebuild path on a
    second handle - the scene with pies_set_rest of the restatement's rests, the state before the tick, one tick.  Schedule LAYERED
    plans its sweep order from the node positions it finds at pies_finalize (test_live_edits_gpu.Case.fresh), so the second handle
    is finalized where A was - at the factory positions - and given the state afterwards: the two then sweep in one order, and
    every bit of the rebuild path's result is the drive's."""
    A, W = body(pies), body(pies)
    A.finalize()
    k, acts = add_random_set(A, 21, 80, 3, bends=20)
    ids, rest = containers(A)
    before = A.launch_counts()
    assert before["layer"] > 0
    S = state_of(A)
    for t in range(10):
        activation = activations(300 + t, 3, first=0.9) * F(0.3)
        rest = drive_actuators(S["positions"], ids, rest, acts, activation)[0]
        A.drive_actuators(k, activation, sums=False)
        B = body(pies)
        for c in rest:
            B.set_rest(c, rest[c])
        B.finalize()
        put_state(B, S)
        for s in (A, B):
            s.tick()
        same_bits(("loop", t), A, B)
        for c in rest:
            assert same(A.rest(c), rest[c]) and same(B.rest(c), rest[c])
        S = state_of(B)
        B.close()
    assert A.launch_counts() == before and not A.failed
    W.tick(10)
    assert any_bit_differs(A, W)
    for s in (A, W):
        s.close()


# ---- 4. a drive survives a rebuild -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [("LAYERED", "COLOURED"), ("COLOURED", "EXACT")])
def test_driven_rests_survive_a_rebuild(pies, first, second):
    A, B = body(pies, first), body(pies, second)
    A.finalize()
    k, acts = add_random_set(A, 31, 70, 3)
    ids, rest = containers(A)
    activation = activations(31, 3)
    new = drive_actuators(A.positions, ids, rest, acts, activation)[0]
    A.drive_actuators(k, activation)
    A.set_schedule(getattr(pies, "SCHEDULE_" + second))
    for t in new:
        B.set_rest(t, new[t])
    for t in range(2):
        A.tick()
        B.tick()
        same_bits(("rebuild", second, t), A, B)
    for t in new:
        assert same(A.rest(t), new[t])
    # the set was staged again with the new plan's slots: another drive, another schedule's order, the same rule
    check_against_restatement(A, k, acts, activations(32, 3))
    A.close()
    B.close()


def test_set_rest_after_a_drive_wins_for_its_range(pies):
    A, B = body(pies), body(pies)
    A.finalize()
    k, acts = add_random_set(A, 41, 90, 2)
    ids, rest = containers(A)
    activation = activations(41, 2)
    new = drive_actuators(A.positions, ids, rest, acts, activation)[0]
    A.drive_actuators(k, activation)
    override = (new[pies.DISTANCE][10:50] * F(1.05)).astype(F)
    new[pies.DISTANCE][10:50] = override
    A.set_rest(pies.DISTANCE, override, first=10)
    for t in new:
        assert same(A.rest(t), new[t])
        B.set_rest(t, new[t])
    driven_in_range = [a for a in acts if a.type == pies.DISTANCE and 10 <= a.index < 50]
    driven_outside = [a for a in acts if a.type == pies.DISTANCE and not 10 <= a.index < 50]
    assert driven_in_range and driven_outside
    for t in range(2):
        A.tick()
        B.tick()
        same_bits(("override", t), A, B)
    # an appended body rebuilds too and keeps the driven values; the set is not disturbed
    for s in (A, B):
        s.create_box(2, 2, 2, translation=(12.0, 2.0, 0.0), w=0.5, triangles=False)
    A.tick()
    B.tick()
    same_bits("appended", A, B)
    assert same(A.rest(pies.DISTANCE)[:len(new[pies.DISTANCE])], new[pies.DISTANCE])
    check_against_restatement(A, k, acts, activations(42, 2))
    A.close()
    B.close()


# ---- 5. renumbered ---------------------------------------------------------------------------------------------------------------
def test_renumbered_scene_gives_the_bits_of_the_unrenumbered_run(pies):
    mesh = shuffled_beam()
    pos, tets, edges = mesh
    got = []
    for renumber in (1, 0):
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=6))
        g.set_flag(pies.FLAG_RENUMBER_NODES, renumber)
        scenes.build_unstructured_pd(g, mesh)
        g.add_distance(edges[::7], 2.0)
        g.add_bend(tets[::11], 0.5)
        scenes.perturb(g, 4, 0.03)
        g.set_prev_positions(g.positions)
        g.finalize()
        assert g.count(pies.NODES_RENUMBERED) == renumber
        k, acts = add_random_set(g, 51, 300, 5)
        activation = activations(51, 5)
        check_against_restatement(g, k, acts, activation)
        g.tick()
        out = g.drive_actuators(k, activations(52, 5), per_actuator=True)
        got.append(out + tuple(g.rest(t) for t in (pies.DISTANCE, pies.BEND)))
        g.close()
    for a, b in zip(*got):
        assert np.array_equal(np.ascontiguousarray(a).view(U), np.ascontiguousarray(b).view(U))


# ---- 6. the device form ----------------------------------------------------------------------------------------------------------
def test_device_form_gives_the_host_forms_bits(pies, hip):
    A, B = body(pies, copies=2), body(pies, copies=2)
    for g in (A, B):
        g.finalize()
        g.tick()
    n, channels = 300, 3
    (k, acts), _ = add_random_set(A, 61, n, channels), add_random_set(B, 61, n, channels)
    activation = activations(61, channels)
    want = A.drive_actuators(k, activation, per_actuator=True)
    act = DevBuf(hip, channels, fill=activation)
    sums, live, per = DevBuf(hip, 2 * channels, offset=1), DevBuf(hip, channels), DevBuf(hip, 2 * n, offset=1)
    B.drive_actuators_device(k, channels, act.ptr, sums.ptr, live.ptr, per.ptr, flags=pies.IO_HOST_SYNC)
    assert same(sums.get(), want[0]) and np.array_equal(live.get(U), want[1]) and same(per.get(), want[2])
    for t in (pies.DISTANCE, pies.BEND):
        assert same(A.rest(t), B.rest(t))
    # without a host synchronisation: the caller's default stream waits for the call's launches
    B.drive_actuators_device(k, channels, act.ptr, sums.ptr, 0, 0)
    assert same(sums.get(), want[0])
    A.tick()
    B.tick()
    same_bits("device form", A, B)
    for b in (act, sums, live, per):
        b.free()
    A.close()
    B.close()


def test_nan_activation_on_the_device_leaves_its_constraints_alone(pies, hip):
    g = body(pies)
    g.finalize()
    n, channels = 120, 4
    k, acts = add_random_set(g, 71, n, channels)
    activation = np.array([1.4, np.nan, -0.6, np.inf], F)
    ids, rest = containers(g)
    trace = []
    new, want_per, want_sums, want_live = drive_actuators(g.positions, ids, rest, acts, activation, trace=trace)
    dead = [a for a, code in zip(acts, trace) if code == B_NOT_LIVE]
    assert 0 < len(dead) < n and want_live[1] == want_live[3] == 0 and want_live[0] > 0
    act = DevBuf(hip, channels, fill=activation)
    sums, live, per = DevBuf(hip, 2 * channels), DevBuf(hip, channels), DevBuf(hip, 2 * n)
    g.drive_actuators_device(k, channels, act.ptr, sums.ptr, live.ptr, per.ptr, flags=pies.IO_HOST_SYNC)
    assert same(sums.get(), want_sums) and np.array_equal(live.get(U), want_live) and same(per.get(), want_per)
    for t in rest:
        assert same(g.rest(t), new[t])
    for a in dead:
        assert bits(g.rest(a.type)[a.index])[0] == bits(rest[a.type][a.index])[0]
    # the host-pointer form refuses the same activations and changes nothing
    with pytest.raises(pies.PiesError):
        g.drive_actuators(k, activation)
    for t in rest:
        assert same(g.rest(t), new[t])
    for b in (act, sums, live, per):
        b.free()
    g.close()


def test_device_pointers_are_checked(pies, hip):
    g = body(pies)
    g.finalize()
    k, acts = add_random_set(g, 81, 50, 2)
    L = pies.load()
    host = np.zeros(2, F)
    rest = containers(g)[1]
    assert L.pies_drive_actuators_device(g._h, k, 2, host.ctypes.data, None, None, None, None, 0) == pies.ERR_INVALID
    act = DevBuf(hip, 2, fill=np.array([0.5, 0.25], F))
    small = DevBuf(hip, 2 * 50 - 16)  # (the sentinels behind the data belong to the allocation)
    assert L.pies_drive_actuators_device(g._h, k, 2, act.ptr, None, None, small.ptr, None, 0) == pies.ERR_INVALID
    assert "allocation" in g.last_error()
    small.get()
    for t in rest:
        assert same(g.rest(t), rest[t])  # nothing was launched
    act.free()
    small.free()
    g.close()


def test_capturing_stream_is_refused(pies, hip):
    g = body(pies)
    g.finalize()
    k, acts = add_random_set(g, 91, 50, 2)
    act = DevBuf(hip, 2, fill=np.array([0.5, 0.25], F))
    g.drive_actuators_device(k, 2, act.ptr, flags=pies.IO_HOST_SYNC)  # (the set is staged: the refused call has nothing to build)
    rest = containers(g)[1]
    L = hip.L
    L.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    L.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.hipGraphDestroy.argtypes = [C.c_void_p]
    stream, graph = C.c_void_p(), C.c_void_p()
    hip.ok(L.hipStreamCreate(C.byref(stream)))
    hip.ok(L.hipStreamBeginCapture(stream, 2))  # hipStreamCaptureModeRelaxed
    rc = pies.load().pies_drive_actuators_device(g._h, k, 2, act.ptr, None, None, None, stream, 0)
    hip.ok(L.hipStreamEndCapture(stream, C.byref(graph)))
    if graph.value:
        hip.ok(L.hipGraphDestroy(graph))
    hip.ok(L.hipStreamDestroy(stream))
    assert rc == pies.ERR_STATE and "capturing" in g.last_error()
    for t in rest:
        assert same(g.rest(t), rest[t])
    g.drive_actuators_device(k, 2, act.ptr, flags=pies.IO_HOST_SYNC)  # the handle still works
    act.free()
    g.close()


@pytest.fixture(scope="module")
def child():
    out = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-800:], out.stderr[-1600:])
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout[-800:]
    return json.loads(lines[0])


def test_torch_bridge_gives_the_host_forms_bits(child):
    assert len(child["runtimes"]) == 1
    assert child["outputs"] == {"sums": True, "live": True, "per_actuator": True, "rest": True}, child["outputs"]
    assert child["nan"] == {"live": True, "rest": True}, child["nan"]
    assert child["refused"] == [True, True, True]  # a CPU tensor, a wrong shape, a wrong dtype


def test_torch_closed_loop_equals_the_host_loop(child):
    """tick_async -> positions() -> a policy on the device -> drive_actuators, no host synchronisation inside the loop, under PD on
    the folding bend sheet: the state of the same loop through the host-pointer form"""
    r = child["loop"]
    assert r["equal"] == [True, True, True] and r["finite"] and not r["failed"] and r["folded"] > 0.0, r


# ---- 7. outputs optional, calls repeat -------------------------------------------------------------------------------------------
def test_every_subset_of_the_outputs_leaves_the_same_rests(pies):
    g = body(pies, copies=2)
    g.finalize()
    n, channels = 300, 3
    k, acts = add_random_set(g, 101, n, channels)
    activation = activations(101, channels)
    L = pies.load()
    counts = g.launch_counts()
    full, rests = None, None
    pf = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    for mask in itertools.product((True, False), repeat=3):
        sums, live, per = np.full((channels, 2), -7.0, F), np.full(channels, 77, U), np.full((n, 2), -7.0, F)
        for rep in range(2):  # two identical calls return identical bits
            rc = L.pies_drive_actuators(g._h, k, channels, pf(activation), pf(sums) if mask[0] else None,
                                        live.ctypes.data_as(C.POINTER(C.c_uint32)) if mask[1] else None, pf(per) if mask[2] else None)
            assert rc == pies.OK
            got = (sums.copy(), live.copy(), per.copy(), g.rest(pies.DISTANCE), g.rest(pies.BEND))
            if full is None:
                full = got
            for j in range(3):
                assert same(got[j].view(F), full[j].view(F)) if mask[j] else (got[j].view(U) == (77 if j == 1 else bits(F(-7.0))[0])).all()
            assert same(got[3], full[3]) and same(got[4], full[4])
    assert g.launch_counts() == counts
    g.close()


# ---- 8. lifetime -----------------------------------------------------------------------------------------------------------------
def test_resources_return_after_destroy(pies):
    gc.collect()
    start = pies.resource_counts()["live"]
    g = body(pies, copies=2)
    g.finalize()
    k0, a0 = add_random_set(g, 111, 100, 2)
    k1, a1 = add_random_set(g, 112, 300, 4)
    g.drive_actuators(k0, activations(1, 2), per_actuator=True)
    g.drive_actuators(k1, activations(2, 4), per_actuator=True)
    staged = pies.resource_counts()["live"]
    assert staged["device_allocations"] > start["device_allocations"]
    g.set_schedule(pies.SCHEDULE_COLOURED)  # one rebuild: the staged copies go with the scene and come back at the next drive
    g.tick()
    g.drive_actuators(k0, activations(3, 2), per_actuator=True)
    g.drive_actuators(k1, activations(4, 4), per_actuator=True)
    g.close()
    assert pies.resource_counts()["live"] == start
