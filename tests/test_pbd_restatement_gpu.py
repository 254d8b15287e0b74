"""The device's PBD tick against the exact float32 restatement of the reference (tests/pbd_restatement.py), in every schedule and
in every form the per-node steps are launched in: fused into layer launches (LAYERED, one strip), as launches of their own over the
level-ordered copy (LAYERED with strips), opening a launch after a collision pass, and as single launches around the wave levels or
the batch sweeps (EXACT, COLOURED).  The options reach those kernels by four routes; no option is at the value the other tests use.

The restatement sweeps each container in the order the device reports after finalize() (the container order under EXACT).  Exact
equality after each of two ticks, no tolerance; the launch counts show that the form a case is about is the form that ran."""
import numpy as np
import pytest

import pbd_restatement as R

pytestmark = pytest.mark.gpu

TICKS = 2
EXACT, COLOURED, LAYERED = 0, 1, 2
SCHEDULES = pytest.mark.parametrize("schedule", [EXACT, COLOURED, LAYERED], ids=["exact", "coloured", "layered"])
STRIPS = (("PIES_LAYER_ONE_STRIP_MAX", "40"), ("PIES_LAYER_TILE_NODES", "90"), ("PIES_LAYER_STRIPS_MIN_NODES", "0"))

_restated = {}


def restated(scene, iterations, zero_radii, hinge, pin_order, dist_order):
    """The restatement's state after each tick, computed once per (scene, sweep orders)"""
    key = (scene.name, iterations, zero_radii, hinge, None if pin_order is None else pin_order.tobytes(),
           None if dist_order is None else dist_order.tobytes())
    if key not in _restated:
        states, state = [], scene.start()
        for _ in range(TICKS):
            state = scene.tick(state, pin_order, dist_order, hinge)
            states.append(state)
        _restated[key] = states
    return _restated[key]


def run(pies, name, schedule, hinge=0, collisions=None, iterations=R.ITERATIONS):
    """Builds the scene on a device handle, ticks it twice against the restatement, returns the handle.
    collisions: None (pass off), "default" (the schedule's own node-node order) or a PIES_COLLISION_ORDER_*; the pass runs on radii 0"""
    zero_radii = collisions is not None
    g = pies.Solver(R.solver_options(pies, name, iterations))
    scene = R.build(g, pies, name, iterations, zero_radii=zero_radii)
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0 if collisions is None else 1)
    if collisions not in (None, "default"):
        g.set_flag(pies.FLAG_COLLISION_ORDER, collisions)
    g.set_flag(pies.FLAG_RELEASE_HINGE, hinge)
    g.set_schedule(schedule)
    g.finalize()
    pin_order = dist_order = None  # EXACT: the container order
    if schedule != EXACT:
        pin_order, dist_order = g.order(pies.POSITION), g.order(pies.DISTANCE)
        assert sorted(pin_order.tolist()) == list(range(len(scene.pins))) and sorted(dist_order.tolist()) == list(range(len(scene.dists)))
    states = restated(scene, iterations, zero_radii, hinge, pin_order, dist_order)
    for t in range(TICKS):
        g.tick()
        R.assert_same((name, schedule, hinge, collisions, iterations, "tick %d" % t), g, states[t])
    assert not g.failed
    if collisions is not None:
        assert g.collision_pairs == 0
    return g


def check_form(pies, g, schedule, iterations=R.ITERATIONS):
    lc = g.launch_counts()
    if schedule == LAYERED:  # the fused form: predict and velocity ride in the layer launches
        assert lc["layer"] == 2 * iterations + 1 and lc["predict"] == 0 and lc["velocity"] == 0, lc
    elif schedule == EXACT:
        assert lc["wave"] > 0, lc
    else:
        assert lc["distance"] > 0 and lc["layer"] == 0 and lc["wave"] == 0, lc


@pytest.mark.parametrize("hinge", [0, 1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
@SCHEDULES
def test_every_schedule_and_option_set(pies, schedule, name, hinge):
    g = run(pies, name, schedule, hinge)
    check_form(pies, g, schedule)


@SCHEDULES
def test_gravity_term_grouping(pies, schedule):
    """Option set D: the one under which ((-g dt) dt) and (-g (dt dt)) are different floats"""
    g = run(pies, "D", schedule)
    check_form(pies, g, schedule)


def test_exact_without_wave_levels(pies, tune):
    """k_predict, k_floor and k_velocity as launches of their own around one launch per container level"""
    tune("PIES_NO_WAVEFRONT", "1")
    lc = run(pies, "B", EXACT).launch_counts()
    assert lc["wave"] == 0 and lc["predict"] == 1 and lc["velocity"] == 1 and lc["floor"] == R.ITERATIONS and lc["distance"] > 0, lc


@pytest.mark.parametrize("name", ["B", "C"])
def test_layered_strips(pies, tune, name):
    """Strips forced onto this scene: predict, floor clamp, position constraints and velocity over the level-ordered copy"""
    for switch, value in STRIPS:
        tune(switch, value)
    lc = run(pies, name, LAYERED).launch_counts()
    assert lc["layer"] > 0 and lc["predict"] == 1 and lc["velocity"] == 1 and lc["floor"] > 0 and lc["position"] > 0, lc


@pytest.mark.parametrize("order", ["default", 0], ids=["default-order", "reference-order"])
@pytest.mark.parametrize("form", [EXACT, COLOURED, LAYERED, "strips"], ids=["exact", "coloured", "layered", "layered-strips"])
def test_collision_pass_cuts_the_launches(pies, tune, form, order):
    """Every radius 0: the node-node pass runs (grid build, resolve launches) and resolves nothing, so the exact answer stays
    known while the pass cuts the wave levels and the layer launches, and per-node steps open launches of their own"""
    if form == "strips":
        for switch, value in STRIPS:
            tune(switch, value)
    schedule = LAYERED if form == "strips" else form
    g = run(pies, "B", schedule, collisions=pies.COLLISION_ORDER_REFERENCE if order == 0 else "default")
    lc = g.launch_counts()
    assert lc["collide"] > 0, lc
    if schedule == LAYERED:
        assert lc["layer"] > 0 and (lc["predict"] == 1) == (form == "strips"), lc
    elif schedule == EXACT:
        assert lc["wave"] > 0, lc


@pytest.mark.parametrize("iterations", [0, 1])
@SCHEDULES
def test_no_and_one_iteration(pies, schedule, iterations):
    """iterations = 0: predict and velocity alone (LAYERED: one layer launch over the even tiles, which cover every node; EXACT: no
    wave plan, the single launches); iterations = 1: the shortest program with every step in it"""
    g = run(pies, "B", schedule, iterations=iterations)
    lc = g.launch_counts()
    if schedule == LAYERED:
        assert lc["layer"] == 2 * iterations + 1 and lc["predict"] == 0 and lc["velocity"] == 0, lc
    elif iterations == 0:
        assert lc["predict"] == 1 and lc["velocity"] == 1 and lc["wave"] == lc["distance"] == lc["floor"] == 0, lc


def test_layered_direct_launches_equal_the_replayed_capture(pies, tune):
    """PIES_NO_GRAPH=1: the three substeps of a tick as direct launches, no graph instantiated - the same bits as the replayed capture"""
    a = run(pies, "B", LAYERED)
    tune("PIES_NO_GRAPH", "1")
    before = pies.resource_counts()["created"]["graph_execs"]
    b = run(pies, "B", LAYERED)
    assert pies.resource_counts()["created"]["graph_execs"] == before
    assert b.launch_counts() == a.launch_counts()
    for name in R.MOTION:
        assert np.array_equal(getattr(a, name).view(np.uint32), getattr(b, name).view(np.uint32)), name
