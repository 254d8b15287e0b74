"""The CPU oracle's PBD tick against an exact float32 restatement of the reference (tests/pbd_restatement.py): predict, position and
distance constraints, floor clamp and velocity update with floor friction, under four option sets that leave no option at the
value every other test uses, hinge held and released.  Exact equality, no tolerance.

The oracle and the device kernels were written by one hand from one reading of the reference; the restatement is a second reading
that shares no code with either.  The teeth test shows, from the restatement's own tally, that the scene takes every branch the
comparison is meant to pin."""
import numpy as np
import pytest

import pbd_restatement as R

TICKS = 2
SETS = sorted(R.OPTION_SETS)

_restated = {}


def restated(name, hinge, zero_radii=False):
    """(Scene, [state after tick 1, after tick 2], tally) of the restatement sweeping in container order; computed once"""
    key = (name, hinge, zero_radii)
    if key not in _restated:
        import oracle_api
        scene = R.build(oracle_api.OracleSolver(R.solver_options(oracle_api, name)), oracle_api, name, zero_radii=zero_radii)
        tally, states, state = R.new_tally(), [], scene.start()
        for _ in range(TICKS):
            state = scene.tick(state, hinge=hinge, tally=tally)
            states.append(state)
        _restated[key] = (scene, states, tally)
    return _restated[key]


def oracle_scene(oracle, name, hinge, zero_radii=False):
    o = oracle.OracleSolver(R.solver_options(oracle, name))
    scene = R.build(o, oracle, name, zero_radii=zero_radii)
    o.set_flag(oracle.FLAG_NODE_COLLISIONS, 0)
    o.set_flag(oracle.FLAG_RELEASE_HINGE, hinge)
    return o, scene


def test_scene_is_what_the_restatement_is_given(oracle):
    """The builder's own account of the scene against what the oracle holds: node arrays, rest lengths (this module's arithmetic
    against the oracle's), constraint counts"""
    o, scene = oracle_scene(oracle, "B", 0)
    assert np.array_equal(o.positions, scene.positions) and np.array_equal(o.prev_positions, scene.positions)
    assert np.array_equal(o.velocities, scene.velocities) and np.array_equal(o.radii, scene.radii)
    assert np.array_equal(o.rest(oracle.DISTANCE), np.float32([d[2] for d in scene.dists]))
    assert o.count(oracle.POSITION) == len(R.PINS) and o.count(oracle.TET) > 0 and o.count(oracle.NODES) > 600
    assert len(scene.rows["threshold"]) == R.THRESHOLD_ROW


@pytest.mark.parametrize("hinge", [0, 1])
@pytest.mark.parametrize("name", SETS)
def test_oracle_equals_restatement(oracle, name, hinge):
    o, _ = oracle_scene(oracle, name, hinge)
    _, states, _ = restated(name, hinge)
    for t in range(TICKS):
        o.tick()
        R.assert_same((name, hinge, "tick %d" % t), o, states[t])


def test_oracle_equals_restatement_in_a_replayed_order(oracle):
    """ora_permute's order is the order the restatement sweeps in: what the device comparison relies on when it hands the
    restatement the order a schedule exports"""
    o, scene = oracle_scene(oracle, "B", 0)
    rng = np.random.default_rng(8)
    pin_order, dist_order = rng.permutation(len(scene.pins)), rng.permutation(len(scene.dists))
    o.permute(oracle.POSITION, pin_order)
    o.permute(oracle.DISTANCE, dist_order)
    state = scene.start()
    for t in range(TICKS):
        o.tick()
        state = scene.tick(state, pin_order, dist_order)
        R.assert_same(("replayed order", "tick %d" % t), o, state)
    assert not np.array_equal(state[0], restated("B", 0)[1][-1][0])  # the order matters on this scene


@pytest.mark.parametrize("rule", [0, 1, 2])
def test_oracle_with_the_node_node_pass_and_radii_zero(oracle, rule):
    """Every radius 0: the node-node pass visits and resolves nothing, in each of the oracle's three orders"""
    o, _ = oracle_scene(oracle, "B", 0, zero_radii=True)
    o.set_flag(oracle.FLAG_NODE_COLLISIONS, 1)
    o.set_flag(oracle.FLAG_COLLISION_RULE, rule)
    _, states, _ = restated("B", 0, zero_radii=True)
    for t in range(TICKS):
        o.tick()
        R.assert_same(("radii 0", rule, "tick %d" % t), o, states[t])
    assert o.collision_pairs == 0


@pytest.mark.parametrize("name", SETS)
def test_teeth(name):
    """Conditions on the inputs, from the restatement's tally alone: over the two ticks every decision class is populated"""
    scene, _, tally = restated(name, 0)
    counts = R.tally_counts(tally)
    print(name, counts)
    assert counts["clamped"] > 0 and counts["clamps"] >= counts["clamped"], counts
    assert counts["touching"] > 0, counts      # `<=` true, `<` false
    assert counts["zeroed"] > 0 and counts["scaled"] > 0, counts
    assert counts["fallbacks"] >= 1, counts
    # exactly one node of the threshold row at l == 5.0f, scaled and not zeroed - and no node anywhere else
    assert len(tally["at_five"]) == 1, tally["at_five"]
    node, was_scaled = tally["at_five"][0]
    assert node in scene.rows["threshold"] and was_scaled
    row = scene.rows["threshold"]
    assert len(tally["scaled"] & set(row.tolist())) >= 32 and len(tally["zeroed"] & set(row.tolist())) >= 32
    if name == "D":  # the gravity term's grouping shows: in the term, and in the predicted height of a node that stays airborne
        dt, g = np.float32(0.02) / np.float32(3), np.float32(9.81)
        assert (-g * dt) * dt != -g * (dt * dt)
        low = scene.rows["near_zero"]
        y = scene.positions[low, 1]
        assert (y + (-g * dt) * dt != y + -g * (dt * dt)).sum() >= 3 and not tally["clamped"] & set(low.tolist())
    if name == "B":  # floorHeight 0.3, radii in [0.2, 0.9]: fl(fl(floor + r) - r) lies on either side of the floor
        assert counts["clamped_reads_above"] >= 5 and counts["clamped_reads_below"] >= 5 and counts["clamped_reads_equal"] >= 5, counts
    if name == "A":  # floorHeight 0: a clamped node always reads on the floor
        assert counts["clamped_reads_above"] == 0 and counts["clamped_reads_below"] == 0, counts
