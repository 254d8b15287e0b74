"""Shared by test_live_edits_gpu.py and test_live_edits_pd_gpu.py: one edit of a LIVE scene - finalized, captured, ticked, its host
mirrors older than HBM - held to a yardstick that never saw a live handle.

Every case: build on the live handle L and on a twin T, tick both k times, take the pre-edit state S from T (reading L would bring
its mirrors up to date, and a write that arrives while they are stale is the path under test), apply ONE edit to L, tick m more
times and compare after each tick.
  PBD: bit for bit against a fresh handle F given the final scene and S (the edit's array overriding), finalized at the
       positions the live handle was last finalized at (schedule LAYERED plans from them: test_live_edits_gpu.Case.fresh);
       F in turn against a fresh oracle permuted once to F's order.  The edit matters: F and a fresh handle without the edit
       differ in at least one bit.
  PD:  test_pd_parity_gpu.yardstick against an fp32 and an fp64 oracle that took the same build, ticks and edit.  The edit matters:
       an fp64 oracle without it is at least 10 gates away at the first compared tick (both sides oracle values)."""
import numpy as np

NODE_ARRAYS = ("positions", "prev_positions", "velocities", "radii", "inv_masses")
MOTION = ("positions", "velocities", "prev_positions")
NODES = 9  # PIES_NODES / the oracle's node count
DT = 0.012


def state_of(s):
    return {name: getattr(s, name).copy() for name in NODE_ARRAYS}


def put_state(s, state):
    """The node arrays of `state` written over the first len(state) nodes of s (a scene with appended nodes keeps their factory state)"""
    for name in NODE_ARRAYS:
        a = getattr(s, name).copy()
        a[: len(state[name])] = state[name]
        getattr(s, "set_" + name)(a)


def node_edit(what, state, radius_factor=1.3):
    """The new value of one node array from the pre-edit state: seeded, and far above rounding"""
    n = len(state["radii"])
    rng = np.random.default_rng(77)
    if what == "positions" or what == "prev_positions":
        return state[what] + rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    if what == "velocities":
        return state[what] + np.float32([1.0, 0.0, 0.0])
    if what == "radii":
        return state[what] * np.float32(radius_factor)
    assert what == "inv_masses"
    return state[what] * rng.choice(np.float32([0.1, 1.0, 10.0]), n)


def same_bits(tag, a, b, names=MOTION):
    """test_handle_reuse_gpu.same_state over positions, velocities and previous positions; a, b: handles or dicts of arrays"""
    for name in names:
        x = a[name] if isinstance(a, dict) else getattr(a, name)
        y = b[name] if isinstance(b, dict) else getattr(b, name)
        assert np.isfinite(y).all(), (tag, name)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), \
            (tag, name, "max |a - b| = %.3g" % float(np.abs(x - y).max()))


def any_bit_differs(a, b, names=MOTION):
    return any(not np.array_equal(getattr(a, name).view(np.uint32), getattr(b, name).view(np.uint32)) for name in names)


def pd_gate(o32, o64, name, spacing=1.0):
    """yardstick()'s gate for one state array"""
    d_ref = float(np.abs(getattr(o32, name) - getattr(o64, name)).max())
    return max(2.0 * d_ref, 1e-4 * spacing / (DT if name == "velocities" else 1.0))


def pd_edit_matters(test, o32, o64, without, names, spacing=1.0, least=10.0):
    """The condition on a PD case's inputs: the fp64 oracle with the edit against the fp64 oracle without it, in gates of the
    yardstick, over the compared arrays (a previous-position write shows in the velocities first).  Oracle values on both sides."""
    ratios = {}
    for name in names:
        a, b = getattr(o64, name), getattr(without, name)
        m = min(len(a), len(b))  # (appended nodes: the nodes both scenes have)
        ratios[name] = float(np.abs(a[:m] - b[:m]).max()) / pd_gate(o32, o64, name, spacing)
    assert max(ratios.values()) >= least, (test, "the edit does not matter", ratios)
    return ratios
