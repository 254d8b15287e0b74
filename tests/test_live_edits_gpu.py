"""Edits of a live PBD scene, and edits around work in flight (see live_edits.py for the pattern).  The live handle after the
edit equals, bit for bit, a fresh handle that was given the final scene and the pre-edit state (Case.fresh: finalized where the
live handle last was); the fresh handle equals the oracle permuted once to its order (bend: TOL, acos).  Every case asserts that
its edit matters.

What an edit can change differs by array, so the scenes are chosen for it: radii act through the floor (the beams start 0.6
above it) and the node-node pass; inverse masses act through bend constraints and the node-node pass only (distance and strain
projections do not read them), so the mass cases without collisions carry a few bend constraints.  Previous positions are
overwritten by the next predict step (Solver.cpp:40-52): a write to them cannot show in any later state, so that case holds that
the write leaves positions and velocities alone while their mirrors are stale, and that the host reads the written values back."""
import numpy as np
import pytest

import scenes
from live_edits import MOTION, any_bit_differs, node_edit, put_state, same_bits, state_of
from test_pbd_parity_gpu import TOL

pytestmark = pytest.mark.gpu

WRITES = ("positions", "prev_positions", "velocities", "radii", "inv_masses")
# schedule, lattice, timeSubsteps, node-node collisions
CONFIGS = {
    "exact": ("EXACT", (4, 4, 8), 1, 0),
    "coloured": ("COLOURED", (4, 4, 8), 1, 0),
    "layered-substeps": ("LAYERED", (4, 4, 15), 3, 0),
    "layered-collisions": ("LAYERED", (4, 4, 15), 1, 1),
}
CONTAINERS = ("POSITION", "DISTANCE", "TET", "BEND")


class Case:
    """One configuration: how a handle and an oracle are made for it"""

    def __init__(self, pies, oracle, schedule, dims, substeps=1, collisions=0, order=None, iterations=4, bend=False, radius=None):
        self.pies, self.oracle, self.dims, self.collisions, self.order, self.bend = pies, oracle, dims, collisions, order, bend
        self.radius = radius  # None: createTetBox's 0.475; 0.5: lattice neighbours touch and the perturbation makes them overlap
        self.schedule = getattr(pies, "SCHEDULE_" + schedule)
        self.expect_layer = schedule == "LAYERED"
        self.opt = dict(iterations=iterations, timeSubsteps=substeps)

    def scene(self, s):
        W, H, D = self.dims
        scenes.build_beam(s, self.dims, translation=(0.0, 0.6, 0.0))
        if self.bend:
            G = lambda i, j, k: k + D * (j + H * i)  # noqa: E731
            s.add_bend(np.uint32([[G(i, 1, k), G(i + 1, 1, k + 1), G(i + 1, 1, k), G(i, 2, k + 1)] for i in range(W - 1) for k in range(0, D - 1, 2)]), 0.6)
        if self.radius is not None:
            s.set_radii(np.full(W * H * D, self.radius, np.float32))
        scenes.perturb(s, 7, 0.05)

    def handle(self, build=None):
        g = self.pies.Solver(scenes.pbd_options(self.pies, **self.opt))
        g.set_schedule(self.schedule)
        g.set_flag(self.pies.FLAG_NODE_COLLISIONS, self.collisions)
        if self.order is not None:
            g.set_flag(self.pies.FLAG_COLLISION_ORDER, self.order)
        (build or self.scene)(g)
        return g

    def fresh(self, state, build=None, rebuilt=True):
        """A fresh handle with `state`.  Schedule LAYERED plans from the node positions it finds at pies_finalize (levels, tiles and
        with them the sweep order), so the fresh handle is finalized where the live one last was: rebuilt=True - the edit makes the
        live handle rebuild at its current state - the state first; rebuilt=False - the edit keeps the live handle's plans (a
        node upload, a re-capture) - finalize at the factory state first, then the state through the same writes (on a handle that
        never ticked: no stale mirror, no sync)."""
        g = self.handle(build)
        if not rebuilt:
            g.finalize()
        put_state(g, state)
        return g

    def fresh_oracle(self, state, F, build=None, rule=None):
        """The oracle of the fresh handle F: the same scene and state, permuted once to F's order, the node-node pass in F's order"""
        pies, oracle = self.pies, self.oracle
        o = oracle.OracleSolver(scenes.pbd_options(oracle, **self.opt))
        (build or self.scene)(o)
        o.set_flag(oracle.FLAG_NODE_COLLISIONS, self.collisions)
        if rule is None:
            rule = self.order if self.order is not None else (0 if self.schedule == pies.SCHEDULE_EXACT else 2)
        o.set_flag(oracle.FLAG_COLLISION_RULE, rule)
        put_state(o, state)
        if self.schedule != pies.SCHEDULE_EXACT:
            for name in CONTAINERS:
                t = getattr(pies, name)
                if F.count(t):
                    o.permute(t, F.order(t))
        return o

    def against_oracle(self, tag, F, O):
        for name in MOTION:
            a, b = getattr(F, name), getattr(O, name)
            d = float(np.abs(a - b).max())
            assert np.isfinite(a).all() and d <= TOL, (tag, name, d)
            if not F.count(self.pies.BEND):
                assert np.array_equal(a, b), (tag, name, d)

    def compare(self, tag, L, F, O, without=None, m=2):
        """m ticks of the live handle, the fresh one and its oracle, compared after each; `without`: a fresh handle that did not get
        the edit - it must differ from F after the first tick"""
        for t in range(m):
            for s in (L, F, O):
                s.tick()
            same_bits((tag, "live against fresh, tick %d" % t), L, F)
            self.against_oracle((tag, "fresh against oracle, tick %d" % t), F, O)
            if t == 0 and without is not None:
                without.tick()
                assert any_bit_differs(F, without), (tag, "the edit does not matter")
        assert not L.failed
        if self.expect_layer:
            assert L.launch_counts()["layer"] > 0 and F.launch_counts()["layer"] > 0
        if self.collisions:
            assert L.launch_counts()["collide"] > 0

    def live_and_state(self, k=2, build=None):
        """(L, S): the live handle after k ticks and the pre-edit state, taken from a twin"""
        L, T = self.handle(build), self.handle(build)
        L.tick(k)
        T.tick(k)
        S = state_of(T)
        T.close()
        return L, S


def case_of(pies, oracle, config, **kw):
    schedule, dims, substeps, collisions = CONFIGS[config]
    return Case(pies, oracle, schedule, dims, substeps, collisions, **kw)


# ---- 1. node-array writes, each alone ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", WRITES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_node_write(pies, oracle, config, what):
    c = case_of(pies, oracle, config, bend=what == "inv_masses" and not CONFIGS[config][3])
    L, S = c.live_and_state()
    after = dict(S)
    after[what] = node_edit(what, S, radius_factor=1.05 if c.collisions else 1.3)  # (1.05 x 0.475 stays below 0.5: no new verdict on the grid)
    getattr(L, "set_" + what)(after[what])
    F, without = c.fresh(after, rebuilt=False), c.fresh(S, rebuilt=False)
    if what == "prev_positions":  # (no later state can show it: module docstring) the host reads it back, the rest is untouched
        assert np.array_equal(L.prev_positions, after[what]) and not np.array_equal(after[what], S[what])
        same_bits((config, what, "after the write"), L, after)
        without = None
    c.compare((config, what), L, F, c.fresh_oracle(after, F), without)
    for name in ("radii", "inv_masses"):
        assert np.array_equal(getattr(L, name), after[name])
    if what == "inv_masses":  # the exported frame carries the new masses
        f = L.tick_begin()
        frame = np.array(L.export_acquire(f))
        L.export_release(f)
        assert np.array_equal(frame[:, 3], after[what])


def test_radius_write_flips_the_fast_verdict(pies, oracle):
    """Radii above 0.5 (grid spacing 2): a node's range spans more than two cells per axis, the group order is no longer possible
    and the scene is rebuilt for the reference's order - a fresh build with these radii decides the same, and the oracle runs
    rule 0."""
    c = case_of(pies, oracle, "layered-collisions", order=pies.COLLISION_ORDER_GROUPS)
    L, S = c.live_and_state()
    after = dict(S)
    after["radii"] = S["radii"].copy()
    after["radii"][::7] = 0.6
    L.set_radii(after["radii"])
    F = c.fresh(after)
    c.compare("radius flip", L, F, c.fresh_oracle(after, F, rule=0), c.fresh(S))


# ---- 2. rest data on a live handle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("container,config", [("DISTANCE", "layered-substeps"), ("TET", "layered-substeps"), ("BEND", "coloured")])
def test_set_rest_partial_range(pies, oracle, container, config):
    """pies_set_rest over constraints 5 .. 44 of a container (strain: 5 .. 12, bend: 2 .. 7 of 12).  Under schedule LAYERED the write brings rest sets the lattice did not
    have: the rest dictionary is rebuilt on the live handle and grows."""
    c = case_of(pies, oracle, config, bend=container == "BEND")
    t = getattr(pies, container)
    L, S = c.live_and_state()
    sets = L.count(pies.LAYER_REST_SETS)
    first, n = {"BEND": (2, 6), "TET": (5, 8), "DISTANCE": (5, 40)}[container]  # (8 new sets: the dictionary still fits in LDS)
    new = L.rest(t)[first:first + n].copy()  # (rest data: host-side, no node array is read)
    assert len(new) == n and first + n < L.count(t)
    new = new * np.linspace(0.9, 1.1, len(new), dtype=np.float32).reshape((-1,) + (1,) * (new.ndim - 1))

    def build(s):
        c.scene(s)
        s.set_rest(t, new, first=first)
    L.set_rest(t, new, first=first)
    F = c.fresh(S, build)
    assert np.array_equal(L.rest(t), F.rest(t)) and not np.array_equal(L.rest(t), c.handle().rest(t))
    c.compare(("set_rest", container), L, F, c.fresh_oracle(S, F, build), c.fresh(S))
    if container == "TET":
        assert sets > 0 and L.count(pies.LAYER_REST_SETS) > sets and F.count(pies.LAYER_REST_SETS) == L.count(pies.LAYER_REST_SETS)


# ---- 4. flags, orders and schedules flipped between ticks -------------------------------------------------------------------

def stretches(pies, oracle, cases, apply, ticks, rebuilt=True):
    """One live handle taken through cases[1:], starting as cases[0]: before each stretch the twin gives the state, apply(g, case)
    makes the edit on both, and the stretch is compared with a fresh build of its case; a fresh build of the case before it, given
    the same state, must end elsewhere."""
    L, T = cases[0].handle(), cases[0].handle()
    for g in (L, T):
        g.tick(2)
    for previous, case, m in zip(cases, cases[1:], ticks):
        S = state_of(T)
        for g in (L, T):
            apply(g, case)
        F = case.fresh(S, rebuilt=rebuilt)
        case.compare(("stretch", cases.index(case)), L, F, case.fresh_oracle(S, F), previous.fresh(S, rebuilt=rebuilt), m=m)
        T.tick(m)


def test_node_collisions_on_off_on(pies, oracle):
    cases = [Case(pies, oracle, "LAYERED", (4, 4, 15), collisions=on, radius=0.5) for on in (1, 0, 1)]
    stretches(pies, oracle, cases, lambda g, c: g.set_flag(pies.FLAG_NODE_COLLISIONS, c.collisions), (2, 2))


@pytest.mark.parametrize("schedule", ["LAYERED", "EXACT"])
def test_collision_order_changed(pies, oracle, schedule):
    """PIES_FLAG_COLLISION_ORDER from the schedule's default through the other two and back: same buffers, another resolve kernel
    in the captured substep.  Each stretch against a fresh build of that order."""
    orders = (None, 0, 1, 2) if schedule == "LAYERED" else (None, 1, 2, 0)  # (the default: 2 under LAYERED, 0 under EXACT)
    cases = [Case(pies, oracle, schedule, (4, 4, 15) if schedule == "LAYERED" else (4, 4, 8), collisions=1, order=o, radius=0.5) for o in orders]
    stretches(pies, oracle, cases, lambda g, c: g.set_flag(pies.FLAG_COLLISION_ORDER, c.order), (2, 1, 1), rebuilt=False)


def test_collision_rounds_changed(pies, oracle):
    """pies_set_collision_rounds on a live handle: three captured level launches where the order is deeper, the tail kernel
    finishes it - the same result as a fresh handle told so before its first finalize (and as the oracle, which has no rounds)"""
    p, v = scenes.loose_particles((4, 3, 4))

    def build(s):
        s.addNodes(p)
        s.set_velocities(v)
    c = Case(pies, oracle, "LAYERED", None, collisions=1)
    c.expect_layer = False  # (no constraints: nothing for the layered schedule to take)
    L, S = c.live_and_state(build=build)
    before = L.launch_counts()
    assert L.collision_pairs > 0  # (reading starts the count over: from here on the live handle counts what the fresh one counts)
    L.set_collision_rounds(3)
    F = c.fresh(S, build, rebuilt=False)
    F.set_collision_rounds(3)
    c.compare("rounds", L, F, c.fresh_oracle(S, F, build))
    assert L.launch_counts() == F.launch_counts() and L.launch_counts() != before  # the edit arrived: another captured sequence
    assert L.collision_pairs == F.collision_pairs > 0


def test_schedule_changed(pies, oracle):
    """LAYERED -> COLOURED -> EXACT on one handle, each stretch against a fresh build of that schedule"""
    cases = [Case(pies, oracle, name, (4, 4, 15), substeps=3) for name in ("LAYERED", "COLOURED", "EXACT")]
    stretches(pies, oracle, cases, lambda g, c: g.set_schedule(c.schedule), (2, 2))


# ---- 5. topology appended to a live scene -----------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["coloured", "layered-substeps", "layered-collisions"])
def test_second_body_appended(pies, oracle, config):
    c = case_of(pies, oracle, config)
    L, S = c.live_and_state()
    n_old = L.count(pies.NODES)

    def second(s):
        scenes.build_beam(s, (3, 3, 4), translation=(1.2, 5.2, 0.4) if c.collisions else (8.0, 0.6, 0.0), triangles=True)

    def build(s):
        c.scene(s)
        second(s)
    second(L)
    F = c.fresh(S, build)
    assert F.count(pies.NODES) == n_old + 36 and F.count(pies.TRIANGLES) > 0
    c.compare(("append", config), L, F, c.fresh_oracle(S, F, build))
    # the edit matters: the new body is there and moving
    assert L.count(pies.NODES) == n_old + 36 and not np.array_equal(L.positions[n_old:], c.handle(build).positions[n_old:])


# ---- 6. edits around work in flight -----------------------------------------------------------------------------------------

def flight_handle(pies, solver):
    if solver == "pd":
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=6))
        g.create_tet_box(3, 3, 6, translation=(0.0, 0.52, 0.0), w=20.0, volume=True, triangles=True)
        g.add_position(np.uint32([6 * (j + 3 * i) for i in range(3) for j in range(3)]), 2.0)
        scenes.perturb(g, 9, 0.08)
        g.set_prev_positions(g.positions)
    else:
        g = pies.Solver(scenes.pbd_options(pies, 4))
        g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
        scenes.build_beam(g, (4, 4, 15), translation=(0.0, 0.6, 0.0))
        scenes.perturb(g, 7, 0.05)
    return g


@pytest.mark.parametrize("solver", ["pbd", "pd"])
def test_write_behind_two_frames_in_flight(pies, solver):
    L, T = flight_handle(pies, solver), flight_handle(pies, solver)
    want = []
    for _ in range(2):
        T.tick()
        want.append(T.positions)
    V = T.velocities + np.float32([1.0, 0.0, 0.0])
    T.set_velocities(V)
    T.tick()
    want.append(T.positions)
    f1, f2 = L.tick_begin(), L.tick_begin()
    L.set_velocities(V)  # no synchronize, nothing acquired yet
    got = [np.array(L.export_acquire(f1))]
    L.export_release(f1)
    f3 = L.tick_begin()
    for f in (f2, f3):
        got.append(np.array(L.export_acquire(f)))
        L.export_release(f)
    for k in range(3):
        same_bits(("frame", k + 1), {"positions": got[k][:, :3].copy()}, {"positions": want[k]}, names=("positions",))
    same_bits("after the frames", L, T)
    U = flight_handle(pies, solver)  # the write matters: three ticks without it end elsewhere
    U.tick(3)
    assert any_bit_differs(U, T)


@pytest.mark.parametrize("solver", ["pbd", "pd"])
def test_write_behind_tick_async(pies, solver):
    L, T = flight_handle(pies, solver), flight_handle(pies, solver)
    T.tick(2)
    V = T.velocities + np.float32([1.0, 0.0, 0.0])
    T.set_velocities(V)
    L.tick_async(2)
    L.set_velocities(V)  # no synchronize in between
    for t in range(2):
        L.tick()
        T.tick()
        same_bits(("tick", t), L, T)
    U = flight_handle(pies, solver)
    U.tick(4)
    assert any_bit_differs(U, T)


@pytest.mark.parametrize("solver", ["pbd", "pd"])
def test_velocity_write_after_collide_props_keeps_the_pushes(pies, solver):
    """pies_collide_props moves positions on the device and marks the host mirrors stale; a velocity-only write behind it must bring
    them up to date before it uploads everything.  The twin reads all three arrays back and writes all three."""
    L, T = flight_handle(pies, solver), flight_handle(pies, solver)
    L.tick(2)
    T.tick(2)
    before = T.positions
    props = [pies.Prop.sphere(before[0].astype(np.float64) + [-0.25, 0.5, -0.125], 1.25, velocity=(0.5, -1.0, 0.25), friction=0.5)]
    hits_l = L.collide_props(props)[2]
    hits_t = T.collide_props(props)[2]
    V = np.tile(np.float32([0.3, -0.2, 0.1]), (len(before), 1))
    L.set_velocities(V)
    pos, prev = T.positions, T.prev_positions
    assert hits_l[0] == hits_t[0] >= 1 and not np.array_equal(pos, before)  # the prop pushed something
    T.set_positions(pos)
    T.set_prev_positions(prev)
    T.set_velocities(V)
    same_bits("after the writes", L, T)
    for t in range(2):
        L.tick()
        T.tick()
        same_bits(("tick", t), L, T)
