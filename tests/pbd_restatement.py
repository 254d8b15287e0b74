"""Shared by test_pbd_restatement.py (CPU oracle) and test_pbd_restatement_gpu.py (device): everything of a PBD substep that needs
neither an SVD nor an acos, restated in numpy float32 from the reference's own lines - Src/Solver.cpp:40-160 (tickPBD),
Src/Constraints.cpp:11-63 (distance and position projections), Include/Pies/Constraints.h:121-129 (pos += w * (projected - pos)) -
and the scene both sides are held to.  Nothing here is taken from pbd_project.h or pies_oracle.cpp.

The arithmetic is add, subtract, multiply, divide and sqrt on np.float32, each correctly rounded, in the source's order, with no
fused multiply-add: the comparison is exact equality, no tolerance.  Two things make that reach every launch form of the device:
  * a tetrahedral or bend constraint of weight 0 is an exact no-op (x += 0 * (projected - x)), so a body goes through colouring,
    tiles, the LDS rest dictionary and every colour step while the exact answer stays known;
  * with every radius 0 the node-node pass resolves nothing (disp = 0 + 0 - dist <= 0 skips every visit, a node's visit of itself
    included), so the launch forms the collision pass cuts can be checked too.
"""
import numpy as np

F = np.float32
ITERATIONS = 3
# Include/Pies/Solver.h:31-32: what an option set that does not name them runs with
REFERENCE_DEFAULTS = dict(damping=0.006, friction=0.01)
OPTION_SETS = {
    "A": dict(fixedTimestepSize=0.012, timeSubsteps=1, gravity=10.0, floorHeight=0.0),
    "B": dict(fixedTimestepSize=0.02, timeSubsteps=3, gravity=7.3, damping=0.13, friction=0.37, floorHeight=0.3),
    "C": dict(fixedTimestepSize=0.016, timeSubsteps=2, gravity=0.0, damping=0.0, friction=1.0, floorHeight=-1.7),
    # Under A, B and C ((-g * dt) * dt) and (-g * (dt * dt)) are the same float, so they cannot tell the source's grouping of the
    # gravity term from the other.  Under D the two differ by one unit in the last place, and the floor lies below the row of nodes
    # that start at rest within 1e-3 of y = 0, where that unit survives the sum with the position (test_teeth asserts both).
    "D": dict(fixedTimestepSize=0.02, timeSubsteps=3, gravity=9.81, damping=0.13, friction=0.37, floorHeight=-1.7),
}
BEAM = (4, 5, 17)
PINS = (3, 3, 40, 119, 7)  # node 3 twice
PIN_W, BOX_W, LOOSE_W = 0.3, 0.5, 0.4
THRESHOLD_ROW = 65
MOTION = ("positions", "prev_positions", "velocities")


def solver_options(mod, name, iterations=ITERATIONS):
    """The option set as the Options of a binding (oracle_api or pies_amd.capi); damping and friction stay the binding's defaults
    where the set does not name them"""
    return mod.Options(solver=mod.PBD, iterations=iterations, **OPTION_SETS[name])


def option_values(name, iterations=ITERATIONS):
    o = dict(REFERENCE_DEFAULTS)
    o.update(OPTION_SETS[name])
    o["iterations"] = iterations
    return o


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def new_tally():
    return dict(clamps=0, clamped=set(), touching=set(), zeroed=set(), scaled=set(), at_five=[], fallbacks=0,
                clamped_reads_above=set(), clamped_reads_below=set(), clamped_reads_equal=set())


def tick(state, radii, opt, pins, dists, pin_order, dist_order, hinge, tally=None):
    """One Solver::tickPBD of a scene without node-node contacts whose tetrahedral and bend constraints weigh 0.
    state: (pos, prev, vel) float32 n x 3;  pins: [(id, target[3], w)];  dists: [(a, b, rest, w)];  pin_order / dist_order: the order
    each container is swept in (indices into pins / dists);  hinge: Solver::releaseHinge.
    Returns (pos, prev, vel); adds the decisions it took to `tally` (new_tally()), node ids in sets."""
    tally = new_tally() if tally is None else tally
    pos, prev, vel = (np.array(a, dtype=F) for a in state)
    radii = np.asarray(radii, dtype=F)
    one, five, eps = F(1.0), F(5.0), F(0.00001)
    floor, g = F(opt["floorHeight"]), F(opt["gravity"])
    dt = F(opt["fixedTimestepSize"]) / F(opt["timeSubsteps"])          # Solver.cpp:41-42 (uint32 -> float, then one division)
    zero = F(0.0)
    gravity = np.array([(zero * dt) * dt, (-g * dt) * dt, (zero * dt) * dt], dtype=F)  # vec3(0, -g, 0) * dt * dt, left to right
    k = one - F(opt["damping"])
    slip = one - F(opt["friction"])
    pins = [(int(i), [F(t[0]), F(t[1]), F(t[2])], F(w)) for i, t, w in pins]
    dists = [(int(a), int(b), F(rest), F(w)) for a, b, rest, w in dists]
    with np.errstate(all="ignore"):
        for _ in range(int(opt["timeSubsteps"])):
            prev = pos.copy()                                           # :48
            pos = pos + (vel * dt + gravity)                            # :49-51
            clamped = np.zeros(len(pos), dtype=bool)
            for _ in range(int(opt["iterations"])):
                X = [list(pos[:, 0]), list(pos[:, 1]), list(pos[:, 2])]  # np.float32 scalars: the Gauss-Seidel sweeps
                if not hinge:                                           # :59-63
                    for c in pin_order:
                        i, t, w = pins[c]
                        for a in range(3):
                            X[a][i] = X[a][i] + w * (t[a] - X[a][i])    # Constraints.cpp:62, Constraints.h:127
                for c in dist_order:                                    # :65-67, Constraints.cpp:15-34
                    a, b, rest, w = dists[c]
                    dx, dy, dz = X[0][b] - X[0][a], X[1][b] - X[1][a], X[2][b] - X[2][a]
                    dist = np.sqrt(dx * dx + dy * dy + dz * dz)          # glm::length: the products summed left to right
                    if dist > eps:
                        ux, uy, uz = dx / dist, dy / dist, dz / dist
                    else:
                        ux, uy, uz = one, zero, zero
                        tally["fallbacks"] += 1
                    nd = -(rest - dist)                                 # -disp
                    px, py, pz = X[0][a] + nd * ux, X[1][a] + nd * uy, X[2][a] + nd * uz
                    X[0][a] = X[0][a] + w * (px - X[0][a])              # node a alone moves (b: += w * (b - b))
                    X[1][a] = X[1][a] + w * (py - X[1][a])
                    X[2][a] = X[2][a] + w * (pz - X[2][a])
                pos = np.stack([np.array(X[0], dtype=F), np.array(X[1], dtype=F), np.array(X[2], dtype=F)], axis=1)
                below = pos[:, 1] - radii < floor                       # :132-136
                pos[below, 1] = floor + radii[below]
                clamped |= below
                tally["clamps"] += int(below.sum())
                tally["clamped"].update(np.nonzero(below)[0].tolist())
            vel = (k * (pos - prev)) / dt                               # :143-144
            reads = pos[:, 1] - radii
            on = reads <= floor                                         # :147
            speed = np.sqrt(vel[:, 0] * vel[:, 0] + vel[:, 2] * vel[:, 2])  # glm::length(vec2(x, z))
            slow = on & (speed < five)                                  # :148-150
            fast = on & ~(speed < five)                                 # :151-154
            vel[slow, 0] = zero
            vel[slow, 2] = zero
            vel[fast, 0] = vel[fast, 0] * slip
            vel[fast, 2] = vel[fast, 2] * slip
            ids = lambda mask: np.nonzero(mask)[0].tolist()  # noqa: E731
            tally["touching"].update(ids(on & ~(reads < floor)))        # `<=` true, `<` false
            tally["zeroed"].update(ids(slow))
            tally["scaled"].update(ids(fast))
            tally["at_five"] += [(i, bool(fast[i])) for i in ids(on & (speed == five))]
            rests = clamped & (pos[:, 1] == floor + radii)             # still where a clamp of this substep put it
            tally["clamped_reads_above"].update(ids(rests & ~on))       # ... and skips friction: fl(fl(floor + r) - r) > floor
            tally["clamped_reads_below"].update(ids(rests & (reads < floor)))
            tally["clamped_reads_equal"].update(ids(rests & (reads == floor)))
    return pos, prev, vel


def tally_counts(t):
    return {name: (len(v) if isinstance(v, (set, list)) else v) for name, v in t.items()}


# ---- the scene ------------------------------------------------------------------------------------------------------------------

def _length(d):
    d = np.asarray(d, dtype=F)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def _reads_on_the_floor(floor, r):
    """fl(fl(floor + r) - r) == floor: a node put down at floor + r is found there again"""
    floor, r = F(floor), np.asarray(r, dtype=F)
    return (floor + r) - r == floor


def _horizontal(rng, n, lo, hi):
    """n horizontal velocities of speed lo .. hi with both components within +-12"""
    out = np.zeros((n, 2))
    for i in range(n):
        while True:
            s, a = rng.uniform(lo, hi), rng.uniform(0.0, 2.0 * np.pi)
            v = s * np.cos(a), s * np.sin(a)
            if max(abs(v[0]), abs(v[1])) <= 12.0:
                out[i] = v
                break
    return out


class Scene:
    """What build() handed to a solver, as the restatement's inputs.  rows: name -> node ids of a class of loose nodes."""

    def __init__(self, name, iterations, positions, velocities, radii, pins, dists, rows):
        self.name, self.opt = name, option_values(name, iterations)
        self.positions, self.velocities, self.radii = positions, velocities, radii
        self.pins, self.dists, self.rows = pins, dists, rows

    def start(self):
        return self.positions.copy(), self.positions.copy(), self.velocities.copy()

    def tick(self, state, pin_order=None, dist_order=None, hinge=False, tally=None):
        pin_order = range(len(self.pins)) if pin_order is None else [int(c) for c in pin_order]
        dist_order = range(len(self.dists)) if dist_order is None else [int(c) for c in dist_order]
        return tick(state, self.radii, self.opt, self.pins, self.dists, pin_order, dist_order, hinge, tally)


def build(s, mod, name, iterations=ITERATIONS, zero_radii=False, seed=2024):
    """The scene, by the same calls on an oracle or a device solver `s` of binding `mod` made with solver_options(mod, name):
    a 4 x 5 x 17 beam whose tetrahedra weigh 0, the box's distance constraints over it at 0.5, five pins (node 3 twice), about 300
    loose nodes of every floor class, and loose distance constraints at the projection's edges.  Returns the Scene."""
    opt = option_values(name, iterations)
    floor = F(opt["floorHeight"])
    rng = np.random.default_rng(seed)
    W, H, D = BEAM
    first = s.count(mod.NODES)
    assert first == 0
    s.create_tet_box(W, H, D, translation=(0.0, float(floor) + 0.9, 0.0), w=0.0, volume=False, triangles=False)
    s.create_box(W, H, D, w=BOX_W, existing_offset=first, triangles=False)
    lattice = s.positions
    nb = len(lattice)
    assert nb == W * H * D

    def radii_of(n, on_floor_exactly=False):
        if zero_radii:
            return np.zeros(n, dtype=F)
        r = rng.uniform(0.2, 0.9, n).astype(F)
        while on_floor_exactly and not _reads_on_the_floor(floor, r).all():  # (the threshold row: every node must take the friction branch)
            bad = ~_reads_on_the_floor(floor, r)
            r[bad] = rng.uniform(0.2, 0.9, int(bad.sum())).astype(F)
        return r

    def vertical(n):
        return rng.uniform(-6.0, 2.0, n)

    blocks, rows = [], {}  # (creation position, final position, velocity, radius) per class of loose nodes

    def block(tag, p, v, r, created=None):
        p, v, r = np.asarray(p, dtype=F), np.asarray(v, dtype=F), np.asarray(r, dtype=F)
        at = nb + sum(len(b[0]) for b in blocks)
        rows[tag] = np.arange(at, at + len(p))
        blocks.append((p if created is None else np.asarray(created, dtype=F), p, v, r))

    def spread(n, x0):
        return np.stack([x0 + rng.uniform(0.0, 6.0, n), np.zeros(n), rng.uniform(0.0, 16.0, n)], axis=1)

    def on_floor(n, r, sunk):
        """n nodes resting on the floor (y = fl(floor + r)); every second one starts up to `sunk` below it"""
        y = (floor + r).astype(F)
        y[1::2] = (y[1::2] - rng.uniform(0.0, sunk, len(y[1::2])).astype(F)).astype(F)
        return y

    n = 60  # airborne
    r = radii_of(n)
    p = spread(n, 6.0)
    p[:, 1] = float(floor) + r + rng.uniform(1.0, 4.0, n)
    block("airborne", p, np.stack([rng.uniform(-12, 12, n), vertical(n), rng.uniform(-12, 12, n)], axis=1), r)
    n = 40  # below the floor, some with their centre below it
    r = radii_of(n)
    p = spread(n, 13.0)
    p[:, 1] = float(floor) + r - rng.uniform(0.05, 1.2, n)
    block("below", p, np.stack([rng.uniform(-12, 12, n), vertical(n), rng.uniform(-12, 12, n)], axis=1), r)
    n = 40  # exactly touching, at rest vertically
    r = radii_of(n)
    p = spread(n, 20.0).astype(F)
    p[:, 1] = floor + r
    block("touching", p, np.stack([rng.uniform(-12, 12, n), np.zeros(n), rng.uniform(-12, 12, n)], axis=1), r)
    n = 50  # on the floor and fast
    r = radii_of(n)
    p = spread(n, 27.0).astype(F)
    p[:, 1] = on_floor(n, r, 0.1)
    h = _horizontal(rng, n, 6.0, 15.0)
    block("fast", p, np.stack([h[:, 0], np.zeros(n), h[:, 1]], axis=1), r)
    n = 40  # on the floor and slow
    r = radii_of(n)
    p = spread(n, 34.0).astype(F)
    p[:, 1] = on_floor(n, r, 0.1)
    h = _horizontal(rng, n, 0.5, 4.5)
    block("slow", p, np.stack([h[:, 0], np.zeros(n), h[:, 1]], axis=1), r)
    n = 12  # at rest within 1e-3 of y = 0: airborne where the floor lies below -0.9, below it elsewhere
    p = spread(n, 41.0)
    p[:, 1] = rng.uniform(1.0e-5, 1.0e-3, n) * np.where(np.arange(n) % 2, -1.0, 1.0)
    block("near_zero", p, np.zeros((n, 3)), radii_of(n))
    # the threshold row: at x = z = 0 with vz = 0, vx the 65 consecutive floats centred on 5 / (1 - damping)
    n = THRESHOLD_ROW
    r = radii_of(n, on_floor_exactly=True)
    p = np.zeros((n, 3), dtype=F)
    p[:, 1] = floor + r
    centre = F(5.0) / (F(1.0) - F(opt["damping"]))
    vx = (np.array([centre]).view(np.int32)[0] + np.arange(-(n // 2), n // 2 + 1, dtype=np.int32)).astype(np.int32).view(F)
    v = np.zeros((n, 3), dtype=F)
    v[:, 0] = vx
    block("threshold", p, v, r)
    # the ends of the loose distance constraints (a, b): two coincident pairs (created 0.5 and 0.25 apart: the fallback direction
    # with something to correct), a pair 3e-5 apart, a pair 2e4 apart (both with a rest length within 10 % of the separation), and a pair
    # one of whose differences is far smaller than the others (5e-13 against 0.7)
    y = float(floor) + 3.0
    final = np.array([[50.0, y, 2.0], [50.0, y, 2.0],
                      [45.5, y + 0.5, 3.0], [45.5, y + 0.5, 3.0],
                      [0.5, y, 40.0], [0.50003, y, 40.0],
                      [48.0, y + 1.0, 5.0], [48.0, y + 1.0, 5.0 + 2.0e4],
                      [0.0, y + 2.0, 30.0], [5.0e-13, y + 2.0, 30.7]])
    created = final.copy()
    created[1] += [0.5, 0.0, 0.0]
    created[3] += [0.0, 0.25, 0.0]
    created[5, 0] = 0.500032
    created[7, 2] = 5.0 + 2.1e4
    created[9, 2] = 30.65
    v = np.stack([rng.uniform(-12, 12, 10), rng.uniform(-6, 2, 10), rng.uniform(-12, 12, 10)], axis=1)
    v[[0, 2, 4]] = v[[1, 3, 5]]    # the coincident pairs stay coincident through the predict step, the close pair close
    v[8:10, 0] = 0.0               # (the tiny difference in x survives it)
    block("pair_ends", final, v, radii_of(10), created=created)

    created = np.concatenate([b[0] for b in blocks])
    s.add_nodes_raw(created, vel=np.concatenate([b[2] for b in blocks]), radius=np.concatenate([b[3] for b in blocks]))
    e = rows["pair_ends"]
    loose = np.array([[e[0], e[1]], [e[2], e[3]], [e[4], e[5]], [e[6], e[7]], [e[9], e[8]]], dtype=np.uint32)
    s.add_distance(loose, LOOSE_W)

    # rest lengths: glm::length of the difference at the time of the call (Constraints.cpp:54), from this module's own arithmetic
    ids = s.ids(mod.DISTANCE).astype(np.int64)
    at_call = np.concatenate([lattice, created.astype(F)])
    rest = _length(at_call[ids[:, 1]] - at_call[ids[:, 0]])
    nbox = len(ids) - len(loose)
    assert np.array_equal(ids[nbox:], loose.astype(np.int64))
    weights = np.concatenate([np.full(nbox, BOX_W), np.full(len(loose), LOOSE_W)]).astype(F)
    dists = [(int(a), int(b), rt, w) for (a, b), rt, w in zip(ids, rest, weights)]

    positions = np.concatenate([lattice + rng.uniform(-0.05, 0.05, lattice.shape).astype(F), np.concatenate([b[1] for b in blocks])]).astype(F)
    velocities = np.concatenate([np.stack([rng.uniform(-12, 12, nb), vertical(nb), rng.uniform(-12, 12, nb)], axis=1),
                                 np.concatenate([b[2] for b in blocks])]).astype(F)
    radii = np.concatenate([radii_of(nb), np.concatenate([b[3] for b in blocks])]).astype(F)
    s.set_positions(positions)
    s.add_position(np.array(PINS, dtype=np.uint32), PIN_W)  # targets: the positions at the time of the call
    s.set_radii(radii)
    s.set_velocities(velocities)
    s.set_prev_positions(positions)
    pins = [(i, positions[i].copy(), PIN_W) for i in PINS]
    return Scene(name, iterations, positions, velocities, radii, pins, dists, rows)


def assert_same(tag, solver, state):
    """positions, previous positions and velocities of a solver against the restatement's: finite, and equal as floats (array_equal:
    a zero of either sign equals the other, which is intended - x + 0 * (...) may change the sign of a zero)"""
    for name, want in zip(MOTION, state):
        got = getattr(solver, name)
        assert np.isfinite(got).all() and np.isfinite(want).all(), (tag, name)
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).any(axis=1))[0]
            raise AssertionError((tag, name, "%d nodes differ, first %s: %s against %s" % (len(bad), bad[:8].tolist(), got[bad[0]], want[bad[0]])))
