"""CPU tests of pies_add_anchors / pies_get_anchors / pies_apply_anchors: the numpy fp32 restatement of the rule of
include/pies_hip.h (`apply_anchors`, the yardstick the device has to match bit for bit in tests/test_anchors_gpu.py), an independent
fp64 formulation it is held to, physics checks on that formulation, and the argument checks of the three entry points on a
host-only handle."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi
from test_forces import _cross, _dot, _vec

F = np.float32
TILE = 256
DT = F(0.015625)

# branch codes of one anchor (apply_anchors(..., trace=[])): what the GPU test asserts the coverage of
A_FIXED, A_RELEASED, A_SPRING, A_PIN = 0, 1, 2, 3  # invMass 0; the frame's strength 0; a live spring; a live pin


# ---- the restatement: fp32, no fused multiply-adds, the operation order of the header --------------------------------------------
def _target(f, local, p):
    """(t, t - pivot, u, x, stretch) of an anchor at `local` of frame f for a node at p"""
    axes = np.array(list(f.axes), F).reshape(3, 3)
    t = ((_vec(f.origin) + axes[0] * F(local[0])) + axes[1] * F(local[1])) + axes[2] * F(local[2])
    arm = t - _vec(f.pivot)
    u = _vec(f.velocity) + _cross(_vec(f.angular), arm)
    x = p - t
    return t, arm, u, x, np.sqrt(_dot(x, x))


def rows_of(anchors, n_nodes):
    """per node the indices of its anchors, ascending"""
    rows = [[] for _ in range(n_nodes)]
    for i, a in enumerate(anchors):
        rows[a.node].append(i)
    return rows


def apply_anchors(pos, vel, inv_mass, anchors, frames, dt, prev=None, trace=None):
    """The rule of pies_apply_anchors in numpy fp32.  Returns (pos, prev, vel, impulse, torque, live, per_anchor): the node state
    after the call (prev None: the previous positions the call finds are the positions), the sums per frame in the fixed order -
    per tile of 256 anchor indices in ascending index from 0, then the tiles in ascending index from 0 -, the live counts and the
    (n, 4) array of j and stretch.  trace: a list that receives the branch code of every anchor."""
    with np.errstate(all="ignore"):
        pos, vel = (np.array(a, F).reshape(-1, 3).copy() for a in (pos, vel))
        prev = pos.copy() if prev is None else np.array(prev, F).reshape(-1, 3).copy()
        w_all = np.asarray(inv_mass, F).reshape(-1)
        h = F(dt)
        n, k = len(anchors), len(frames)
        J, T = np.zeros((n, 3), F), np.zeros((n, 3), F)
        stretch, live = np.zeros(n, F), np.zeros(n, bool)
        codes = np.zeros(n, np.int64)
        out_pos, out_prev, out_vel = pos.copy(), prev.copy(), vel.copy()
        for node, row in enumerate(rows_of(anchors, len(pos))):
            if not row:
                continue
            p, v, w = pos[node], vel[node], w_all[node]
            targets = {i: _target(frames[anchors[i].frame], anchors[i].local, p) for i in row}
            springs = []
            for i in row:
                a, f = anchors[i], frames[anchors[i].frame]
                stretch[i] = targets[i][4]
                live[i] = bool(w > 0) and bool(F(f.strength) > 0)
                codes[i] = (A_PIN if a.flags & capi.ANCHOR_PIN else A_SPRING) if live[i] else (A_RELEASED if w > 0 else A_FIXED)
                if live[i] and not a.flags & capi.ANCHOR_PIN:
                    springs.append(i)
            A, G, terms = F(0), np.zeros(3, F), {}
            for i in springs:
                a, strength = anchors[i], F(frames[anchors[i].frame].strength)
                t, arm, u, x, _ = targets[i]
                kk, cc = F(a.stiffness) * strength, F(a.damping) * strength
                ai = cc + kk * h
                gi = x * kk + (v - u) * ai
                A, G = A + ai, G + gi
                terms[i] = (ai, gi)
            if springs:
                hw = h * w
                e = -((G * hw) / (F(1) + hw * A))
                out_vel[node] = v + e
                for i in springs:
                    ai, gi = terms[i]
                    J[i] = (gi + e * ai) * (-h)
            for i in row:
                if live[i] and anchors[i].flags & capi.ANCHOR_PIN:
                    t, arm, u, x, _ = targets[i]
                    out_pos[node], out_prev[node], out_vel[node] = t, t, u
                    J[i] = (u - v) * (F(1) / w)
                if live[i]:
                    T[i] = _cross(targets[i][1], J[i])
        frame_of = np.array([a.frame for a in anchors], np.int64)
        mine = (frame_of[None, :] == np.arange(k)[:, None])  # k x n
        impulse, torque = np.zeros((k, 3), F), np.zeros((k, 3), F)
        for first in range(0, n, TILE):
            si, st = np.zeros((k, 3), F), np.zeros((k, 3), F)
            for i in range(first, min(first + TILE, n)):
                si = si + np.where(mine[:, i, None], J[i][None], F(0))  # (another frame's anchor adds 0)
                st = st + np.where(mine[:, i, None], T[i][None], F(0))
            impulse, torque = impulse + si, torque + st
        counts = (mine & live[None]).sum(axis=1).astype(np.uint32)
        if trace is not None:
            trace.extend(codes.tolist())
        return out_pos, out_prev, out_vel, impulse, torque, counts, np.concatenate([J, stretch[:, None]], axis=1).astype(F)


# ---- an independent fp64 formulation: (m + h A) e = -h G per node, pins and sums formed directly ------------------------------------
def _frame64(f):
    g = lambda a: np.array(list(a), np.float64)
    return g(f.origin), g(f.axes).reshape(3, 3), g(f.velocity), g(f.angular), g(f.pivot), float(f.strength)


def apply_anchors_f64(pos, vel, inv_mass, anchors, frames, dt):
    """Returns (pos, prev, vel, impulse, torque, live (n) bool, per_anchor (n, 4))."""
    x0, v0 = np.array(pos, np.float64).reshape(-1, 3), np.array(vel, np.float64).reshape(-1, 3)
    w = np.asarray(inv_mass, np.float64).reshape(-1)
    h = float(dt)
    n, k = len(anchors), len(frames)
    fr = [_frame64(f) for f in frames]
    node = np.array([a.node for a in anchors], np.int64)
    frame = np.array([a.frame for a in anchors], np.int64)
    local = np.array([list(a.local) for a in anchors], np.float64).reshape(n, 3)
    pin = np.array([bool(a.flags & capi.ANCHOR_PIN) for a in anchors])
    strength = np.array([fr[f][5] for f in frame])
    kk = np.array([a.stiffness for a in anchors], np.float64) * strength
    cc = np.array([a.damping for a in anchors], np.float64) * strength
    t = np.array([fr[f][0] + local[i] @ fr[f][1] for i, f in enumerate(frame)]).reshape(n, 3)
    pivot = np.array([fr[f][4] for f in frame]).reshape(n, 3)
    u = np.array([fr[f][2] + np.cross(fr[f][3], t[i] - fr[f][4]) for i, f in enumerate(frame)]).reshape(n, 3)
    live = (w[node] > 0) & (strength > 0)
    spring = live & ~pin
    mass = np.where(w > 0, 1.0 / np.where(w > 0, w, 1.0), 0.0)
    # the node's system: (m + h sum(c + k h)) e = -h sum(k x + (c + k h)(v - u))
    a = cc + kk * h
    A, G = np.zeros(len(x0)), np.zeros((len(x0), 3))
    np.add.at(A, node[spring], a[spring])
    np.add.at(G, node[spring], kk[spring, None] * (x0[node[spring]] - t[spring]) + a[spring, None] * (v0[node[spring]] - u[spring]))
    held = np.zeros(len(x0), bool)
    held[node[spring]] = True
    e = np.zeros_like(v0)
    e[held] = -h * G[held] / (mass[held] + h * A[held])[:, None]
    v1, x1, prev1 = v0 + e, x0.copy(), x0.copy()
    # what the spring pulled with over the step, at the end-of-step state
    end = (x0[node] - t) + h * (v1[node] - u)
    j = np.where(spring[:, None], -h * (kk[:, None] * end + cc[:, None] * (v1[node] - u)), 0.0)
    pinned = live & pin
    x1[node[pinned]], prev1[node[pinned]], v1[node[pinned]] = t[pinned], t[pinned], u[pinned]
    j[pinned] = (u[pinned] - v0[node[pinned]]) * mass[node[pinned]][:, None]
    tq = np.cross(t - pivot, j)
    impulse, torque = np.zeros((k, 3)), np.zeros((k, 3))
    np.add.at(impulse, frame, j)
    np.add.at(torque, frame, tq)
    stretch = np.linalg.norm(x0[node] - t, axis=1)
    return x1, prev1, v1, impulse, torque, live, np.concatenate([j, stretch[:, None]], axis=1)


# ---- test scenes (shared with tests/test_anchors_gpu.py) ----------------------------------------------------------------------------
HUB_ANCHORS = 40
STRENGTHS = (0.125, 0.5, 1.0, 2.5)  # a strength is exactly 0 or >= 2^-3: no `live` decision sits on a rounding edge


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[2] = -q[2]
    return q


def make_frames(n_frames, seed=0):
    """frame 0 rotates about a pivot away from its origin; with three and more frames, frame 1 is released (strength 0); one
    frame in four spins"""
    rng = np.random.default_rng(4000 + seed * 97 + n_frames)
    out = []
    for k in range(n_frames):
        origin = np.round(rng.uniform(-2, 2, 3) * 16) / 16
        spins = k % 4 == 0
        f = capi.AnchorFrame.make(origin, _rotation(rng), velocity=rng.normal(size=3), angular=rng.normal(size=3) * 2 if spins else (0, 0, 0),
                                  pivot=origin + np.round(rng.uniform(-1, 1, 3) * 8) / 8 if spins else None,
                                  strength=0.0 if (k == 1 and n_frames >= 3) else STRENGTHS[k % 4])
        out.append(f)
    return out


def make_scene(n_nodes, n_anchors, n_frames, seed=0):
    """(pos, vel, inv_mass, anchors, frames, marks): loose nodes, invMass in {0, 0.25, 0.5, 1, 2}, and a set listed in shuffled node
    order.  When the sizes allow it (marks is then not empty): a hub with 40 springs across several frames, one node with exactly
    one and one with exactly two springs, four pinned nodes - a live one on the rotating frame 0, one on the released frame 1, one
    with invMass 0, one more live -, a spring on a node with invMass 0, and nodes that carry nothing."""
    rng = np.random.default_rng(seed * 7919 + n_nodes * 31 + n_anchors * 7 + n_frames)
    frames = make_frames(n_frames, seed)
    pos = rng.uniform(-3, 3, (n_nodes, 3)).astype(F)
    vel = (rng.normal(size=(n_nodes, 3)) * 2).astype(F)
    inv_mass = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], F), n_nodes)

    def spring(node, frame):
        return capi.Anchor.make(node, frame, rng.uniform(-1, 1, 3), stiffness=float(F(rng.uniform(1.0, 2000.0))),
                                damping=float(F(rng.choice([0.0, rng.uniform(0.0, 20.0)]))))

    anchors, marks = [], {}
    free = list(range(n_nodes))
    if n_nodes >= 63 and n_anchors >= 255:
        hub, one, two, fixed, bare = 5, 6, 7, 8, 9
        pins = [10, 11, 12, 13]
        marks = dict(hub=hub, one=one, two=two, fixed=fixed, pins=pins, bare=list(range(14, 14 + n_nodes // 8)))
        inv_mass[[hub, one, two, pins[0], pins[1], pins[3]]] = F(1), F(0.5), F(2), F(1), F(0.5), F(0.25)
        inv_mass[[fixed, pins[2]]] = F(0)
        anchors += [spring(hub, j % n_frames) for j in range(HUB_ANCHORS)]
        anchors += [spring(one, n_frames - 1), spring(two, 0), spring(two, n_frames - 1), spring(fixed, 0)]
        pin_frames = [0, 1 if n_frames >= 3 else 0, 0, n_frames - 1]
        anchors += [capi.Anchor.make(node, f, rng.uniform(-1, 1, 3), pin=True) for node, f in zip(pins, pin_frames)]
        free = list(range(14 + n_nodes // 8, n_nodes))
    while len(anchors) < n_anchors:
        anchors.append(spring(int(rng.choice(free)), int(rng.integers(n_frames))))
    anchors = [anchors[i] for i in rng.permutation(len(anchors))]
    return pos, vel, inv_mass, anchors, frames, marks


def required_branches(n_frames):
    return {A_FIXED, A_SPRING, A_PIN} | ({A_RELEASED} if n_frames >= 3 else set())


def check_marks(anchors, frames, inv_mass, marks, trace):
    """the scene holds what make_scene promises (with marks)"""
    rows = rows_of(anchors, len(inv_mass))
    assert len(rows[marks["hub"]]) == HUB_ANCHORS and len({anchors[i].frame for i in rows[marks["hub"]]}) == min(len(frames), HUB_ANCHORS)
    assert len(rows[marks["one"]]) == 1 and len(rows[marks["two"]]) == 2 and all(not rows[b] for b in marks["bare"])
    assert trace[rows[marks["fixed"]][0]] == A_FIXED
    pin_codes = [trace[rows[p][0]] for p in marks["pins"]]
    assert all(len(rows[p]) == 1 for p in marks["pins"])
    assert pin_codes == [A_PIN, A_RELEASED if len(frames) >= 3 else A_PIN, A_FIXED, A_PIN]
    assert any(frames[0].angular) and set(trace) == required_branches(len(frames))


GPU_SCENES = [(600, 255, 3), (600, 700, 64), (257, 700, 3), (255, 257, 64), (63, 255, 1)]


def test_every_branch_occurs_in_the_shared_scenes():
    for n_nodes, n_anchors, n_frames in GPU_SCENES:
        pos, vel, inv_mass, anchors, frames, marks = make_scene(n_nodes, n_anchors, n_frames)
        assert len(anchors) == n_anchors and marks
        trace = []
        out = apply_anchors(pos, vel, inv_mass, anchors, frames, DT, trace=trace)
        check_marks(anchors, frames, inv_mass, marks, trace)
        assert [a.node for a in anchors] != sorted(a.node for a in anchors)  # shuffled
        moved = (out[0].view(np.uint32) != pos.view(np.uint32)).any(axis=1)
        live_pins = [p for p, i in ((p, rows_of(anchors, n_nodes)[p][0]) for p in marks["pins"]) if trace[i] == A_PIN]
        assert sorted(np.nonzero(moved)[0].tolist()) == sorted(live_pins)
        assert out[5].sum() == sum(c in (A_SPRING, A_PIN) for c in trace) and (out[6][:, 3] > 0).all()


# ---- restatement against fp64 --------------------------------------------------------------------------------------------------------
# Measured on the scenes below (the GPU tests' scenes): see test_restatement_against_fp64.  Each gate is the next power of two above
# the measured figure.
GATE_VEL_ULP = 4.0
GATE_SUM = 2.0 ** -20
GATE_POS_ULP = 2.0
GATE_ANCHOR = 2.0 ** -22


def _deviation(pos, vel, inv_mass, anchors, frames):
    trace = []
    r = apply_anchors(pos, vel, inv_mass, anchors, frames, DT, trace=trace)
    d = apply_anchors_f64(pos, vel, inv_mass, anchors, frames, DT)
    live32 = np.array([c in (A_SPRING, A_PIN) for c in trace])
    excluded = int((live32 != d[5]).sum())
    speed = max(np.abs(d[2]).max(), np.abs(np.asarray(vel, np.float64)).max())
    ulp = float(np.spacing(F(speed)))
    dev_vel = np.abs(r[2] - d[2]).max() / ulp
    dev_sum = max(np.abs(r[3] - d[3]).max() / np.abs(d[3]).max(), np.abs(r[4] - d[4]).max() / np.abs(d[4]).max())
    dev_pos = max(np.abs(r[0] - d[0]).max(), np.abs(r[1] - d[1]).max()) / float(np.spacing(F(np.abs(d[0]).max())))
    dev_anchor = np.abs(r[6] - d[6]).max() / np.abs(d[6]).max()
    return excluded, dev_vel, dev_sum, dev_pos, dev_anchor


def test_restatement_against_fp64():
    """The fp32 restatement against the fp64 solve of (m + h A) e = -h G on the scenes the GPU tests use.  Strengths are exactly 0
    or at least 2^-3 and invMass exactly 0 or at least 0.25, so no `live` decision differs for any (node, anchor) pair: the count
    of excluded pairs is asserted to be 0.  Measured: velocities deviate by at most 2.44 ulp of the scene's largest speed, the
    per-frame sums of impulse and torque by at most 4.84e-7 of the largest component of the largest sum; the gates are the next
    powers of two above, 4 ulp and 2^-20.  Beside what was asked for: pinned positions deviate by at most 1.21 ulp of the scene's
    largest coordinate (gate 2 ulp) and the per-anchor array by at most 2.31e-7 of its largest entry (gate 2^-22)."""
    worst_vel, worst_sum, worst_pos, worst_anchor = 0.0, 0.0, 0.0, 0.0
    for n_nodes, n_anchors, n_frames in GPU_SCENES:
        pos, vel, inv_mass, anchors, frames, _ = make_scene(n_nodes, n_anchors, n_frames)
        excluded, dev_vel, dev_sum, dev_pos, dev_anchor = _deviation(pos, vel, inv_mass, anchors, frames)
        assert excluded == 0
        worst_vel, worst_sum = max(worst_vel, dev_vel), max(worst_sum, dev_sum)
        worst_pos, worst_anchor = max(worst_pos, dev_pos), max(worst_anchor, dev_anchor)
    print("restatement vs fp64: velocities %.3g ulp of the largest speed; sums %.3g relative; pinned positions %.3g ulp; per anchor %.3g"
          % (worst_vel, worst_sum, worst_pos, worst_anchor))
    assert worst_vel <= GATE_VEL_ULP and worst_sum <= GATE_SUM
    assert worst_pos <= GATE_POS_ULP and worst_anchor <= GATE_ANCHOR


# ---- physics on the fp64 form ------------------------------------------------------------------------------------------------------
def _still_frame(**kw):
    return capi.AnchorFrame.make((0.0, 0.0, 0.0), **kw)


@pytest.mark.parametrize("kdt2", [1e-3, 1.0, 1e6])
def test_an_undamped_spring_never_gains_energy(kdt2):
    h, m = 0.01, 2.0
    k = kdt2 / (h * h)
    anchors, frames = [capi.Anchor.make(0, 0, (0.0, 0.0, 0.0), stiffness=k)], [_still_frame()]
    x, v = np.array([[0.75, -0.5, 0.25]]), np.array([[1.0, 2.0, -3.0]])
    energy = lambda: 0.5 * m * (v ** 2).sum() + 0.5 * k * (x ** 2).sum()
    before = first = energy()
    for _ in range(200):
        v = apply_anchors_f64(x, v, [1.0 / m], anchors, frames, h)[2]
        x = x + h * v
        now = energy()
        assert now <= before * (1.0 + 1e-12)
        before = now
    assert before < first


def test_a_very_stiff_spring_reaches_the_moving_target_in_one_step():
    h = 0.01
    frame = capi.AnchorFrame.make((1.0, 2.0, 3.0), velocity=(0.5, -1.0, 2.0), angular=(0.0, 3.0, 1.0), pivot=(0.0, 1.0, 0.0))
    anchors = [capi.Anchor.make(0, 0, (0.25, -0.5, 1.0), stiffness=1e12)]
    x, v = np.array([[2.0, -1.0, 0.5]]), np.array([[3.0, 0.0, -2.0]])
    v1 = apply_anchors_f64(x, v, [0.5], anchors, [frame], h)[2]
    t = np.array([1.25, 1.5, 4.0])
    u = np.array([0.5, -1.0, 2.0]) + np.cross([0.0, 3.0, 1.0], t - np.array([0.0, 1.0, 0.0]))
    assert np.abs((x[0] + h * v1[0]) - (t + h * u)).max() <= 1e-6 * np.linalg.norm(x[0] - t)


def test_the_impulses_of_a_node_sum_to_its_change_of_momentum():
    pos, vel, inv_mass, anchors, frames, marks = make_scene(600, 700, 64)
    out = apply_anchors_f64(pos, vel, inv_mass, anchors, frames, DT)
    per_node = np.zeros((len(pos), 3))
    np.add.at(per_node, [a.node for a in anchors], out[6][:, :3])
    w = np.asarray(inv_mass, np.float64)
    momentum = (out[2] - np.asarray(vel, np.float64)) * np.where(w > 0, 1.0 / np.where(w > 0, w, 1.0), 0.0)[:, None]
    assert np.abs(per_node - momentum).max() <= 1e-12 * np.abs(momentum).max() and np.abs(momentum[marks["hub"]]).max() > 0


def test_a_pin_on_a_rotating_frame_moves_with_it():
    frame = capi.AnchorFrame.make((1.0, 0.0, 0.0), angular=(0.0, 0.0, 2.0), pivot=(0.0, 0.0, 0.0))
    out = apply_anchors_f64([[5.0, 5.0, 5.0]], [[1.0, 1.0, 1.0]], [0.5], [capi.Anchor.make(0, 0, (1.0, 0.0, 0.0), pin=True)], [frame], 0.01)
    assert np.array_equal(out[0][0], [2.0, 0.0, 0.0]) and np.array_equal(out[1][0], [2.0, 0.0, 0.0])
    assert np.array_equal(out[2][0], np.cross([0.0, 0.0, 2.0], [2.0, 0.0, 0.0])) and np.array_equal(out[3][0], (out[2][0] - 1.0) * 2.0)
    r = apply_anchors(F([[5.0, 5.0, 5.0]]), F([[1.0, 1.0, 1.0]]), F([0.5]), [capi.Anchor.make(0, 0, (1.0, 0.0, 0.0), pin=True)], [frame], DT)
    assert np.array_equal(r[2][0], F([0.0, 4.0, 0.0])) and np.array_equal(r[4][0], F([0.0, 4.0, 12.0])) and r[5].tolist() == [1]


def test_a_call_is_one_implicit_solve():
    """two springs on one node as one set are solved together; applied one after the other the second sees the first's velocity"""
    a = capi.Anchor.make(0, 0, (1.0, 0.0, 0.0), stiffness=400.0, damping=2.0)
    b = capi.Anchor.make(0, 0, (0.0, 1.0, 0.0), stiffness=900.0)
    x, v, w, frames = [[0.25, 0.5, -1.0]], [[1.0, 0.0, 2.0]], [1.0], [_still_frame()]
    together = apply_anchors_f64(x, v, w, [a, b], frames, 0.01)[2]
    first = apply_anchors_f64(x, v, w, [a], frames, 0.01)[2]
    sequence = apply_anchors_f64(x, first, w, [b], frames, 0.01)[2]
    assert np.abs(together - sequence).max() > 1e-3 * np.abs(together - np.asarray(v)).max()


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------
def test_dt_zero_and_released_frames():
    pos, vel, w = F([[1.0, 2.0, 3.0], [0.0, 1.0, 0.0], [4.0, 4.0, 4.0]]), F([[1.0, -1.0, 0.5], [0.0, 2.0, 0.0], [1.0, 1.0, 1.0]]), F([1.0, 0.5, 2.0])
    anchors = [capi.Anchor.make(0, 0, (0.0, 0.0, 0.0), stiffness=100.0, damping=3.0), capi.Anchor.make(1, 0, (0.5, 0.0, 0.0), pin=True),
               capi.Anchor.make(2, 1, (0.0, 0.0, 0.0), pin=True)]
    frames = [_still_frame(velocity=(0.0, 0.0, 1.0)), _still_frame(strength=0.0)]
    out = apply_anchors(pos, vel, w, anchors, frames, F(0))
    assert np.array_equal(out[2][0].view(np.uint32), vel[0].view(np.uint32)) and not out[6][0, :3].any()  # the spring does nothing
    assert np.array_equal(out[0][1], F([0.5, 0.0, 0.0])) and np.array_equal(out[2][1], F([0.0, 0.0, 1.0]))  # the pin holds
    assert np.array_equal(out[0][2], pos[2]) and np.array_equal(out[2][2], vel[2]) and out[5].tolist() == [2, 0]
    assert out[6][2, 3] == np.sqrt(F(48.0)) and not out[6][2, :3].any()  # a released pin: no impulse, the stretch is given


# ---- the entry points on a host-only handle ----------------------------------------------------------------------------------------
def _host_box():
    g = capi.Solver(capi.Options(solver=capi.PBD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def test_add_and_get_on_a_host_only_handle():
    g = _host_box()
    n = g.count(capi.NODES)
    anchors = [capi.Anchor.make(n - 1, 1, (0.5, 0.25, -1.0), stiffness=3.0, damping=0.5), capi.Anchor.make(0, 0, (1.0, 2.0, 3.0), pin=True),
               capi.Anchor.make(n - 1, 0, (0.0, 0.0, 0.0), stiffness=0.0)]
    assert g.add_anchors(anchors, 2) == 0 and g.add_anchors(anchors[:1], 64) == 1
    got, n_frames = g.get_anchors(0)
    assert n_frames == 2 and [bytes(a) for a in got] == [bytes(a) for a in anchors]
    assert [bytes(a) for a in g.get_anchors(1)[0]] == [bytes(anchors[0])] and g.get_anchors(1)[1] == 64
    L, h = capi.load(), g._h
    small = (capi.Anchor * 2)()
    assert L.pies_get_anchors(h, 0, small, 2, None, None) == capi.ERR_INVALID and "capacity" in g.last_error()
    assert L.pies_get_anchors(h, 2, None, 0, None, None) == capi.ERR_INVALID and "unknown set" in g.last_error()
    assert L.pies_get_anchors(None, 0, None, 0, None, None) == capi.ERR_INVALID
    # sets survive a finalize and a scene edit, and end with clear: ids start from 0 again
    g.finalize()
    g.create_tet_box(2, 2, 2, translation=(5.0, 1.5, 0.5))
    g.finalize()
    assert [bytes(a) for a in g.get_anchors(0)[0]] == [bytes(a) for a in anchors]
    g.clear()
    assert L.pies_get_anchors(h, 0, None, 0, None, None) == capi.ERR_INVALID
    g.create_tet_box(3, 3, 3)
    assert g.add_anchors(anchors[:2], 3) == 0 and g.get_anchors(0)[1] == 3


def test_argument_checks_of_add_anchors():
    g = _host_box()
    L, h, n = capi.load(), g._h, g.count(capi.NODES)
    inf, nan = float("inf"), float("nan")
    good = capi.Anchor.make(3, 1, (0.5, 0.25, -1.0), stiffness=3.0, damping=0.5)

    def add(*anchors, n_frames=2, count=None, null=False):
        arr = (capi.Anchor * max(len(anchors), 1))(*anchors)
        return L.pies_add_anchors(h, len(anchors) if count is None else count, None if null else arr, n_frames, None)

    def broken(**kw):
        a = capi.Anchor.from_buffer_copy(good)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(a, name)[value[0]] = value[1]
            else:
                setattr(a, name, value)
        return a

    assert add(count=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()
    assert add() == capi.ERR_INVALID and add(count=0, null=True) == capi.ERR_INVALID
    assert add(good, broken(node=n)) == capi.ERR_INVALID and "anchor 1" in g.last_error() and "node id" in g.last_error()
    for bad in (0, 65):
        assert add(good, n_frames=bad) == capi.ERR_INVALID and "n_frames" in g.last_error(), bad
    assert add(broken(frame=2)) == capi.ERR_INVALID and "frame" in g.last_error()
    assert add(broken(frame=63), n_frames=64) == capi.OK
    for bad in (nan, inf, -inf):
        assert add(broken(local=(1, bad))) == capi.ERR_INVALID and "local" in g.last_error(), bad
        for name in ("stiffness", "damping"):
            assert add(broken(**{name: bad})) == capi.ERR_INVALID and "stiffness and damping" in g.last_error(), (name, bad)
    for name in ("stiffness", "damping"):
        assert add(broken(**{name: -0.5})) == capi.ERR_INVALID and "stiffness and damping" in g.last_error(), name
    for bad in (2, 3, 0x80000000):
        assert add(broken(flags=bad)) == capi.ERR_INVALID and "unknown flag" in g.last_error(), bad
    pin = broken(flags=capi.ANCHOR_PIN)
    for pair in ((pin, good), (good, pin), (pin, pin)):
        assert add(*pair) == capi.ERR_INVALID and "carries a pin and another anchor" in g.last_error()
    assert add(pin, broken(node=4)) == capi.OK  # a pin beside another node's spring
    assert add(good, count=(1 << 24) + 1) == capi.ERR_UNSUPPORTED and "2^24" in g.last_error()  # (refused before the list is read)
    assert L.pies_add_anchors(None, 1, (capi.Anchor * 1)(good), 2, None) == capi.ERR_INVALID
    made = 2
    while made < capi.ANCHOR_SET_MAX:
        assert add(good) == capi.OK
        made += 1
    assert add(good) == capi.ERR_UNSUPPORTED and "PIES_ANCHOR_SET_MAX" in g.last_error()
    with pytest.raises(capi.PiesError):
        g.add_anchors([good], 2)


def test_argument_checks_of_apply_anchors_come_before_the_device_check():
    g = _host_box()
    L, h = capi.load(), g._h
    inf, nan = float("inf"), float("nan")
    anchor_set = g.add_anchors([capi.Anchor.make(3, 1, (0.5, 0.25, -1.0), stiffness=3.0), capi.Anchor.make(0, 0, (0.0, 0.0, 0.0), pin=True)], 2)
    good = [capi.AnchorFrame.make((0.0, 1.0, 0.0)), capi.AnchorFrame.make((1.0, 1.0, 0.0), angular=(0.0, 1.0, 0.0), strength=0.0)]

    def call(*frames, which=anchor_set, n=None, null=False, dt=0.01):
        arr = (capi.AnchorFrame * max(len(frames), 1))(*frames)
        return L.pies_apply_anchors(h, which, len(frames) if n is None else n, None if null else arr, dt, None, None, None, None)

    def broken(base, **kw):
        f = capi.AnchorFrame.from_buffer_copy(base)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(f, name)[value[0]] = value[1]
            else:
                setattr(f, name, value)
        return f

    assert call(*good, which=1) == capi.ERR_INVALID and "unknown set" in g.last_error()
    for frames in (good[:1], good + good[:1]):
        assert call(*frames) == capi.ERR_INVALID and "n_frames must be the set's (2)" in g.last_error()
    assert call(n=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()
    for name, size in (("origin", 3), ("axes", 9), ("velocity", 3), ("angular", 3), ("pivot", 3)):
        for bad in (nan, inf, -inf):
            assert call(good[0], broken(good[1], **{name: (size - 1, bad)})) == capi.ERR_INVALID and "frame 1" in g.last_error(), (name, bad)
    for bad in (nan, inf, -0.5):
        assert call(broken(good[0], strength=bad), good[1]) == capi.ERR_INVALID and "strength" in g.last_error(), bad
    for bad in (-0.01, nan, inf, -inf):
        assert call(*good, dt=bad) == capi.ERR_INVALID and "dt" in g.last_error(), bad
    assert call(*good) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert call(*good, dt=0.0) == capi.ERR_HIP
    assert L.pies_apply_anchors(None, 0, 2, (capi.AnchorFrame * 2)(*good), 0.01, None, None, None, None) == capi.ERR_INVALID
    with pytest.raises(capi.PiesError):
        g.apply_anchors(anchor_set, good, 0.01)


def test_binding_declares_the_entry_points():
    for name in ("pies_add_anchors", "pies_get_anchors", "pies_apply_anchors"):
        assert name in capi.SYMBOLS
    assert C.sizeof(capi.Anchor) == 32 and C.sizeof(capi.AnchorFrame) == 88 and capi.ANCHOR_SET_MAX == 64 and capi.ANCHOR_FRAME_MAX == 64
    L = capi.load()
    assert len(L.pies_add_anchors.argtypes) == 5 and len(L.pies_get_anchors.argtypes) == 6 and len(L.pies_apply_anchors.argtypes) == 9
    assert L.pies_abi_version() == 4
    frame = capi.AnchorFrame.make((1.0, 2.0, 3.0), axes=[[0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    assert list(frame.pivot) == [1.0, 2.0, 3.0] and frame.strength == 1.0
    a = capi.Anchor.at(7, 2, frame, (1.5, 2.25, 2.0), stiffness=4.0, pin=True)
    assert (a.node, a.frame, list(a.local), a.stiffness, a.flags) == (7, 2, [0.25, -0.5, -1.0], 4.0, capi.ANCHOR_PIN)
