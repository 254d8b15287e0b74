"""CPU tests of pies_add_ties / pies_get_ties / pies_apply_ties / pies_get_tie_state / pies_reset_ties: the numpy fp32 restatement of
the rule of include/pies_hip.h (`apply_ties`, the yardstick the device has to match bit for bit in tests/test_ties_gpu.py), an
independent fp64 formulation in matrix form it is held to, physics checks on that formulation, and the argument checks of the entry
points on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi
from test_forces import _cross, _dot

F = np.float32
TILE = 256
DT = F(0.015625)
HUB_TIES = 70  # a CSR row longer than a wavefront
BREAK_STRETCH = 4.0

# branch codes of one tie (apply_ties(..., trace=[])): what the GPU test asserts the coverage of
T_FIXED, T_RELEASED, T_BROKEN, T_LIVE = 0, 1, 2, 3  # W == 0; the group's strength 0; broken, now or before; live


# ---- the restatement: fp32, no fused multiply-adds, the operation order of the header --------------------------------------------
def _columns(ties):
    node = np.array([t.node for t in ties], np.int64)
    to = np.array([list(t.to) for t in ties], np.int64).reshape(-1, 3)
    beta = np.array([list(t.weight) for t in ties], F).reshape(-1, 3)
    k = np.array([t.stiffness for t in ties], F)
    c = np.array([t.damping for t in ties], F)
    group = np.array([t.group for t in ties], np.int64)
    return node, to, beta, k, c, group


def entries_of(ties):
    """the set's (node, tie, coefficient) entries in ascending tie index, slot order a 0 1 2: slot a always, a `to` slot iff its
    weight is not 0"""
    out = []
    for i, t in enumerate(ties):
        out.append((t.node, i, F(1)))
        for j in range(3):
            if F(t.weight[j]) != 0:
                out.append((t.to[j], i, -F(t.weight[j])))
    return out


def counts_of(ties, n_nodes):
    cnt = np.zeros(n_nodes, np.int64)
    for node, _, _ in entries_of(ties):
        cnt[node] += 1
    return cnt


def _carried(b0, b1, b2, beta):
    return (b0 * beta[:, 0:1] + b1 * beta[:, 1:2]) + b2 * beta[:, 2:3]


def apply_ties(pos, vel, inv_mass, ties, groups, dt, iterations, broken=None, trace=None):
    """The rule of pies_apply_ties in numpy fp32.  Returns (vel, impulse, torque, live, per_tie, broken): the velocities after the
    call, the sums per group in the fixed order - per tile of 256 tie indices in ascending index from 0, then the tiles in ascending
    index from 0 -, the live counts, the (n, 4) array of J and stretch and the broken bytes after the call (broken: those before
    it, None: none).  trace: a list that receives the branch code of every tie."""
    with np.errstate(all="ignore"):
        pos, vel = (np.array(a, F).reshape(-1, 3).copy() for a in (pos, vel))
        w = np.asarray(inv_mass, F).reshape(-1)
        h = F(dt)
        n, g = len(ties), len(groups)
        node, to, beta, kk, cc, group = _columns(ties)
        cnt = counts_of(ties, len(pos)).astype(F)
        pivot = np.array([list(x.pivot) for x in groups], F).reshape(g, 3)[group]
        strength = np.array([x.strength for x in groups], F)[group]
        limit = np.array([x.break_stretch for x in groups], F)[group]
        was = np.zeros(n, bool) if broken is None else np.asarray(broken).astype(bool)

        q = _carried(pos[to[:, 0]], pos[to[:, 1]], pos[to[:, 2]], beta)
        x = pos[node] - q
        stretch = np.sqrt(_dot(x, x))
        b0, b1, b2 = beta[:, 0], beta[:, 1], beta[:, 2]
        W = w[node] * cnt[node] + (((b0 * b0) * (w[to[:, 0]] * cnt[to[:, 0]]) + (b1 * b1) * (w[to[:, 1]] * cnt[to[:, 1]]))
                                   + (b2 * b2) * (w[to[:, 2]] * cnt[to[:, 2]]))
        k = kk * strength
        c = cc * strength
        a = c + k * h
        den = F(1) + (h * a) * W
        now = was | ((limit > 0) & (stretch > limit))
        live = ~now & (strength > 0) & (W > 0)
        codes = np.where(now, T_BROKEN, np.where(~(strength > 0), T_RELEASED, np.where(~(W > 0), T_FIXED, T_LIVE)))

        J = np.zeros((n, 3), F)
        rows = [(v, i, coefficient) for v, i, coefficient in entries_of(ties) if live[i]]
        for _ in range(iterations if h > 0 else 0):  # dt == 0: the iterations do not run
            uq = _carried(vel[to[:, 0]], vel[to[:, 1]], vel[to[:, 2]], beta)
            r = vel[node] - uq
            rho = (x * k[:, None] + r * a[:, None]) * h + J
            dJ = np.where(live[:, None], -(rho / den[:, None]), F(0)).astype(F)
            J = np.where(live[:, None], J + dJ, J).astype(F)
            sums, has = np.zeros((len(pos), 3), F), np.zeros(len(pos), bool)
            for v, i, coefficient in rows:  # ascending tie index
                sums[v] = sums[v] + dJ[i] * coefficient
                has[v] = True
            write = has & ~(w == 0)
            vel[write] = vel[write] + sums[write] * w[write, None]
        T = np.where(live[:, None], _cross(q - pivot, J), F(0)).astype(F)

        mine = (group[None, :] == np.arange(g)[:, None])  # g x n
        impulse, torque = np.zeros((g, 3), F), np.zeros((g, 3), F)
        for first in range(0, n, TILE):
            si, st = np.zeros((g, 3), F), np.zeros((g, 3), F)
            for i in range(first, min(first + TILE, n)):
                si = si + np.where(mine[:, i, None], J[i][None], F(0))  # (another group's tie adds 0)
                st = st + np.where(mine[:, i, None], T[i][None], F(0))
            impulse, torque = impulse + si, torque + st
        counts = (mine & live[None]).sum(axis=1).astype(np.uint32)
        if trace is not None:
            trace.extend(codes.tolist())
        return vel, impulse, torque, counts, np.concatenate([J, stretch[:, None]], axis=1).astype(F), now.astype(np.uint8)


# ---- an independent fp64 formulation: the same iteration in matrix form, C (ties x nodes) and the split masses W -----------------------
def tie_matrix(ties, n_nodes):
    Cm = np.zeros((len(ties), n_nodes))
    for i, t in enumerate(ties):
        Cm[i, t.node] += 1.0
        for j in range(3):
            Cm[i, t.to[j]] -= float(t.weight[j])
    return Cm


def system_f64(pos, vel, inv_mass, ties, groups, dt, broken=None):
    """(C, W, X, k, a, den, live, broken, q - pivot) of the call in fp64"""
    p, w, h = np.array(pos, np.float64).reshape(-1, 3), np.asarray(inv_mass, np.float64).reshape(-1), float(dt)
    Cm = tie_matrix(ties, len(p))
    cnt = (Cm != 0).sum(axis=0)
    W = (Cm * Cm) @ (w * cnt)
    group = np.array([t.group for t in ties])
    strength = np.array([float(x.strength) for x in groups])[group]
    limit = np.array([float(x.break_stretch) for x in groups])[group]
    pivot = np.array([list(x.pivot) for x in groups], np.float64).reshape(-1, 3)[group]
    X = Cm @ p
    stretch = np.linalg.norm(X, axis=1)
    k = np.array([float(t.stiffness) for t in ties]) * strength
    a = np.array([float(t.damping) for t in ties]) * strength + k * h
    now = (np.zeros(len(ties), bool) if broken is None else np.asarray(broken).astype(bool)) | ((limit > 0) & (stretch > limit))
    live = ~now & (strength > 0) & (W > 0)
    arm = p[[t.node for t in ties]] - X - pivot  # q = p_a - x
    return Cm, W, X, k, a, 1.0 + h * a * W, live, now, arm


def apply_ties_f64(pos, vel, inv_mass, ties, groups, dt, iterations, broken=None, history=None):
    """Returns (vel, impulse, torque, live (n) bool, per_tie (n, 4), broken (n) bool); history receives the velocities after every
    iteration."""
    Cm, W, X, k, a, den, live, now, arm = system_f64(pos, vel, inv_mass, ties, groups, dt, broken)
    v, w, h = np.array(vel, np.float64).reshape(-1, 3).copy(), np.asarray(inv_mass, np.float64).reshape(-1), float(dt)
    J = np.zeros((len(ties), 3))
    for _ in range(iterations if h > 0 else 0):
        rho = h * (k[:, None] * X + a[:, None] * (Cm @ v)) + J
        dJ = np.where(live[:, None], -rho / den[:, None], 0.0)
        J += dJ
        v += w[:, None] * (Cm.T @ dJ)
        if history is not None:
            history.append(v.copy())
    g = len(groups)
    mine = np.array([t.group for t in ties])[None, :] == np.arange(g)[:, None]
    impulse = mine.astype(np.float64) @ J
    torque = mine.astype(np.float64) @ np.cross(arm, J)
    return v, impulse, torque, live, np.concatenate([J, np.linalg.norm(X, axis=1)[:, None]], axis=1), now


def dense_solve_f64(pos, vel, inv_mass, ties, groups, dt):
    """the coupled solve (1 + h a C M^-1 C^T) J = -h (k x + a r) over the live ties: (vel, J)"""
    Cm, W, X, k, a, den, live, now, arm = system_f64(pos, vel, inv_mass, ties, groups, dt)
    v0, w, h = np.array(vel, np.float64).reshape(-1, 3), np.asarray(inv_mass, np.float64).reshape(-1), float(dt)
    A = np.eye(len(ties)) + (h * a)[:, None] * ((Cm * w[None, :]) @ Cm.T)
    rhs = -h * (k[:, None] * X + a[:, None] * (Cm @ v0))
    J = np.zeros_like(rhs)
    J[live] = np.linalg.solve(A[np.ix_(live, live)], rhs[live])
    return v0 + w[:, None] * (Cm.T @ J), J


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
STRENGTHS = (1.0, 0.5, 2.0, 0.125)


def make_groups(n_groups, seed=0):
    """with three and more groups, group 1 is released (strength 0); the last group breaks ties longer than BREAK_STRETCH"""
    rng = np.random.default_rng(5000 + seed * 97 + n_groups)
    return [capi.TieGroup.make(np.round(rng.uniform(-2, 2, 3) * 16) / 16, strength=0.0 if (k == 1 and n_groups >= 3) else STRENGTHS[k % 4],
                               break_stretch=BREAK_STRETCH if k == n_groups - 1 else 0.0) for k in range(n_groups)]


def make_scene(n_nodes, n_ties, n_groups, seed=0):
    """(pos, vel, inv_mass, ties, groups, marks): loose nodes, invMass in {0, 0.25, 0.5, 1, 2}, and a set listed in shuffled order:
    triangle ties, edge ties (weight[2] == 0, the unused slot naming the tied node itself) and node-node ties.  When the sizes allow
    it (marks is then not empty): a hub that is a corner of 70 triangles, a node in exactly one tie - to a fixed carrier - and one
    in exactly two - the tied node of one, a carrier of the other -, nodes in no tie, a tie whose four nodes are all fixed, a tie of
    the released group 1 (three and more groups), and in the last group, which breaks, a short tie that holds and a long one
    that breaks."""
    rng = np.random.default_rng(seed * 7919 + n_nodes * 31 + n_ties * 7 + n_groups)
    groups = make_groups(n_groups, seed)
    pos = rng.uniform(-3, 3, (n_nodes, 3)).astype(F)
    vel = (rng.normal(size=(n_nodes, 3)) * 2).astype(F)
    inv_mass = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], F), n_nodes)
    last = n_groups - 1

    def spring():
        return dict(stiffness=float(F(rng.uniform(1.0, 2000.0))), damping=float(F(rng.choice([0.0, rng.uniform(0.0, 20.0)]))))

    def triangle(node, corners, group):
        u, v = rng.uniform(0.05, 0.45, 2)
        return capi.Tie.on_triangle(int(node), [int(i) for i in corners], u, v, group=group, **spring())

    def edge(node, ends, group):
        t = F(rng.uniform(0.1, 0.9))
        return capi.Tie.make(int(node), [int(ends[0]), int(ends[1]), int(node)], (F(1) - t, t, 0.0), group=group, **spring())

    def single(node, other, group):
        return capi.Tie.make(int(node), int(other), group=group, **spring())

    ties, marks = [], {}
    free = np.arange(n_nodes)
    if n_nodes >= 63 and n_ties >= 255:
        hub, one, two, fixed = 5, 6, 7, 8
        dead = [9, 10, 11, 12]
        short, long_, released = (13, 14), (15, 16), (17, 18)
        free = np.arange(30 + n_nodes // 8, n_nodes)
        marks = dict(hub=hub, one=one, two=two, fixed=fixed, dead=dead, short=short, long=long_, released=released,
                     bare=list(range(19, 30 + n_nodes // 8)))
        inv_mass[[hub, one, two, 13, 14, 15, 16, 17, 18]] = F(1), F(0.5), F(2), F(1), F(0.5), F(1), F(2), F(1), F(1)
        inv_mass[[fixed] + dead] = F(0)
        pos[14] = pos[13] + np.array([1.0, 0.0, 0.0], F)
        pos[16] = pos[15] + np.array([0.0, 6.0, 0.0], F)
        pos[fixed] = pos[one] + np.array([0.5, 0.5, 0.0], F)  # (short: with one group, group 0 is the one that breaks)
        for j, d in enumerate(dead[1:]):
            pos[d] = pos[dead[0]] + np.array([0.25 * (j + 1), 0.5, -0.25 * j], F)
        for _ in range(HUB_TIES):
            a, b, c = rng.choice(free, 3, replace=False)
            ties.append(triangle(a, (hub, b, c), int(rng.integers(n_groups))))
        a, b, c, d, e = rng.choice(free, 5, replace=False)
        ties += [single(one, fixed, 0), triangle(two, (a, b, c), 0), edge(d, (two, e), 0), triangle(dead[0], dead[1:], 0),
                 single(short[0], short[1], last), single(long_[0], long_[1], last)]
        if n_groups >= 3:
            ties.append(single(released[0], released[1], 1))
    while len(ties) < n_ties:
        a, b, c, d = rng.choice(free, 4, replace=False)
        kind, group = rng.integers(5), int(rng.integers(n_groups))
        ties.append(triangle(a, (b, c, d), group) if kind < 3 else edge(a, (b, c), group) if kind == 3 else single(a, b, group))
    ties = [ties[i] for i in rng.permutation(len(ties))]
    return pos, vel, inv_mass, ties, groups, marks


def check_marks(ties, groups, inv_mass, marks, trace):
    """the scene holds what make_scene promises (with marks)"""
    cnt = counts_of(ties, len(inv_mass))
    index = {(t.node, t.to[0]): i for i, t in enumerate(ties)}
    assert cnt[marks["hub"]] == HUB_TIES > 64 and cnt[marks["one"]] == 1 and cnt[marks["two"]] == 2 and not cnt[marks["bare"]].any()
    assert sum(t.node == marks["two"] for t in ties) == 1  # the tied node of one tie, a carrier of the other
    assert trace[index[(marks["one"], marks["fixed"])]] == T_LIVE and inv_mass[marks["fixed"]] == 0  # a fixed carrier
    assert trace[index[(marks["dead"][0], marks["dead"][1])]] == T_FIXED
    assert trace[index[marks["short"]]] == T_LIVE and trace[index[marks["long"]]] == T_BROKEN
    if len(groups) >= 3:
        assert trace[index[marks["released"]]] == T_RELEASED
    kinds = {sum(w != 0 for w in t.weight) for t in ties}
    assert kinds == {1, 2, 3} and set(trace) == {T_FIXED, T_BROKEN, T_LIVE} | ({T_RELEASED} if len(groups) >= 3 else set())


GPU_SCENES = [(600, 255, 3), (600, 700, 64), (257, 700, 3), (65, 257, 64), (63, 255, 1)]


def test_every_branch_occurs_in_the_shared_scenes():
    for n_nodes, n_ties, n_groups in GPU_SCENES:
        pos, vel, inv_mass, ties, groups, marks = make_scene(n_nodes, n_ties, n_groups)
        assert len(ties) == n_ties and marks
        trace = []
        out = apply_ties(pos, vel, inv_mass, ties, groups, DT, 2, trace=trace)
        check_marks(ties, groups, inv_mass, marks, trace)
        live = np.array(trace) == T_LIVE
        assert out[3].sum() == live.sum() and (out[4][:, 3] > 0).all() and not out[4][~live, :3].any()
        assert out[5].sum() == sum(c == T_BROKEN for c in trace) >= 1
        changed = (out[0].view(np.uint32) != vel.view(np.uint32)).any(axis=1)
        touched = np.zeros(n_nodes, bool)
        for v, i, _ in entries_of(ties):
            touched[v] |= live[i]
        assert (changed <= (touched & (inv_mass != 0))).all() and changed.any() and not changed[marks["bare"]].any()


# ---- restatement against fp64 --------------------------------------------------------------------------------------------------------
# Measured on the scenes below (the GPU tests' scenes) at 1, 4 and 16 iterations: see test_restatement_against_fp64.  Each gate is
# four times the measured figure: the margin is for other scenes of the same generator.
MEASURED_VEL = {1: 1.63e-7, 4: 1.01e-7, 16: 1.11e-7}
MEASURED_J = {1: 1.06e-7, 4: 9.32e-8, 16: 1.28e-7}
DECISION_MARGIN = 1e-4  # every stretch of the scenes is this far, relatively, from its group's break_stretch (the nearest: 2.06e-3)


def _deviation(scene, iterations):
    pos, vel, inv_mass, ties, groups, _ = scene
    trace = []
    r = apply_ties(pos, vel, inv_mass, ties, groups, DT, iterations, trace=trace)
    d = apply_ties_f64(pos, vel, inv_mass, ties, groups, DT, iterations)
    trace = np.array(trace)
    disagree = int(((trace == T_LIVE) != d[3]).sum() + (r[5].astype(bool) != d[5]).sum())
    limit = np.array([float(g.break_stretch) for g in groups])[[t.group for t in ties]]
    margin = np.abs(d[4][:, 3] - limit)[limit > 0] / limit[limit > 0]
    speed = max(np.abs(d[0]).max(), np.abs(np.asarray(vel, np.float64)).max())
    return disagree, margin.min(), np.abs(r[0] - d[0]).max() / speed, np.abs(r[4][:, :3] - d[4][:, :3]).max() / np.abs(d[4][:, :3]).max()


def test_restatement_against_fp64():
    """The fp32 restatement against the fp64 matrix form on the scenes the GPU tests use, at 1, 4 and 16 iterations.  Strengths are
    exactly 0 or at least 2^-3, invMass exactly 0 or at least 0.25 and weights positive, so W is 0 in both precisions or in neither;
    every stretch is asserted to be DECISION_MARGIN away from its break_stretch, so no live or broken decision differs: the count of
    disagreements is asserted to be 0 and nothing is left out.  Velocities are compared relative to the scene's largest speed, J
    relative to the largest |J|; the measured figures stand in MEASURED_VEL and MEASURED_J and the gates are four times those."""
    scenes_ = [make_scene(*sizes) for sizes in GPU_SCENES]
    for iterations in (1, 4, 16):
        worst_vel, worst_j = 0.0, 0.0
        for scene in scenes_:
            disagree, margin, dev_vel, dev_j = _deviation(scene, iterations)
            assert disagree == 0 and margin > DECISION_MARGIN
            worst_vel, worst_j = max(worst_vel, dev_vel), max(worst_j, dev_j)
        print("restatement vs fp64, %2d iterations: velocities %.3g of the largest speed; J %.3g of the largest" % (iterations, worst_vel, worst_j))
        assert worst_vel <= 4 * MEASURED_VEL[iterations] and worst_j <= 4 * MEASURED_J[iterations]


# ---- physics on the fp64 form ------------------------------------------------------------------------------------------------------
def _free_scene(n_nodes, n_ties, stiffness, seed=3, damping=2.0):
    rng = np.random.default_rng(seed)
    pos, vel = rng.normal(size=(n_nodes, 3)), rng.normal(size=(n_nodes, 3))
    inv_mass = rng.uniform(0.25, 2.0, n_nodes)
    ties = []
    for _ in range(n_ties):
        ids = rng.choice(n_nodes, 4, replace=False)
        u, v = rng.integers(1, 8, 2) / 16.0  # (the three weights sum to 1 exactly)
        ties.append(capi.Tie.on_triangle(int(ids[0]), [int(i) for i in ids[1:]], u, v, stiffness=stiffness, damping=damping))
    return pos, vel, inv_mass, ties, [capi.TieGroup.make()]


def _momenta(pos, vel, out, inv_mass):
    dp = (out[0] - vel) / inv_mass[:, None]
    return dp.sum(axis=0), np.cross(pos, dp).sum(axis=0)


def test_momentum_and_angular_momentum_are_conserved():
    """No node is fixed.  A sewn seam - every tied node sits on the point that carries it, x = 0 - exchanges equal and opposite
    impulses at one point: momentum and angular momentum vanish to 1e-12 of the largest impulse.  A STRETCHED tie pulls along
    k x + a r, not along x (the spring-damper is isotropic), so it conserves momentum and turns the pair by x_i x J_i: the change
    of angular momentum is the sum of those, to the same bound."""
    pos, vel, inv_mass, _, groups = _free_scene(80, 1, 500.0)
    rng = np.random.default_rng(11)
    sewn, ties = pos.copy(), []
    for a in range(40):  # nodes 0 .. 39 sit on triangles of the nodes 40 .. 79, which are shared among them
        u, v = rng.integers(1, 8, 2) / 16.0
        ties.append(capi.Tie.on_triangle(a, [int(i) for i in 40 + rng.choice(40, 3, replace=False)], u, v, stiffness=500.0, damping=2.0))
        sewn[a] = sum(float(ties[-1].weight[j]) * sewn[ties[-1].to[j]] for j in range(3))
    out = apply_ties_f64(sewn, vel, inv_mass, ties, groups, DT, 8)
    largest = np.abs(out[4][:, :3]).max()
    linear, angular = _momenta(sewn, vel, out, inv_mass)
    assert largest > 0.1 and out[4][:, 3].max() < 1e-15
    assert np.abs(linear).max() <= 1e-12 * largest and np.abs(angular).max() <= 1e-12 * largest
    pos, vel, inv_mass, ties, groups = _free_scene(80, 60, 500.0)
    out = apply_ties_f64(pos, vel, inv_mass, ties, groups, DT, 8)
    largest = np.abs(out[4][:, :3]).max()
    linear, angular = _momenta(pos, vel, out, inv_mass)
    x = tie_matrix(ties, len(pos)) @ pos
    assert np.abs(linear).max() <= 1e-12 * largest and np.abs(angular).max() > 0.1
    assert np.abs(angular - np.cross(x, out[4][:, :3]).sum(axis=0)).max() <= 1e-12 * largest


def test_the_iteration_converges_to_the_dense_solve():
    pos, vel, inv_mass, ties, groups = _free_scene(200, 60, 96.0)  # k h = 1.5, fewer ties than nodes
    dense, _ = dense_solve_f64(pos, vel, inv_mass, ties, groups, DT)
    history = []
    apply_ties_f64(pos, vel, inv_mass, ties, groups, DT, 64, history=history)
    error = [np.abs(history[t - 1] - dense).max() for t in (1, 8, 64)]
    print("error against the dense solve after 1, 8, 64 iterations: %.3g %.3g %.3g" % tuple(error))
    assert error[0] > error[1] > error[2]


def test_a_very_stiff_seam_stays_bounded():
    pos, vel, inv_mass, ties, groups = _free_scene(200, 60, 1e12)
    dense, _ = dense_solve_f64(pos, vel, inv_mass, ties, groups, DT)
    out = apply_ties_f64(pos, vel, inv_mass, ties, groups, DT, 64)
    assert np.isfinite(out[0]).all() and np.abs(out[0]).max() < np.abs(dense).max() + np.abs(vel).max()


def test_one_stiff_tie_closes_in_one_iteration():
    pos = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, -1.0]])
    vel = np.array([[1.0, -2.0, 0.5], [0.0, 3.0, 1.0]])
    inv_mass = np.array([0.5, 2.0])
    ties = [capi.Tie.make(0, 1, stiffness=1e20)]
    out = apply_ties_f64(pos, vel, inv_mass, ties, [capi.TieGroup.make()], DT, 1)
    h = float(DT)
    assert np.abs((pos[0] + h * out[0][0]) - (pos[1] + h * out[0][1])).max() < 1e-12
    assert np.abs(out[0] - vel).max() > 1.0


def test_dt_zero_released_groups_and_breaks():
    pos, vel, inv_mass, ties, groups, marks = make_scene(600, 255, 3)
    trace = []
    out = apply_ties(pos, vel, inv_mass, ties, groups, F(0), 4, trace=trace)
    assert np.array_equal(out[0].view(np.uint32), vel.view(np.uint32)) and not out[4][:, :3].any() and not out[1].any()
    assert out[5].any() and out[3].sum() == trace.count(T_LIVE) > 0  # ties still break and are counted
    off = make_groups(3)
    for g in off:
        g.strength = 0.0
    out = apply_ties(pos, vel, inv_mass, ties, off, DT, 4)
    assert np.array_equal(out[0].view(np.uint32), vel.view(np.uint32)) and not out[3].any() and out[5].any()
    # a broken tie stays broken: with the bytes of a first call the second one has fewer live ties, whatever the positions do
    first = apply_ties(pos, vel, inv_mass, ties, groups, DT, 2)
    near = np.zeros_like(pos)
    again = apply_ties(near, vel, inv_mass, ties, groups, DT, 2, broken=first[5])
    fresh = apply_ties(near, vel, inv_mass, ties, groups, DT, 2)
    assert np.array_equal(again[5], first[5]) and not fresh[5].any() and again[3].sum() == fresh[3].sum() - first[5].sum()


# ---- the entry points on a host-only handle ----------------------------------------------------------------------------------------
def _host_box():
    g = capi.Solver(capi.Options(solver=capi.PBD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    return g


def test_add_get_state_and_reset_on_a_host_only_handle():
    g = _host_box()
    n = g.count(capi.NODES)
    ties = [capi.Tie.on_triangle(n - 1, (0, 1, 2), 0.25, 0.5, stiffness=3.0, damping=0.5, group=1), capi.Tie.make(3, [4, 5], (0.5, 0.5), stiffness=1.0),
            capi.Tie.make(6, 7)]
    assert list(ties[0].weight) == [0.25, 0.25, 0.5] and list(ties[1].to) == [4, 5, 4] and list(ties[1].weight) == [0.5, 0.5, 0.0]
    assert g.add_ties(ties, 2) == 0 and g.add_ties(ties[1:], 64) == 1
    got, n_groups = g.get_ties(0)
    assert n_groups == 2 and [bytes(t) for t in got] == [bytes(t) for t in ties]
    assert g.get_ties(1)[1] == 64 and len(g.get_ties(1)[0]) == 2
    assert g.tie_state(0).tolist() == [0, 0, 0]
    g.reset_ties(0)
    L, h = capi.load(), g._h
    small = (capi.Tie * 2)()
    count = C.c_uint32(7)
    assert L.pies_get_ties(h, 0, small, 2, None, None) == capi.ERR_INVALID and "capacity" in g.last_error()
    assert L.pies_get_ties(h, 2, None, 0, None, None) == capi.ERR_INVALID and "unknown set" in g.last_error()
    assert L.pies_get_tie_state(h, 0, (C.c_uint8 * 2)(), 2, None) == capi.ERR_INVALID and "capacity" in g.last_error()
    assert L.pies_get_tie_state(h, 0, None, 0, C.byref(count)) == capi.OK and count.value == 0
    assert L.pies_get_tie_state(h, 2, None, 0, None) == capi.ERR_INVALID and "unknown set" in g.last_error()
    assert L.pies_reset_ties(h, 2) == capi.ERR_INVALID and "unknown set" in g.last_error()
    for call in (lambda: L.pies_get_ties(None, 0, None, 0, None, None), lambda: L.pies_get_tie_state(None, 0, None, 0, None),
                 lambda: L.pies_reset_ties(None, 0)):
        assert call() == capi.ERR_INVALID
    # sets survive a finalize and a scene edit, and end with clear: ids start from 0 again
    g.finalize()
    g.create_tet_box(2, 2, 2, translation=(5.0, 1.5, 0.5))
    g.finalize()
    assert [bytes(t) for t in g.get_ties(0)[0]] == [bytes(t) for t in ties]
    g.clear()
    assert L.pies_get_ties(h, 0, None, 0, None, None) == capi.ERR_INVALID
    g.create_tet_box(3, 3, 3)
    assert g.add_ties(ties[:2], 3) == 0 and g.get_ties(0)[1] == 3


def test_argument_checks_of_add_ties():
    g = _host_box()
    L, h, n = capi.load(), g._h, g.count(capi.NODES)
    inf, nan = float("inf"), float("nan")
    good = capi.Tie.on_triangle(3, (4, 5, 6), 0.25, 0.5, stiffness=3.0, damping=0.5, group=1)

    def add(*ties, n_groups=2, count=None, null=False):
        arr = (capi.Tie * max(len(ties), 1))(*ties)
        return L.pies_add_ties(h, len(ties) if count is None else count, None if null else arr, n_groups, None)

    def broken(**kw):
        t = capi.Tie.from_buffer_copy(good)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(t, name)[value[0]] = value[1]
            else:
                setattr(t, name, value)
        return t

    assert add(count=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()
    assert add() == capi.ERR_INVALID and add(count=0, null=True) == capi.ERR_INVALID
    assert add(good, broken(node=n)) == capi.ERR_INVALID and "tie 1" in g.last_error() and "node id" in g.last_error()
    for slot in range(3):
        assert add(broken(to=(slot, n))) == capi.ERR_INVALID and "node id" in g.last_error(), slot
    assert add(broken(to=(2, n), weight=(2, 0.0))) == capi.ERR_INVALID and "node id" in g.last_error()  # (a zero weight's slot is read)
    for bad in (nan, inf, -inf):
        assert add(broken(weight=(1, bad))) == capi.ERR_INVALID and "weights must be finite" in g.last_error(), bad
        for name in ("stiffness", "damping"):
            assert add(broken(**{name: bad})) == capi.ERR_INVALID and "stiffness and damping" in g.last_error(), (name, bad)
    for name in ("stiffness", "damping"):
        assert add(broken(**{name: -0.5})) == capi.ERR_INVALID and "stiffness and damping" in g.last_error(), name
    zero = capi.Tie.make(3, [4, 5, 6], (0.0, 0.0, -0.0))
    assert add(zero) == capi.ERR_INVALID and "all three weights" in g.last_error()
    assert add(broken(group=2)) == capi.ERR_INVALID and "group" in g.last_error()
    assert add(broken(group=63), n_groups=64) == capi.OK
    for bad in (0, 65):
        assert add(good, n_groups=bad) == capi.ERR_INVALID and "n_groups" in g.last_error(), bad
    for twice in (broken(to=(0, 3)), broken(to=(2, 3)), broken(to=(1, 4)), broken(to=(2, 5))):
        assert add(twice) == capi.ERR_INVALID and "pairwise distinct" in g.last_error()
    assert add(broken(to=(2, 3), weight=(2, 0.0))) == capi.OK  # a slot with weight 0 may name any node
    assert add(broken(weight=(0, -0.5))) == capi.OK            # weights need not be barycentric
    assert add(good, count=(1 << 24) + 1) == capi.ERR_UNSUPPORTED and "2^24" in g.last_error()  # (refused before the list is read)
    assert L.pies_add_ties(None, 1, (capi.Tie * 1)(good), 2, None) == capi.ERR_INVALID
    made = 3
    while made < capi.TIE_SET_MAX:
        assert add(good) == capi.OK
        made += 1
    assert add(good) == capi.ERR_UNSUPPORTED and "PIES_TIE_SET_MAX" in g.last_error()
    with pytest.raises(capi.PiesError):
        g.add_ties([good], 2)


def test_argument_checks_of_apply_ties_come_before_the_device_check():
    g = _host_box()
    L, h = capi.load(), g._h
    inf, nan = float("inf"), float("nan")
    tie_set = g.add_ties([capi.Tie.on_triangle(3, (4, 5, 6), 0.25, 0.5, stiffness=3.0, group=1), capi.Tie.make(0, 1, stiffness=1.0)], 2)
    good = [capi.TieGroup.make((0.0, 1.0, 0.0)), capi.TieGroup.make((1.0, 1.0, 0.0), strength=0.0, break_stretch=0.5)]

    def call(*groups, which=tie_set, n=None, null=False, dt=0.01, iterations=4):
        arr = (capi.TieGroup * max(len(groups), 1))(*groups)
        return L.pies_apply_ties(h, which, len(groups) if n is None else n, None if null else arr, dt, iterations, None, None, None, None)

    def broken(base, **kw):
        f = capi.TieGroup.from_buffer_copy(base)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(f, name)[value[0]] = value[1]
            else:
                setattr(f, name, value)
        return f

    assert call(*good, which=1) == capi.ERR_INVALID and "unknown set" in g.last_error()
    for groups in (good[:1], good + good[:1]):
        assert call(*groups) == capi.ERR_INVALID and "n_groups must be the set's (2)" in g.last_error()
    assert call(n=2, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()
    for bad in (nan, inf, -inf):
        assert call(good[0], broken(good[1], pivot=(2, bad))) == capi.ERR_INVALID and "group 1" in g.last_error() and "pivot" in g.last_error()
    for name in ("strength", "break_stretch"):
        for bad in (nan, inf, -0.5):
            assert call(broken(good[0], **{name: bad}), good[1]) == capi.ERR_INVALID and name in g.last_error(), (name, bad)
    for bad in (-0.01, nan, inf, -inf):
        assert call(*good, dt=bad) == capi.ERR_INVALID and "dt" in g.last_error(), bad
    for bad in (0, 65, 0xFFFFFFFF):
        assert call(*good, iterations=bad) == capi.ERR_INVALID and "iterations" in g.last_error(), bad
    for fine in (1, 64):
        assert call(*good, iterations=fine) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert call(*good, dt=0.0) == capi.ERR_HIP
    assert L.pies_apply_ties(None, 0, 2, (capi.TieGroup * 2)(*good), 0.01, 4, None, None, None, None) == capi.ERR_INVALID
    with pytest.raises(capi.PiesError):
        g.apply_ties(tie_set, good, 0.01)


def test_binding_declares_the_entry_points():
    for name in ("pies_add_ties", "pies_get_ties", "pies_apply_ties", "pies_get_tie_state", "pies_reset_ties"):
        assert name in capi.SYMBOLS
    assert C.sizeof(capi.Tie) == 40 and C.sizeof(capi.TieGroup) == 20 and capi.TIE_SET_MAX == 64 and capi.TIE_GROUP_MAX == 64
    L = capi.load()
    assert len(L.pies_add_ties.argtypes) == 5 and len(L.pies_get_ties.argtypes) == 6 and len(L.pies_apply_ties.argtypes) == 10
    assert len(L.pies_get_tie_state.argtypes) == 5 and len(L.pies_reset_ties.argtypes) == 2
    assert L.pies_abi_version() == 4
    t = capi.Tie.on_triangle(7, (1, 2, 3), 0.3, 0.6, stiffness=4.0, damping=1.0, group=2)
    u, v = F(0.3), F(0.6)
    assert (t.node, list(t.to), t.stiffness, t.damping, t.group) == (7, [1, 2, 3], 4.0, 1.0, 2)
    assert [F(x) for x in t.weight] == [(F(1) - u) - v, u, v]
    group = capi.TieGroup.make((1.0, 2.0, 3.0), break_stretch=0.5)
    assert list(group.pivot) == [1.0, 2.0, 3.0] and group.strength == 1.0 and group.break_stretch == 0.5
