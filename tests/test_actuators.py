"""CPU tests of pies_add_actuators / pies_get_actuators / pies_drive_actuators(_device): the numpy fp32 restatement of the rule of
include/pies_hip.h (`drive_actuators`, the yardstick the device has to match bit for bit in tests/test_actuators_gpu.py), an
independent fp64 formulation it is held to with a rounding bound derived from the operation count, a marked scene in which every
branch of the rule occurs, and the argument checks of the four entry points on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi

F = np.float32
U = np.uint32
TILE = 256
EPS = 2.0 ** -24  # unit roundoff of fp32

# branch codes of one actuator (drive_actuators(..., trace=[])): what the scene builder asserts the coverage of
B_NOT_LIVE, B_FREE, B_AT_LO, B_AT_HI = 0, 1, 2, 3  # the activation is not finite; r inside (lo, hi); clamped at lo; clamped at hi


def bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(U)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def fields(actuators):
    """the set as arrays: type, index, channel (int64), gain, lo, hi, base (float32), offset (bool)"""
    g = lambda name, t: np.array([getattr(a, name) for a in actuators], t)  # noqa: E731
    return (g("type", np.int64), g("index", np.int64), g("channel", np.int64), g("gain", F), g("lo", F), g("hi", F), g("base", F),
            (g("flags", np.int64) & capi.ACTUATOR_OFFSET) != 0)


# ---- the restatement: fp32, no fused multiply-adds, the operation order of the header --------------------------------------------
def drive_actuators(pos, ids, rest, actuators, activation, trace=None):
    """The rule of pies_drive_actuators in numpy fp32.  pos (n, 3): the state the call finds; ids, rest: {capi.DISTANCE: (m, 2) ids,
    capi.BEND: (k, 4) ids} and the containers' rest data in host order; actuators: a sequence of capi.Actuator with `base` filled
    in; activation: one float per channel.  Returns (rest, out_actuator, out_sums, out_live): the containers' rest data after the
    call (new arrays), the (n, 2) array of (rest, value), the (c, 2) sums in the fixed order - per tile of 256 actuator indices in
    ascending index from 0, then the tiles in ascending index from 0 - and the live counts.  trace: a list that receives the
    branch code of every actuator."""
    with np.errstate(all="ignore"):
        pos = np.array(pos, F).reshape(-1, 3)
        act = np.array(activation, F).reshape(-1)
        new = {t: np.array(r, F).reshape(-1).copy() for t, r in rest.items()}
        typ, index, channel, gain, lo, hi, base, offset = fields(actuators)
        n, c = len(typ), len(act)
        u = act[channel]
        live = (u - u) == F(0)
        gu = gain * u
        r = np.where(offset, base + gu, base * (F(1) + gu))
        r = np.fmin(np.fmax(r, lo), hi)
        value, kept = np.zeros(n, F), np.zeros(n, F)
        d = typ == capi.DISTANCE
        if d.any():
            e = np.asarray(ids[capi.DISTANCE], np.int64).reshape(-1, 2)[index[d]]
            x = pos[e[:, 0]] - pos[e[:, 1]]
            value[d] = np.sqrt(_dot(x, x))
            kept[d] = new[capi.DISTANCE][index[d]]
        b = typ == capi.BEND
        if b.any():
            q = np.asarray(ids[capi.BEND], np.int64).reshape(-1, 4)[index[b]]
            p2, p3, p4 = pos[q[:, 1]] - pos[q[:, 0]], pos[q[:, 2]] - pos[q[:, 0]], pos[q[:, 3]] - pos[q[:, 0]]
            e, f = _cross(p2, p3), _cross(p2, p4)
            n1, n2 = e / np.sqrt(_dot(e, e))[:, None], f / np.sqrt(_dot(f, f))[:, None]
            value[b] = _dot(n1, n2)
            kept[b] = new[capi.BEND][index[b]]
        r = np.where(live, r, kept).astype(F)  # (an actuator that is not live: the rest its constraint keeps)
        for t, mask in ((capi.DISTANCE, d), (capi.BEND, b)):
            if mask.any():
                new[t][index[mask & live]] = r[mask & live]
        mine = (channel[None, :] == np.arange(c)[:, None]) & live[None, :]  # c x n
        sums = np.zeros((c, 2), F)
        for first in range(0, n, TILE):
            s = np.zeros((c, 2), F)
            for i in range(first, min(first + TILE, n)):
                s = s + np.where(mine[:, i, None], np.array([value[i], r[i]], F)[None], F(0))  # (another channel's actuator adds 0)
            sums = sums + s
        if trace is not None:
            trace.extend(np.where(~live, B_NOT_LIVE, np.where(r == lo, B_AT_LO, np.where(r == hi, B_AT_HI, B_FREE))).tolist())
        return new, np.stack([r, value], axis=1).astype(F), sums.astype(F), mine.sum(axis=1).astype(U)


# ---- an independent fp64 formulation, and what fp32 may lose against it ------------------------------------------------------------
def drive_actuators_f64(pos, ids, rest, actuators, activation):
    """Returns (r, value, bound_r, bound_value, live): per actuator in fp64, with the fp32 rule's rounding bounds.
    r: gain * u, 1 + gu and base * (..) round once each (offset: gain * u and the sum); the clamp is monotone and exact, so
        |r32 - r64| <= eps |base| (|gu| + 2 |1 + gu|)   resp.   eps (|gu| + |r|)   (first order, before the clamp).
    length: each difference rounds once (eps), a square 2 eps + eps, the two sums of non-negative terms eps each, the root halves
        the 5 eps and adds its own: 3.5 eps, stated as 4 eps L.
    cosine: a cross component a b - c d of differences: 3 eps per product, eps for the difference, |a b| + |c d| <= |p2| |p3|, so
        the cross is off by at most 4 sqrt(3) eps |p2| |p3| in norm; normalising turns that into an angle error of at most that over
        |cross| = 1 / sin of the angle between the edges (kappa); the length and the division scale the unit vector by 4.5 eps;
        the final dot product adds 3 eps: eps (7 (kappa_1 + kappa_2) + 13)."""
    x = np.array(pos, np.float64).reshape(-1, 3)
    act = np.array(activation, F).astype(np.float64)
    typ, index, channel, gain, lo, hi, base, offset = fields(actuators)
    gain, lo, hi, base = (a.astype(np.float64) for a in (gain, lo, hi, base))
    u = act[channel]
    live = np.isfinite(u)
    with np.errstate(all="ignore"):
        gu = gain * u
        raw = np.where(offset, base + gu, base * (1.0 + gu))
        r = np.clip(raw, lo, hi)
        bound_r = np.where(offset, np.abs(gu) + np.abs(raw), np.abs(base) * (np.abs(gu) + 2.0 * np.abs(1.0 + gu))) * EPS * 1.01
    n = len(typ)
    value, bound_v = np.zeros(n), np.zeros(n)
    d = typ == capi.DISTANCE
    if d.any():
        e = np.asarray(ids[capi.DISTANCE], np.int64).reshape(-1, 2)[index[d]]
        value[d] = np.linalg.norm(x[e[:, 0]] - x[e[:, 1]], axis=1)
        bound_v[d] = 4.0 * EPS * value[d]
    b = typ == capi.BEND
    if b.any():
        q = np.asarray(ids[capi.BEND], np.int64).reshape(-1, 4)[index[b]]
        p2, p3, p4 = x[q[:, 1]] - x[q[:, 0]], x[q[:, 2]] - x[q[:, 0]], x[q[:, 3]] - x[q[:, 0]]
        e, f = np.cross(p2, p3), np.cross(p2, p4)
        le, lf = np.linalg.norm(e, axis=1), np.linalg.norm(f, axis=1)
        value[b] = np.einsum("ij,ij->i", e, f) / (le * lf)
        n2 = np.linalg.norm(p2, axis=1)
        kappa = n2 * np.linalg.norm(p3, axis=1) / le + n2 * np.linalg.norm(p4, axis=1) / lf
        bound_v[b] = EPS * (7.0 * kappa + 13.0)
    return r, value, bound_r, bound_v, live


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def lattice_and_sheet(s, seed=3, amplitude=0.08, copies=1):
    """createBox 4 x 3 x 3 (192 distance constraints) beside createBendSheet 6 x 5 (44 bend constraints), perturbed so that no length
    and no dihedral cosine is special; copies: as many of each, side by side"""
    for b in range(copies):
        s.create_box(4, 3, 3, translation=(0.0, 2.0, 5.0 * b), w=0.5, triangles=False)
        s.create_bend_sheet(6, 5, translation=(6.0, 2.0, 7.0 * b), w=0.6)
    rng = np.random.default_rng(seed)
    p = s.positions
    s.set_positions(p + rng.uniform(-amplitude, amplitude, p.shape).astype(F))


def random_set(rng, counts, n, channels, bends=None):
    """n actuators over distinct constraints of the containers (counts: {type: size}), every mode, bounds that clamp now and then;
    bends: how many of them drive bend constraints (None: as the draw falls)"""
    pool = [(t, i) for t, m in counts.items() for i in range(m)]
    assert n <= len(pool)
    picks = [pool[k] for k in rng.permutation(len(pool))]
    if bends is not None:
        picks = [q for q in picks if q[0] == capi.BEND][:bends] + [q for q in picks if q[0] != capi.BEND]
        assert sum(q[0] == capi.BEND for q in picks[:n]) == bends
    out = []
    for t, i in picks[:n]:
        offset = bool(rng.integers(2))
        lo, hi = (0.9, 1.6) if t == capi.DISTANCE else (2.0, 3.5)  # (rest lengths 1 .. 1.73, rest angles pi)
        out.append(capi.Actuator.make(t, i, int(rng.integers(channels)), float(rng.uniform(-0.8, 0.8)), lo, hi, offset))
    return out


def with_base(actuators, rest):
    """the set as pies_get_actuators returns it: base = the constraint's rest datum"""
    out = []
    for a in actuators:
        b = capi.Actuator.from_buffer_copy(a)
        b.base = float(rest[a.type][a.index])
        out.append(b)
    return out


def containers(g):
    t = (capi.DISTANCE, capi.BEND)
    return {k: g.ids(k) for k in t if g.count(k)}, {k: g.rest(k) for k in t if g.count(k)}


def marked_scene():
    """A host-only handle with the lattice and the sheet, a set in which every branch occurs, and its activations: scale and offset
    mode, a clamp at lo and at hi, a non-finite activation (channels 3 and 4: the device form only), a channel without an actuator
    (5), both types in one set.  Returns (g, set id, actuators with base, activation)."""
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    lattice_and_sheet(g)
    nd, nb = g.count(capi.DISTANCE), g.count(capi.BEND)
    A = capi.Actuator.make
    acts = [A(capi.DISTANCE, 0, 0, 0.5, 0.25, 4.0), A(capi.DISTANCE, nd - 1, 0, 0.25, 0.25, 4.0, offset=True),
            A(capi.DISTANCE, 7, 1, 1.0, 0.9, 4.0), A(capi.DISTANCE, 9, 2, 1.0, 0.25, 1.1),
            A(capi.BEND, 0, 0, -0.25, 0.125, 3.0), A(capi.BEND, nb - 1, 1, 1.0, 0.125, 3.0, offset=True),
            A(capi.BEND, 3, 2, 0.5, 0.125, 0.5, offset=True), A(capi.DISTANCE, 11, 3, 1.0, 0.25, 4.0), A(capi.BEND, 5, 4, 1.0, 0.125, 3.0),
            A(capi.DISTANCE, 12, 4, 1.0, 0.25, 4.0, offset=True)]
    k = g.add_actuators(acts, 6)
    activation = np.array([0.5, -0.75, 2.0, np.nan, np.inf, 1.0], F)
    return g, k, g.get_actuators(k)[0], activation


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_every_branch_occurs_in_the_marked_scene():
    g, k, acts, activation = marked_scene()
    ids, rest = containers(g)
    trace = []
    new, per, sums, live = drive_actuators(g.positions, ids, rest, acts, activation, trace=trace)
    assert set(trace) == {B_NOT_LIVE, B_FREE, B_AT_LO, B_AT_HI}
    offset = [bool(a.flags & capi.ACTUATOR_OFFSET) for a in acts]
    assert any(offset) and not all(offset) and {a.type for a in acts} == {capi.DISTANCE, capi.BEND}
    for code in (B_FREE, B_AT_LO, B_AT_HI):  # in both modes something is written; each clamp is met
        assert code in trace
    assert any(o and c == B_FREE for o, c in zip(offset, trace)) and any(not o and c == B_FREE for o, c in zip(offset, trace))
    assert live.tolist() == [3, 2, 2, 0, 0, 0]  # channels 3 and 4 are not finite, channel 5 has no actuator
    assert sums[3:].tolist() == [[0.0, 0.0]] * 3
    # an actuator that is not live leaves its constraint alone and reports the rest it keeps
    for i, a in enumerate(acts):
        if trace[i] == B_NOT_LIVE:
            assert new[a.type][a.index] == rest[a.type][a.index] == per[i, 0]
        else:
            assert new[a.type][a.index] == per[i, 0] != rest[a.type][a.index]
    touched = {(a.type, a.index) for a in acts}
    for t in rest:  # constraints outside the set keep their rest bits
        keep = np.array([(t, i) not in touched for i in range(len(rest[t]))])
        assert np.array_equal(bits(new[t][keep]), bits(rest[t][keep]))
    g.close()


@pytest.mark.parametrize("seed,n,channels", [(1, 40, 3), (2, 63, 1), (3, 64, 64)])
def test_restatement_against_fp64(seed, n, channels):
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    lattice_and_sheet(g, seed=seed)
    rng = np.random.default_rng(seed)
    ids, rest = containers(g)
    acts = with_base(random_set(rng, {t: len(r) for t, r in rest.items()}, n, channels), rest)
    activation = rng.uniform(-1.5, 1.5, channels).astype(F)
    activation[0] = 1.4  # (with gains in -0.8 .. 0.8 the first channel alone reaches both bounds)
    if channels > 2:
        activation[1] = np.nan
    trace = []
    new, per, sums, live = drive_actuators(g.positions, ids, rest, acts, activation, trace=trace)
    r, value, bound_r, bound_v, live64 = drive_actuators_f64(g.positions, ids, rest, acts, activation)
    assert {B_FREE, B_AT_LO, B_AT_HI} <= set(trace)
    is_live = np.array(trace) != B_NOT_LIVE
    assert np.array_equal(is_live, live64)
    assert (np.abs(per[is_live, 0] - r[is_live]) <= bound_r[is_live]).all(), float((np.abs(per[is_live, 0] - r[is_live]) / bound_r[is_live]).max())
    assert (np.abs(per[:, 1] - value) <= bound_v).all(), float((np.abs(per[:, 1] - value) / bound_v).max())
    assert (np.abs(per[:, 1] - value) > 0).any()  # (the bound is not met by equality of formulas)
    # the sums: m sequential additions lose at most m eps of the sum of magnitudes, on top of what the terms carry
    channel = np.array([a.channel for a in acts])
    for c in range(channels):
        m = is_live & (channel == c)
        assert live[c] == m.sum()
        for col, exact, bound in ((0, value, bound_v), (1, r, bound_r)):
            want = exact[m].sum()
            slack = bound[m].sum() + (m.sum() + 1) * EPS * np.abs(exact[m]).sum()
            assert abs(float(sums[c, col]) - want) <= slack, (c, col, float(sums[c, col]), want, slack)
    g.close()


def test_get_actuators_round_trip_fills_base():
    g, k, acts, activation = marked_scene()
    ids, rest = containers(g)
    assert k == 0 and g.get_actuators(k)[1] == 6 and len(acts) == 10
    for a in acts:
        assert a.base == rest[a.type][a.index] and a.base > 0
    # a second set is the next id; sets are assets: they survive finalize and end with clear
    assert g.add_actuators([capi.Actuator.make(capi.BEND, 1, 0, 1.0, 0.0, 3.0)], 1) == 1
    g.finalize()
    again = g.get_actuators(0)[0]
    assert [bytes(a) for a in again] == [bytes(a) for a in acts]
    # base follows a pies_set_rest made before the set is added
    g.set_rest(capi.DISTANCE, np.array([1.75], F), first=2)
    k2 = g.add_actuators([capi.Actuator.make(capi.DISTANCE, 2, 0, 1.0, 0.0, 3.0)], 1)
    assert g.get_actuators(k2)[0][0].base == 1.75
    g.clear()
    with pytest.raises(capi.PiesError):
        g.get_actuators(0)
    g.close()


def _rc(g, acts, channels):
    arr = (capi.Actuator * max(len(acts), 1))(*acts)
    out = C.c_uint32(99)
    return g._L.pies_add_actuators(g._h, len(acts), arr if acts else None, channels, C.byref(out))


def test_add_actuators_argument_checks():
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    lattice_and_sheet(g)
    nd, nb = g.count(capi.DISTANCE), g.count(capi.BEND)
    A = capi.Actuator.make
    good = A(capi.DISTANCE, 0, 0, 1.0, 0.0, 2.0)
    assert _rc(g, [good], 1) == capi.OK
    assert g._L.pies_add_actuators(g._h, 1, None, 1, None) == capi.ERR_INVALID
    assert _rc(g, [], 1) == capi.ERR_INVALID
    bad = [A(capi.TET, 0), A(capi.POSITION, 0), A(capi.DISTANCE, nd), A(capi.BEND, nb), A(capi.DISTANCE, 0, channel=1),
           A(capi.DISTANCE, 0, gain=float("nan")), A(capi.DISTANCE, 0, gain=float("inf")), A(capi.DISTANCE, 0, lo=float("nan")),
           A(capi.DISTANCE, 0, hi=float("inf")), A(capi.DISTANCE, 0, lo=2.0, hi=1.0), A(capi.DISTANCE, 0, lo=-0.5, hi=1.0)]
    for a in bad:
        assert _rc(g, [a], 1) == capi.ERR_INVALID, (a.type, a.index, a.channel, a.gain, a.lo, a.hi)
    assert _rc(g, [A(capi.BEND, 0, lo=-0.5, hi=1.0)], 1) == capi.OK  # (a bend angle may be driven below 0)
    flagged = A(capi.DISTANCE, 0)
    flagged.flags = 2
    assert _rc(g, [flagged], 1) == capi.ERR_INVALID
    assert _rc(g, [good], 0) == capi.ERR_INVALID and _rc(g, [good], capi.ACTUATOR_CHANNEL_MAX + 1) == capi.ERR_INVALID
    assert _rc(g, [good], capi.ACTUATOR_CHANNEL_MAX) == capi.OK
    assert _rc(g, [good, A(capi.DISTANCE, 1), A(capi.DISTANCE, 0, gain=2.0)], 1) == capi.ERR_INVALID  # a constraint listed twice
    assert _rc(g, [A(capi.DISTANCE, 0), A(capi.BEND, 0)], 1) == capi.OK  # (the same index in two containers is two constraints)
    have = 4
    for _ in range(capi.ACTUATOR_SET_MAX - have):
        assert _rc(g, [good], 1) == capi.OK
    assert _rc(g, [good], 1) == capi.ERR_UNSUPPORTED
    g.close()


def test_get_and_drive_argument_checks_on_a_host_only_handle():
    g, k, acts, activation = marked_scene()
    L, h = g._L, g._h
    n, c = C.c_uint32(), C.c_uint32()
    assert L.pies_get_actuators(h, 5, None, 0, C.byref(n), C.byref(c)) == capi.ERR_INVALID
    assert L.pies_get_actuators(h, k, None, 0, C.byref(n), C.byref(c)) == capi.OK and (n.value, c.value) == (10, 6)
    arr = (capi.Actuator * 10)()
    assert L.pies_get_actuators(h, k, arr, 9, None, None) == capi.ERR_INVALID
    assert L.pies_get_actuators(h, k, arr, 10, None, None) == capi.OK
    pf = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    finite = np.zeros(6, F)
    # the arguments are checked first, then the handle has no device
    assert L.pies_drive_actuators(h, 5, 6, pf(finite), None, None, None) == capi.ERR_INVALID
    assert L.pies_drive_actuators(h, k, 5, pf(finite), None, None, None) == capi.ERR_INVALID
    assert L.pies_drive_actuators(h, k, 6, None, None, None, None) == capi.ERR_INVALID
    assert L.pies_drive_actuators(h, k, 6, pf(activation), None, None, None) == capi.ERR_INVALID  # a non-finite activation
    assert L.pies_drive_actuators(h, k, 6, pf(finite), None, None, None) == capi.ERR_HIP
    assert L.pies_drive_actuators_device(h, 5, 6, 4096, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.pies_drive_actuators_device(h, k, 7, 4096, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.pies_drive_actuators_device(h, k, 6, None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.pies_drive_actuators_device(h, k, 6, 4098, None, None, None, None, 0) == capi.ERR_INVALID  # not 4-byte aligned
    assert L.pies_drive_actuators_device(h, k, 6, 4096, 4097, None, None, None, 0) == capi.ERR_INVALID
    assert L.pies_drive_actuators_device(h, k, 6, 4096, None, None, None, None, 0) == capi.ERR_HIP
    with pytest.raises(capi.PiesError):
        g.drive_actuators(k, finite)
    # nothing above changed the rest data
    assert np.array_equal(g.rest(capi.DISTANCE), containers(g)[1][capi.DISTANCE])
    g.close()
