"""CPU tests of pies_measure_elements / pies_measure_nodes: the numpy fp32 restatements of the two rules of include/pies_hip.h
(`measure_elements`, `measure_nodes`: the yardsticks the device has to match bit for bit in tests/test_measure_gpu.py; the
singular values come from benchlib.oracle_api.svd3, the oracle's arithmetic, never from the library under test), an independent
fp64 formulation they are held to on the scenes of tests/golden/measure_tiny.npz, physics checks on that formulation, and the
argument checks of the entry points on a host-only handle."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_api
from pies_amd import capi

F = np.float32
TILE = 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "measure_tiny.npz")
TET_LIMITS, VOLUME_LIMITS = (F(0.8), F(1.2)), (F(0.9), F(1.1))  # (min_strain, max_strain), (compression, stretching) of the scenes
MARGIN = 1.0e-3  # the builders keep every discontinuous decision this far (relative, see decisions_f64) from its threshold

# branch bits of one element (measure_elements(..., trace=[])): the record's four flags, and what else the walk can meet
T_INVERTED, T_OVER, T_UNDER, T_NONFINITE = capi.ELEMENT_INVERTED, capi.ELEMENT_OVER, capi.ELEMENT_UNDER, capi.ELEMENT_NONFINITE
T_COLLAPSED, T_IDENTITY, T_SWAP01, T_SWAP12, T_SWAP01B = 16, 32, 64, 128, 256  # j == 0; F is exactly 1; the three compare-exchanges
# the elements make_element_scene sets up on nodes of their own, in this order
SPECIALS = ("rest", "rotated", "over", "under", "inverted", "collapsed", "nan")


# ---- the restatements: fp32, no fused multiply-adds but svd3's own, the operation order of the header -----------------------------
def _det_cm(m):
    return ((m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 2, 1] * m[..., 1, 2])
             - m[..., 1, 0] * (m[..., 0, 1] * m[..., 2, 2] - m[..., 2, 1] * m[..., 0, 2]))
            + m[..., 2, 0] * (m[..., 0, 1] * m[..., 1, 2] - m[..., 1, 1] * m[..., 0, 2]))


def _ordered_sum(terms):
    """the terms (k, ...) added in ascending k to a sum that starts at 0.0f (numpy's accumulate is sequential)"""
    terms = np.asarray(terms, F)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + terms.shape[1:], F), terms]), axis=0, dtype=F)[-1]


class _Walk:
    """a minimum or maximum of the header: the first value met, replaced iff the next one is smaller (larger)"""

    def __init__(self, smaller):
        self.held, self.have, self.smaller = F(0), False, smaller

    def take(self, x):
        if not self.have or (x < self.held if self.smaller else x > self.held):
            self.held = x
        self.have = True


def element_frames(pos, ids, rest):
    """(P, F) of every element as the arrays [c][r] the kernels hold"""
    pos, rest = np.asarray(pos, F), np.asarray(rest, F).reshape(-1, 3, 3)
    x = pos[np.asarray(ids, np.int64).reshape(-1, 4)]
    P = x[:, 1:4, :] - x[:, 0:1, :]
    Fm = np.empty_like(P)
    for c in range(3):
        for r in range(3):
            Fm[:, c, r] = (P[:, 0, r] * rest[:, c, 0] + P[:, 1, r] * rest[:, c, 1]) + P[:, 2, r] * rest[:, c, 2]
    return P, Fm


def measure_elements(pos, ids, rest, lo, hi, volume=False, first=0, n=None, trace=None):
    """(records of ELEMENT_MEASURE_DTYPE for elements [first, first + n), summary as a dict) of the rule; trace: one word of T_* bits per
    element of the range.  A NONFINITE record holds its flags alone (its other words are unspecified)."""
    ids = np.asarray(ids).reshape(-1, 4)
    n = len(ids) - first if n is None else n
    lo, hi = np.broadcast_to(np.asarray(lo, F), (len(ids),)), np.broadcast_to(np.asarray(hi, F), (len(ids),))
    rec = np.zeros(n, capi.ELEMENT_MEASURE_DTYPE)
    low = np.zeros(n, F)  # fabsf(s[2])
    bits = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        P, Fm = element_frames(pos, ids[first:first + n], np.asarray(rest, F).reshape(-1, 9)[first:first + n])
        j, vol = _det_cm(Fm), _det_cm(P) / F(6)
        i1 = Fm[:, 0, 0] * Fm[:, 0, 0]
        for c in range(3):
            for r in range(3):
                if c or r:
                    i1 = i1 + Fm[:, c, r] * Fm[:, c, r]
        finite = (np.abs(Fm) < F(np.inf)).all(axis=(1, 2))
        for k in range(n):
            e = first + k
            if not finite[k]:
                rec[k]["flags"], bits[k] = T_NONFINITE, T_NONFINITE
                continue
            a = [F(v) for v in oracle_api.svd3(Fm[k])[0]]
            for (p, q), bit in zip(((0, 1), (1, 2), (0, 1)), (T_SWAP01, T_SWAP12, T_SWAP01B)):
                if a[p] < a[q]:
                    a[p], a[q] = a[q], a[p]
                    bits[k] |= bit
            inverted = bool(j[k] < F(0))
            if volume:
                prod = (a[0] * a[1]) * a[2]
                over, under = bool(prod > hi[e]), bool(prod < lo[e])
            else:
                over, under = bool(a[0] > hi[e]), bool(a[2] < lo[e])
            low[k] = a[2]
            s = [a[0], a[1], -a[2] if inverted else a[2]]
            g = [v * v - F(1) for v in s]
            green = F(0.5) * np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            flags = (T_INVERTED if inverted else 0) | (T_OVER if over else 0) | (T_UNDER if under else 0)
            rec[k] = (s, j[k], vol[k], i1[k], green, flags)
            bits[k] |= flags | (T_COLLAPSED if j[k] == 0 else 0) | (T_IDENTITY if np.array_equal(Fm[k], np.eye(3, dtype=F)) else 0)
    if trace is not None:
        trace.append(bits)
    # ---- the summary: tiles of 256 indices of the container, then the tiles ----
    names = ("max_stretch", "min_stretch", "min_j", "max_j", "max_green")
    source = (rec["s"][:, 0], low, rec["j"], rec["j"], rec["green"])
    total = [_Walk(smaller=name.startswith("min")) for name in names]
    tile_volumes = []
    for t in range(first // TILE, (first + n - 1) // TILE + 1 if n else 0):
        idx = np.array([k for k in range(max(t * TILE, first) - first, min((t + 1) * TILE, first + n) - first) if finite[k]], np.int64)
        if not len(idx):
            continue  # (a tile without an element that counts adds +0.0f and sets nothing)
        tile_volumes.append(_ordered_sum(rec["volume"][idx]))
        for walk, values, name in zip(total, source, names):
            tile = _Walk(smaller=name.startswith("min"))
            for k in idx:
                tile.take(values[k])
            walk.take(tile.held)
    summary = {name: walk.held for name, walk in zip(names, total)}
    summary["volume"] = _ordered_sum(tile_volumes) if tile_volumes else F(0)
    counted = rec["flags"][finite[:n]] if n else np.zeros(0, np.uint32)
    summary.update(inverted=int(((counted & T_INVERTED) != 0).sum()), over=int(((counted & T_OVER) != 0).sum()),
                   under=int(((counted & T_UNDER) != 0).sum()), nonfinite=int(n - len(counted)))
    return rec, summary


SUMMARY_FLOATS = ("max_stretch", "min_stretch", "min_j", "max_j", "max_green", "volume")
SUMMARY_COUNTS = ("inverted", "over", "under", "nonfinite")


def summary_words(summary):
    """the ten words of a summary (a dict of the restatement or a capi.ElementSummary): floats as their bits"""
    get = (lambda k: summary[k]) if isinstance(summary, dict) else (lambda k: getattr(summary, k))
    return np.array([F(get(k)) for k in SUMMARY_FLOATS], F).view(np.uint32).tolist() + [int(get(k)) for k in SUMMARY_COUNTS]


def node_tiles(first, count):
    return range(first // TILE, (first + count - 1) // TILE + 1) if count else range(0)


def measure_nodes(pos, vel, inv_mass, ranges, about=None, trace=None):
    """a structured array of NODE_SUMS_DTYPE, one entry per (first, count) range; trace: per range (tiles met, dynamic, fixed)"""
    pos, vel, w = np.asarray(pos, F), np.asarray(vel, F), np.asarray(inv_mass, F)
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    out = np.zeros(len(ranges), capi.NODE_SUMS_DTYPE)
    with np.errstate(all="ignore"):
        m = F(1) / w
        vm = vel * m[:, None]
        pm = pos * m[:, None]
        kinetic = F(0.5) * (m * ((vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]) + vel[:, 2] * vel[:, 2]))
        for r, (first, count) in enumerate(ranges):
            d = pos - (np.zeros(3, F) if about is None else np.asarray(about, F).reshape(-1, 3)[r])[None]
            ang = np.stack([d[:, 1] * vm[:, 2] - d[:, 2] * vm[:, 1], d[:, 2] * vm[:, 0] - d[:, 0] * vm[:, 2],
                            d[:, 0] * vm[:, 1] - d[:, 1] * vm[:, 0]], axis=1)
            terms = np.concatenate([m[:, None], vm, ang, pm, kinetic[:, None]], axis=1)  # the record's eleven floats
            tiles = []
            for t in node_tiles(first, count):
                idx = np.arange(max(t * TILE, first), min((t + 1) * TILE, first + count))
                tiles.append(_ordered_sum(terms[idx[w[idx] != 0]]) if (w[idx] != 0).any() else np.zeros(11, F))
            total = _ordered_sum(tiles) if tiles else np.zeros(11, F)
            inside = w[first:first + count]
            out[r] = (total[0], total[1:4], total[4:7], total[7:10], total[10], int((inside != 0).sum()), int((inside == 0).sum()))
            if trace is not None:
                trace.append((len(tiles), int(out[r]["dynamic"]), int(out[r]["fixed"])))
    return out


# ---- the independent fp64 formulation ------------------------------------------------------------------------------------------------
def measure_elements_f64(pos, ids, rest):
    """dict of s (m, 3; the last negated on an inverted element), j, volume, i1, green, finite and scale = the largest singular value"""
    pos = np.asarray(pos, np.float64)
    x = pos[np.asarray(ids, np.int64).reshape(-1, 4)]
    P = np.transpose(x[:, 1:4, :] - x[:, 0:1, :], (0, 2, 1))                         # columns x2 - x1, x3 - x1, x4 - x1
    Q = np.transpose(np.asarray(rest, np.float64).reshape(-1, 3, 3), (0, 2, 1))  # word 3 c + r -> row r, column c
    with np.errstate(all="ignore"):
        Fm = P @ Q
        finite = np.isfinite(Fm).all(axis=(1, 2))
        safe = np.where(finite[:, None, None], Fm, np.eye(3)[None])
        s = np.linalg.svd(safe, compute_uv=False)
        j = np.linalg.det(safe)
        s[:, 2] = np.where(j < 0, -s[:, 2], s[:, 2])
        vol = np.linalg.det(np.where(finite[:, None, None], P, np.eye(3)[None])) / 6.0
        green = 0.5 * np.sqrt(((s * s - 1.0) ** 2).sum(axis=1))
        pscale = np.linalg.norm(P, axis=1).prod(axis=1) / 6.0  # Hadamard: |det P| / 6 <= this
    return dict(s=s, j=j, volume=vol, i1=(safe * safe).sum(axis=(1, 2)), green=green, finite=finite, scale=s[:, 0], pscale=pscale)


def decisions_f64(m64, lo, hi, volume):
    """per element the relative distance of every discontinuous decision from its threshold, in units that do not depend on the
    element's size: j against 0 in units of s0^3; TET: s0 against max and |s2| against min in units of s0; VOLUME: the product of
    the unsigned values against both limits in units of s0^3.  (m, 3); an element whose j is exactly 0 reports +inf for j."""
    s, j, s0 = m64["s"], m64["j"], m64["scale"]
    dj = np.where(j == 0, np.inf, np.abs(j) / s0 ** 3)
    if volume:
        prod = s[:, 0] * s[:, 1] * np.abs(s[:, 2])
        return np.stack([dj, np.abs(prod - hi) / s0 ** 3, np.abs(prod - lo) / s0 ** 3], axis=1)
    return np.stack([dj, np.abs(s[:, 0] - hi) / s0, np.abs(np.abs(s[:, 2]) - lo) / s0], axis=1)


def flags_f64(m64, lo, hi, volume):
    s, j = m64["s"], m64["j"]
    if volume:
        prod = s[:, 0] * s[:, 1] * np.abs(s[:, 2])
        over, under = prod > hi, prod < lo
    else:
        over, under = s[:, 0] > hi, np.abs(s[:, 2]) < lo
    flags = (j < 0) * T_INVERTED + over * T_OVER + under * T_UNDER
    return np.where(m64["finite"], flags, T_NONFINITE).astype(np.uint32)


def measure_nodes_f64(pos, vel, inv_mass, ranges, about=None):
    """(sums (k, 11), the sums of the terms' magnitudes (k, 11): what a sum's rounding is a fraction of)"""
    pos, vel, w = np.asarray(pos, np.float64), np.asarray(vel, np.float64), np.asarray(inv_mass, np.float64)
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    sums, mags = np.zeros((len(ranges), 11)), np.zeros((len(ranges), 11))
    for r, (first, count) in enumerate(ranges):
        idx = np.arange(first, first + count)
        idx = idx[w[idx] != 0]
        m = 1.0 / w[idx]
        p, v = pos[idx], vel[idx] * m[:, None]
        a = np.zeros(3) if about is None else np.asarray(about, np.float64).reshape(-1, 3)[r]
        terms = np.concatenate([m[:, None], v, np.cross(p - a[None], v), p * m[:, None],
                                (0.5 * m * (vel[idx] ** 2).sum(axis=1))[:, None]], axis=1)
        sums[r], mags[r] = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    return sums, mags


def node_sums_matrix(out):
    """the eleven floats of every entry of a NODE_SUMS_DTYPE array, (k, 11)"""
    return np.concatenate([out["mass"][:, None], out["momentum"], out["angular"], out["moment"], out["kinetic"][:, None]], axis=1)


# ---- the scenes the CPU and GPU tests share ---------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_element_scene(n_elems, volume=False, seed=0):
    """Loose tetrahedra: the first min(7, n) elements are SPECIALS on lattice nodes of their own (unit corners: P = Qinv = 1 at
    creation), the others join random nodes of a shared cloud.  pos0: the rest pose the elements are created in; pos1: the pose
    that is measured.  Every decision of every element keeps MARGIN from its threshold in fp64 (decisions_f64) but the collapsed
    element's j, which is exactly 0."""
    rng = np.random.default_rng(1000 * n_elems + 10 * seed + int(volume))
    lo, hi = VOLUME_LIMITS if volume else TET_LIMITS
    specials = min(len(SPECIALS), n_elems)
    loose = n_elems - specials
    cloud = max(6, loose // 2) if loose else 0
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    pos0 = np.concatenate([corner + [2.0 * k, 0.0, 8.0] for k in range(specials)] + [np.round(rng.uniform(0, 4, (cloud, 3)) * 64) / 64])
    ids = [[4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3] for k in range(specials)]
    while len(ids) < n_elems:
        pick = 4 * specials + rng.choice(cloud, 4, replace=False)
        x = pos0[pick]
        if abs(np.linalg.det(x[1:] - x[0])) > 0.5:  # (a rest shape worth the name)
            ids.append(pick.tolist())
    ids = np.array(ids, np.uint32)
    pos0 = pos0.astype(F)
    pos1 = pos0.astype(np.float64)
    for k, name in enumerate(SPECIALS[:specials]):
        x = pos1[4 * k:4 * k + 4]
        if name == "rotated":
            x[1:] = x[0] + (x[1:] - x[0]) @ _rotation((1, 2, 3), 0.7).T
        elif name == "over":
            x[1] = x[0] + [1.5, 0, 0]
        elif name == "under":
            x[3] = x[0] + [0, 0, 0.5]
        elif name == "inverted":
            x[1] = x[0] + [-1.0, 0, 0]
        elif name == "collapsed":
            x[3] = x[0] + [1.0, 1.0, 0]
        elif name == "nan":
            x[2, 1] = np.nan
    rest = build_elements(capi, dict(pos0=pos0, ids=ids, lo=lo, hi=hi, volume=volume), capi.PBD, device=capi.DEVICE_NONE).rest(
        capi.VOLUME if volume else capi.TET)  # Qinv as the factory took it at pos0 (pies_get_rest: data, word 3 c + r)
    first_loose = 4 * specials
    pos1[first_loose:] += rng.normal(size=(cloud, 3)) * 0.12
    for _ in range(200):  # move the nodes of an element whose decision is too close to call
        near = (decisions_f64(measure_elements_f64(pos1.astype(F), ids, rest), lo, hi, volume) < 4 * MARGIN).any(axis=1)
        near[:specials] = False
        if not near.any():
            break
        nodes = np.unique(ids[near])
        pos1[nodes] = pos0[nodes] + rng.normal(size=(len(nodes), 3)) * 0.12
    else:
        raise AssertionError("no pose with the margin found")
    marks = {name: k for k, name in enumerate(SPECIALS[:specials])}
    return dict(pos0=pos0, pos1=pos1.astype(F), ids=ids, rest=rest, lo=lo, hi=hi, volume=volume, marks=marks)


def build_elements(pies, scene, solver, device=0):
    """the scene on a handle: nodes at pos0, the elements created there (TET, or VOLUME), then - the caller's step - pos1 written"""
    g = pies.Solver(pies.Options(solver=solver), device=device) if device else pies.Solver(pies.Options(solver=solver))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(scene["pos0"], radius=np.full(len(scene["pos0"]), 0.05, F))
    if scene["volume"]:
        g.add_volume(scene["ids"], 1.0, compression=float(scene["lo"]), stretching=float(scene["hi"]))
    else:
        g.add_tet(scene["ids"], 1.0, minStrain=float(scene["lo"]), maxStrain=float(scene["hi"]))
    return g


def make_node_scene(n_nodes, seed=0):
    """(pos, vel, inv_mass): a cloud with random masses, a tenth of it fixed, and a run of five fixed nodes from n // 3 on"""
    rng = np.random.default_rng(77 * n_nodes + seed)
    pos = (np.round(rng.uniform(-2, 2, (n_nodes, 3)) * 1024) / 1024).astype(F)
    vel = (rng.normal(size=(n_nodes, 3)) * 2).astype(F)
    inv_mass = (1.0 / rng.uniform(0.5, 2.0, n_nodes)).astype(F)
    inv_mass[rng.random(n_nodes) < 0.1] = 0
    if n_nodes >= 63:
        inv_mass[n_nodes // 3:n_nodes // 3 + 5] = 0
        inv_mass[0] = 1
    return pos, vel, inv_mass


def make_ranges(n_nodes, n_ranges, seed=0):
    """(ranges (k, 2), about (k, 3)): everything; the run of fixed nodes; an empty range; a range inside one tile; ranges that straddle
    one and two tile boundaries and overlap; random ones"""
    rng = np.random.default_rng(5 * n_nodes + n_ranges + seed)
    n = n_nodes
    ranges = [(0, n), (n // 3, min(5, n - n // 3)), (n // 2, 0), (min(3, n), min(40, n - min(3, n))), (min(200, n), min(100, n - min(200, n))),
              (min(250, n), min(300, n - min(250, n))), (n, 0)]
    while len(ranges) < n_ranges:
        first = int(rng.integers(0, n + 1))
        ranges.append((first, int(rng.integers(0, n - first + 1))))
    about = np.round(rng.uniform(-2, 2, (n_ranges, 3)) * 8) / 8
    return np.array(ranges[:n_ranges], np.uint32), about.astype(F)


# ---- the restatement against fp64 on the fixture ----------------------------------------------------------------------------------------
def element_deviation(scene):
    """(deviations of s, j, volume, i1, green - each a fraction of its natural scale -, the smallest decision margin, flags differing)
    of the restatement against fp64 on a scene of make_element_scene's layout"""
    rec, _ = measure_elements(scene["pos1"], scene["ids"], scene["rest"], scene["lo"], scene["hi"], bool(scene["volume"]))
    m64 = measure_elements_f64(scene["pos1"], scene["ids"], scene["rest"])
    ok = m64["finite"]
    s0 = m64["scale"][ok]
    dev = dict(
        s=float((np.abs(rec["s"][ok] - m64["s"][ok]).max(axis=1) / s0).max()),
        j=float((np.abs(rec["j"][ok] - m64["j"][ok]) / s0 ** 3).max()),
        volume=float((np.abs(rec["volume"][ok] - m64["volume"][ok]) / m64["pscale"][ok]).max()),
        i1=float((np.abs(rec["i1"][ok] - m64["i1"][ok]) / m64["i1"][ok]).max()),
        green=float((np.abs(rec["green"][ok] - m64["green"][ok]) / np.maximum(s0 ** 2, 1.0) ** 2).max()))
    margins = decisions_f64(m64, float(scene["lo"]), float(scene["hi"]), bool(scene["volume"]))[ok]
    differing = int((rec["flags"] != flags_f64(m64, float(scene["lo"]), float(scene["hi"]), bool(scene["volume"]))).sum())
    exact_zero = int(((m64["j"][ok] == 0) != (rec["j"][ok] == 0)).sum())  # the collapsed element is collapsed in both
    return dev, float(margins.min()), differing + exact_zero


def node_deviation(pos, vel, inv_mass, ranges, about):
    got = node_sums_matrix(measure_nodes(pos, vel, inv_mass, ranges, about)).astype(np.float64)
    want, mags = measure_nodes_f64(pos, vel, inv_mass, ranges, about)
    return float((np.abs(got - want) / np.where(mags > 0, mags, 1.0)).max())


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_scene(z, prefix):
    return {k: z[prefix + k] for k in ("pos1", "ids", "rest", "lo", "hi", "volume")}


def test_restatement_against_fp64():
    """The fp32 restatements against numpy.linalg.svd / det and fp64 sums on the fixture's scenes (600 elements with TET and with
    VOLUME limits, every special among them; 600 nodes in 64 ranges).  Each gate is four times the deviation the restatement showed
    when the fixture was written (recorded in the fixture and in DESIGN.md 8h): stretches 6.87e-7 of the element's largest singular
    value, j 5.49e-7 of s0^3, volume 1.44e-7 of the Hadamard bound, i1 1.06e-6, green 2.77e-7 of max(s0^2, 1)^2, node sums 3.24e-7 of
    the sum of the terms' magnitudes (the loose elements' rest shapes are random and far from regular: most of an element's figure is
    the conditioning of F = P Qinv, not the SVD).  Every decision (j < 0, over, under) keeps a margin of at least MARGIN = 1e-3 from its threshold in
    fp64 - thousands of deviations - so the restatement and fp64 agree on every flag of every element, none left out; the
    collapsed element's j is exactly 0 in both."""
    z = golden()
    for prefix in ("tet_", "vol_"):
        dev, margin, differing = element_deviation(golden_scene(z, prefix))
        print(prefix, "restatement vs fp64:", dev, "smallest margin %.3g" % margin)
        assert differing == 0
        for name, value in dev.items():
            recorded = float(z["dev_" + name])
            assert value <= 4 * recorded, (prefix, name, value, recorded)
            assert margin >= MARGIN > 4 * recorded
    dev = node_deviation(z["node_pos"], z["node_vel"], z["node_inv_mass"], z["node_ranges"], z["node_about"])
    print("node sums vs fp64: %.3g of the terms' magnitudes" % dev)
    assert dev <= 4 * float(z["dev_nodes"])
    # the recorded figures are the size such deviations have: a few 2^-24 for one element, n 2^-24 at the very worst for a sum
    assert all(float(z["dev_" + k]) < 2.0e-6 for k in ("s", "j", "volume", "i1", "green")) and float(z["dev_nodes"]) < 600 * 2.0 ** -24


def test_every_branch_occurs_in_the_shared_scenes():
    for volume in (False, True):
        scene = make_element_scene(600, volume)
        trace = []
        rec, summary = measure_elements(scene["pos1"], scene["ids"], scene["rest"], scene["lo"], scene["hi"], volume, trace=trace)
        bits, marks = trace[0], scene["marks"]
        assert bits[marks["rest"]] == T_IDENTITY and rec["green"][marks["rest"]] < 1e-6
        assert not bits[marks["rotated"]] & (T_IDENTITY | 15) and rec["green"][marks["rotated"]] < 1e-6
        assert bits[marks["over"]] & 15 == T_OVER and bits[marks["under"]] & 15 == T_UNDER
        assert bits[marks["inverted"]] & 15 == T_INVERTED and rec["s"][marks["inverted"]][2] < 0
        assert bits[marks["collapsed"]] & (15 - T_OVER | T_COLLAPSED) == T_UNDER | T_COLLAPSED and rec["j"][marks["collapsed"]] == 0
        assert bits[marks["nan"]] == T_NONFINITE and summary["nonfinite"] == 1
        loose = bits[len(SPECIALS):]
        for bit in (T_OVER, T_UNDER, T_SWAP01, T_SWAP12, T_SWAP01B):
            assert (loose & bit).any() and not (loose & bit).all(), bit
        assert summary["inverted"] >= 1 and summary["over"] > 1 and summary["under"] > 1
        assert summary["min_j"] < 0 < summary["max_j"] and summary["min_stretch"] == 0 and summary["max_stretch"] >= F(1.5)
    trace = []
    pos, vel, inv_mass = make_node_scene(600)
    ranges, about = make_ranges(600, 64)
    measure_nodes(pos, vel, inv_mass, ranges, about, trace=trace)
    assert {t for t, _, _ in trace} == {0, 1, 2, 3} and trace[1][1:] == (0, 5) and trace[2] == (0, 0, 0)
    assert trace[3][0] == 1 and trace[4][0] == 2 and trace[5][0] == 3 and trace[0][1] + trace[0][2] == 600 and trace[0][2] > 5


def test_rest_data_of_the_scenes():
    scene = make_element_scene(65)
    assert np.array_equal(scene["rest"][0], np.eye(3, dtype=F).reshape(9)) and scene["rest"].shape == (65, 9)
    P, Fm = element_frames(scene["pos0"], scene["ids"], scene["rest"])
    assert np.abs(Fm - np.eye(3, dtype=F)[None]).max() < 1e-5  # at pos0 every element is at rest


def test_sub_ranges_are_the_whole_ranges_records():
    scene = make_element_scene(600)
    args = (scene["pos1"], scene["ids"], scene["rest"], scene["lo"], scene["hi"])
    whole, total = measure_elements(*args)
    part, summary = measure_elements(*args, first=200, n=100)  # straddles a tile boundary: two tiles
    assert part.tobytes() == whole[200:300].tobytes() and summary["volume"] != 0
    a, b = measure_elements(*args, first=200, n=56)[1]["volume"], measure_elements(*args, first=256, n=44)[1]["volume"]
    assert summary["volume"] == F(F(0) + a) + b
    assert summary_words(measure_elements(*args, first=3, n=0)[1]) == [0] * 10


# ---- physics, on the fp64 formulation --------------------------------------------------------------------------------------------------
def _rest_body(seed=3, n=40):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 2, (12, 3))
    ids = []
    while len(ids) < n:
        pick = rng.choice(12, 4, replace=False)
        if abs(np.linalg.det(pos[pick][1:] - pos[pick][0])) > 0.3:
            ids.append(pick)
    ids = np.array(ids)
    rest = np.stack([np.linalg.inv((pos[e][1:] - pos[e][0]).T).T.reshape(9) for e in ids])  # word 3 c + r of inv(P)
    return pos, ids, rest


def test_a_rigid_motion_leaves_every_measure_at_rest():
    pos, ids, rest = _rest_body()
    at_rest = measure_elements_f64(pos, ids, rest)
    moved = measure_elements_f64(pos @ _rotation((2, -1, 0.5), 1.1).T + [3.0, -2.0, 0.25], ids, rest)
    assert np.abs(moved["s"] - 1).max() < 1e-12 and np.abs(moved["green"]).max() < 1e-12 and np.abs(moved["j"] - 1).max() < 1e-12
    assert np.allclose(moved["volume"], at_rest["volume"], rtol=1e-12, atol=0)


def test_a_uniform_scale_scales_stretch_and_volume():
    pos, ids, rest = _rest_body()
    at_rest, k = measure_elements_f64(pos, ids, rest), 1.75
    scaled = measure_elements_f64(pos * k, ids, rest)
    assert np.abs(scaled["s"] - k).max() < 1e-12 and np.allclose(scaled["volume"], at_rest["volume"] * k ** 3, rtol=1e-12, atol=0)
    assert np.allclose(scaled["green"], 0.5 * np.sqrt(3) * (k * k - 1), rtol=1e-12) and np.allclose(scaled["i1"], 3 * k * k, rtol=1e-12)


def test_a_mirrored_element_is_inverted():
    pos, ids, rest = _rest_body()
    mirrored = measure_elements_f64(pos * [-1.0, 1.0, 1.0], ids, rest)
    assert (flags_f64(mirrored, 0.8, 1.2, False) == T_INVERTED).all() and (mirrored["s"][:, 2] < 0).all()
    assert np.abs(mirrored["s"] - [1, 1, -1]).max() < 1e-12 and np.abs(mirrored["green"]).max() < 1e-12


def test_momentum_of_a_translating_body():
    pos, _, inv_mass = make_node_scene(300)
    v = np.array([1.5, -0.25, 2.0])
    vel = np.broadcast_to(v, pos.shape)
    sums, mags = measure_nodes_f64(pos, vel, inv_mass, [(0, 300), (40, 100)])
    for row, mag in zip(sums, mags):
        mass, com = row[0], row[7:10] / row[0]
        assert np.allclose(row[1:4], mass * v, rtol=1e-13) and np.isclose(row[10], 0.5 * mass * (v @ v), rtol=1e-13)
    # ... and about its centre of mass it has no angular momentum, within the sums' rounding
    for k, (first, count) in enumerate([(0, 300), (40, 100)]):
        com = sums[k, 7:10] / sums[k, 0]
        about_com, mags = measure_nodes_f64(pos, vel, inv_mass, [(first, count)], about=com)
        assert (np.abs(about_com[0, 4:7]) <= 1e-13 * mags[0, 4:7]).all()
        # the fp32 restatement: zero within the deviation the fixture records, as a fraction of the terms' magnitudes
        got = node_sums_matrix(measure_nodes(pos, vel, inv_mass, [(first, count)], about=com.astype(F)))[0]
        bound = 4 * float(golden()["dev_nodes"]) + 2.0 ** -23  # (+ the rounding of the centre itself to fp32)
        assert (np.abs(got[4:7]) <= bound * mags[0, 4:7] + 2.0 ** -23 * np.abs(v).max() * sums[k, 0] * np.abs(com).max()).all()


# ---- the entry points on a host-only handle ---------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device_check():
    g = capi.Solver(capi.Options(solver=capi.PD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    L, h = capi.load(), g._h
    tets, vols, nodes = g.count(capi.TET), g.count(capi.VOLUME), g.count(capi.NODES)
    assert tets > 0 and vols == tets
    summary = capi.ElementSummary()
    summary.over = 7

    def elements(type, first, n):
        return L.pies_measure_elements(h, type, first, n, None, C.byref(summary))

    for bad in (capi.POSITION, capi.DISTANCE, capi.BEND, capi.SHAPE, -1, 99):
        assert elements(bad, 0, 1) == capi.ERR_INVALID and "type" in g.last_error(), bad
    for type, size in ((capi.TET, tets), (capi.VOLUME, vols)):
        assert elements(type, 0, size + 1) == capi.ERR_INVALID and "range" in g.last_error()
        assert elements(type, size, 1) == capi.ERR_INVALID and elements(type, 0xFFFFFFFF, 2) == capi.ERR_INVALID
        assert summary.over == 7  # (a refused call writes nothing)
        assert elements(type, 0, size) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
        assert elements(type, size - 1, 1) == capi.ERR_HIP
        summary.over = 7
        assert elements(type, 3, 0) == capi.OK and elements(type, size, 0) == capi.OK and summary_words(summary) == [0] * 10
        summary.over = 7
    assert L.pies_measure_elements(h, capi.TET, 0, 0, None, None) == capi.OK
    assert L.pies_measure_elements(None, capi.TET, 0, 0, None, None) == capi.ERR_INVALID
    with pytest.raises(capi.PiesError):
        g.measure_elements(capi.TET)
    rec, summ = g.measure_elements(capi.TET, 5, 0)
    assert len(rec) == 0 and summary_words(summ) == [0] * 10

    out = (capi.NodeSums * 65)()

    def sums(ranges, about=None, n=None, null=False):
        r = np.array(ranges, np.uint32).reshape(-1, 2)
        a = None if about is None else np.array(about, F).reshape(-1, 3)
        return L.pies_measure_nodes(h, len(r) if n is None else n, None if null else r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    None if a is None else a.ctypes.data_as(C.POINTER(C.c_float)), out)

    assert sums([(0, 1)] * 65) == capi.ERR_UNSUPPORTED and "64" in g.last_error()
    assert sums([(0, 1)], n=1, null=True) == capi.ERR_INVALID and "NULL" in g.last_error()
    assert L.pies_measure_nodes(h, 1, np.zeros(2, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == capi.ERR_INVALID
    for bad in ((0, nodes + 1), (nodes, 1), (nodes + 1, 0), (0xFFFFFFFF, 2)):
        assert sums([(0, nodes), bad]) == capi.ERR_INVALID and "range 1" in g.last_error(), bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert sums([(0, nodes), (1, 2)], about=[(0, 0, 0), (0, bad, 0)]) == capi.ERR_INVALID and "about" in g.last_error()
    assert sums([(0, nodes), (nodes, 0), (3, 0)]) == capi.ERR_HIP and "PIES_DEVICE_NONE" in g.last_error()
    assert sums([(0, nodes)] * 64, about=np.ones((64, 3))) == capi.ERR_HIP
    assert sums([], n=0, null=True) == capi.OK and L.pies_measure_nodes(h, 0, None, None, None) == capi.OK
    assert L.pies_measure_nodes(None, 0, None, None, None) == capi.ERR_INVALID
    with pytest.raises(capi.PiesError):
        g.measure_nodes([(0, nodes)])
    assert len(g.measure_nodes([])) == 0


def test_binding_declares_the_entry_points():
    assert {"pies_measure_elements", "pies_measure_nodes"} <= set(capi.SYMBOLS) and capi.MEASURE_RANGE_MAX == 64
    assert C.sizeof(capi.ElementMeasure) == 32 == capi.ELEMENT_MEASURE_DTYPE.itemsize and C.sizeof(capi.ElementSummary) == 40
    assert C.sizeof(capi.NodeSums) == 52 == capi.NODE_SUMS_DTYPE.itemsize
    L = capi.load()
    assert L.pies_measure_elements.restype is C.c_int and len(L.pies_measure_elements.argtypes) == 6
    assert L.pies_measure_nodes.restype is C.c_int and len(L.pies_measure_nodes.argtypes) == 5
    assert L.pies_abi_version() == 4
    assert (capi.ELEMENT_INVERTED, capi.ELEMENT_OVER, capi.ELEMENT_UNDER, capi.ELEMENT_NONFINITE) == (1, 2, 4, 8)
