"""The tetrahedral projection of k_layer with columns 0, 1 of its matrices held side by side (tet_rows.h) at the class sizes at which
the colour loop can go wrong - 1 element, 63, 64 and 65 (the wavefront's edge), 300 elements against a workgroup forced to 256 threads
(the loop for the rest of a class) - on elements that take each path of the decomposition.  After 2 ticks positions, previous
positions and velocities equal, byte for byte, the same build with PIES_LAYER_TET_FORM=0 (tet_core) and the oracle replaying the
exported order.  Each size runs with the rest dictionary (4 sets) and with more than 64 sets (the streamed records).

The scene: N fans of K tetrahedra.  The tetrahedra of a fan share their first node and nothing else, so they conflict with each
other and with no element of another fan: K colour classes of N elements each.  Qinv = I and the shared node sits at the origin, so
the matrix handed to the SVD is an element's three other nodes as they stand, and the blend (quirk Q2: node 1 is drawn towards 0)
leaves the shared node where it is: every element meets the matrix it was given, whatever its colour.  The matrices are those of
tests/cpp/tet_rows_example.cpp, whose statistics say which path each kind takes:
  rest        the identity, diagonal matrices, a diagonal matrix and one more entry: fewer than two pairs out of tolerance
  flattened   a column exactly zero, and R1 diag(s0, s1, 0) R2: the completion of a collapsed direction
  inverted    a perturbed identity with a negative determinant: the smallest singular value flipped
  sweeps      R1 diag(s0, s1, s2) R2 with condition numbers of 1e3 .. 1e6: the rotating sweeps
  generic     a perturbed identity: closed form, one rotation, polish, one clean snapshot (the path of the headline)
(K = 2, and K = 66 for the class of 1 so that the scene has more than 64 elements to give more than 64 sets.  Every node is
kept at x >= 0 - an edge and its negative span the same singular values - so that the planner's levelling starts at the shared
nodes and the scene is one tile: the largest colour class is then N, asserted here and on host-only handles.)"""
import numpy as np
import pytest

STATE = ("positions", "prev_positions", "velocities")
KINDS = ("rest", "flattened", "inverted", "sweeps", "generic")
# name: (N = elements of a colour class, K = classes, forced workgroup or None)
SIZES = {"class_1": (1, 66, None), "class_63": (63, 2, None), "class_64": (64, 2, None), "class_65": (65, 2, None),
         "class_300_block256": (300, 2, 256)}


def _rotation(rng):
    q = rng.uniform(-1.0, 1.0, 4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _matrix(kind, n, rng):
    """the n-th matrix of a kind (row j = edge j of the element)"""
    if kind == "rest":
        a = np.diag([1.0, 1.0, 1.0] if n % 3 == 0 else rng.uniform(0.3, 2.0, 3))
        if n % 3 == 2:
            i, k = ((0, 1), (0, 2), (1, 2))[(n // 3) % 3]
            a[i, k] = rng.uniform(-1.0, 1.0)
        return a
    if kind == "flattened":
        if n % 2:
            return _rotation(rng) @ np.diag([rng.uniform(0.3, 2.0), rng.uniform(0.3, 2.0), 0.0]) @ _rotation(rng)
        a = np.diag(rng.uniform(0.3, 2.0, 3))
        z = (n // 2) % 3
        a[z, z] = 0.0
        a[(z + 1) % 3, (z + 2) % 3] = rng.uniform(-1.0, 1.0)
        return a
    if kind == "inverted":
        a = np.eye(3) + rng.uniform(-0.3, 0.3, (3, 3))
        a[:, n % 3] *= -1.0
        return a
    if kind == "sweeps":
        s = [rng.uniform(0.5, 2.0), 10.0 ** -rng.uniform(0.0, 6.0), 10.0 ** -rng.uniform(3.0, 6.0)]
        return _rotation(rng) @ np.diag(s) @ _rotation(rng)
    return np.eye(3) + rng.uniform(-0.3, 0.3, (3, 3))


def elements(size, seed=11):
    """node positions (fans x (1 + 3 K) x 3, the shared node first) and the kind of every element, fan by fan"""
    n_fans, k, _ = SIZES[size]
    rng = np.random.default_rng(seed)
    x = np.zeros((n_fans, 1 + 3 * k, 3), np.float32)
    kinds = []
    for f in range(n_fans):
        for e in range(k):
            kind = KINDS[(f + 2 * e) % len(KINDS)]  # (every class meets every kind; so does a class of 1 over its 66 colours)
            a = np.diag([5.0, 1.0, 1.0]) if f == 0 and e == 0 else _matrix(kind, f * k + e, rng)
            # every node at x >= 0 (an edge and its negative span the same singular values), and then the sign of the determinant
            # the kind wants, by mirroring y: the shared nodes, at x = 0, are where the planner's levelling starts, every other
            # node is one level on, and the scene is one tile; fan 0's first element makes x the longest axis
            a[a[:, 0] < 0.0] *= -1.0
            if kind in ("inverted", "generic") and (np.linalg.det(a) < 0.0) != (kind == "inverted"):
                a[:, 1] *= -1.0
            x[f, 1 + 3 * e:4 + 3 * e] = a.astype(np.float32)
            kinds.append(kind)
    return x, kinds


def _build(pies_like, s, size, streamed):
    n_fans, k, _ = SIZES[size]
    x, _ = elements(size)
    s.add_nodes_raw(x.reshape(-1, 3), radius=0.01)
    per = 1 + 3 * k
    ids = np.uint32([[f * per, f * per + 1 + 3 * e, f * per + 2 + 3 * e, f * per + 3 + 3 * e] for f in range(n_fans) for e in range(k)])
    n = len(ids)
    # the dictionary: 4 sets (two w values x two strain intervals); streamed: every element its own w, more than 64 sets
    for j in range(n if streamed else 4):
        part = ids[j:j + 1] if streamed else ids[j::4]
        w = 0.05 + 0.9 * j / n if streamed else (0.35, 0.8)[j % 2]
        lo, hi = (0.8, 1.0) if streamed or j < 2 else (0.6, 1.2)
        s.add_tet(part, float(w), lo, hi)
    s.set_rest(pies_like.TET, np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1)))
    return n


def _options(m):
    return m.Options(solver=m.PBD, iterations=2, timeSubsteps=1, fixedTimestepSize=0.012, gravity=0.0, floorHeight=-1.0e6, damping=0.0)


def _solver(pies, size, streamed, device=0):
    g = pies.Solver(_options(pies), device=device)
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    n = _build(pies, g, size, streamed)
    g.finalize()
    return g, n


def _check_plan(pies, g, size, streamed, n):
    n_fans, k, block = SIZES[size]
    assert g.count(pies.LAYER_MAX_CLASS) == n_fans, g.count(pies.LAYER_MAX_CLASS)  # a colour class is one element of every fan
    assert g.count(pies.LAYER_MAX_TILES) <= 256  # (an instantiation that has the row-pair form)
    if block:
        assert n_fans > block  # the largest class exceeds the forced workgroup: the loop for the rest of a class
    assert n > 64
    sets = g.count(pies.LAYER_REST_SETS)
    assert sets == (0 if streamed else 4), sets


def _run(pies, size, streamed, oracle=None):
    g, n = _solver(pies, size, streamed)
    _check_plan(pies, g, size, streamed, n)
    assert g.launch_counts()["layer"] > 0  # schedule LAYERED is what runs
    o = None
    if oracle is not None:
        o = oracle.OracleSolver(_options(oracle))
        o.set_flag(oracle.FLAG_NODE_COLLISIONS, 0)
        _build(oracle, o, size, streamed)
        o.permute(pies.TET, g.order(pies.TET))
        o.tick(2)
    g.tick(2)
    out = {k: getattr(g, k) for k in STATE}
    g.close()
    return out, o


@pytest.mark.gpu
@pytest.mark.parametrize("streamed", [False, True], ids=["dictionary", "over_64_sets"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_row_pairs_at_class_sizes(pies, oracle, tune, size, streamed):
    if SIZES[size][2]:
        tune("PIES_LAYER_BLOCK", str(SIZES[size][2]))
    new, o = _run(pies, size, streamed, oracle)
    tune("PIES_LAYER_TET_FORM", "0")
    old, _ = _run(pies, size, streamed)
    for k in STATE:
        assert np.isfinite(new[k]).all(), k
        assert new[k].tobytes() == old[k].tobytes(), k
        assert new[k].tobytes() == getattr(o, k).astype(new[k].dtype, copy=False).tobytes(), k


@pytest.mark.parametrize("streamed", [False, True], ids=["dictionary", "over_64_sets"])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_scene_has_its_classes(pies, tune, size, streamed):
    """(host only) the plan of the scene: the largest colour class, the tiles, the sets of the rest dictionary; every kind present"""
    if SIZES[size][2]:
        tune("PIES_LAYER_BLOCK", str(SIZES[size][2]))
    g, n = _solver(pies, size, streamed, device=pies.DEVICE_NONE)
    _check_plan(pies, g, size, streamed, n)
    g.close()
    assert set(elements(size)[1]) == set(KINDS)
