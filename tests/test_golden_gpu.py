"""The committed fp64 golden vectors (tests/golden/*.npz, generator tests/golden/make_golden.py) run through the HIP path.

tests/test_oracle_golden.py pins the CPU oracle with these vectors; the device's 3x3 SVD, its CCD and its projections share
their hand-made algorithms with that oracle, so device == oracle says nothing about the algorithms themselves.  Here every
record goes through the C ABI - one-constraint scenes built with the bulk raw ingestion (pies_add_*_constraints +
pies_set_rest), one tick - and is compared with the fp64 expectation at the tolerance the oracle's test uses:

* PBD (Src/Solver.cpp:58-75 through Include/Pies/Constraints.h:121-129): w = 1, one iteration, no gravity: the tick leaves
  pos + 1 * (projection - pos);  tetrahedral strain (Src/Constraints.cpp:76-128), distance (:11-37), bend (:312-366), in all
  three schedules (k_wave, k_tet / k_distance / k_bend, k_layer);
* PD local steps (Src/Solver.cpp:270-349, Src/Constraints.cpp:205-255): one local/global iteration of a scene of independent
  elements is a 4 x 4 (2 x 2) solve per element whose right-hand side holds the projection: positions against the fp64 solve
  with the golden projections, for the strain and the volume step alone (k_pd_local_tet), the fused pair (tiles / packed) and
  distance / bend;
* point-triangle CCD (Src/CollisionDetection.cpp:227-302): two-triangle scenes, the contact list (pies_get_tri_contacts)
  against the fp64 decisions;
* PD group constraints (Src/ShapeMatchingConstraint.cpp:6-177): isolated shape groups (shape_projection.npz), one scalar equation
  per node with the projection on the right-hand side, through k_pd_local_shape and the fp64 contribution slots;
* PD contacts (Src/Solver.cpp:240-262, 367-484, 680-875; Src/CollisionConstraint.cpp): the ordered contact list with the reference's
  duplicates, the node-pair list, the contact rows of the global step, the stabilisation passes (they shift prevPosition) and the
  three friction loops in the reference's order - isolated records (pd_contact_response.npz) in every variant of the contact
  rows, the sequential passes, the launch path, the CG and the right-hand side, and a whole loop with all three contact families
  (pd_contacts_tiny.npz), also renumbered.  Before these the contact response was held to the oracle alone, which shares its
  algorithms - and, for the node contacts, was fed the device's own list;
* the whole-loop PBD restatement (pbd_tiny_coll{0,1}.npz) tick by tick under schedule EXACT, pd_tiny.npz under PD
  (test_pd_parity_gpu.py), pd_groups_tiny.npz - shape groups, a goal and a mass write on the live scene - under PD.
"""
import importlib.util
import os

import numpy as np
import pytest

from test_oracle_golden import (build_contact_scene, build_pd_contacts_tiny, build_pd_groups, build_shape_scene, contact_options, contact_records,
                                contact_tick_lists, pd_groups_edits, run_contact_response_oracle, set_contact_tick, shape_gate, shape_options,
                                shape_records)
from test_pd_parity_gpu import record

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = np.float32(0.012)  # fixedTimestepSize, one substep


def load(name):
    return np.load(os.path.join(G, name))


def golden_module():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(G, "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


SCHEDULES = ["exact", "coloured", "layered"]


def pbd_solver(pies, schedule):
    # no gravity, the floor far below, no node-node pass: one iteration of one container is the whole tick
    g = pies.Solver(pies.Options(solver=pies.PBD, iterations=1, timeSubsteps=1, fixedTimestepSize=float(H), gravity=0.0,
                                 floorHeight=-1.0e6, damping=0.0), device=0)
    g.set_flag(pies.FLAG_NODE_COLLISIONS, 0)
    g.set_schedule({"exact": pies.SCHEDULE_EXACT, "coloured": pies.SCHEDULE_COLOURED, "layered": pies.SCHEDULE_LAYERED}[schedule])
    return g


def blend(x, proj):
    """Constraints.h:125-128 with w = 1, in fp32 like the device: pos += 1 * (proj - pos) moves pos to proj up to an ulp of |pos|"""
    return np.abs(x).max() * 2.4e-7


# ---- PBD projections -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_tet_strain_projection_goldens_through_pbd(pies, schedule):
    d = load("tet_projection.npz")
    x, q, exp = d["x"], d["qinv"], d["expected"]
    n = len(x)
    g = pbd_solver(pies, schedule)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01)
    g.add_tet(np.arange(4 * n, dtype=np.uint32).reshape(n, 4), 1.0, float(d["lo"]), float(d["hi"]))
    g.set_rest(pies.TET, q)  # the golden's rest state (the factory took it from the deformed positions)
    assert np.array_equal(g.rest(pies.TET), q)
    g.tick(1)
    out = g.positions.reshape(n, 4, 3)
    g.close()
    worst = 0.0
    for k in range(n):
        scale = max(1.0, np.abs(exp[k]).max())
        err = np.abs(out[k] - exp[k]).max()
        assert err <= 5e-5 * scale + blend(x[k], exp[k]), (k, err)
        worst = max(worst, err)
    assert worst > 0


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_svd_goldens_through_pbd(pies, schedule):
    """svd_fixed.npz: fixed(F) of 600 matrices (well and ill conditioned, inverted, nearly equal singular values) - a unit
    reference tetrahedron at the origin (Qinv = I) whose edges are the columns of A reproduces it"""
    d = load("svd_fixed.npz")
    A, exp = d["A"], d["expected"]
    n = len(A)
    x = np.zeros((n, 4, 3), np.float32)
    x[:, 1:] = np.transpose(A, (0, 2, 1))
    g = pbd_solver(pies, schedule)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01)
    g.add_tet(np.arange(4 * n, dtype=np.uint32).reshape(n, 4), 1.0, float(d["lo"]), float(d["hi"]))
    g.set_rest(pies.TET, np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1)))
    g.tick(1)
    out = g.positions.reshape(n, 4, 3)
    g.close()
    for k in range(n):
        Fh = out[k, 1:].T
        cond = np.linalg.cond(A[k].astype(np.float64))
        tol = 2e-5 if cond < 1e3 else 2e-4
        assert np.abs(Fh - exp[k]).max() <= tol + blend(x[k], exp[k]), (k, cond)
        assert np.abs(out[k, 0]).max() <= 1e-6  # the first node goes to the origin (Constraints.cpp:124)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_distance_projection_goldens_through_pbd(pies, schedule):
    d = load("distance_projection.npz")
    x, t, exp = d["x"], d["target"], d["expected"]
    n = len(x)
    g = pbd_solver(pies, schedule)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01)
    g.add_distance(np.arange(2 * n, dtype=np.uint32).reshape(n, 2), 1.0)
    g.set_rest(pies.DISTANCE, t)
    g.tick(1)
    out = g.positions.reshape(n, 2, 3)
    g.close()
    for k in range(n):
        assert np.abs(out[k] - exp[k]).max() <= 1e-5 + blend(x[k], exp[k]), k
        assert np.array_equal(out[k, 1], x[k, 1])  # node b never moves (Constraints.cpp:34-36)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_bend_projection_goldens_through_pbd(pies, schedule):
    d = load("bend_projection.npz")
    x, im, a, exp = d["x"], d["invMass"], d["angle"], d["expected"]
    n = len(x)
    g = pbd_solver(pies, schedule)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01, invMass=im.reshape(-1))
    g.add_bend(np.arange(4 * n, dtype=np.uint32).reshape(n, 4), 1.0)
    g.set_rest(pies.BEND, a)
    g.tick(1)
    out = g.positions.reshape(n, 4, 3)
    g.close()
    for k in range(n):
        scale = max(1.0, np.abs(exp[k] - x[k]).max())
        assert np.abs(out[k] - exp[k]).max() <= 2e-4 * scale + blend(x[k], exp[k]), k


# ---- PD local steps --------------------------------------------------------------------------------------------------------
def tet_A(q):
    """A = [0; Qinv^T D] (Constraints.cpp:157-176) from a column-major Qinv, fp64"""
    Qm = q.astype(np.float64).reshape(3, 3)  # Qm[r][k] = Qinv[col r][row k]
    Dm = np.array([[-1, 1, 0, 0], [-1, 0, 1, 0], [-1, 0, 0, 1]], dtype=np.float64)
    A = np.zeros((4, 4))
    A[1:] = Qm @ Dm
    return A


def pd_solver(pies):
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=1, timeSubsteps=1, fixedTimestepSize=float(H), gravity=0.0,
                                 floorHeight=-1.0e6, damping=0.0), device=0)
    g.set_flag(pies.FLAG_TRIANGLE_COLLISIONS, 0)
    g.set_pcg(1e-7, 128)
    return g


def inertia(inv_mass):
    """diag of Solver.cpp:179-182 as the device computes it: 1 / (invMass * h^2) in fp32"""
    return (np.float32(1.0) / (np.float32(inv_mass) * (H * H))).astype(np.float64)


# fp32 noise of an element's 4 x 4 solve with the inertia term at the size of the constraint term (condition number 2-3): the
# matrix entries, the right-hand side and the CG (relative residual 1e-7) each contribute a few ulp of the largest coordinate
SOLVE_NOISE = 1.5e-6


@pytest.mark.parametrize("which", ["strain", "volume", "pair"])
def test_tet_and_volume_projection_goldens_through_the_pd_local_step(pies, which):
    """One local/global iteration of independent elements: x_new = (m/h^2 + sum A^T A)^-1 (m/h^2 x + sum A^T p) with the projections p
    of the golden files (fp64).  Every element's nodes get the mass that puts m/h^2 at the largest eigenvalue of its sum A^T A:
    the 4 x 4 system then has condition number ~ 2, and an error dp of the device's projection moves x_new by K^-1 A^T dp - the
    test asks for that to stay below what the oracle's golden tolerance (5e-5 x scale on p) allows, plus the solve's fp32 noise."""
    ds, dv = load("tet_projection.npz"), load("volume_projection.npz")
    assert np.array_equal(ds["x"], dv["x"]) and np.array_equal(ds["qinv"], dv["qinv"])
    x, q = ds["x"], ds["qinv"]
    n = len(x)
    ids = np.arange(4 * n, dtype=np.uint32).reshape(n, 4)
    # (on, golden projections, tolerance on p: the oracle's test passes both at 5e-5 x scale.  The device's PD volume step computes
    # computeD's ten fixed-point iterations (Constraints.cpp:186-203) with one division and three products instead of three divisions
    # and shares one recomposition with the strain step: on the records the iteration has not converged on - a
    # uniformly compressed element, sigma = 0.3 -> 1 - the different rounding is carried through the ten iterations and shows as up to
    # 1.3e-4 against 5e-5 for the reference's own order of operations; PD parity is by tolerance: four times the oracle's)
    parts = [(which in ("strain", "pair"), ds["expected"], 5e-5), (which in ("volume", "pair"), dv["expected"], 2e-4)]
    AtA = np.array([sum(tet_A(q[k]).T @ tet_A(q[k]) for on, _, _ in parts if on) for k in range(n)])
    lam = np.array([np.linalg.eigvalsh(M)[-1] for M in AtA])
    inv_mass = (1.0 / (lam * float(H) ** 2)).astype(np.float32)
    g = pd_solver(pies)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01, invMass=np.repeat(inv_mass, 4))
    if parts[0][0]:
        g.add_tet(ids, 1.0, float(ds["lo"]), float(ds["hi"]))
        g.set_rest(pies.TET, q)
    if parts[1][0]:
        g.add_volume(ids, 1.0, float(dv["lo"]), float(dv["hi"]))
        g.set_rest(pies.VOLUME, q)
    g.tick(1)
    out = g.positions.reshape(n, 4, 3)
    if which == "pair":
        assert g.launch_counts().get("pd_local_volume", 0) == 0  # the fused strain + volume step ran (tiles or packed pairs)
    g.close()
    sharp = 0
    worst = []
    for k in range(n):
        A = tet_A(q[k])
        m = float(inertia(inv_mass[k]))
        K = m * np.eye(4) + AtA[k]
        rhs = m * x[k].astype(np.float64)
        ptol = 0.0
        for on, exp, tp in parts:
            if on:
                rhs = rhs + A.T @ exp[k]
                ptol += tp * max(1.0, np.abs(exp[k]).max())
        want = np.linalg.solve(K, rhs)
        gain = np.abs(np.linalg.solve(K, A.T)).sum(axis=1).max()  # |dx|_inf <= gain |dp|_inf (per projection)
        tol = gain * ptol + SOLVE_NOISE * max(np.abs(want).max(), np.abs(x[k]).max())
        err = np.abs(out[k] - want).max()
        worst.append((err / tol, k, err, tol))
        sharp += np.abs(want - x[k]).max() > 50 * tol  # the element moves by far more than the tolerance: the check has teeth
    worst.sort(reverse=True)
    print("PD local step [%s]: largest error / tolerance over %d records:" % (which, n), ["%.2f (record %d)" % (w[0], w[1]) for w in worst[:5]])
    assert worst[0][0] <= 1.0, worst[:5]
    assert sharp > 0.8 * n


def test_distance_projection_goldens_through_the_pd_local_step(pies):
    d = load("distance_projection.npz")
    x, t, exp = d["x"], d["target"], d["expected"]
    n = len(x)
    INV_MASS = np.float32(1.0) / (H * H)  # m / h^2 = 1 against A^T A = [[.5, -.5], [-.5, .5]]
    g = pd_solver(pies)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01, invMass=float(INV_MASS))
    g.add_distance(np.arange(2 * n, dtype=np.uint32).reshape(n, 2), 1.0)
    g.set_rest(pies.DISTANCE, t)
    g.tick(1)
    out = g.positions.reshape(n, 2, 3)
    g.close()
    m = float(inertia(INV_MASS))
    A = np.array([[0.5, -0.5], [-0.5, 0.5]])  # A = B (Constraints.cpp:44-52)
    for k in range(n):
        want = np.linalg.solve(m * np.eye(2) + A.T @ A, m * x[k].astype(np.float64) + A.T @ (A @ exp[k]))
        assert np.abs(out[k] - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), k


def test_bend_projection_goldens_through_the_pd_local_step(pies):
    d = load("bend_projection.npz")
    x, im, a, exp = d["x"], d["invMass"], d["angle"], d["expected"]
    n = len(x)
    w = 7000.0  # of the order of m / h^2 = 3 500 ... 14 000 for these inverse masses
    g = pd_solver(pies)
    g.add_nodes_raw(x.reshape(-1, 3), radius=0.01, invMass=im.reshape(-1))
    g.add_bend(np.arange(4 * n, dtype=np.uint32).reshape(n, 4), w)
    g.set_rest(pies.BEND, a)
    g.tick(1)
    out = g.positions.reshape(n, 4, 3)
    g.close()
    for k in range(n):
        m = inertia(im[k])[:, None]  # A = B = I (Constraints.cpp:376-384): one scalar equation per node
        want = (m * x[k].astype(np.float64) + w * exp[k]) / (m + w)
        scale = max(1.0, np.abs(exp[k] - x[k]).max())
        assert np.abs(out[k] - want).max() <= 2e-4 * scale, k


# ---- PD group constraints: shape and goal matching ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_reference(oracle):
    """shape_projection.npz and what the oracle makes of it (one scene, one tick, shared by the variants below)"""
    recs = shape_records()
    o = oracle.OracleSolver(shape_options(oracle))
    build_shape_scene(o, recs)
    o.tick()
    assert not o.failed
    return recs, o.positions


SHAPE_VARIANTS = {"default": {}, "rhs_kernel": {"PIES_PD_FUSE_RHS": "0"}, "rhs_fused": {"PIES_PD_FUSE_RHS": "1"},
                  "cg_two_launch": {"PIES_PD_CG_SINGLE": "0"}, "cg_single": {"PIES_PD_CG_SINGLE": "1"},
                  "no_graph": {"PIES_NO_GRAPH": "1"}, "renumber_flag": {}}


@pytest.mark.parametrize("variant", list(SHAPE_VARIANTS))
def test_shape_projection_goldens_through_the_pd_local_step(pies, tune, shape_reference, variant):
    """k_pd_local_shape, one workgroup per group, and the fp64 contribution slots rhs_of_node adds: every isolated group of
    shape_projection.npz (sizes below, at and above a wavefront and a workgroup, and 600; rotations up to 2.8 rad; groups at the
    origin and 100 units away) in one scene on node ranges of their own, one tick, against the fp64 restatement
    x_new = (m x + w p) / (m + w).  Gate per record: twice the oracle's own distance from the restatement, or the solve's fp32
    noise.  The variants change who adds up the slots (k_pd_rhs or the CG's residual kernel), the CG form and the launch path; all
    meet the same gate.  (renumber_flag: K of this scene is diagonal, so the library finds nothing to gain and keeps the host's
    order - the variant holds that decision path to the gate; groups under a renumbering that does apply are in
    test_pd_groups_tiny_scene_goldens[renumbered].)"""
    recs, ora = shape_reference
    for name, value in SHAPE_VARIANTS[variant].items():
        tune(name, value)
    g = pd_solver(pies)
    if variant == "renumber_flag":
        g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
    build_shape_scene(g, recs)
    g.tick(1)
    out = g.positions
    assert not g.failed and g.pcg_health()["short_solves"] == 0 and np.isfinite(out).all()
    assert g.count(pies.PD_CG_SINGLE) == (0 if variant == "cg_two_launch" else 1) and g.count(pies.NODES_RENUMBERED) == 0
    g.close()
    first, worst, by_size = 0, [], {}
    for k, (r, x, im, w, exp) in enumerate(recs):
        n = len(r)
        d_ora = float(np.abs(ora[first:first + n] - exp).max())
        assert d_ora <= shape_gate(x), (k, d_ora)  # (the oracle's own gate: a gate made of its distance needs it close)
        gate = max(2.0 * d_ora, SOLVE_NOISE * max(float(np.abs(x).max()), float(np.abs(exp).max())))
        err = float(np.abs(out[first:first + n] - exp).max())
        worst.append((err / gate, k, n, err, gate))
        by_size[n] = max(by_size.get(n, 0.0), err / gate)
        first += n
    for n, ratio in by_size.items():
        record("golden_shape_projection[%s]" % variant, "error_over_gate_size_%d" % n, ratio, 1.0)
    worst.sort(reverse=True)
    print("shape matching [%s]: largest error / gate:" % variant, ["%.2f (record %d, n = %d)" % w[:3] for w in worst[:5]])
    assert worst[0][0] <= 1.0, worst[:5]


def build_pd_groups_shuffled(s, d, hid):
    """build_pd_groups with the node ids of the two bodies shuffled together (fixture node i is host node hid[i]): the box from
    raw nodes and containers, since createTetBox numbers its own"""
    gm = golden_module()
    W, Hh, D = (int(v) for v in d["dims"])
    box, tets, _ = gm.lattice(W, Hh, D, d["translation"], 1.0)
    rest = np.concatenate([box.astype(np.float32), d["loose"]])
    n = len(rest)
    at = np.empty_like(rest)
    at[hid] = rest
    im = np.empty(n, np.float32)
    im[hid] = d["invMass"]
    s.add_nodes_raw(at, radius=0.475, invMass=im)
    s.add_tet(hid[tets].astype(np.uint32), 1.0, 0.8, 1.0)
    s.add_volume(hid[tets].astype(np.uint32), 1.0, 1.0, 1.0)
    s.add_triangles(hid[gm.box_triangles(W, Hh, D)].astype(np.uint32))
    off = d["group_offsets"]
    for k in range(len(off) - 1):
        s.add_shape(hid[d["group_ids"][off[k]:off[k + 1]]].astype(np.uint32), float(d["group_w"][k]))
    s.add_goal(hid[d["goal_ids"]].astype(np.uint32), float(d["goal_w"]))
    for name in ("pos", "vel"):
        a = np.empty_like(d[name])
        a[hid] = d[name]
        (s.set_velocities if name == "vel" else s.set_positions)(a)
        if name == "pos":
            s.set_prev_positions(a)


@pytest.mark.parametrize("layout", ["plain", "renumbered"])
def test_pd_groups_tiny_scene_goldens(pies, tune, layout):
    """pd_groups_tiny.npz: the whole PD loop with shape groups (nodes in one to four of them: the fp64 slot loop of rhs_of_node), a
    goal whose transform is set before tick 0 and again before tick 2, and pies_write_nodes(INV_MASS) on every node before tick 3 -
    the rebuilt system takes the new masses into K and P and keeps each group's Qinv (the rebuild starts the rotations over from
    the identity; the iteration converges, so that cannot show).  Tick by tick against the fp64 restatement at pd_tiny's gates.
    renumbered: the two bodies' host ids shuffled together and 64-row chunks, so that the library does renumber these 156 nodes."""
    d = load("pd_groups_tiny.npz")
    n = len(d["pos"])
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=int(d["iterations"])), device=0)
    g.set_pcg(1e-7, 256)  # (the written masses spread 40 : 1, see test_live_edits_pd_gpu.test_node_write)
    if layout == "renumbered":
        tune("PIES_CG_CHUNK_ROWS", "64")
        g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
        hid = np.random.default_rng(3).permutation(n)
        build_pd_groups_shuffled(g, d, hid)
    else:
        hid = np.arange(n)
        build_pd_groups(g, d)
    g.finalize()
    assert g.count(pies.NODES_RENUMBERED) == (1 if layout == "renumbered" else 0)
    assert g.count(pies.SHAPE) == len(d["group_w"]) and g.count(pies.GOAL) == 1
    for t, (p, v) in enumerate(zip(d["expected_pos"], d["expected_vel"])):
        pd_groups_edits(g, d, t, hid)
        g.tick()
        ep, ev = float(np.abs(g.positions[hid] - p).max()), float(np.abs(g.velocities[hid] - v).max())
        record("golden_pd_groups_tiny[%s]" % layout, "positions", ep, 2e-4)
        record("golden_pd_groups_tiny[%s]" % layout, "velocities", ev, 2e-4 / 0.012)
        print("pd_groups_tiny [%s] tick %d: |dpos| %.3g |dvel| %.3g" % (layout, t, ep, ev))
        assert ep <= 2e-4 and ev <= 2e-4 / 0.012, (t, ep, ev)
    assert g.pcg_health()["short_solves"] == 0 and not g.failed
    g.close()


# ---- PD contacts: lists and response -------------------------------------------------------------------------------------------
CONTACT_VARIANTS = {"default": {}, "rows_inline": {"PIES_TRI_FAST_ROWS": "0"}, "rows_pass": {"PIES_TRI_FAST_ROWS": "1"},
                    "rows_pass_unmerged": {"PIES_TRI_FAST_ROWS": "1", "PIES_ROW_MAX_UNIQUE": "4"}, "sequential_l2": {"PIES_TRI_LDS": "0"},
                    "no_graph": {"PIES_NO_GRAPH": "1"}, "cg_two_launch": {"PIES_PD_CG_SINGLE": "0"}, "rhs_kernel": {"PIES_PD_FUSE_RHS": "0"}}


@pytest.fixture(scope="module")
def contact_reference(oracle):
    """pd_contact_response.npz and what the oracle makes of its two scenes (one tick each, shared by the variants below)"""
    out = {}
    for which in ("pt", "nn"):
        d, o = run_contact_response_oracle(oracle, which)
        out[which] = (d, o.positions, o.prev_positions, o.velocities)
    return out


def contact_gates(test, d, which, ora, dev, records):
    """Per record and state array: the oracle's own distance from the restatement within shape_gate (velocities: over h), the
    device within max(twice that distance, the solve's fp32 noise on the record's coordinates); recorded, then asserted."""
    worst = []
    for label, a, b in records:
        x = d[which + "_pos"][a:b]
        size = max(float(np.abs(x).max()), float(np.abs(d[which + "_expected_pos"][a:b]).max()))
        for k, (name, key, per) in enumerate((("positions", "pos", 1.0), ("prev_positions", "prev", 1.0), ("velocities", "vel", float(H)))):
            exp = d[which + "_expected_" + key][a:b]
            d_ora = float(np.abs(ora[k][a:b] - exp).max())
            assert d_ora <= shape_gate(x) / per, (label, name, d_ora)  # (a gate made of the oracle's distance needs it close)
            gate = max(2.0 * d_ora, SOLVE_NOISE * size / per)
            err = float(np.abs(dev[k][a:b] - exp).max())
            print("%s %-14s %-62s device %.3g oracle %.3g gate %.3g" % (test, name, label, err, d_ora, gate))
            record(test, name, err / gate, 1.0)
            worst.append((err / gate, label, name, err, gate))
    worst.sort(reverse=True)
    assert worst[0][0] <= 1.0, worst[:5]


@pytest.mark.parametrize("variant", list(CONTACT_VARIANTS))
def test_pd_contact_response_goldens(pies, tune, contact_reference, variant):
    """pd_contact_response.npz through the device, one tick per variant of the global step's contact rows (summed inline, in a
    pass of their own, unmerged), of the order-dependent stabilisation and friction passes (on the LDS copy or through L2), of
    the launch path, the CG form and the right-hand side.  Point-triangle scene: pies_get_tri_contacts equals the restatement's
    ordered list - the device keeps a triangle once per bucket walk and multiplies by the cells two ranges share, the reference
    lists a hit once per shared cell: 1, 2, 4 and 8 copies here, and none for the target that lies exactly in an integer plane.
    Node-node scene (PIES_FLAG_PD_NODE_CONTACTS): the pair list in its order.  Positions, previous positions (the stabilisation
    shifts them) and velocities (three friction loops in the reference's order) per record at twice the oracle's own distance
    from fp64 or the solve's noise.  These scenes' passes run level by level; the single-wavefront walk needs more than 2048
    levels and has no fp64 scene - test_chain_deeper_than_the_level_cap_takes_the_walk holds it bit for bit to the level form,
    and this test holds the level form to fp64."""
    for name, value in CONTACT_VARIANTS[variant].items():
        tune(name, value)
    for which in ("pt", "nn"):
        d, *ora = contact_reference[which]
        g = pies.Solver(contact_options(pies, d), device=0)
        g.set_pcg(1e-7, 256)
        if which == "nn":
            g.set_flag(pies.FLAG_PD_NODE_CONTACTS, 1)
        build_contact_scene(g, d, which)
        g.tick(1)
        dev = (g.positions, g.prev_positions, g.velocities)
        tri, pairs = g.tri_collisions.reshape(-1, 4), g.node_contacts().reshape(-1, 2)
        health, failed = g.pcg_health(), g.failed
        g.close()
        assert not failed and health["short_solves"] == 0 and all(np.isfinite(a).all() for a in dev)
        if which == "pt":
            assert np.array_equal(tri, d["pt_contacts"]), (len(tri), len(d["pt_contacts"]))
            assert len(pairs) == 0
        else:
            assert len(tri) == 0
            assert [tuple(sorted(p)) for p in pairs.tolist()] == [tuple(p) for p in d["nn_pairs"].tolist()]
        contact_gates("golden_pd_contact_response[%s,%s]" % (variant, which), d, which, ora, dev, contact_records(d, which))


BYSTANDERS = 37  # loose nodes far from the scene: with them the system has more rows than one 64-row chunk, so a numbering can gain


def build_pd_contacts_tiny_shuffled(s, d, hid):
    """build_pd_contacts_tiny with the host ids of all bodies shuffled together (fixture node i is host node hid[i]), built like
    build_pd_groups_shuffled: the boxes from raw nodes and containers, since createTetBox numbers its own.  The host ids that hid
    leaves out are bystanders: single nodes 40 units away that touch nothing.  Returns the bystanders' state arrays."""
    gm = golden_module()
    W, Hh, D = (int(v) for v in d["dims"])
    nb = W * Hh * D
    n = len(d["radius"])
    total = n + BYSTANDERS
    rest = d["pos"][0].copy()
    tets, tris = [], []
    for k, tr in enumerate(d["translations"]):
        box, t, _ = gm.lattice(W, Hh, D, tr.astype(np.float64), float(d["spacing"]))
        rest[k * nb:(k + 1) * nb] = box.astype(np.float32)  # the elements' rest state is where the nodes are added
        tets.append(t + k * nb)
        tris.append(gm.box_triangles(W, Hh, D) + k * nb)
    tets, tris = np.concatenate(tets), np.concatenate(tris + [d["loose_triangles"].astype(np.int64)])
    far = np.float32([[40.0 + 3.0 * (k % 7), 5.0 + 3.0 * (k // 7), 40.0] for k in range(total)])
    at, radius, im = far.copy(), np.full(total, 0.2, np.float32), np.ones(total, np.float32)
    at[hid], radius[hid], im[hid] = rest, d["radius"], d["invMass"]
    s.add_nodes_raw(at, radius=radius, invMass=im)
    s.add_tet(hid[tets].astype(np.uint32), 1.0, 0.8, 1.0)
    s.add_volume(hid[tets].astype(np.uint32), 1.0, 1.0, 1.0)
    s.add_triangles(hid[tris].astype(np.uint32))
    return dict(pos=far, prev=far, vel=np.zeros_like(far))


def pairs_per_node(pairs):
    """node -> its pairs in list order: what the sequential friction loop's result depends on (pairs without a common node commute)"""
    out = {}
    for p in pairs:
        for v in p:
            out.setdefault(v, []).append(p)
    return out


TINY_CONTACT_VARIANTS = {"default": {}, "rows_pass": {"PIES_TRI_FAST_ROWS": "1"}, "sequential_l2": {"PIES_TRI_LDS": "0"}, "no_graph": {"PIES_NO_GRAPH": "1"},
                         "renumbered": {"PIES_CG_CHUNK_ROWS": "64"}}


@pytest.mark.parametrize("variant", list(TINY_CONTACT_VARIANTS))
def test_pd_contacts_tiny_scene_goldens(pies, tune, variant):
    """pd_contacts_tiny.npz: two tet boxes, one landing on the other, and loose spheres - point-triangle contacts both ways (listed
    up to eighteen times each), floor contacts and node pairs in one system, nodes on which two and all three friction loops meet.
    Tick by tick from the stored fp32 state against the fp64 restatement: the contact list in its order with its duplicates, the
    node-pair set, the state at pd_tiny's gates.  (The floor contacts have no getter on the device; the oracle's list is held to
    the restatement's in test_oracle_golden.py, and a wrong one shows in the positions of the bottom layer.)  renumbered: the host
    ids of all bodies shuffled together (and 37 bystanders, so that there is more than one 64-row chunk): the library renumbers,
    the lists come back in host ids, and the pair key is the host ids' whatever the device's numbering - a friction loop in the
    order of the device's ids, as it ran before this test existed, missed the velocity gate of tick 2 by a factor of three under
    the shuffle first tried."""
    d = load("pd_contacts_tiny.npz")
    for name, value in TINY_CONTACT_VARIANTS[variant].items():
        tune(name, value)
    n = len(d["radius"])
    g = pies.Solver(contact_options(pies, d), device=0)
    g.set_pcg(1e-7, 256)
    g.set_flag(pies.FLAG_PD_NODE_CONTACTS, 1)
    if variant == "renumbered":
        g.set_flag(pies.FLAG_RENUMBER_NODES, 1)
        # (the pair key is taken over the host's ids, so a shuffle of them reorders the friction loop: this one - most do not -
        # keeps the order of every node's pairs in all six ticks, which is all the loop's result depends on; asserted below)
        hid = np.random.default_rng(0).permutation(n + BYSTANDERS)[:n]
        others = build_pd_contacts_tiny_shuffled(g, d, hid)
    else:
        hid, others = np.arange(n), None
        build_pd_contacts_tiny(g, d)
    g.finalize()
    assert g.count(pies.NODES_RENUMBERED) == (1 if variant == "renumbered" else 0)
    back = {int(h): i for i, h in enumerate(hid)}
    test = "golden_pd_contacts_tiny[%s]" % variant
    for t in range(len(d["pos"])):
        tri, floor, pairs = contact_tick_lists(d, t)
        set_contact_tick(g, d, t, hid, others)
        g.tick()
        assert np.array_equal(g.tri_collisions.reshape(-1, 4), hid[tri]), (t, len(g.tri_collisions), len(tri))
        listed = [tuple(sorted(int(back[v]) for v in p)) for p in g.node_contacts().reshape(-1, 2).tolist()]  # in the fixture's ids
        want = [tuple(p) for p in pairs.tolist()]
        assert set(listed) == set(want) and len(listed) == len(want) == g.count(pies.NODE_CONTACTS), (t, listed)
        if variant != "renumbered":
            assert listed == want, (t, listed)  # ascending pair key: the friction loop's order
        assert pairs_per_node(listed) == pairs_per_node(want), (t, listed)  # every node meets its partners in the fixture's order
        ep, eq, ev = (float(np.abs(getattr(g, name)[hid] - d["expected_" + key][t]).max())
                      for name, key in (("positions", "pos"), ("prev_positions", "prev"), ("velocities", "vel")))
        print("%s tick %d: |dpos| %.3g |dprev| %.3g |dvel| %.3g" % (test, t, ep, eq, ev))
        record(test, "positions", ep, 2e-4)
        record(test, "prev_positions", eq, 2e-4)
        record(test, "velocities", ev, 2e-4 / 0.012)
        assert ep <= 2e-4 and eq <= 2e-4 and ev <= 2e-4 / 0.012, (t, ep, eq, ev)
    assert g.pcg_health()["short_solves"] == 0 and not g.failed
    g.close()


# ---- point-triangle CCD ----------------------------------------------------------------------------------------------------
def test_point_triangle_ccd_goldens_through_the_contact_list(pies, tune):
    """Every golden case (a point a against a moving triangle b, c, d, relative to b) as a scene of two triangles: (b, c, d) with b
    at the origin - the differences the device forms are the golden's bits - and (a, e, f) with e, f three units off the
    plane.  The reference tests each node of a searching triangle against the other triangle, both ways (Solver.cpp:757-797): the
    contact list must hold (a, b, c, d) exactly when the golden says hit, and the other five tests must come out as the fp64
    CCD of the generator decides them (cases on an edge of a triangle are left out of that part, as in the generator)."""
    gm = golden_module()
    d = load("point_triangle_ccd.npz")
    thr = float(d["threshold"])
    tune("PIES_NO_GRAPH", "1")  # 400 tiny scenes: eager launches instead of 400 graph instantiations
    hits = checked_aux = 0
    for case, (args, (hit, _t)) in enumerate(zip(d["args"], d["expected"])):
        ap0, ab0, ac0, ap1, ab1, ac1 = (v.astype(np.float32) for v in args)
        n0 = np.cross(ab0.astype(np.float64), ac0.astype(np.float64))
        n0 /= np.linalg.norm(n0)
        up = (3.0 * n0 * (1.0 if n0 @ ap0 >= 0 else -1.0))
        e = (ap0 + up + [0.4, 0.1, -0.2]).astype(np.float32)
        f = (ap0 + up + [-0.3, 0.2, 0.5]).astype(np.float32)
        zero = np.zeros(3, np.float32)
        prev = np.stack([ap0, e, f, zero, ab0, ac0])  # nodes 0..5 = a, e, f, b, c, d
        cur = np.stack([ap1, e, f, zero, ab1, ac1])
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=1, gravity=0.0, floorHeight=-1.0e6, collisionThresholdDistance=thr), device=0)
        g.add_nodes_raw(cur, radius=0.01)
        g.add_triangles(np.uint32([[0, 1, 2], [3, 4, 5]]))
        g.set_prev_positions(prev)  # the swept test runs from prevPosition to position; zero velocity: the predict step moves nothing
        g.tick(1)
        got = {tuple(int(v) for v in c) for c in g.tri_collisions.reshape(-1, 4)}
        assert not g.failed
        g.close()
        assert ((0, 3, 4, 5) in got) == bool(hit), (case, hit, got)
        hits += bool(hit)
        # the other five tests of the pair, decided by the generator's fp64 CCD on the same fp32 positions
        want, sure = set(), True
        for tri, other in (((0, 1, 2), (3, 4, 5)), ((3, 4, 5), (0, 1, 2))):
            B, Cn, Dn = other
            for A in tri:
                if (A, B, Cn, Dn) == (0, 3, 4, 5):
                    continue
                rel = [(prev[A] - prev[B]), (prev[Cn] - prev[B]), (prev[Dn] - prev[B]), (cur[A] - cur[B]), (cur[Cn] - cur[B]), (cur[Dn] - cur[B])]
                ok, _, margin = gm.ccd_fp64(*rel, thr)
                if abs(margin) < 1e-3:
                    sure = False
                if ok:
                    want.add((A, B, Cn, Dn))
        if sure:
            checked_aux += 1
            assert got - {(0, 3, 4, 5)} == want, (case, got, want)
    assert 100 < hits < 300 and checked_aux > 300


# ---- whole loops -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", [0, 1])
def test_pbd_tiny_scene_goldens_under_the_reference_order(pies, coll):
    """pbd_tiny_coll{0,1}.npz: an independent fp64 restatement of Solver::tickPBD (with the hash / node-node loop for coll = 1),
    one tick at a time from the stored fp32 state, schedule EXACT (the reference's container order and node-node order)"""
    d = load("pbd_tiny_coll%d.npz" % coll)
    W, Hh, D = (int(v) for v in d["dims"])
    g = pies.Solver(pies.Options(solver=pies.PBD, iterations=int(d["iterations"])), device=0)
    g.create_tet_box(W, Hh, D, translation=d["translation"], scale=float(d["spacing"]), w=float(d["w_tet"]), volume=False, triangles=False)
    g.create_box(W, Hh, D, scale=float(d["spacing"]), w=float(d["w_dist"]), existing_offset=0, triangles=False)
    g.set_radii(np.full(W * Hh * D, d["radius"], np.float32))
    g.set_flag(pies.FLAG_NODE_COLLISIONS, int(d["collisions"]))
    g.set_schedule(pies.SCHEDULE_EXACT)
    for t in range(len(d["pos"]) - 1):
        g.set_positions(d["pos"][t])
        g.set_velocities(d["vel"][t])
        g.tick(1)
        assert np.abs(g.positions - d["pos"][t + 1]).max() <= 2e-4, t
        assert np.abs(g.velocities - d["vel"][t + 1]).max() <= 2e-4 / 0.012, t
    if coll:
        assert g.collision_pairs > 0
    g.close()
