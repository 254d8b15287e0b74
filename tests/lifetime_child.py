"""Child process of tests/test_handle_lifetime_gpu.py: `python lifetime_child.py <scenario>` runs one scenario in a process whose
resource ledger (pies_resource_counts) starts at zero and prints one JSON line per checkpoint,
    {"at": tag, "live": {kind: n}, "created": {kind: n}, ...};
the parent asserts on them.  Scenarios: cycle-layered, cycle-rest, extensions, edits-pbd, edits-pd, errors (see the parent's docstring).  The device buffers of
tests/device_buffers.py come from the runtime directly, not through the library: the ledger does not see them."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "benchlib")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import scenes  # noqa: E402
from pies_amd import capi  # noqa: E402

U, F = np.uint32, np.float32
DT = 0.012
T0 = time.perf_counter()


def mark(tag, **extra):
    r = capi.resource_counts()
    print(json.dumps(dict(at=tag, live=r["live"], created=r["created"], seconds=round(time.perf_counter() - T0, 3), **extra)), flush=True)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def pbd(iterations=4, **kw):
    return capi.Solver(scenes.pbd_options(capi, iterations, **kw))


def pbd_layered():
    """test_handle_reuse_gpu.scene_a: the 6 x 6 x 12 beam, schedule LAYERED, node-node collisions"""
    from test_handle_reuse_gpu import options, scene_a
    g = capi.Solver(options(capi))
    scene_a(capi, g)
    return g


def pbd_exact():
    """schedule EXACT: a beam, a bend sheet and position constraints"""
    g = pbd()
    g.set_schedule(capi.SCHEDULE_EXACT)
    scenes.build_beam(g, (4, 4, 8), translation=(0.0, 0.6, 0.0))
    g.create_bend_sheet(6, 5, translation=(6.0, 2.0, 0.0))
    g.add_position(U([0, 1, 2, 3]), 2.0)
    scenes.perturb(g, 7, 0.05)
    return g


def loose(order, turns=False):
    def build():
        p, v = scenes.loose_particles((6, 7, 8))
        g = pbd()
        g.addNodes(p)
        g.set_velocities(v)
        g.set_flag(capi.FLAG_COLLISION_ORDER, order)
        return g
    build.turns = turns
    return build


def pd_beam():
    """test_handle_reuse_gpu.scene_b: volume, triangles, node contacts, a listed pair"""
    from test_handle_reuse_gpu import options, scene_b
    g = capi.Solver(options(capi))
    scene_b(capi, g)
    return g


def pd_groups():
    """PD with shape and goal groups (the scene of test_pd_parity_gpu's group test, one box)"""
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
    g.create_shape_matching_box((0, 1.0, 0), 4, 3, 5, 30.0)
    g.add_shape(np.arange(10, 40, dtype=U), 3.0)
    g.add_goal(np.arange(0, 12, dtype=U), 20.0)
    scenes.perturb(g, 4, 0.03)
    g.set_prev_positions(g.positions)
    return g


CYCLE = [("pbd-layered", pbd_layered), ("pbd-exact", pbd_exact), ("loose-reference", loose(0)), ("loose-groups", loose(1)),
         ("loose-pairs", loose(2)), ("loose-reference-turns", loose(0, turns=True)), ("pd-beam", pd_beam), ("pd-groups", pd_groups)]


def cycle(scenes_=None):
    mark("start")
    for name, build in (CYCLE if scenes_ is None else [c for c in CYCLE if c[0] in scenes_]):
        turns = getattr(build, "turns", False)
        if turns:
            capi.set_tuning("PIES_REFERENCE_TURNS", "1")
        try:
            g = build()
            nodes = g.count(capi.NODES)
            g.finalize()
            mark(name + ":finalized", nodes=nodes)
            g.tick(2)
            mark(name + ":ticked", nodes=nodes)
            g.tick()
            mark(name + ":first", nodes=nodes)
            g.tick(19)
            pbd_counters = dict(g.collision_health(), fallbacks=g.collision_fallbacks) if name.startswith(("pbd", "loose")) else {}
            mark(name + ":last", nodes=nodes, failed=bool(g.failed), finite=bool(np.isfinite(g.positions).all()), **pbd_counters)
            g.close()
        finally:
            if turns:
                capi.set_tuning("PIES_REFERENCE_TURNS", None)
        mark(name + ":closed")


# ---- extensions ------------------------------------------------------------------------------------------------------------------
BEAM = (4, 4, 8)


def sphere_mesh(centre):
    from test_trimesh import icosphere
    v, tri = icosphere(1, 1.0, centre)
    return np.asarray(v, F), np.asarray(tri, U)


def extension_scene(g, kind):
    """the beam with surface triangles, a lattice body from a closed mesh (pies_add_tri_mesh_volume: before the first finalize, it
    changes the scene), a skin on the beam and two fields; returns what the calls need"""
    if kind == "pd":
        g.create_tet_box(*BEAM, translation=(0.0, 0.52, 0.0), w=1.0, volume=True, triangles=True)
        g.add_position(U([BEAM[2] * (j + BEAM[1] * i) for i in range(BEAM[0]) for j in range(BEAM[1])]), 2.0)
    else:
        g.set_schedule(capi.SCHEDULE_LAYERED)
        g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
        scenes.build_beam(g, BEAM, translation=(0.0, 0.52, 0.0), triangles=True)
    beam_nodes, beam_tris = g.count(capi.NODES), g.count(capi.TRIANGLES)
    tets = g.ids(capi.TET).reshape(-1, 4).copy()
    v, tri = sphere_mesh((8.0, 2.0, 1.5))
    g.add_tri_mesh_volume(v, tri, 4)
    scenes.perturb(g, 9, 0.03)
    g.set_prev_positions(g.positions)
    p = g.positions
    verts = np.stack([p[tets[k]].mean(0) for k in range(0, len(tets), 3)]).astype(F)
    skin_tri = U([[k, k + 1, k + 2] for k in range(0, len(verts) - 2, 3)])
    skin = g.add_skin(verts, tets, skin_tri)
    from test_fields import box_mesh, sphere_field
    samples, origin, cell = sphere_field()
    f0 = g.add_field(samples, origin, float(cell))
    f1 = g.add_field_tri_mesh(*box_mesh(), 0.37, 0.6)
    return dict(kind=kind, beam_nodes=beam_nodes, beam_tris=beam_tris, skin=skin, skin_verts=len(verts), fields=(f0, f1),
                mesh=(v, tri))


def extension_calls(g, S, hip, scale=1):
    """every entry point that allocates lazily, once; `scale` multiplies the rays, points and props"""
    from device_buffers import DevBuf
    from test_trimesh import lattice_of
    rng = np.random.default_rng(3)
    lo, hi = F([-1.0, 0.0, -1.0]), F([4.0, 4.5, 8.0])

    def points(n):
        return (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F)

    def rays(n):
        o = points(n) + F([0.0, 6.0, 0.0])
        return o, np.tile(F([0.1, -1.0, 0.05]), (n, 1))
    g.raycast(*rays(64 * scale))                                    # narrow
    g.raycast(*rays(600 * scale))                                   # wide
    g.raycast(*rays(64 * scale), target=capi.RAY_SKIN, skin=S["skin"])
    g.closest_points(points(100 * scale), winding=True)
    centres = points(8 * scale)
    g.collide_props([capi.Prop.sphere(c, 0.4) for c in centres], node_prop=True)
    g.collide_field_props([capi.FieldProp.make(S["fields"][k % 2], c) for k, c in enumerate(centres)], node_prop=True)
    g.apply_forces([capi.Force.wind((1.0, 0.0, 0.0), 1.0, shear=0.2)], DT)
    g.apply_surface_loads([capi.SurfaceLoad.gas(1.0, 60.0, first=0, count=S["beam_tris"]).with_drag(0.5, (1.0, 0.0, 0.0))], DT)
    g.measure_elements(capi.TET)
    n = g.count(capi.NODES)
    g.measure_nodes([[0, S["beam_nodes"]], [S["beam_nodes"], n - S["beam_nodes"]]])
    g.read_skin(S["skin"])
    frame = g.tick_begin()
    g.export_acquire(frame)
    g.export_acquire_skin(frame, S["skin"])
    g.export_release(frame)
    bufs = [DevBuf(hip, 3 * n) for _ in range(3)] + [DevBuf(hip, 3 * S["skin_verts"]) for _ in range(2)]
    g.read_nodes_device(position=bufs[0].ptr, prev_position=bufs[1].ptr, velocity=bufs[2].ptr, flags=capi.IO_HOST_SYNC)
    g.write_nodes_device(position=bufs[0].ptr, prev_position=bufs[1].ptr, velocity=bufs[2].ptr, flags=capi.IO_HOST_SYNC)
    g.read_skin_device(S["skin"], bufs[3].ptr, bufs[4].ptr, flags=capi.IO_HOST_SYNC)
    for b in bufs:
        b.get()
        b.free()
    v, tri = S["mesh"]
    origin, cell, dims = lattice_of(v, 4 * min(scale, 2))
    g.voxelize_tri_mesh(v, tri, origin, float(cell), dims)
    g.profile_in_situ(capi.KERNEL_NAMES.index("pd_cg_update" if S["kind"] == "pd" else "layer"), 2)
    g.tick()


def extensions():
    from device_buffers import Hip
    hip = Hip()
    mark("start")
    for kind in ("pbd", "pd"):
        g = pbd() if kind == "pbd" else capi.Solver(capi.Options(solver=capi.PD, iterations=10))
        S = extension_scene(g, kind)
        g.finalize()
        mark(kind + ":finalized", nodes=g.count(capi.NODES), skin_vertices=g.count(capi.SKIN_VERTICES))
        extension_calls(g, S, hip)
        mark(kind + ":L1")
        for k in range(3):
            extension_calls(g, S, hip)
            mark(kind + ":same-%d" % k)
        for k in range(2):
            extension_calls(g, S, hip, scale=4)
            mark(kind + ":big-%d" % k)
            extension_calls(g, S, hip)
            mark(kind + ":small-%d" % k)
        g.clear()
        mark(kind + ":cleared")
        S = extension_scene(g, kind)
        g.finalize()
        mark(kind + ":rebuilt-finalized")
        extension_calls(g, S, hip)
        mark(kind + ":rebuilt-L1", failed=bool(g.failed), finite=bool(np.isfinite(g.positions).all()))
        g.close()
        mark(kind + ":closed")


# ---- edits -----------------------------------------------------------------------------------------------------------------------
def edit_round(g, kind, rnd, S0):
    """the edits of tests/live_edits.py's users on a live handle, ticks between.  A round ends where the first began: every flag
    and setting is back, and the node state S0 is written back before the last rebuild - buffers sized by the scene's state (the
    layered plan's tiles and colours are planned from the positions) then have the size they had a round ago"""
    from live_edits import node_edit, put_state, state_of
    pd = kind == "pd"
    S = state_of(g)
    for what in ("positions", "prev_positions", "velocities", "radii"):
        getattr(g, "set_" + what)(node_edit(what, S, radius_factor=1.0 + 0.01 * (rnd % 2)))
        g.tick()
    m = S["inv_masses"].copy()
    m[1::2] *= F(2.0 if rnd % 2 == 0 else 0.5)
    g.set_inv_masses(m)  # PD: the system is rebuilt
    g.tick()
    container = capi.TET if pd else capi.DISTANCE
    rest = g.rest(container)
    g.set_rest(container, rest[3:9], first=3)  # a partial write
    g.tick()
    if pd:
        t = np.eye(4, dtype=F)
        t[1, 3] = F(0.01 * (rnd + 1))
        g.set_goal_transform(0, t.T.reshape(16))  # column-major
        g.tick()
    # every flag of the API, on either solver (a flag the solver does not read still dirties the scene: the rebuild is the point).
    # PD with FLAG_RENUMBER_NODES: off, the device holds host numbering and the renumbering's tables go; on, they come back
    for flag, was in EDIT_FLAGS[kind]:
        g.set_flag(flag, 1 - was)
        g.tick()
        if pd and flag == capi.FLAG_RENUMBER_NODES:
            assert g.count(capi.NODES_RENUMBERED) == 0
        g.set_flag(flag, was)
        g.tick()
    if pd:
        assert g.count(capi.NODES_RENUMBERED) == 1
    # the legacy spelling of the collision order: 1 = the reference's order, 0 = the pair order (where both handles stand)
    g.set_flag(capi.FLAG_REFERENCE_COLLISION_ORDER, 1)
    g.tick()
    g.set_flag(capi.FLAG_REFERENCE_COLLISION_ORDER, 0)
    g.tick()
    if not pd:
        for order in (capi.COLLISION_ORDER_REFERENCE, capi.COLLISION_ORDER_GROUPS, capi.COLLISION_ORDER_PAIRS):
            g.set_flag(capi.FLAG_COLLISION_ORDER, order)
            g.tick()
        for rounds in (16, 96):
            g.set_collision_rounds(rounds)
            g.tick()
        for schedule in (capi.SCHEDULE_COLOURED, capi.SCHEDULE_EXACT, capi.SCHEDULE_LAYERED):
            if schedule == capi.SCHEDULE_LAYERED:
                put_state(g, S0)
            g.set_schedule(schedule)
            g.tick()
    else:
        put_state(g, S0)
        g.tick()


# (flag, the value the handle is built with): toggled to the other value and back in every round
EDIT_FLAGS = {
    "pbd": ((capi.FLAG_RELEASE_HINGE, 0), (capi.FLAG_NODE_COLLISIONS, 1), (capi.FLAG_TRIANGLE_COLLISIONS, 1),
            (capi.FLAG_RENUMBER_NODES, 0), (capi.FLAG_PD_NODE_CONTACTS, 0)),
    "pd": ((capi.FLAG_RELEASE_HINGE, 0), (capi.FLAG_NODE_COLLISIONS, 1), (capi.FLAG_TRIANGLE_COLLISIONS, 1),
           (capi.FLAG_RENUMBER_NODES, 1), (capi.FLAG_PD_NODE_CONTACTS, 1)),
}


def pd_body(g, b):
    """body b: the shuffled unstructured beam of test_live_edits_pd_gpu (280 nodes in an order the library's renumbering does not
    keep - a createTetBox lattice would keep the identity), strain and volume per element, surface triangles, a pinned cap, a goal"""
    from test_live_edits_pd_gpu import SHUFFLED
    pos, tets, _ = SHUFFLED
    first = g.count(capi.NODES)
    g.add_nodes_raw(pos + F([9.0 * b, 0.0, 0.0]), radius=0.3)
    t = (tets + first).astype(U)
    g.add_tet(t, 20.0)
    g.add_volume(t, 20.0)
    g.add_triangles((scenes.boundary_triangles(pos, tets) + first).astype(U))
    g.add_position((np.nonzero(pos[:, 2] < 0.5)[0] + first).astype(U), 2.0)
    g.add_goal((np.nonzero(pos[:, 2] > pos[:, 2].max() - 0.8)[0] + first).astype(U), 20.0)


def edit_scene(g, kind, bodies=(0,)):
    """body b of the row; on a live scene the new bodies are appended and every node is perturbed again"""
    for b in bodies:
        t = (6.0 * b, 0.6, 0.0)
        if kind == "pd":
            pd_body(g, b)
        else:
            # held by distance constraints alone: the reference's PBD strain projection flattens a tetrahedral body within a few
            # ticks (quirk Q2) into a pile whose node-node passes take a third of a second each
            scenes.build_beam(g, (4, 4, 15), translation=t, tets=False)
    scenes.perturb(g, 7, 0.05)
    g.set_prev_positions(g.positions)


def edits(kinds=("pbd", "pd")):
    mark("start")
    for kind in kinds:
        if kind == "pd":
            g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
            g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1)
            g.set_flag(capi.FLAG_RENUMBER_NODES, 1)
            g.set_pcg(3e-7, 32)  # a short ladder of graphs: most of these edits rebuild the scene and capture every rung again
        else:
            g = pbd()
            g.set_schedule(capi.SCHEDULE_LAYERED)
            g.set_flag(capi.FLAG_NODE_COLLISIONS, 1)
            g.set_flag(capi.FLAG_COLLISION_ORDER, capi.COLLISION_ORDER_PAIRS)
            g.set_collision_rounds(96)
        edit_scene(g, kind)
        g.tick(2)
        mark(kind + ":live", nodes=g.count(capi.NODES), renumbered=g.count(capi.NODES_RENUMBERED))
        from live_edits import state_of
        S0 = state_of(g)
        for rnd in range(5):
            edit_round(g, kind, rnd, S0)
            mark(kind + ":round-%d" % (rnd + 1))
        # the one-body scene afresh, a second body appended to it while it is live, then the one-body scene again
        g.clear()
        edit_scene(g, kind)
        g.tick(2)
        mark(kind + ":one-body")
        edit_scene(g, kind, bodies=(1,))
        g.tick(2)
        mark(kind + ":two-bodies", nodes=g.count(capi.NODES))
        g.clear()
        edit_scene(g, kind)
        g.tick(2)
        mark(kind + ":one-body-again", failed=bool(g.failed), finite=bool(np.isfinite(g.positions).all()))
        g.close()
        mark(kind + ":closed")


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def broken_records(good):
    """every record that differs from `good` in one field: floats and the first element of float arrays become NaN, integers -1
    (an unknown type, shape, field or range)"""
    out = []
    for name, ctype in good._fields_:
        r = type(good).from_buffer_copy(good)
        if ctype is C.c_float:
            setattr(r, name, float("nan"))
        elif ctype in (C.c_int32, C.c_uint32):
            setattr(r, name, -1 if ctype is C.c_int32 else 0xFFFFFFFF)
        else:
            getattr(r, name)[0] = float("nan")
        out.append((name, r))
    return out


def errors():
    from test_skin import lattice
    mark("start")
    L = capi.load()
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
    tets = lattice(g)
    samples = np.ones((4, 4, 4), F)
    g.add_field(samples, (0.0, 0.0, 0.0), 0.5)
    g.tick(2)
    # the buffers of every entry point exist before the failing calls: what they may leak is what a failure leaves half done
    calls = {
        "collide_props": (capi.Prop.sphere((1.0, 2.0, 1.0), 0.5),
                          lambda arr, n: L.pies_collide_props(g._h, n, arr, None, None, None, None)),
        "collide_field_props": (capi.FieldProp.make(0, (1.0, 2.0, 1.0)),
                                lambda arr, n: L.pies_collide_field_props(g._h, n, arr, None, None, None, None)),
        "apply_forces": (capi.Force.wind((1.0, 0.0, 0.0), 1.0).within((1.0, 2.0, 1.0), 3.0),
                         lambda arr, n: L.pies_apply_forces(g._h, n, arr, DT, None, None, None)),
        "apply_surface_loads": (capi.SurfaceLoad.gas(1.0, 8.0).with_drag(0.5),
                                lambda arr, n: L.pies_apply_surface_loads(g._h, n, arr, DT, None, None, None, None, None)),
    }
    for name, (good, call) in calls.items():
        assert call((type(good) * 2)(good, good), 2) == capi.OK, (name, g.last_error())
    mark("ready")
    for name, (good, call) in calls.items():
        codes = []
        for field, bad in broken_records(good):
            before = capi.resource_counts()["live"]
            rc = call((type(good) * 2)(good, bad), 2)
            codes.append(rc)
            mark("%s:%s" % (name, field), rc=rc, unchanged=capi.resource_counts()["live"] == before)
        before = capi.resource_counts()["live"]
        rc_null = call(None, 2)
        rc_many = call((type(good) * 65)(*([good] * 65)), 65)
        mark(name + ":null-and-too-many", rc=rc_null, rc_many=rc_many, unchanged=capi.resource_counts()["live"] == before,
             invalid=sum(1 for c in codes if c == capi.ERR_INVALID), records=len(codes))
    # a skin vertex beyond max_distance (tests/test_skin.py: test_vertex_beyond_max_distance_fails_and_adds_nothing)
    p = g.positions
    inside = p[tets[0]].mean(0)
    v = F([inside, p.min(0) - F([0.2, 0.0, 0.0]), inside])
    before = capi.resource_counts()["live"]
    try:
        g.add_skin(v, tets, max_distance=0.1)
        raised = ""
    except capi.PiesError as e:
        raised = str(e)
    mark("skin-beyond-max-distance", raised=raised, unchanged=capi.resource_counts()["live"] == before, skins=g.count(capi.SKINS))
    g.tick()
    mark("after", failed=bool(g.failed), unchanged=capi.resource_counts()["live"] == before)
    # an open mesh: the device voxelises it (temporaries) before the host decides.  The library does not refuse an open surface
    # as such - a cell that holds a vertex is kept - so the call may succeed; either way it holds nothing new when it returns
    # (the scene is rebuilt at the next tick), and a mesh whose triangles name a missing vertex is refused after the same checks
    mv, mt = sphere_mesh((6.0, 2.0, 0.0))
    nodes = g.count(capi.NODES)
    try:
        g.add_tri_mesh_volume(mv, mt[:-3], 4)
        raised = ""
    except capi.PiesError as e:
        raised = str(e)
    mark("open-mesh", raised=raised, unchanged=capi.resource_counts()["live"] == before, added=g.count(capi.NODES) - nodes)
    g.close()
    mark("closed")
    # test_collisions_gpu.test_a_box_that_outgrows_the_captured_sort_is_latched: a latched handle gives everything back too
    p, v = scenes.loose_particles((6, 7, 8))
    v = (9000.0 * (p - p.mean(0))).astype(F)
    g = pbd(2, floorHeight=-1.0e5)
    g.addNodes(p)
    g.set_velocities(v)
    g.tick(2)
    mark("latched", failed=bool(g.failed), error=g.last_error())
    g.close()
    mark("latched:closed")


SCENARIOS = {"cycle-layered": lambda: cycle(("pbd-layered",)), "cycle-rest": lambda: cycle([c[0] for c in CYCLE[1:]]),
             "extensions": extensions, "edits-pbd": lambda: edits(("pbd",)), "edits-pd": lambda: edits(("pd",)),
             "errors": errors}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]]()
    print(json.dumps({"done": sys.argv[1]}), flush=True)
