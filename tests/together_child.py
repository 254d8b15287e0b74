"""Child process of tests/test_handles_together_gpu.py: `python together_child.py <scenario>` drives several handles at once - from
one thread with their work interleaved, or one thread per handle - and compares every handle with its own run alone, computed
first in the same process.  One JSON line per scenario: per handle, whether every compared array has the same bits, with the
figures beside it.  A thread that does not come back ends the process with exit code 3 (the parent stops its session then)."""
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "benchlib")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import scenes  # noqa: E402
from pies_amd import capi  # noqa: E402

U, F = np.uint32, np.float32
DT = 0.012
JOIN_SECONDS = 60.0


# ---- handles -----------------------------------------------------------------------------------------------------------------------
def pbd_layered_pairs():
    """schedule LAYERED, node-node collisions in the pair order (test_handle_reuse_gpu.scene_a)"""
    from test_handle_reuse_gpu import options, scene_a
    g = capi.Solver(options(capi))
    scene_a(capi, g)
    g.set_flag(capi.FLAG_COLLISION_ORDER, capi.COLLISION_ORDER_PAIRS)
    return g


def pbd_groups():
    p, v = scenes.loose_particles((6, 7, 8))
    g = capi.Solver(scenes.pbd_options(capi, 4))
    g.addNodes(p)
    g.set_velocities(v)
    g.set_flag(capi.FLAG_COLLISION_ORDER, capi.COLLISION_ORDER_GROUPS)
    return g


def pd_contacts():
    """test_tri_collisions_gpu.two_boxes: point-triangle contacts from the second tick on"""
    from test_tri_collisions_gpu import two_boxes
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
    two_boxes(g)
    return g


def pd_beam():
    from test_pd_parity_gpu import build_pd_beam
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
    build_pd_beam(g, (4, 4, 10))
    scenes.perturb(g, 9, 0.03)
    g.set_prev_positions(g.positions)
    return g


def rays(n=96):
    rng = np.random.default_rng(11)
    o = (F([-0.5, 6.0, -0.5]) + rng.uniform(0, 1, (n, 3)) * F([4.0, 0.0, 10.0])).astype(F)
    return o, np.tile(F([0.05, -1.0, 0.02]), (n, 1))


def between_ticks(g):
    """one edit and one query per tick, as a host with a character in the scene makes them"""
    out = list(g.apply_forces([capi.Force.wind((1.0, 0.0, 0.5), 0.8, shear=0.1)], DT))
    out += list(g.collide_props([capi.Prop.sphere((1.5, 1.5, 5.0), 1.2, velocity=(0.0, -0.5, 0.0))]))
    out += list(g.raycast(*rays()))
    return out


def result(g, extra=()):
    r = {"positions": g.positions, "velocities": g.velocities, "prev_positions": g.prev_positions,
         "collision_pairs": np.uint64([g.collision_pairs]), "failed": np.uint32([g.failed])}
    if g.options.solver == capi.PD:
        r["tri_collisions"] = g.tri_collisions
        h = g.pcg_health()
        r["pcg_health"] = np.uint64([h["short_solves"], h["solves"], h["substeps_retried"], h["budget"]])
    for k, a in enumerate(extra):
        r["extra-%d" % k] = np.asarray(a)
    return r


def same(a, b):
    """per name: the same shape and the same bits"""
    out = {}
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        out[name] = bool(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes())
    return out


def figures(r):
    out = {"finite": bool(np.isfinite(r["positions"]).all()), "failed": int(r["failed"][0]), "nodes": len(r["positions"]),
           "collision_pairs": int(r["collision_pairs"][0])}
    if "pcg_health" in r:
        out["tri_collisions"] = len(r["tri_collisions"])
        out["pcg_health"] = [int(x) for x in r["pcg_health"]]
    return out


def live():
    return capi.resource_counts()["live"]


# ---- interleaved: one thread, work of two handles queued alternately, a third handle born and gone in between ---------------------
def interleaved_rounds(A, B, third):
    extra_a, extra_b = [], []
    for rnd in range(8):
        if A is not None:
            A.tick_async()
        if B is not None:
            B.tick_async()
        if rnd == 2:
            if A is not None:
                extra_a = list(A.raycast(*rays()))
            if B is not None:
                extra_b = list(B.collide_props([capi.Prop.sphere((1.0, 1.5, 1.0), 0.8, velocity=(0.0, -0.5, 0.0))]))
        if rnd == 4 and third:
            C = pd_beam()  # captures a ladder of graphs and frees it again while A and B have ticks queued
            C.finalize()
            C.tick()
            C.close()
    return extra_a, extra_b


def make_a():
    """PBD, schedule LAYERED, node-node collisions, surface triangles for the ray cast"""
    g = capi.Solver(scenes.pbd_options(capi, 4))
    g.set_schedule(capi.SCHEDULE_LAYERED)
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 1)
    scenes.build_beam(g, (6, 6, 12), triangles=True)
    scenes.perturb(g, 21, 0.05)
    g.set_prev_positions(g.positions)
    return g


def interleaved():
    A = make_a()
    A.finalize()
    ea, _ = interleaved_rounds(A, None, False)
    alone_a = result(A, ea)
    layer = A.launch_counts()["layer"]
    A.close()
    B = pd_contacts()
    B.finalize()
    _, eb = interleaved_rounds(None, B, False)
    alone_b = result(B, eb)
    B.close()
    A, B = make_a(), pd_contacts()
    A.finalize()
    B.finalize()
    ea, eb = interleaved_rounds(A, B, True)
    ra, rb = result(A, ea), result(B, eb)
    A.close()
    B.close()
    return {"A": {"same": same(ra, alone_a), "figures": figures(ra), "layer_launches": layer},
            "B": {"same": same(rb, alone_b), "figures": figures(rb)}, "live": live()}


# ---- threads: one handle per thread ------------------------------------------------------------------------------------------------
KINDS = [("pbd-layered-pairs", pbd_layered_pairs, False), ("pd-contacts", pd_contacts, False), ("pbd-groups", pbd_groups, False),
         ("pd-edits", pd_beam, True)]


def life(build, edits, barrier=None, ticks=6):
    """build -> finalize -> ticks -> read -> close"""
    if barrier is not None:
        barrier.wait(timeout=JOIN_SECONDS)
    g = build()
    g.finalize()
    extra = []
    for _ in range(ticks):
        if edits:
            extra = between_ticks(g)
        g.tick()
    r = result(g, extra)
    g.close()
    return r


def run_threads(jobs):
    """jobs: (name, callable taking the barrier); returns name -> result or error text; a thread that stays away ends the process"""
    barrier = threading.Barrier(len(jobs))
    out = {}

    def work(name, fn):
        try:
            out[name] = fn(barrier)
        except BaseException as e:  # noqa: BLE001 - reported to the parent
            out[name] = "%s: %s" % (type(e).__name__, e)
    threads = [threading.Thread(target=work, args=job, daemon=True) for job in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_SECONDS)
    if any(t.is_alive() for t in threads):
        print(json.dumps({"hung": [job[0] for job, t in zip(jobs, threads) if t.is_alive()]}), flush=True)
        os._exit(3)
    return out


def threads():
    alone = {name: life(build, edits) for name, build, edits in KINDS}
    out = {"alone": {name: figures(r) for name, r in alone.items()}}
    for count in (2, 4):
        jobs = [(name, (lambda barrier, b=build, e=edits: life(b, e, barrier))) for name, build, edits in KINDS[:count]]
        got = run_threads(jobs)
        out["threads-%d" % count] = {name: ({"error": r} if isinstance(r, str) else {"same": same(r, alone[name]), "figures": figures(r)})
                                     for name, r in got.items()}
        out["live-%d" % count] = live()
    return out


# ---- sized: two handles whose grids are sized for sharing the device -------------------------------------------------------------
def big_particles():
    p, v = scenes.loose_particles((30, 25, 40))
    g = capi.Solver(scenes.pbd_options(capi, 4))
    g.addNodes(p)
    g.set_velocities(v)
    g.set_flag(capi.FLAG_COLLISION_ORDER, capi.COLLISION_ORDER_PAIRS)
    return g


def pbd_life(barrier=None):
    if barrier is not None:
        barrier.wait(timeout=JOIN_SECONDS)
    g = big_particles()
    g.finalize()
    g.tick(2)
    r = result(g)
    health = dict(g.collision_health(), fallbacks=g.collision_fallbacks)
    g.close()
    return r, health


def sized():
    alone, health = pbd_life()
    got = run_threads([("pbd-%d" % k, pbd_life) for k in range(2)])
    out = {"pbd-alone": {"figures": figures(alone), "health": health}}
    for name, r in got.items():
        out[name] = {"error": r} if isinstance(r, str) else {"same": same(r[0], alone), "figures": figures(r[0]), "health": r[1]}
    out["live"] = live()
    return out


# The smallest 32 x 32 x D beam whose CG grid reaches the cap of pd_setup.cpp: a launch has one workgroup per four slices of 64 rows,
# min(1 024, (ceil(n / 64) + 3) / 4), and at most half of what the device holds resident at once - on an MI355X 256 compute units
# x 4 workgroups of k_cg1_iter / 2 = 512 workgroups, first reached at ceil(n / 64) = 2 045, n >= 130 817: D = 128 (131 072 nodes).
SIZED_PD_BEAM = (32, 32, 128)


def big_beam():
    from test_pd_parity_gpu import build_pd_beam
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
    build_pd_beam(g, SIZED_PD_BEAM)
    scenes.perturb(g, 9, 0.03)
    g.set_prev_positions(g.positions)
    return g


def pd_life(barrier=None):
    if barrier is not None:
        barrier.wait(timeout=JOIN_SECONDS)
    g = big_beam()
    g.finalize()
    blocks = g.count(capi.PD_CG_BLOCKS)
    g.tick(4)
    r = result(g)
    g.close()
    return r, {"cg_blocks": blocks}


def sized_pd():
    alone, info = pd_life()
    got = run_threads([("pd-%d" % k, pd_life) for k in range(2)])
    out = {"pd-alone": {"figures": figures(alone), "info": info}}
    for name, r in got.items():
        out[name] = {"error": r} if isinstance(r, str) else {"same": same(r[0], alone), "figures": figures(r[0]), "info": r[1]}
    out["live"] = live()
    return out


# ---- layered_lds: two layered handles whose tiles need unlike amounts of LDS above 64 KB ---------------------------------------------
# A tile of schedule LAYERED with one strip is a pair of levels perpendicular to the longest axis: 2 W H nodes of 20 bytes.  The
# kernels' limit of dynamic LDS is process-wide state (layer_prepare): the handle with smaller tiles finalizes second, and the
# larger one must still be able to capture and launch afterwards.  By default a pair of levels wider than 2 560 nodes is not given
# one tile (51 KB); the tuning switch PIES_LAYER_ONE_STRIP_MAX raises that to what the LDS holds, as a host with squat bodies may.
LDS_BIG, LDS_SMALL = (46, 46, 47), (41, 41, 42)  # 2 x 46 x 46 x 20 = 84 640 bytes and 2 x 41 x 41 x 20 = 67 240 bytes of node records


def layered_beam(dims):
    g = capi.Solver(scenes.pbd_options(capi, 2))
    g.set_schedule(capi.SCHEDULE_LAYERED)
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
    scenes.build_beam(g, dims)
    g.add_position(U([0, 1, 2, 3]), 2.0)
    scenes.perturb(g, 5, 0.03)
    g.set_prev_positions(g.positions)
    return g


def layered_lds():
    def first_half(g):
        g.finalize()
        g.tick()

    def second_half(g):
        g.set_flag(capi.FLAG_RELEASE_HINGE, 1)  # the substep is captured again, with the tiles the handle has
        g.tick(2)
        r = result(g)
        info = {"tiles": g.count(capi.LAYER_MAX_TILES), "layer_launches": g.launch_counts()["layer"]}
        g.close()
        return r, info
    capi.set_tuning("PIES_LAYER_ONE_STRIP_MAX", "7936")  # (before any handle exists; the process ends with the scenario)
    alone = {}
    for name, dims in (("big", LDS_BIG), ("small", LDS_SMALL)):
        g = layered_beam(dims)
        first_half(g)
        alone[name] = second_half(g)
    big, small = layered_beam(LDS_BIG), layered_beam(LDS_SMALL)
    first_half(big)
    first_half(small)  # lowers nothing: the limit only grows
    got = {"big": second_half(big), "small": second_half(small)}
    out = {name: {"same": same(got[name][0], alone[name][0]), "figures": figures(got[name][0]), "info": got[name][1]} for name in got}
    out["live"] = live()
    return out


SCENARIOS = {"layered_lds": layered_lds, "interleaved": interleaved, "threads": threads, "sized": sized, "sized_pd": sized_pd}

if __name__ == "__main__":
    print(json.dumps({"scenario": sys.argv[1], "result": SCENARIOS[sys.argv[1]]()}), flush=True)
