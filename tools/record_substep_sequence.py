"""Records what the substep sequencer (pies_amd/csrc/substep_graph.cpp) does on a set of small scenes, through the public binding
only: launch counts after finalize and after the last tick, the captured CG budget after every tick (PD), a SHA-256 of the final
positions and velocities, and - for two scenes - the launches and units the two profile passes report for every kernel class.

tests/test_substep_sequence_gpu.py rebuilds every scene and compares with tests/golden/substep_sequence.json, so a change of the
host code that moves a launch, a bracket or an adaptation shows.  To re-record (on a gfx950 device, at the commit to pin):

    python tools/record_substep_sequence.py --commit $(git rev-parse HEAD) --out a.json
    python tools/record_substep_sequence.py --commit $(git rev-parse HEAD) --out b.json
    python tools/record_substep_sequence.py --merge a.json b.json --out tests/golden/substep_sequence.json

--merge checks that the two recordings agree.  Counts and budgets must; a state hash that differs between the two runs is dropped
from the merged file ("state": null), which is tolerated for the contact-onset scenes (11*) only.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "benchlib"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scenes  # noqa: E402

PBD_ITERATIONS, PBD_TICKS = 4, 6
PD_ITERATIONS, PD_TICKS = 10, 8
STRIPS = {"PIES_LAYER_ONE_STRIP_MAX": "40", "PIES_LAYER_TILE_NODES": "90", "PIES_LAYER_STRIPS_MIN_NODES": "0"}
NODES, PD_TILES = 9, 13  # pies_count selectors
MAY_DROP_STATE = ("11a", "11b", "11c")  # scenes whose state hash --merge may drop when two recordings differ


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def _state(g):
    return {"positions": _sha(g.positions), "velocities": _sha(g.velocities)}


def _profiles(capi, g):
    """launches and units of both profile passes for every class the substep launches"""
    out = {}
    for k, (name, n) in enumerate(g.launch_counts().items()):
        if n == 0:
            continue
        launches, _, units = g.profile_substep(k)
        il, _, iu, _ = g.profile_in_situ(k, 2)
        out[name] = {"substep": [launches, units], "in_situ": [il, iu]}
    return out


# ---- PBD ----------------------------------------------------------------------------------------------------------------------
def _small_beam(s):
    scenes.build_beam(s, (4, 5, 6))
    scenes.perturb(s, 7, 0.05)


def _layered_bodies(s):
    """a beam, a bend sheet and a hinged sheet (position constraints)"""
    scenes.build_beam(s, (6, 6, 14))
    s.create_bend_sheet(7, 9, translation=(12.0, 3.0, 0.0))
    s.create_sheet(9, 7, translation=(24, 3, 0), scale=0.5, mass=2.0, w=0.7)
    scenes.perturb(s, 4, 0.05)


def _loose(dims):
    def build(s):
        p, v = scenes.loose_particles(dims)
        s.addNodes(p)
        s.set_velocities(v)
    return build


def _pbd(capi, build, schedule=None, collisions=1, order=None, rounds=None, hinge_after=None, profile=False, expect=None):
    g = capi.Solver(scenes.pbd_options(capi, PBD_ITERATIONS))
    try:
        build(g)
        if schedule is not None:
            g.set_schedule(schedule)
        g.set_flag(capi.FLAG_NODE_COLLISIONS, collisions)
        if order is not None:
            g.set_flag(capi.FLAG_COLLISION_ORDER, order)
        if rounds is not None:
            g.set_collision_rounds(rounds)
        g.finalize()
        out = {"launch_counts_finalize": g.launch_counts()}
        for t in range(PBD_TICKS):
            if hinge_after is not None and t == hinge_after:
                g.set_flag(capi.FLAG_RELEASE_HINGE, 1)
            g.tick()
        out["launch_counts_end"] = g.launch_counts()
        out["state"] = _state(g)
        assert not g.failed, g.last_error()
        if expect:
            expect(g, out)
        if profile:
            out["profile"] = _profiles(capi, g)
        return out
    finally:
        g.close()


def _expect_one_strip(g, out):
    lc = out["launch_counts_end"]
    assert lc["layer"] > 0 and lc["predict"] == 0 and lc["collide"] > 0, lc


def _expect_strips(g, out):
    lc = out["launch_counts_end"]
    assert lc["layer"] > 0 and lc["predict"] == 1 and lc["floor"] == PBD_ITERATIONS and lc["collide"] > 0, lc


def _expect_wave(g, out):
    lc = out["launch_counts_end"]
    assert lc["wave"] > 0 and lc["collide"] > 0, lc


def _expect_plain(g, out):
    lc = out["launch_counts_end"]
    assert lc["wave"] == 0 and lc["layer"] == 0 and lc["collide"] > 0, lc


def _expect_turns(g, out):
    assert g.count(NODES) >= 1024 and g.collision_health()["levels"] > 0, g.collision_health()


# ---- PD -----------------------------------------------------------------------------------------------------------------------
def _small_box(s):
    s.create_tet_box(3, 3, 3, translation=(0, 2.0, 0), volume=False)


def _rest_box(s):
    s.create_tet_box(7, 6, 23, translation=(0, 0.02, 0), volume=True, triangles=True)


_MESH = []


def _beam_onto_box(s):
    """an unstructured beam (end cap pinned) moving down onto a tet box that rests on the floor: contacts from the third tick on"""
    if not _MESH:
        pos, tets, edges = scenes.delaunay_beam((6, 5, 14))
        pos = pos.copy()
        pos[:, 1] += 1.02 + 0.25 - pos[:, 1].min()  # 0.25 above the box's top face
        _MESH.append((pos, tets, edges))
    scenes.build_unstructured_pd(s, _MESH[0])  # (the mesh's ids are its own: it comes first)
    n = s.count(NODES)
    s.create_tet_box(8, 2, 16, translation=(-1.0, 0.02, -1.0), triangles=True)
    v = s.velocities
    v[:n, 1] = -3.0
    s.set_velocities(v)
    s.set_prev_positions(s.positions)


def _node_contacts(s):
    from test_pd_node_contacts_gpu import motion_scene
    motion_scene(s)


def _pd(capi, build, node_contacts=False, asynchronous=0, profile=False, expect=None, **options):
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=PD_ITERATIONS, **options))
    try:
        if node_contacts:
            g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1)
        build(g)
        g.finalize()
        out = {"launch_counts_finalize": g.launch_counts(), "budgets": []}
        for _ in range(asynchronous or PD_TICKS):
            if asynchronous:
                g.tick_async()  # never pies_synchronize: the forced one every 16 ticks
            else:
                g.tick()
            out["budgets"].append(g.pcg_health()["budget"])
        out["launch_counts_end"] = g.launch_counts()
        out["state"] = _state(g)
        assert not g.failed, g.last_error()
        if expect:
            expect(g, out)
        if profile:
            out["profile"] = _profiles(capi, g)
        return out
    finally:
        g.close()


def _expect_tiles(g, out):
    assert g.count(PD_TILES) > 0, "no PD tiles"


def _expect_unpaired(g, out):
    lc = out["launch_counts_end"]
    assert g.count(PD_TILES) == 0 and lc["pd_local_tet"] == PD_ITERATIONS and lc["pd_local_volume"] == 0, lc


def _expect_tri_contacts(g, out):
    assert len(g.tri_collisions) > 0, "the beam did not reach the box"


def _expect_node_contacts(g, out):
    assert out["launch_counts_end"]["hash"] > 0 and out["launch_counts_end"]["collide"] > 0, out["launch_counts_end"]


def _expect_pinned(g, out):
    assert set(out["budgets"]) == {2}, out["budgets"]


# name -> (tunings, runner).  The names' numbers are those of the scene list in the sequencer's test plan.
SCENES = {
    "01_beam_coloured": ({}, lambda c: _pbd(c, _small_beam, c.SCHEDULE_COLOURED, collisions=0)),
    "02_beam_exact_wavefront": ({}, lambda c: _pbd(c, _small_beam, c.SCHEDULE_EXACT, expect=_expect_wave)),
    "03_beam_exact_plain_loop": ({"PIES_NO_WAVEFRONT": "1"}, lambda c: _pbd(c, _small_beam, c.SCHEDULE_EXACT, expect=_expect_plain)),
    "04_layered_one_strip": ({}, lambda c: _pbd(c, _layered_bodies, c.SCHEDULE_LAYERED, profile=True, expect=_expect_one_strip)),
    "05_layered_strips": (STRIPS, lambda c: _pbd(c, _layered_bodies, c.SCHEDULE_LAYERED, expect=_expect_strips)),
    "06_layered_release_hinge": ({}, lambda c: _pbd(c, _layered_bodies, c.SCHEDULE_LAYERED, hinge_after=3, expect=_expect_one_strip)),
    "07a_particles_pair_order": ({}, lambda c: _pbd(c, _loose((6, 6, 6)))),
    "07b_particles_group_order": ({}, lambda c: _pbd(c, _loose((6, 6, 6)), order=c.COLLISION_ORDER_GROUPS)),
    "07c_particles_three_rounds": ({}, lambda c: _pbd(c, _loose((6, 6, 6)), rounds=3)),
    "08_particles_reference_turns": ({}, lambda c: _pbd(c, _loose((10, 10, 11)), order=c.COLLISION_ORDER_REFERENCE, expect=_expect_turns)),
    "09_pd_unpaired": ({}, lambda c: _pd(c, _small_box, expect=_expect_unpaired)),
    "10_pd_tiles_at_rest": ({}, lambda c: _pd(c, _rest_box, profile=True, expect=_expect_tiles)),
    "11a_pd_contact_onset": ({}, lambda c: _pd(c, _beam_onto_box, expect=_expect_tri_contacts)),
    "11b_pd_contact_onset_fast_rows": ({"PIES_TRI_FAST_ROWS": "1"}, lambda c: _pd(c, _beam_onto_box, expect=_expect_tri_contacts)),
    "11c_pd_contact_onset_levels_in_line": ({"PIES_TRI_SIDE": "0"}, lambda c: _pd(c, _beam_onto_box, expect=_expect_tri_contacts)),
    "12_pd_node_contacts": ({}, lambda c: _pd(c, _node_contacts, node_contacts=True, friction=0.3, expect=_expect_node_contacts)),
    "13_pd_budget_pinned": ({"PIES_PCG_BUDGET": "2"}, lambda c: _pd(c, _rest_box, expect=_expect_pinned)),
    "14_pd_no_graph": ({"PIES_NO_GRAPH": "1"}, lambda c: _pd(c, _rest_box)),
    "15_pd_async_forced_sync": ({}, lambda c: _pd(c, _rest_box, asynchronous=40)),
}


def record_scene(capi, name):
    tunings, run = SCENES[name]
    try:
        for k, v in tunings.items():
            capi.set_tuning(k, v)
        return run(capi)
    finally:
        for k in tunings:
            capi.set_tuning(k, None)


def merge(a, b):
    assert a["parent_commit"] == b["parent_commit"] and sorted(a["scenes"]) == sorted(b["scenes"])
    out = {"parent_commit": a["parent_commit"], "scenes": {}}
    for name, ra in a["scenes"].items():
        rb = b["scenes"][name]
        for key in ra:
            if key != "state":
                assert ra[key] == rb[key], (name, key, ra[key], rb[key])
        rec = dict(ra)
        if ra["state"] != rb["state"]:
            assert name.startswith(MAY_DROP_STATE), (name, "state differs between the two recordings")
            print("state not reproducible, hash dropped:", name)
            rec["state"] = None
        out["scenes"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", help="hash of the commit the recording pins")
    ap.add_argument("--merge", nargs=2, metavar="JSON")
    args = ap.parse_args()
    if args.merge:
        res = merge(*(json.load(open(p)) for p in args.merge))
    else:
        from pies_amd import capi
        capi.load()
        res = {"parent_commit": args.commit, "scenes": {}}
        for name in sorted(SCENES):
            res["scenes"][name] = record_scene(capi, name)
            print(name, "ok", flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
