"""What a handle holds, and whether it gives it back: the library's resource ledger (pies_resource_counts: live and created device
allocations and bytes, pinned allocations and bytes, streams, events, graphs, executable graphs, over all handles of the process)
read at checkpoints of four scenarios.  Each scenario runs in a fresh child process (tests/lifetime_child.py): its ledger starts at
zero and no garbage handle of an earlier test disturbs it.  Every assertion is an equality between counts, or `>=` against a size
the scene dictates; nothing is fitted.

  cycle       create -> build -> finalize -> tick -> close for eight unlike scenes, one after the other (the layered beam with
              node-node collisions in a process of its own: its ticks take longest): zero after every close, nothing created by
              a tick but re-captured graphs
  extensions  every entry point that allocates lazily, on a PBD and a PD handle: repeats hold the counts, growth is bounded,
              clear() and a rebuild return to the first build's counts, close to zero
  edits       five rounds of every between-tick edit on a live PBD and a live PD handle (a process each): every round ends at
              the counts of the first.  Every flag of the API is toggled and put back, with a tick after each change, on both
              solvers - PIES_FLAG_RENUMBER_NODES on a PD scene whose renumbering is kept (the shuffled beam), the legacy
              PIES_FLAG_REFERENCE_COLLISION_ORDER included
  errors      failing calls hold nothing when they return; a latched handle gives everything back.  The four record-taking entry
              points (props, field props, forces, surface loads) get a good record followed by one broken in a single field -
              every field in turn: NaN for floats, -1 for integers -, a NULL array and 65 records, on a device handle whose
              buffers exist (the argument checks of tests/test_props.py, test_forces.py, test_loads.py, test_fields.py run on
              host-only handles, where nothing could be held).  A skin vertex beyond max_distance is refused after the binding
              search.  An open mesh is NOT refused by pies_add_tri_mesh_volume (a cell that holds a vertex is kept): the call
              is held to leaving nothing behind on the device whichever way it ends."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lifetime_child.py")
KINDS = ("device_bytes", "device_allocations", "pinned_bytes", "pinned_allocations", "streams", "events", "graphs", "graph_execs")
ZERO = {k: 0 for k in KINDS}
_cache = {}


def run(scenario):
    """the scenario's checkpoints by tag, in order; run once per session"""
    if scenario not in _cache:
        # a child that hangs or dies on a signal ends the session: nothing more is started on the card (as in
        # test_handles_together_gpu.run)
        try:
            out = subprocess.run([sys.executable, CHILD, scenario], capture_output=True, text=True, timeout=180)
        except subprocess.TimeoutExpired as e:
            pytest.exit("lifetime_child.py %s did not end within %d s: a hang on the device; nothing more is started (%s)"
                        % (scenario, e.timeout, (e.stdout or b"")[-400:]), returncode=3)
        if out.returncode < 0:
            pytest.exit("lifetime_child.py %s died on signal %d: nothing more is started\n%s\n%s"
                        % (scenario, -out.returncode, out.stdout[-800:], out.stderr[-1600:]), returncode=3)
        assert out.returncode == 0, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
        lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
        assert lines and lines[-1] == {"done": scenario}, out.stdout[-800:]
        marks = {}
        for x in lines[:-1]:
            assert x["at"] not in marks and tuple(x["live"]) == KINDS and tuple(x["created"]) == KINDS, x
            marks[x["at"]] = x
        _cache[scenario] = marks
    return _cache[scenario]


@pytest.mark.parametrize("part,count", [("layered", 1), ("rest", 7)])
def test_cycle(part, count):
    m = run("cycle-" + part)
    assert m["start"]["live"] == ZERO and m["start"]["created"] == ZERO
    names = [tag[:-len(":closed")] for tag in m if tag.endswith(":closed")]
    assert len(names) == count
    for name in names:
        closed, fin, first, last = (m["%s:%s" % (name, k)] for k in ("closed", "finalized", "first", "last"))
        assert closed["live"] == ZERO, (name, closed["live"])
        # while open the counters count: five float4-sized node arrays at the least, two streams, the substep's graph
        assert fin["live"]["device_bytes"] >= 32 * fin["nodes"] and fin["live"]["device_allocations"] >= 5, (name, fin)
        assert fin["live"]["streams"] == 2 and fin["live"]["events"] >= 2, (name, fin["live"])
        assert fin["live"]["graphs"] >= 1 and fin["live"]["graph_execs"] >= 1, (name, fin["live"])
        assert not last["failed"] and last["finite"], name
        # twenty ticks: nothing more is held, and nothing was created but graphs (a captured launch count that follows the scene)
        assert last["live"] == first["live"], (name, first["live"], last["live"])
        moved = [k for k in KINDS if last["created"][k] != first["created"][k]]
        assert set(moved) <= {"graphs", "graph_execs"}, (name, moved)
        for k in KINDS:
            assert closed["created"][k] >= last["created"][k] >= first["created"][k] >= fin["created"][k]


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_extensions(kind):
    m = run("extensions")
    at = lambda tag: m["%s:%s" % (kind, tag)]  # noqa: E731
    L1 = at("L1")["live"]
    assert L1["device_bytes"] > at("finalized")["live"]["device_bytes"]  # the calls do allocate
    assert L1["pinned_allocations"] > 0 and L1["streams"] == 3 and L1["events"] > at("finalized")["live"]["events"]
    for k in range(3):  # the same calls at the same sizes: the same counts
        assert at("same-%d" % k)["live"] == L1, (k, at("same-%d" % k)["live"], L1)
    # four times the rays, points and props, then the first sizes again: buffers may grow, once
    assert at("big-0")["live"]["device_bytes"] >= L1["device_bytes"]
    assert at("big-1")["live"] == at("big-0")["live"], (at("big-0")["live"], at("big-1")["live"])
    assert at("small-1")["live"] == at("small-0")["live"], (at("small-0")["live"], at("small-1")["live"])
    for k in KINDS[1:]:  # (device bytes may have grown; what is held is the same set of things)
        assert at("small-0")["live"][k] == L1[k], (k, at("small-0")["live"], L1)
    # pies_clear leaves what pies_hip.h says it leaves (pies_resource_counts): the two streams and two events of pies_create, the
    # export path's stream, four events and frame buffers (one device and two pinned buffers each for the nodes and for the skins),
    # the two events of the device-side access - and nothing sized by the scene: no graph, no pinned staging buffer
    cleared = at("cleared")["live"]
    assert {k: cleared[k] for k in KINDS[1:] if k != "pinned_bytes"} == \
        {"device_allocations": 2, "pinned_allocations": 4, "streams": 3, "events": 8, "graphs": 0, "graph_execs": 0}, cleared
    nodes, skin_vertices = at("finalized")["nodes"], at("finalized")["skin_vertices"]
    assert cleared["device_bytes"] == 16 * nodes + 24 * skin_vertices, (cleared, nodes, skin_vertices)
    assert cleared["pinned_bytes"] == 2 * cleared["device_bytes"], cleared
    # the same scene finalized again holds what the first build held, beside what the clear left
    rebuilt, fin = at("rebuilt-finalized")["live"], at("finalized")["live"]
    assert rebuilt["device_bytes"] == fin["device_bytes"] + cleared["device_bytes"], (rebuilt, fin, cleared)
    assert rebuilt["device_allocations"] == fin["device_allocations"] + 2 and rebuilt["graphs"] == fin["graphs"], (rebuilt, fin)
    assert rebuilt["graph_execs"] == fin["graph_execs"] and rebuilt["streams"] == 3 and rebuilt["events"] == 8, rebuilt
    assert at("rebuilt-L1")["live"] == L1, (at("rebuilt-L1")["live"], L1)
    assert not at("rebuilt-L1")["failed"] and at("rebuilt-L1")["finite"]
    assert at("closed")["live"] == ZERO, at("closed")["live"]


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_edits(kind):
    m = run("edits-" + kind)
    at = lambda tag: m["%s:%s" % (kind, tag)]  # noqa: E731
    first = at("round-1")["live"]
    assert first["device_bytes"] >= 32 * at("live")["nodes"]
    assert at("live")["renumbered"] == (1 if kind == "pd" else 0)  # the PD scene is one whose renumbering is kept
    for rnd in range(2, 6):
        assert at("round-%d" % rnd)["live"] == first, (rnd, at("round-%d" % rnd)["live"], first)
    one, two, again = at("one-body")["live"], at("two-bodies")["live"], at("one-body-again")["live"]
    assert two["device_bytes"] > one["device_bytes"] and at("two-bodies")["nodes"] == 2 * at("live")["nodes"]
    assert again == one, (again, one)
    assert not at("one-body-again")["failed"] and at("one-body-again")["finite"]
    assert at("closed")["live"] == ZERO, at("closed")["live"]


# The one-field breakages that MUST be refused with PIES_ERR_INVALID: the fields the argument checks of tests/test_props.py,
# test_fields.py, test_forces.py and test_loads.py hold to that (a sphere does not read end, axes and half; a force's flags word has
# no invalid value listed there; a load's count of 0xFFFFFFFF means "to the container's end").
MUST_BE_INVALID = {
    "collide_props": {"shape", "radius", "centre", "velocity", "angular", "pivot", "friction"},
    "collide_field_props": {"field", "radius", "centre", "axes", "velocity", "angular", "pivot", "friction"},
    "apply_forces": {"type", "centre", "radius", "falloff", "vector", "strength", "shear"},
    "apply_surface_loads": {"type", "flags", "first", "strength", "rest_volume", "point", "up", "velocity", "drag"},
}


def test_errors():
    m = run("errors")
    ready = m["ready"]["live"]
    assert ready["device_bytes"] > 0
    for entry in ("collide_props", "collide_field_props", "apply_forces", "apply_surface_loads"):
        tags = [t for t in m if t.startswith(entry + ":")]
        assert len(tags) >= 9
        for t in tags:  # (a one-field change that leaves the record valid is a call like the first: it holds what that one held)
            assert m[t]["unchanged"] and m[t]["live"] == ready, (t, m[t])
        last = m[entry + ":null-and-too-many"]
        assert last["rc"] == 1 and last["rc_many"] == 4  # PIES_ERR_INVALID, PIES_ERR_UNSUPPORTED
        fields = {t.split(":", 1)[1]: m[t]["rc"] for t in tags if t != entry + ":null-and-too-many"}
        assert MUST_BE_INVALID[entry] <= set(fields), (entry, sorted(fields))
        for field, rc in fields.items():  # 1: PIES_ERR_INVALID; a field the record's kind does not read may pass (0: PIES_OK)
            assert rc == 1 if field in MUST_BE_INVALID[entry] else rc in (0, 1), (entry, field, rc)
    skin = m["skin-beyond-max-distance"]
    assert "vertex 1" in skin["raised"] and skin["unchanged"] and skin["skins"] == 0
    assert m["after"]["unchanged"] and not m["after"]["failed"]
    assert m["open-mesh"]["unchanged"] and (m["open-mesh"]["raised"] or m["open-mesh"]["added"] > 0), m["open-mesh"]
    assert m["closed"]["live"] == ZERO, m["closed"]["live"]
    assert m["latched"]["failed"] and "cell box" in m["latched"]["error"]
    assert m["latched:closed"]["live"] == ZERO, m["latched:closed"]["live"]
