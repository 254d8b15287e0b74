"""Several handles busy at once (INTEGRATION.md "Several solvers in one process"): handles are independent, may be driven from any
threads - one thread per handle at a time - and give the bits of a run alone, PD included.  tests/together_child.py runs each
scenario in a process of its own, so that a hang ends at the time limit here; every handle's expected result is computed first,
alone, in that same process.

  interleaved  one thread: A (PBD, schedule LAYERED, node-node collisions) and B (PD, point-triangle contacts) with eight ticks
               queued alternately and no synchronisation between them, a ray cast and a prop call in round 3, and in round 5 a
               third handle created, finalized (a ladder of graphs), ticked and destroyed while A and B have work queued
  threads      2, then 4 threads behind a barrier, each build -> finalize -> 6 ticks -> read -> close on a handle of its own:
               PBD LAYERED in the pair order, PD with contacts, PBD in the group order, PD with one apply_forces / collide_props
               / raycast per tick; afterwards the resource ledger is at zero
  sized        two threads, two handles of particles((30, 25, 40)) in the pair order, whose bounded grid barriers may find their
               workgroups not co-resident: the sequential fallback is exact by construction, so only the bits are asserted and
               the health counters of both runs are printed
  sized_pd     two threads, two PD beams of 32 x 32 x 128 nodes - the smallest such beam whose CG grid is at its cap of half the
               resident workgroups (512 on an MI355X; together_child.SIZED_PD_BEAM has the arithmetic), the case the cap is
               sized for: 4 ticks, the bits of the run alone, no solve left short and no substep run again
  layered_lds  one thread, two layered PBD beams whose tiles need 84 640 and 67 240 bytes of LDS for their node records - both above
               the 64 KB a kernel gets without asking (PIES_LAYER_ONE_STRIP_MAX raised to the LDS's capacity); the smaller finalizes second, then the larger captures its substep again
               and ticks: the kernels' limit of dynamic LDS is shared by the handles of a process and must only grow

If a child runs into the time limit, dies on a signal or reports a thread that did not come back, the session ends there: nothing
more is started on the card."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "together_child.py")
ZERO = {k: 0 for k in ("device_bytes", "device_allocations", "pinned_bytes", "pinned_allocations", "streams", "events", "graphs",
                       "graph_execs")}


def run(scenario):
    try:
        out = subprocess.run([sys.executable, CHILD, scenario], capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired as e:
        pytest.exit("together_child.py %s did not end within %d s: a hang on the device; nothing more is started (%s)"
                    % (scenario, e.timeout, (e.stdout or b"")[-400:]), returncode=3)
    if out.returncode < 0 or out.returncode == 3:
        pytest.exit("together_child.py %s ended with %d (a signal, or a thread that did not come back): nothing more is started\n%s\n%s"
                    % (scenario, out.returncode, out.stdout[-800:], out.stderr[-1600:]), returncode=3)
    assert out.returncode == 0, (out.returncode, out.stdout[-800:], out.stderr[-3000:])
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1 and lines[0]["scenario"] == scenario, out.stdout[-800:]
    return lines[0]["result"]


def exact(tag, r):
    assert "error" not in r, (tag, r)
    assert all(r["same"].values()), (tag, [k for k, v in r["same"].items() if not v], r["figures"])
    assert r["figures"]["finite"] and not r["figures"]["failed"], (tag, r["figures"])


def test_interleaved():
    r = run("interleaved")
    print(json.dumps(r))
    exact("A", r["A"])
    exact("B", r["B"])
    assert {"positions", "velocities", "collision_pairs", "extra-0"} <= set(r["A"]["same"])
    assert {"positions", "velocities", "tri_collisions", "pcg_health", "extra-0"} <= set(r["B"]["same"])
    # the scenes do what they are here for: layered launches and resolved pairs in A, contacts in B
    assert r["A"]["layer_launches"] > 0 and r["A"]["figures"]["collision_pairs"] > 0
    assert r["B"]["figures"]["tri_collisions"] > 0
    assert r["live"] == ZERO, r["live"]


def test_threads():
    r = run("threads")
    print(json.dumps(r))
    for count in (2, 4):
        got = r["threads-%d" % count]
        assert len(got) == count
        for name, x in got.items():
            exact((count, name), x)
            if name.startswith("pd"):
                assert {"tri_collisions", "pcg_health"} <= set(x["same"])
        assert r["live-%d" % count] == ZERO, (count, r["live-%d" % count])
    assert r["alone"]["pbd-layered-pairs"]["collision_pairs"] > 0 and r["alone"]["pbd-groups"]["collision_pairs"] > 0
    assert r["alone"]["pd-contacts"]["tri_collisions"] > 0


def test_sized():
    r = run("sized")
    print(json.dumps(r))
    assert r["pbd-alone"]["figures"]["nodes"] == 30000 and r["pbd-alone"]["figures"]["collision_pairs"] > 10000
    for name in ("pbd-0", "pbd-1"):
        exact(name, r[name])
        assert r[name]["figures"]["collision_pairs"] == r["pbd-alone"]["figures"]["collision_pairs"]
    assert r["live"] == ZERO, r["live"]


def test_sized_pd():
    r = run("sized_pd")
    print(json.dumps(r))
    assert r["pd-alone"]["figures"]["nodes"] == 32 * 32 * 128
    assert r["pd-alone"]["info"]["cg_blocks"] == 512  # at the cap: half of 256 compute units x 4 resident workgroups
    for name in ("pd-alone", "pd-0", "pd-1"):
        if name != "pd-alone":
            exact(name, r[name])
            assert r[name]["info"] == r["pd-alone"]["info"]
        short, solves, retried, _ = r[name]["figures"]["pcg_health"]
        assert short == 0 and retried == 0 and solves == 4 * 6, (name, r[name]["figures"])
    assert r["live"] == ZERO, r["live"]


def test_layered_lds():
    r = run("layered_lds")
    print(json.dumps(r))
    for name, levels, nodes in (("big", 47, 46 * 46 * 47), ("small", 42, 41 * 41 * 42)):
        exact(name, r[name])
        assert r[name]["figures"]["nodes"] == nodes and r[name]["info"]["layer_launches"] > 0
        # one strip: a phase has about one tile per two levels, so a tile is a pair of whole levels (2 W H nodes, above 64 KB);
        # cut into strips a phase would have at least twice as many
        assert 0 < r[name]["info"]["tiles"] <= levels // 2 + 2, r[name]["info"]
    assert r["live"] == ZERO, r["live"]
