"""pies_apply_ties at the sizes the project is built for: loose nodes on the 20 x 20 x 250 lattice of BASELINE config 3 (100 000
nodes), unit spacing, random velocities; sets of 1 000, 10 000 and 100 000 ties - random tied nodes on triangles of random lattice
neighbours, four groups - at 1, 4 and 16 iterations, with and without the reaction outputs.  The cost of the call does not depend on
the constraints of a scene (it runs outside the substep), so the nodes carry none and the handle is a PBD one without node-node
collisions.  Positions never change and the call's cost does not depend on the velocities it finds.

  us_per_call        host clock around pies_apply_ties (the call ends in a stream synchronisation; the copy of the groups in and of
                     the reaction out are part of it), median of the repeats; min_us the fastest
  first_call_us      the first call of a set: it stages the set's device copy
  rows               10 000 ties of which L share one carrier node - a CSR row of L entries walked by one lane of k_tie_scatter -, 4
                     iterations without outputs: the row length from which that lane dominates the call
  seam               two tet boxes side by side, an eighth apart, under PBD without node-node collisions: the second one's facing nodes
                     are sewn to the first one's surface by the recipe of INTEGRATION.md; the boxes fall and land; ticks with a
                     call after each, the seam's largest stretch on the way and at the end
  kernels            per launch, from a rocprofv3 --kernel-trace --stats run of `--calls TIES` (its kernel stats CSV is given
                     with --stats SIZE=CSV)

    PIES_PROFILER_SAFE=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_ties.py --calls 100000
    python tools/probe_ties.py profiles/ties_probe.json [--stats 100000=CSV]
"""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib")):
    sys.path.insert(0, p)
import scenes  # noqa: E402
from pies_amd import capi  # noqa: E402

SIZES = (1000, 10000, 100000)
ITERATIONS = (1, 4, 16)
ROWS = (0, 64, 256, 1024, 4096)
REPEATS, WARM = 15, 3
DT = 1.0 / 60.0
N_GROUPS = 4


def lattice(dims):
    W, H, D = dims
    p = np.stack(np.meshgrid(np.arange(W), np.arange(H), np.arange(D), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    v = np.random.default_rng(7).normal(size=p.shape).astype(np.float32)
    return p + np.float32([0.0, 2.0, 0.0]), v


def loose(pos, vel):
    g = capi.Solver(capi.Options(solver=capi.PBD))
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=0.05)
    g.finalize()
    return g


def groups_now():
    return [capi.TieGroup.make((5.0 * k, 2.0, 30.0 * k)) for k in range(N_GROUPS)]


def tie_set(n_nodes, count, hub_row=0):
    """`count` ties: distinct random tied nodes while they last, each on a triangle of three nodes a little further along the
    lattice's node order (neighbours in memory, as a seam's are); the first hub_row ties share node 0 as a corner"""
    rng = np.random.default_rng(5)
    tied = rng.permutation(n_nodes - 500)[:count] if count <= n_nodes - 500 else rng.integers(0, n_nodes - 500, count)
    ties = []
    for k, a in enumerate(tied):
        a = int(a) + 1
        b = [a + int(x) for x in rng.choice(np.arange(1, 499), 3, replace=False)]
        if k < hub_row:
            b[0] = 0
        u, v = rng.uniform(0.1, 0.4, 2)
        ties.append(capi.Tie.on_triangle(a, b, u, v, stiffness=500.0, damping=2.0, group=k % N_GROUPS))
    return ties


def timed(call):
    ts = []
    for k in range(WARM + REPEATS):
        t0 = time.perf_counter()
        call()
        if k >= WARM:
            ts.append((time.perf_counter() - t0) * 1e6)
    return {"us_per_call": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1)}


def kernel_stats(path):
    """per-launch microseconds of the call's kernels from a rocprofv3 kernel stats CSV"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for kernel in ("k_tie_evaluate<true>", "k_tie_evaluate<false>", "k_tie_scatter", "k_anchor_sums", "k_prop_fold"):
                if kernel in name:
                    out[kernel] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                   "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def calls_only(count):
    """for the profiler: one set size, ten calls of 4 iterations with the reaction"""
    pos, vel = lattice(scenes.L100K)
    g = loose(pos, vel)
    s = g.add_ties(tie_set(len(pos), count), N_GROUPS)
    for _ in range(10):
        g.apply_ties(s, groups_now(), DT, 4)
    g.close()


def sewn_boxes(ticks=120):
    """the sewing recipe of INTEGRATION.md: closest points of the rim on the body's surface, then the second body, then the ties"""
    g = capi.Solver(capi.Options(solver=capi.PBD))
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)  # (the facing nodes are closer than their radii: the seam is what is looked at)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5))
    n = g.count(capi.NODES)
    pos = g.positions
    face = pos[pos[:, 0] == pos[:, 0].max()] + np.float32([0.125, 0.0, 0.0])  # where the second box's facing nodes will be
    tri, dist, uv, _ = g.closest_points(face)
    corners = g.ids(capi.TRIANGLES)[tri]
    g.create_tet_box(3, 3, 3, translation=(float(face[0, 0]), 1.5, 0.5))
    pos = g.positions
    ties = []
    for point, c, (u, v) in zip(face, corners, uv):
        a = n + int(np.argmin(np.abs(pos[n:] - point).sum(axis=1)))
        ties.append(capi.Tie.on_triangle(a, [int(i) for i in c], u, v, stiffness=600.0, damping=2.0))
    s = g.add_ties(ties)
    dt = float(g.options.fixedTimestepSize)  # the ties act for the time a tick covers
    first = largest = last = 0.0
    for t in range(ticks):
        g.tick()
        stretch = g.apply_ties(s, [capi.TieGroup.make()], dt, 4, reaction=False, per_tie=True)[0][:, 3]
        first = float(stretch.max()) if t == 0 else first
        largest, last = max(largest, float(stretch.max())), float(stretch.max())
    ok = bool(np.isfinite(g.positions).all()) and not g.failed
    lowest = float(g.positions[:, 1].min())
    g.close()
    return {"ticks": ticks, "ties": len(ties), "iterations": 4, "dt": dt, "stretch_at_start": round(float(dist.max()), 5),
            "after_first_tick": round(first, 5), "largest": round(largest, 5), "at_end": round(last, 5), "lowest_node_y": round(lowest, 4),
            "finite": ok}


def main():
    if sys.argv[1] == "--calls":
        return calls_only(int(sys.argv[2]))
    if sys.argv[1] == "--seam":
        return print(json.dumps(sewn_boxes()), flush=True)
    out_path = sys.argv[1]
    pos, vel = lattice(scenes.L100K)
    g = loose(pos, vel)
    r = {"timing": "host clock, median (min) of %d calls after %d warm-up calls" % (REPEATS, WARM), "dt": DT, "nodes": len(pos),
         "groups": N_GROUPS, "sets": [], "rows": [], "forces_us": {}}
    forces = [capi.Force.directional((0.0, 0.0, 3.0)) if k % 2 else capi.Force.drag(1.5, velocity=(1.0, 0.0, 0.0)) for k in range(8)]
    for reaction in (False, True):
        r["forces_us"]["reaction" if reaction else "no reaction"] = timed(lambda: g.apply_forces(forces, DT, reaction=reaction))
    print(json.dumps(r["forces_us"]), flush=True)
    groups = groups_now()
    for count in SIZES:
        s = g.add_ties(tie_set(len(pos), count), N_GROUPS)
        t0 = time.perf_counter()
        live = g.apply_ties(s, groups, DT, 1)[2]
        row = {"ties": count, "live": int(live.sum()), "first_call_us": round((time.perf_counter() - t0) * 1e6, 1)}
        for it in ITERATIONS:
            row["iterations_%d" % it] = {"no_reaction": timed(lambda: g.apply_ties(s, groups, DT, it, reaction=False)),
                                         "reaction": timed(lambda: g.apply_ties(s, groups, DT, it)),
                                         "reaction_and_per_tie": timed(lambda: g.apply_ties(s, groups, DT, it, per_tie=True))}
        r["sets"].append(row)
        print(json.dumps(row), flush=True)
    for length in ROWS:
        s = g.add_ties(tie_set(len(pos), 10000, hub_row=length), N_GROUPS)
        g.apply_ties(s, groups, DT, 1)
        row = {"ties": 10000, "longest_row": max(length, 1), "iterations_4": timed(lambda: g.apply_ties(s, groups, DT, 4, reaction=False))}
        r["rows"].append(row)
        print(json.dumps(row), flush=True)
    assert np.isfinite(g.velocities).all()
    g.close()
    r["seam"] = sewn_boxes()
    print(json.dumps(r["seam"]), flush=True)
    for k, arg in enumerate(sys.argv):
        if arg == "--stats":
            size, path = sys.argv[k + 1].split("=", 1)
            r.setdefault("kernels", {})[size] = kernel_stats(path)
    if "kernels" in r:
        print(json.dumps(r["kernels"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
