"""pies_apply_anchors at the sizes the project is built for: loose nodes on the 20 x 20 x 250 lattice of BASELINE config 3 (100 000
nodes), unit spacing, random velocities; a set of 100 anchors, one of 10 000 (random nodes, a tenth of them with a second spring)
and one with an anchor on every node; four frames that move and turn; with and without the reaction outputs, and with the
per-anchor array.  The cost of the call does not depend on the constraints of a scene (it runs outside the substep), so the nodes
carry none and the handle is a PBD one without node-node collisions.  Springs only: nothing is put back between calls, positions
never change and the call's cost does not depend on the velocities it finds.

  us_per_call        host clock around pies_apply_anchors (the call ends in a stream synchronisation; the copy of the frames in and
                     of the reaction out are part of it), median of the repeats; min_us the fastest
  first_call_us      the first call of a set: it stages the set's device copy
  forces_us          the comparison: pies_apply_forces with 8 point forces that act everywhere, on the same scene in the same run
  kernels            per launch, from a rocprofv3 --kernel-trace --stats run of `--calls ANCHORS` (one run per set size; its kernel
                     stats CSV is given with --stats SIZE=CSV, as often as there are sizes)

    PIES_PROFILER_SAFE=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_anchors.py --calls 10000
    python tools/probe_anchors.py profiles/anchors_probe.json [--stats 100=CSV --stats 10000=CSV --stats 100000=CSV]
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

SIZES = (100, 10000, 100000)
REPEATS, WARM = 15, 3
DT = 1.0 / 60.0
N_FRAMES = 4


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


def frames_now():
    return [capi.AnchorFrame.make((5.0 * k, 2.0, 30.0 * k), velocity=(0.5, 0.0, 1.0), angular=(0.0, 0.25 * k, 0.0), strength=1.0)
            for k in range(N_FRAMES)]


def anchor_set(pos, count):
    """`count` spring anchors: every node once when count is the node count, else random nodes, a tenth of them twice"""
    rng = np.random.default_rng(5)
    n = len(pos)
    nodes = np.arange(n) if count >= n else rng.choice(n, count - count // 10, replace=False)
    nodes = np.concatenate([nodes, nodes[:count - len(nodes)]])
    rest = frames_now()
    for f in rest:
        f.origin[1] += 0.05  # the springs are stretched
    return [capi.Anchor.at(int(i), int(k % N_FRAMES), rest[k % N_FRAMES], pos[i], stiffness=500.0, damping=2.0) for k, i in enumerate(nodes)]


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
            for kernel in ("k_anchor_evaluate", "k_anchor_sums", "k_prop_fold"):
                if kernel in name:
                    out[kernel] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                   "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def calls_only(count):
    """for the profiler: one set size, ten calls with the reaction (evaluate with its second walk, sums, fold)"""
    pos, vel = lattice(scenes.L100K)
    g = loose(pos, vel)
    s = g.add_anchors(anchor_set(pos, count), N_FRAMES)
    for _ in range(10):
        g.apply_anchors(s, frames_now(), DT)
    g.close()


def main():
    if sys.argv[1] == "--calls":
        return calls_only(int(sys.argv[2]))
    out_path = sys.argv[1]
    pos, vel = lattice(scenes.L100K)
    g = loose(pos, vel)
    r = {"timing": "host clock, median (min) of %d calls after %d warm-up calls" % (REPEATS, WARM), "dt": DT, "nodes": len(pos),
         "frames": N_FRAMES, "sets": [], "forces_us": {}}
    forces = [capi.Force.directional((0.0, 0.0, 3.0)) if k % 2 else capi.Force.drag(1.5, velocity=(1.0, 0.0, 0.0)) for k in range(8)]
    for reaction in (False, True):
        r["forces_us"]["reaction" if reaction else "no reaction"] = timed(lambda: g.apply_forces(forces, DT, reaction=reaction))
    print(json.dumps(r["forces_us"]), flush=True)
    frames = frames_now()
    for count in SIZES:
        s = g.add_anchors(anchor_set(pos, count), N_FRAMES)
        t0 = time.perf_counter()
        live = g.apply_anchors(s, frames, DT)[2]
        row = {"anchors": count, "live": int(live.sum()), "first_call_us": round((time.perf_counter() - t0) * 1e6, 1)}
        row["no_reaction"] = timed(lambda: g.apply_anchors(s, frames, DT, reaction=False))
        row["reaction"] = timed(lambda: g.apply_anchors(s, frames, DT))
        row["reaction_and_per_anchor"] = timed(lambda: g.apply_anchors(s, frames, DT, per_anchor=True))
        r["sets"].append(row)
        print(json.dumps(row), flush=True)
    assert np.isfinite(g.velocities).all()
    g.close()
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
