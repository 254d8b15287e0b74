"""pies_collide_props at the sizes the project is built for: loose nodes on the 20 x 20 x 250 lattice of BASELINE config 3 (100 000
nodes) and on a 100 x 100 x 100 lattice (1 000 000), unit spacing, radius 0.5, random velocities; 1, 8 and 64 spheres that touch no
node, a few nodes or every node; with and without the reaction outputs.  The cost of the call does not depend on the constraints
of a scene (it runs outside the substep), so the nodes carry none and the handle is a PBD one without node-node collisions.
Recorded, not gated:

  us_per_call        host clock around pies_collide_props (the call ends in a stream synchronisation; the copy of the props in and
                     of the reaction out are part of it), median of the repeats.  The node state is put back before every call
                     (write + upload), and one untimed call with a prop that touches nothing follows the upload: the first
                     call after an upload was observed to take 10 - 27 ms longer at 100 000 nodes (it follows the upload's copies
                     from pageable memory, whatever the call), which belongs to the upload, not to the call timed
  nodes_touched      nodes at least one prop touched, hits summed over the props
  write_route_us     (median; write_route_min_us the fastest) the route the call replaces, on the same scene: pies_read_nodes of
                     positions and velocities, pies_write_nodes of positions, previous positions and velocities, and the upload the next tick would start with (pies_finalize
                     of a scene whose node state alone is dirty) - without the host's own loop over the nodes

    python tools/probe_props.py profiles/props_probe.json
"""
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

SIZES = (("100k", scenes.L100K), ("1M", scenes.L1M))
PROPS = (1, 8, 64)
REPEATS, WARM = 7, 2


def lattice(dims):
    W, H, D = dims
    p = np.stack(np.meshgrid(np.arange(W), np.arange(H), np.arange(D), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    v = np.random.default_rng(7).normal(size=p.shape).astype(np.float32)
    return p + np.float32([0.0, 2.0, 0.0]), v


def spheres(pos, count, touch):
    """none: far from the body; few: radius 1 inside it (a node's own 0.5 counts: some thirty nodes each); all: one far centre and
    a radius that holds the whole body, every prop"""
    rng = np.random.default_rng(3)
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    out = []
    for _ in range(count):
        c = rng.uniform(lo + 2, hi - 2)
        motion = dict(velocity=rng.normal(size=3), angular=rng.normal(size=3) * 0.1, friction=0.5)
        if touch == "none":
            out.append(capi.Prop.sphere(c + [0.0, 1.0e4, 0.0], 1.0, **motion))
        elif touch == "few":
            out.append(capi.Prop.sphere(c, 1.0, **motion))
        else:
            out.append(capi.Prop.sphere(0.5 * (lo + hi) - [0.0, 1.0e3, 0.0], 1.0e3 + float(np.linalg.norm(hi - lo)), **motion))
    return out


def put_back(g, pos, vel):
    g.set_positions(pos)
    g.set_prev_positions(pos)
    g.set_velocities(vel)
    g.finalize()  # the upload


def main():
    out_path = sys.argv[1]
    r = {"timing": "host clock, median (min) of %d calls after %d warm-up calls; before every call the node state is put back and one call that touches nothing is made" % (REPEATS, WARM),
         "scenes": []}
    for name, dims in SIZES:
        pos, vel = lattice(dims)
        g = capi.Solver(capi.Options(solver=capi.PBD))
        g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
        g.add_nodes_raw(pos, vel=vel, radius=0.5)
        g.finalize()
        row = {"scene": name, "nodes": len(pos), "calls": []}
        # the route the call replaces (the state does not change: what is written is what was read)
        ts = []
        for k in range(WARM + REPEATS):
            g.collide_props(spheres(pos, 1, "none"), reaction=False)  # marks the mirror stale, as a tick would have
            t0 = time.perf_counter()
            p, v = g.positions, g.velocities
            g.set_positions(p)
            g.set_prev_positions(p)
            g.set_velocities(v)
            g.finalize()
            g.synchronize()
            if k >= WARM:
                ts.append(time.perf_counter() - t0)
        row["write_route_us"] = round(float(np.median(ts)) * 1e6, 1)
        row["write_route_min_us"] = round(float(np.min(ts)) * 1e6, 1)
        print(json.dumps({k: v for k, v in row.items() if k != "calls"}), flush=True)
        far = spheres(pos, 1, "none")
        for count in PROPS:
            for touch in ("none", "few", "all"):
                props = spheres(pos, count, touch)
                for reaction in (False, True):
                    ts, hits, who = [], None, None
                    for k in range(WARM + REPEATS):
                        put_back(g, pos, vel)
                        g.collide_props(far, reaction=False)  # touches nothing; takes the delay that follows an upload
                        t0 = time.perf_counter()
                        out = g.collide_props(props, reaction=reaction)
                        if k >= WARM:
                            ts.append(time.perf_counter() - t0)
                    put_back(g, pos, vel)
                    _, _, hits, who = g.collide_props(props, node_prop=True)
                    call = {"props": count, "touch": touch, "reaction": reaction, "us_per_call": round(float(np.median(ts)) * 1e6, 1),
                            "min_us": round(float(np.min(ts)) * 1e6, 1), "nodes_touched": int((who != capi.PROP_NONE).sum()),
                            "hits": int(hits.sum())}
                    row["calls"].append(call)
                    print(json.dumps(call), flush=True)
        put_back(g, pos, vel)
        g.close()
        r["scenes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
