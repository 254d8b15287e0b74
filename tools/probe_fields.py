"""pies_collide_field_props on the scenes of tools/probe_props.py - 100 000 and 1 000 000 loose nodes, unit spacing, radius 0.5,
random velocities - with its method: 1, 8 and 64 field props of a 64 x 64 x 64 field that touch no node, a few nodes or every
node, with and without the reaction outputs, and beside every row pies_collide_props with spheres of the same extent in the same
run.  Recorded, not gated:

  us_per_call        host clock around the call (it ends in a stream synchronisation; the copy of the records in and of the
                     reaction out are part of it), median of the repeats, after probe_props' preparation: the node state is put
                     back (write + upload) and one untimed call that touches nothing follows the upload
  spheres_us         the same for pies_collide_props with probe_props' spheres
  nodes_touched      nodes at least one prop touched, hits summed over the props
  build              pies_add_field_tri_mesh on a lattice of 64 samples along the mesh's longest axis: host clock around the call
                     (uploads, the brute-force distance and winding launches, the copy of the samples back), the 432-triangle
                     turned box and the same box with 4 800 triangles; the first build of a handle also allocates its buffers

The fields: "few" and "none" place a sampled sphere of radius 1 (cell 0.05: the lattice spans 3.15, enough for the node's own
0.5) where probe_props places its spheres of radius 1; "all" places a lattice that spans the whole body, sampled from a sphere that
holds it, as probe_props' one large sphere does.

    python tools/probe_fields.py profiles/fields_probe.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from pies_amd import capi  # noqa: E402
from probe_props import PROPS, REPEATS, SIZES, WARM, lattice, put_back, spheres  # noqa: E402
from test_raycast import turned_box  # noqa: E402

N = 64


def sampled_sphere(cell, radius):
    """(samples (N, N, N), origin, cell): a sphere about the local origin, which is the lattice's middle"""
    half = 0.5 * (N - 1) * cell
    axis = -half + np.arange(N) * cell
    z, y, x = np.meshgrid(axis, axis, axis, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - radius).astype(np.float32), (-half, -half, -half), cell


def field_props(pos, balls, touch, small, large):
    """probe_props' spheres as field props: the same centres and motion"""
    out = []
    for b in balls:
        motion = dict(velocity=list(b.velocity), angular=list(b.angular), friction=b.friction)
        if touch == "all":
            mid = 0.5 * (pos.min(0).astype(np.float64) + pos.max(0).astype(np.float64))
            out.append(capi.FieldProp.make(large, mid, **motion))
        else:
            out.append(capi.FieldProp.make(small, list(b.centre), **motion))
    return out


def timed(g, pos, vel, far, call):
    ts = []
    for k in range(WARM + REPEATS):
        put_back(g, pos, vel)
        g.collide_props(far, reaction=False)  # touches nothing; takes the delay that follows an upload
        t0 = time.perf_counter()
        call()
        if k >= WARM:
            ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1), round(float(np.min(ts)) * 1e6, 1)


def build_times():
    rows = []
    g = capi.Solver(capi.Options(solver=capi.PBD))
    for n in (6, 20, 6):
        P, tri = turned_box(n)
        margin = 0.5
        cell = float((P.max(0) - P.min(0)).max() + 2 * margin) / (N - 1)
        t0 = time.perf_counter()
        field = g.add_field_tri_mesh(P, tri, cell, margin)
        ms = (time.perf_counter() - t0) * 1e3
        samples = g.get_field(field)[0]
        rows.append({"triangles": len(tri), "dims": list(samples.shape[::-1]), "samples": int(samples.size), "build_ms": round(ms, 2),
                     "inside": int(np.signbit(samples).sum()), "first_build_of_the_handle": field == 0})
        print(json.dumps(rows[-1]), flush=True)
    g.close()
    return rows


def main():
    out_path = sys.argv[1]
    r = {"timing": "host clock, median (min) of %d calls after %d warm-up calls; before every call the node state is put back and one call that touches nothing is made" % (REPEATS, WARM),
         "build": build_times(), "scenes": []}
    for name, dims in SIZES:
        pos, vel = lattice(dims)
        g = capi.Solver(capi.Options(solver=capi.PBD))
        g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
        g.add_nodes_raw(pos, vel=vel, radius=0.5)
        extent = float(np.linalg.norm(pos.max(0) - pos.min(0)))
        small = g.add_field(*sampled_sphere(0.05, 1.0))
        large = g.add_field(*sampled_sphere(1.05 * extent / (N - 1), extent))
        g.finalize()
        row = {"scene": name, "nodes": len(pos), "calls": []}
        far = spheres(pos, 1, "none")
        for count in PROPS:
            for touch in ("none", "few", "all"):
                balls = spheres(pos, count, touch)
                props = field_props(pos, balls, touch, small, large)
                for reaction in (False, True):
                    us, lo = timed(g, pos, vel, far, lambda: g.collide_field_props(props, reaction=reaction))
                    sus, slo = timed(g, pos, vel, far, lambda: g.collide_props(balls, reaction=reaction))
                    put_back(g, pos, vel)
                    _, _, hits, who = g.collide_field_props(props, node_prop=True)
                    put_back(g, pos, vel)
                    _, _, shits, _ = g.collide_props(balls, node_prop=True)
                    call = {"props": count, "touch": touch, "reaction": reaction, "us_per_call": us, "min_us": lo, "spheres_us": sus,
                            "spheres_min_us": slo, "nodes_touched": int((who != capi.PROP_NONE).sum()), "hits": int(hits.sum()),
                            "spheres_hits": int(shits.sum())}
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
