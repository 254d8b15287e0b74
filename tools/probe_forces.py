"""pies_apply_forces at the sizes the project is built for: loose nodes on the 20 x 20 x 250 lattice of BASELINE config 3 (100 000
nodes) and on a 100 x 100 x 100 lattice (1 000 000), unit spacing, random velocities; 1, 8 and 64 point forces (the types cycle
radial, vortex, drag, directional; the falloffs none, linear, smooth) that act everywhere or in a sphere of radius 3 inside the body;
with and without the reaction outputs; and a wind - everywhere, and in a sphere that holds a tenth of the sheet - on a 300 x 300
triangulated sheet (90 000 nodes, 178 802 triangles).  The cost of the call does not depend on the constraints of a scene (it runs
outside the substep), so the nodes carry none and the handle is a PBD one without node-node collisions.  Nothing is put back between
calls: the call's cost does not depend on the velocities it finds, and positions never change.

  us_per_call        host clock around pies_apply_forces (the call ends in a stream synchronisation; the copy of the records in and
                     of the reaction out are part of it), median of the repeats; min_us the fastest
  nodes_affected     out_nodes summed over the forces
  write_route_us     (median; write_route_min_us the fastest) the route the call replaces, on the same scene in the same run:
                     pies_read_nodes of positions and velocities (both stale, as after a tick), pies_write_nodes of the velocities
                     and the upload the next tick would start with (pies_finalize of a scene whose node state alone is dirty) -
                     without the host's own loop over the nodes
  gate               the one cost requirement: at both sizes every 8-force call (median) is cheaper than write_route_min_us

    python tools/probe_forces.py profiles/forces_probe.json
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
FORCES = (1, 8, 64)
REPEATS, WARM = 9, 2
DT = 1.0 / 60.0
SHEET = 300


def lattice(dims):
    W, H, D = dims
    p = np.stack(np.meshgrid(np.arange(W), np.arange(H), np.arange(D), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    v = np.random.default_rng(7).normal(size=p.shape).astype(np.float32)
    return p + np.float32([0.0, 2.0, 0.0]), v


def point_forces(pos, count, where):
    rng = np.random.default_rng(3)
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    out = []
    for k in range(count):
        c = rng.uniform(lo + 2, hi - 2)
        f = (capi.Force.radial(c, 2.0), capi.Force.vortex(c, (0.0, 1.0, 0.0), 0.5), capi.Force.drag(1.5, velocity=(1.0, 0.0, 0.0)),
             capi.Force.directional((0.0, 0.0, 3.0), is_force=True))[k % 4]
        out.append(f.within(c, float("inf") if where == "everywhere" else 3.0, k % 3))
    return out


def sheet(n):
    gx, gz = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([gx * 0.1, 5.0 + 0.05 * np.sin(gx * 0.3) * np.cos(gz * 0.2), gz * 0.1], axis=-1).reshape(-1, 3).astype(np.float32)
    a = (gx[:-1, :-1] * n + gz[:-1, :-1]).ravel()
    tris = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.uint32)
    return pos, np.random.default_rng(9).normal(size=pos.shape).astype(np.float32), tris


def loose(pos, vel, tris=None):
    g = capi.Solver(capi.Options(solver=capi.PBD))
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=0.05)
    if tris is not None:
        g.add_triangles(tris)
    g.finalize()
    return g


def time_calls(g, forces, reaction):
    ts, nodes = [], 0
    for k in range(WARM + REPEATS):
        t0 = time.perf_counter()
        out = g.apply_forces(forces, DT, reaction=reaction)
        if k >= WARM:
            ts.append(time.perf_counter() - t0)
        if reaction:
            nodes = int(out[2].sum())
    return {"reaction": reaction, "us_per_call": round(float(np.median(ts)) * 1e6, 1), "min_us": round(float(np.min(ts)) * 1e6, 1),
            **({"nodes_affected": nodes} if reaction else {})}


def write_route(g, pos):
    """the route the call replaces (the state does not change: what is written is what was read)"""
    far = [capi.Prop.sphere(pos.max(0).astype(np.float64) + [0.0, 1.0e4, 0.0], 1.0)]
    ts = []
    for k in range(WARM + REPEATS):
        g.collide_props(far, reaction=False)  # touches nothing; marks the mirror stale, as a tick would have
        t0 = time.perf_counter()
        p, v = g.positions, g.velocities
        g.set_velocities(v)
        g.finalize()
        g.synchronize()
        if k >= WARM:
            ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1), round(float(np.min(ts)) * 1e6, 1)


def main():
    out_path = sys.argv[1]
    r = {"timing": "host clock, median (min) of %d calls after %d warm-up calls" % (REPEATS, WARM), "dt": DT, "scenes": [], "gate": {}}
    for name, dims in SIZES:
        pos, vel = lattice(dims)
        g = loose(pos, vel)
        row = {"scene": name, "nodes": len(pos), "calls": []}
        row["write_route_us"], row["write_route_min_us"] = write_route(g, pos)
        print(json.dumps({k: v for k, v in row.items() if k != "calls"}), flush=True)
        for count in FORCES:
            for where in ("everywhere", "sphere of radius 3"):
                forces = point_forces(pos, count, where)
                for reaction in (False, True):
                    call = {"forces": count, "region": where, **time_calls(g, forces, reaction)}
                    row["calls"].append(call)
                    print(json.dumps(call), flush=True)
        eight = max(c["us_per_call"] for c in row["calls"] if c["forces"] == 8)
        r["gate"][name] = {"slowest_8_force_call_us": eight, "write_route_min_us": row["write_route_min_us"],
                           "cheaper": bool(eight < row["write_route_min_us"])}
        assert np.isfinite(g.velocities).all()
        g.close()
        r["scenes"].append(row)
    pos, vel, tris = sheet(SHEET)
    g = loose(pos, vel, tris)
    row = {"scene": "sheet %d x %d" % (SHEET, SHEET), "nodes": len(pos), "triangles": len(tris), "calls": []}
    row["write_route_us"], row["write_route_min_us"] = write_route(g, pos)
    middle = pos[len(pos) // 2 + SHEET // 2].astype(np.float64)
    for where, wind in (("everywhere", capi.Force.wind((3.0, 0.5, 8.0), 1.2, shear=0.2)),
                        ("a tenth of the sheet", capi.Force.wind((3.0, 0.5, 8.0), 1.2, shear=0.2).within(middle, 5.35, capi.FALLOFF_SMOOTH))):
        for reaction in (False, True):
            call = {"forces": 1, "type": "wind", "region": where, **time_calls(g, [wind], reaction)}
            row["calls"].append(call)
            print(json.dumps(call), flush=True)
    call = {"forces": 2, "type": "wind + drag", "region": "everywhere",
            **time_calls(g, [capi.Force.wind((3.0, 0.5, 8.0), 1.2, shear=0.2), capi.Force.drag(0.5)], True)}
    row["calls"].append(call)
    print(json.dumps(call), flush=True)
    assert np.isfinite(g.velocities).all()
    g.close()
    r["scenes"].append(row)
    print(json.dumps(r["gate"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)
    if not all(v["cheaper"] for v in r["gate"].values()):
        sys.exit("pies_apply_forces with 8 forces is not cheaper than the route it replaces")


if __name__ == "__main__":
    main()
