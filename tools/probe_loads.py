"""pies_apply_surface_loads at the sizes the project is built for: a closed surface - a torus of 316 x 316 nodes (99 856 nodes,
199 712 triangles) and one of 1 000 x 1 000 (1 000 000 nodes, 2 000 000 triangles), wound outward, random velocities - under 1 and 8
loads of each type on the whole surface (the worst case: every load meets every triangle): a constant pressure, a gas, a fluid
whose surface cuts the torus in half, the same fluid with drag; with and without the reaction outputs.  The cost of the call does
not depend on the constraints of a scene (it runs outside the substep), so the nodes carry none and the handle is a PBD one
without node-node collisions.  Nothing is put back between calls: the call's cost does not depend on the velocities it finds, and
positions never change.

  us_per_call        host clock around pies_apply_surface_loads (the call ends in a stream synchronisation; the copy of the records
                     in and of the outputs back are part of it), median of the repeats; min_us the fastest
  nodes_affected     out_nodes summed over the loads
  write_route_us     (median; write_route_min_us the fastest) the route the call replaces, on the same scene in the same run:
                     pies_read_nodes of positions and velocities (both stale, as after a tick), pies_write_nodes of the velocities
                     and the upload the next tick would start with (pies_finalize of a scene whose node state alone is dirty) -
                     without the host's own loop over the triangles
  gate               the one cost requirement: at both sizes every 8-load call with the reaction (median) is cheaper than
                     write_route_min_us

    python tools/probe_loads.py profiles/loads_probe.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pies_amd import capi  # noqa: E402

SIZES = (("100k", 316), ("1M", 1000))
LOADS = (1, 8)
REPEATS, WARM = 9, 2
DT = 1.0 / 60.0
MAJOR, MINOR, CENTRE = 6.0, 2.0, (0.0, 10.0, 0.0)


def torus(n):
    """(positions, velocities, triangles) of an n x n torus about the y axis, wound outward"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    u, v = i * (2 * np.pi / n), j * (2 * np.pi / n)
    ring = MAJOR + MINOR * np.cos(v)
    pos = (np.stack([ring * np.cos(u), MINOR * np.sin(v), ring * np.sin(u)], axis=-1).reshape(-1, 3) + CENTRE).astype(np.float32)
    a, b, c, d = i * n + j, ((i + 1) % n) * n + j, ((i + 1) % n) * n + (j + 1) % n, i * n + (j + 1) % n
    tris = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([a, d, c], -1).reshape(-1, 3)]).astype(np.uint32)
    return pos, np.random.default_rng(7).normal(size=pos.shape).astype(np.float32), tris


def make_loads(kind, count, volume):
    out = []
    for k in range(count):
        if kind == "pressure":
            out.append(capi.SurfaceLoad.pressure(0.5 + 0.125 * k, about=CENTRE))
        elif kind == "gas":
            out.append(capi.SurfaceLoad.gas(1.0, volume * (1.0 + 0.0625 * (k + 1)), about=CENTRE))
        else:
            L = capi.SurfaceLoad.fluid(9.8125, (0.0, CENTRE[1] + 0.001 * (k + 1), 0.0))
            out.append(L.with_drag(0.5, (0.25, 0.0, 0.0)) if kind == "fluid with drag" else L)
    return out


def loose(pos, vel, tris):
    g = capi.Solver(capi.Options(solver=capi.PBD))
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
    g.add_nodes_raw(pos, vel=vel, radius=0.05)
    g.add_triangles(tris)
    g.finalize()
    return g


def time_calls(g, loads, reaction):
    ts, nodes = [], 0
    for k in range(WARM + REPEATS):
        t0 = time.perf_counter()
        out = g.apply_surface_loads(loads, DT, reaction=reaction)
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
    for name, n in SIZES:
        pos, vel, tris = torus(n)
        g = loose(pos, vel, tris)
        measured = g.apply_surface_loads([capi.SurfaceLoad.pressure(0.0)], DT)  # a zero-strength call: the volume and the area
        volume, area = float(measured[3][0]), float(measured[4][0])
        row = {"scene": name, "nodes": len(pos), "triangles": len(tris), "volume": volume, "area": area,
               "volume_exact": 2 * np.pi ** 2 * MAJOR * MINOR ** 2, "area_exact": 4 * np.pi ** 2 * MAJOR * MINOR, "calls": []}
        assert volume > 0, "the torus is wound outward"
        row["write_route_us"], row["write_route_min_us"] = write_route(g, pos)
        print(json.dumps({k: v for k, v in row.items() if k != "calls"}), flush=True)
        for count in LOADS:
            for kind in ("pressure", "gas", "fluid", "fluid with drag"):
                loads = make_loads(kind, count, volume)
                for reaction in (False, True):
                    call = {"loads": count, "type": kind, **time_calls(g, loads, reaction)}
                    row["calls"].append(call)
                    print(json.dumps(call), flush=True)
        eight = max(c["us_per_call"] for c in row["calls"] if c["loads"] == 8 and c["reaction"])
        r["gate"][name] = {"slowest_8_load_call_with_reaction_us": eight, "write_route_min_us": row["write_route_min_us"],
                           "cheaper": bool(eight < row["write_route_min_us"])}
        assert np.isfinite(g.velocities).all()
        g.close()
        r["scenes"].append(row)
    print(json.dumps(r["gate"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)
    if not all(v["cheaper"] for v in r["gate"].values()):
        sys.exit("pies_apply_surface_loads with 8 loads is not cheaper than the route it replaces")


if __name__ == "__main__":
    main()
