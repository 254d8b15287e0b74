"""PIES_FLAG_PD_NODE_CONTACTS: what the PD node-node contacts cost.  Per run: PD substeps/s, in-situ us per substep of the node
grid's build (class hash) and of the detection, the contacts' local steps and their friction pass (class collide), the contacts
of the last substep, launches per substep.

    python tools/probe_pd_node_contacts.py [out.json] [NAME=VALUE ...]   (NAME=VALUE: pies_set_tuning before the runs)

Scenes: BASELINE config 3 (the 100k-node PD beam at rest: the pure detection cost) with the flag off and on; scenes.L500K loose
particles under PD with the flag on, while the block bursts apart and once it has settled; a 2 000-node PD rope coiling onto the
floor.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib")):
    sys.path.insert(0, p)
import bench  # noqa: E402
import scenes  # noqa: E402
from pies_amd import capi  # noqa: E402


def config3(on):
    W, H, D = scenes.L100K
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=0)
    g.create_tet_box(W, H, D, translation=(0.0, 2.0, 0.0), w=1.0, volume=True, triangles=True)
    g.add_position(np.array([D * (j + H * i) for i in range(W) for j in range(H)], dtype=np.uint32), 2.0)
    g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1 if on else 0)
    return g


def particles():
    p, v = bench.config4_particles()
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10, gravity=0.0), device=0)
    g.add_nodes_raw(p, vel=v, radius=0.5)
    g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1)
    return g


def rope(n=2000, spacing=0.4, r=0.2):
    """A rope of distance constraints (spacing 0.4, r 0.2) laid out as a helix of radius 1.5 that falls onto a floor and coils on
    itself.  (PD's floor acts through surface triangles only, so the floor is a 24 x 24 plate of particles held by position
    constraints.)"""
    t = np.arange(n) * spacing / 1.5
    p = np.stack([1.5 * np.cos(t), 1.0 + 0.25 * t, 1.5 * np.sin(t)], 1).astype(np.float32)
    X, Z = np.meshgrid(np.arange(24) * 0.35 - 4.0, np.arange(24) * 0.35 - 4.0, indexing="ij")
    plate = np.stack([X.ravel(), np.full(X.size, 0.2), Z.ravel()], 1).astype(np.float32)
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=0)
    g.add_nodes_raw(p, radius=r)
    g.add_distance(np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.uint32), 100.0)
    first = g.add_nodes_raw(plate, radius=r)
    g.add_position(np.arange(first, first + len(plate), dtype=np.uint32), 1000.0)
    g.set_flag(capi.FLAG_PD_NODE_CONTACTS, 1)
    return g


def measure(g, tag, settle, steps=20):
    t0 = time.perf_counter()
    g.finalize()
    fin = time.perf_counter() - t0
    for _ in range(settle):
        g.tick_async(1)
        g.synchronize()
    el = bench.timed_ticks(g, steps, 2, lambda: None)
    r = {"scene": tag, "nodes": g.count(capi.NODES), "substeps_per_s": round(steps / el, 1), "finalize_s": round(fin, 2),
         "contacts": g.count(capi.NODE_CONTACTS), "launches_per_substep": sum(g.launch_counts().values()),
         "pcg_health": g.pcg_health(), "failed": g.failed}
    for name in ("hash", "collide"):
        cnt, ms, units, ov = g.profile_in_situ(bench.K[name], 2)
        r[name + "_us_per_substep"] = round((1e3 * ms - 1e3 * ov * cnt) / 2, 1) if cnt else 0.0
        r[name + "_brackets_per_substep"] = cnt // 2
    print("%-26s %8d nodes %8.1f substeps/s  hash %7.1f us  collide %7.1f us  contacts %8d  launches %4d%s" % (
        tag, r["nodes"], r["substeps_per_s"], r["hash_us_per_substep"], r["collide_us_per_substep"], r["contacts"],
        r["launches_per_substep"], "  FAILED: " + g.last_error() if g.failed else ""), flush=True)
    return r


def main():
    out = None
    for a in sys.argv[1:]:
        if "=" in a:
            k, v = a.split("=", 1)
            capi.set_tuning(k, v)
        else:
            out = a
    rows = []
    for on in (False, True):
        g = config3(on)
        rows.append(dict(measure(g, "config3 flag " + ("on" if on else "off"), 34), flag=int(on)))
        g.close()
    g = particles()
    rows.append(dict(measure(g, "L500K particles bursting", 0, 10), flag=1))
    for _ in range(200):
        g.tick_async(1)
    g.synchronize()
    rows.append(dict(measure(g, "L500K particles settled", 20, 10), flag=1))
    g.close()
    g = rope()
    for _ in range(150):  # falling and coiling
        g.tick_async(1)
    g.synchronize()
    rows.append(dict(measure(g, "2000-node rope coiling", 10), flag=1))
    g.close()
    if rows[0]["substeps_per_s"]:
        print("config3: flag on / off = %.3f" % (rows[1]["substeps_per_s"] / rows[0]["substeps_per_s"]))
    if out:
        with open(out, "w") as f:
            json.dump({"runs": rows}, f, indent=1)


if __name__ == "__main__":
    main()
