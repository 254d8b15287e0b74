"""pies_raycast at the size the project is built for: rays against the surface of BASELINE config 3's PD beam (20 x 20 x 250
lattice, 39 292 surface triangles), both kernel variants pinned in turn.  Recorded, not gated:

  us_per_call            host clock around pies_raycast (the call ends in a stream synchronisation; the copies of the rays in and
                         of the hits out are part of it), median of the repeats after warm-up calls
  pairs_per_s            rays x triangles / that time
  crossover_rays         the largest ray count of the sweep (powers of two up to 4 096) at which the narrow variant is no slower
                         than the wide one: the figure for PIES_RAY_NARROW_MAX

    python tools/probe_raycast.py profiles/raycast_probe.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import bench  # noqa: E402
import scenes  # noqa: E402
from pies_amd import capi  # noqa: E402

HEADLINE = (1, 64, 4096, 1048576)
SWEEP = tuple(2 ** k for k in range(13))


def rays(g, count, seed=1):
    """Origins around the beam, directions towards random points inside its bounding box: most rays hit"""
    rng = np.random.default_rng(seed)
    p = g.positions
    lo, hi = p.min(0), p.max(0)
    inside = rng.uniform(lo, hi, (count, 3))
    u = rng.normal(size=(count, 3))
    o = inside + 30.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    return o.astype(np.float32), (inside - o).astype(np.float32)


def time_call(g, o, d, repeats, warm):
    for _ in range(warm):
        g.raycast(o, d)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        g.raycast(o, d)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    out_path = sys.argv[1]
    g = bench.pd_beam(scenes.L100K, 0, settle=3)
    n_tri = g.count(capi.TRIANGLES)
    r = {"scene": "BASELINE configs[2]: 20x20x250 PD beam, its %d surface triangles (PIES_RAY_SCENE_TRIANGLES) after 3 ticks" % n_tri,
         "triangles": n_tri, "timing": "host clock around pies_raycast, median (min) over the repeats; includes the copies in and out",
         "calls": []}
    results = {}
    for count in sorted(set(HEADLINE + SWEEP)):
        o, d = rays(g, count)
        repeats, warm = (5, 1) if count > 100000 else (100, 10)
        row = {"rays": count}
        for variant in ("narrow", "wide"):
            capi.set_tuning("PIES_RAY_VARIANT", variant)
            med, low = time_call(g, o, d, repeats, warm)
            tri = g.raycast(o, d)[0]
            row[variant] = {"us_per_call": round(med * 1e6, 1), "min_us": round(low * 1e6, 1), "pairs_per_s": round(count * n_tri / med, 1),
                            "repeats": repeats}
            row["hits"] = int((tri != capi.RAY_MISS).sum())
            results[(count, variant)] = tri
        assert np.array_equal(results[(count, "narrow")], results[(count, "wide")])
        capi.set_tuning("PIES_RAY_VARIANT", None)
        row["headline"] = count in HEADLINE
        r["calls"].append(row)
        print(json.dumps(row), flush=True)
    sweep = [row for row in r["calls"] if row["rays"] in SWEEP]
    faster = [row["rays"] for row in sweep if row["narrow"]["us_per_call"] <= row["wide"]["us_per_call"]]
    r["crossover_rays"] = max(faster) if faster else 0
    r["narrow_no_slower_at"] = faster
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps({k: v for k, v in r.items() if k != "calls"}))


if __name__ == "__main__":
    main()
