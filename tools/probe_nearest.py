"""pies_closest_points at the size the project is built for: query points against the surface of BASELINE config 3's PD beam
(20 x 20 x 250 lattice, 39 292 surface triangles) after three ticks, both kernel variants of the distance pass pinned in turn, with
and without the winding pass.  Recorded, not gated:

  us_per_call            host clock around pies_closest_points (the call ends in a stream synchronisation; the copies of the
                         points in and of the answers out are part of it), median of the repeats after warm-up calls
  pairs_per_s            points x triangles / that time
  winding_us             what asking for the winding number adds to the call (same variant, median against median)
  crossover_points       the largest point count of the sweep (powers of two up to 4 096) at which the narrow variant is no slower
                         than the wide one: the figure for PIES_NEAR_NARROW_MAX

    python tools/probe_nearest.py profiles/nearest_probe.json
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


def points(g, count, seed=1):
    """Uniform points in the beam's bounding box grown by a quarter about its centre: inside and outside both occur"""
    rng = np.random.default_rng(seed)
    p = g.positions.astype(np.float64)
    mid, half = 0.5 * (p.min(0) + p.max(0)), 0.625 * (p.max(0) - p.min(0))
    return rng.uniform(mid - half, mid + half, (count, 3)).astype(np.float32)


def time_call(g, p, winding, repeats, warm):
    for _ in range(warm):
        g.closest_points(p, winding=winding)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        g.closest_points(p, winding=winding)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    out_path = sys.argv[1]
    g = bench.pd_beam(scenes.L100K, 0, settle=3)
    n_tri = g.count(capi.TRIANGLES)
    r = {"scene": "BASELINE configs[2]: 20x20x250 PD beam, its %d surface triangles (PIES_RAY_SCENE_TRIANGLES) after 3 ticks" % n_tri,
         "triangles": n_tri,
         "timing": "host clock around pies_closest_points, median (min) over the repeats; includes the copies in and out",
         "calls": []}
    for count in sorted(set(HEADLINE + SWEEP)):
        p = points(g, count)
        repeats, warm = (5, 1) if count > 100000 else (100, 10)
        row = {"points": count}
        answers = {}
        for variant in ("narrow", "wide"):
            capi.set_tuning("PIES_NEAR_VARIANT", variant)
            med, low = time_call(g, p, False, repeats, warm)
            wmed, wlow = time_call(g, p, True, repeats, warm)
            answers[variant] = g.closest_points(p, winding=True)
            row[variant] = {"us_per_call": round(med * 1e6, 1), "min_us": round(low * 1e6, 1), "pairs_per_s": round(count * n_tri / med, 1),
                            "with_winding_us_per_call": round(wmed * 1e6, 1), "with_winding_min_us": round(wlow * 1e6, 1),
                            "winding_us": round((wmed - med) * 1e6, 1), "repeats": repeats}
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(answers["narrow"], answers["wide"]))
        capi.set_tuning("PIES_NEAR_VARIANT", None)
        row["inside"] = int((np.abs(answers["wide"][4]) > 0.5).sum())
        row["headline"] = count in HEADLINE
        r["calls"].append(row)
        print(json.dumps(row), flush=True)
    sweep = [row for row in r["calls"] if row["points"] in SWEEP]
    faster = [row["points"] for row in sweep if row["narrow"]["us_per_call"] <= row["wide"]["us_per_call"]]
    r["crossover_points"] = max(faster) if faster else 0
    r["narrow_no_slower_at"] = faster
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps({k: v for k, v in r.items() if k != "calls"}))


if __name__ == "__main__":
    main()
