"""pies_measure_elements / pies_measure_nodes at the sizes the project is built for: BASELINE config 2's beam (PBD, 20 x 20 x 250 =
100 000 particles, 539 334 tetrahedral constraints) and the PD configuration at the same size (createTetBox with volume
constraints), perturbed (and, for the timing, ticked a few times) so that the elements are strained.

  summary_us / records_us / nodes64_us   host clock around one call (each call ends in a stream synchronisation; the copies out
                     are part of it): the summary alone, records + summary, and 64 ranges of node sums; median of the repeats
                     with the fastest and the spread (max - min) beside it
  bytes_per_element  what the element kernel must move: 16 (ids) + 48 (rest) + 64 (four gathered positions), + 32 stored when
                     records are written
  kernel_us          k_measure_elements per launch, from a rocprofv3 --kernel-trace --stats run of `--calls` (its kernel stats
                     CSV is given with --stats); hbm_fraction = bytes that must move / average kernel time / 8 TB/s

    PIES_PROFILER_SAFE=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_measure.py --calls
    python tools/probe_measure.py profiles/measure_probe.json [--stats DIR/.../*_kernel_stats.csv]
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

REPEATS, WARM, TICKS = 15, 3, 3
HBM_BYTES_PER_S = 8.0e12


def pbd_beam():
    g = capi.Solver(scenes.pbd_options(capi, 20))
    scenes.build_beam(g, scenes.L100K)
    scenes.perturb(g, 1234, 0.05)
    return g


def pd_beam():
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10))
    W, H, D = scenes.L100K
    g.create_tet_box(W, H, D, translation=(0.0, 2.0, 0.0), w=1.0, volume=True, triangles=True)
    scenes.perturb(g, 1234, 0.05)
    return g


def ranges_of(n):
    rng = np.random.default_rng(11)
    first = rng.integers(0, n // 2, 64)
    return np.stack([first, rng.integers(1, n // 2, 64)], axis=1).astype(np.uint32)


def timed(call):
    ts = []
    for k in range(WARM + REPEATS):
        t0 = time.perf_counter()
        call()
        if k >= WARM:
            ts.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1), "spread_us": round(float(np.max(ts) - np.min(ts)), 1)}


def kernel_stats(path):
    """per-launch microseconds of the measure kernels from a rocprofv3 kernel stats CSV"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "k_measure" in name:
                short = name.split("k_measure")[1].split("(")[0].split("E")[0]
                out["k_measure" + short] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                            "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def calls_only():
    """for the profiler: both scenes as perturbed (no tick: the trace holds the measure kernels alone), a few calls of each kind"""
    for build in (pbd_beam, pd_beam):
        g = build()
        n = g.count(capi.NODES)
        for _ in range(5):
            g.measure_elements(capi.TET, records=False)
            g.measure_elements(capi.TET)
            g.measure_nodes(ranges_of(n))
        g.close()


def main():
    if sys.argv[1] == "--calls":
        return calls_only()
    out_path = sys.argv[1]
    r = {"timing": "host clock, median / min / max - min of %d calls after %d warm-up calls" % (REPEATS, WARM),
         "bytes_per_element": {"summary": 128, "records": 160}, "scenes": []}
    for name, build in (("config 2 beam, PBD", pbd_beam), ("tet box 20 x 20 x 250, PD", pd_beam)):
        g = build()
        g.tick(TICKS)
        n, tets = g.count(capi.NODES), g.count(capi.TET)
        ranges = ranges_of(n)
        row = {"scene": name, "nodes": n, "tets": tets}
        first = time.perf_counter()
        _, summary = g.measure_elements(capi.TET, records=False)
        row["first_call_us"] = round((time.perf_counter() - first) * 1e6, 1)  # stages the container
        row["summary_us"] = timed(lambda: g.measure_elements(capi.TET, records=False))
        row["records_us"] = timed(lambda: g.measure_elements(capi.TET))
        row["nodes64_us"] = timed(lambda: g.measure_nodes(ranges))
        row["nodes1_us"] = timed(lambda: g.measure_nodes(ranges[:1]))
        row["summary"] = {k: getattr(summary, k) for k, _ in capi.ElementSummary._fields_}
        row["failed"] = bool(g.failed)
        g.close()
        r["scenes"].append(row)
        print(json.dumps(row), flush=True)
    if "--stats" in sys.argv:
        r["kernels"] = kernel_stats(sys.argv[sys.argv.index("--stats") + 1])
        k = r["kernels"].get("k_measure_elements")
        if k:
            tets = r["scenes"][0]["tets"]
            # (--calls launches the kernel as often with records as without: 144 bytes per element on average)
            r["hbm_fraction"] = round(144.0 * tets / (k["average_us"] * 1e-6) / HBM_BYTES_PER_S, 3)
        print(json.dumps(r["kernels"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
