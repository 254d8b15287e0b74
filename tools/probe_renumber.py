"""PIES_FLAG_RENUMBER_NODES on the 100k-node Delaunay beam (BASELINE config 3's size, strain + volume per element, surface
triangles, end cap pinned) in three node orders - lattice (z fastest), 5 x 5 x 10 bricks, random - each with the flag off and on.
Per run: PD substeps/s, in-situ us of pd_spmv (the CG iteration), pd_rhs and pd_local_tet, halo columns per row of the windowed
matrix, NODES_RENUMBERED and finalize time.  The export's gather (k_gather_nodes, once per exported frame) is timed by rocprofv3:

    python tools/probe_renumber.py [out.json]
    PIES_PROFILER_SAFE=1 rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/probe_renumber.py --export
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


def reorder(mesh, order):
    """order[new] = old node"""
    pos, tets, edges = mesh
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    return pos[order], inv[tets].astype(np.uint32), np.sort(inv[edges], axis=1).astype(np.uint32)


def export_frames(frames=50):
    """--export: exported frames of the random-order beam with the flag on, for a rocprofv3 --kernel-trace --stats run
    (k_gather_nodes is the export's gather; PIES_PROFILER_SAFE=1)"""
    mesh = scenes.delaunay_beam(scenes.L100K)
    mesh = reorder(mesh, np.random.default_rng(1).permutation(len(mesh[0])))
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=0)
    scenes.build_unstructured_pd(g, mesh)
    g.set_flag(capi.FLAG_RENUMBER_NODES, 1)
    g.finalize()
    assert g.count(capi.NODES_RENUMBERED) == 1
    for _ in range(frames):
        f = g.tick_begin()
        g.export_acquire(f)
        g.export_release(f)
    g.close()


def run(mesh, tag, renumber):
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=0)
    scenes.build_unstructured_pd(g, mesh)
    g.set_flag(capi.FLAG_RENUMBER_NODES, 1 if renumber else 0)
    t0 = time.perf_counter()
    g.finalize()
    fin = time.perf_counter() - t0
    for _ in range(20):
        g.tick_async(1)
        g.synchronize()
    el = bench.timed_ticks(g, 20, 2, lambda: None)
    n = g.count(capi.NODES)
    r = {"order": tag, "flag": int(renumber), "renumbered": g.count(capi.NODES_RENUMBERED), "substeps_per_s": round(20 / el, 1),
         "halo_per_row": round(g.count(capi.PD_WINDOW_HALO) / n, 3), "finalize_s": round(fin, 3)}
    for name in ("pd_spmv", "pd_rhs", "pd_local_tet"):
        cnt, ms, units, ov = g.profile_in_situ(bench.K[name], 2)
        r[name + "_us"] = round(1e3 * ms / cnt - 1e3 * ov, 2) if cnt else None
    g.close()
    print("%-8s flag %d: renumbered %d  %7.1f substeps/s  spmv %6.2f us  rhs %6.2f us  local_tet %6.2f us  halo/row %6.3f  "
          "finalize %.2f s" % (tag, r["flag"], r["renumbered"], r["substeps_per_s"], r["pd_spmv_us"] or 0, r["pd_rhs_us"] or 0,
                               r["pd_local_tet_us"] or 0, r["halo_per_row"], r["finalize_s"]), flush=True)
    return r


def main():
    if sys.argv[1:2] == ["--export"]:
        return export_frames()
    mesh = scenes.delaunay_beam(scenes.L100K)
    W, H, D = scenes.L100K
    ijk = np.stack(np.meshgrid(np.arange(W), np.arange(H), np.arange(D), indexing="ij"), -1).reshape(-1, 3)
    bx, by, bz = 5, 5, 10
    key = ((ijk[:, 2] // bz) * 1000 + (ijk[:, 0] // bx) * 30 + (ijk[:, 1] // by)) * 100000 + \
        ((ijk[:, 0] % bx) * by + (ijk[:, 1] % by)) * bz + (ijk[:, 2] % bz)
    meshes = [("lattice", mesh), ("bricks", reorder(mesh, np.argsort(key, kind="stable"))),
              ("random", reorder(mesh, np.random.default_rng(1).permutation(len(mesh[0]))))]
    rows = [run(m, tag, flag) for tag, m in meshes for flag in (False, True)]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump({"mesh": "delaunay_beam%s, %d nodes" % (str(scenes.L100K), len(mesh[0])), "runs": rows}, f, indent=1)


if __name__ == "__main__":
    main()
