"""Embedded surface meshes (pies_add_skin) at the size the project is built for: BASELINE config 3's 100k-node PD beam
(20 x 20 x 250 lattice, 539 334 elements) with the beam's own boundary subdivided to ~1M skin vertices.  Recorded, not gated:

  bind_s                 host time of pies_add_skin for that skin, and for 1M vertices against 500k elements
                         (the 50 x 100 x 100 lattice's elements, truncated to 500 000)
  substeps_per_s         pies_tick_begin + acquire + release per frame, with and without the skin
  k_skin_*_us            per launch, from a rocprofv3 --kernel-trace --stats run of `--frames` (its kernel stats CSV is given
                         with --stats), and the HBM fraction the byte counts of skin_kernels.hip give at that time

    python tools/probe_skin.py out.json [--stats DIR_OR_CSV]
    PIES_PROFILER_SAFE=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_skin.py --frames
"""
import csv
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

PER_UNIT = 7  # skin squares per lattice spacing and axis: 2 * 134^2 + 4 * 134 * 1744 = 970 696 vertices, 1 925 308 triangles


def box_faces(lo, hi, n):
    """The six faces of the box [lo, hi] as separate grids of n[u] x n[v] squares, two triangles each, wound outward (vertices on
    the box's edges belong to one face each, as in a render mesh with hard edges): (vertices x 3 float32, triangles x 3 uint32)"""
    verts, tris, base = [], [], 0
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        a, b = np.meshgrid(np.arange(n[u] + 1), np.arange(n[v] + 1), indexing="ij")
        i, j = np.meshgrid(np.arange(n[u]), np.arange(n[v]), indexing="ij")
        q = [(i + di) * (n[v] + 1) + (j + dj) for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1))]
        for side in (0, 1):
            p = np.zeros((a.size, 3))
            p[:, axis] = lo[axis] if side == 0 else hi[axis]
            p[:, u] = lo[u] + a.ravel() / n[u] * (hi[u] - lo[u])
            p[:, v] = lo[v] + b.ravel() / n[v] * (hi[v] - lo[v])
            c = q if side else q[::-1]
            t = np.concatenate([np.stack([c[0], c[1], c[2]], -1).reshape(-1, 3), np.stack([c[0], c[2], c[3]], -1).reshape(-1, 3)])
            verts.append(p)
            tris.append(t + base)
            base += len(p)
    return np.concatenate(verts).astype(np.float32), np.concatenate(tris).astype(np.uint32)


def beam(device=0):
    return bench.pd_beam(scenes.L100K, device, settle=0)


def beam_skin(g):
    p = g.positions
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    v, tri = box_faces(lo, hi, [int(round(PER_UNIT * e)) for e in hi - lo])
    # exactly on the boundary: a vertex may round a last bit outside its element's box
    return v, tri, g.ids(capi.TET), 1e-4


def frames(n=100):
    """--frames: n exported frames with the skin bound, for a kernel trace"""
    g = beam()
    v, tri, tets, md = beam_skin(g)
    g.add_skin(v, tets, tri, max_distance=md)
    for _ in range(n):
        f = g.tick_begin()
        g.export_acquire_skin(f, 0)
        g.export_release(f)
    g.close()


def frame_rate(g, skin, n=60, warm=10):
    def loop(k):
        for _ in range(k):
            f = g.tick_begin()
            if skin:
                g.export_acquire_skin(f, 0)
            else:
                g.export_acquire(f)
            g.export_release(f)
    loop(warm)
    g.synchronize()
    t0 = time.perf_counter()
    loop(n)
    g.synchronize()
    return n / (time.perf_counter() - t0)


def kernel_stats(path):
    """average ns per launch of the two kernels from a rocprofv3 kernel stats CSV (or a directory that holds one)"""
    files = [path] if os.path.isfile(path) else [os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs if f.endswith("kernel_stats.csv")]
    out = {}
    for name in files:
        with open(name, newline="") as f:
            for row in csv.DictReader(f):
                for k in ("k_skin_positions", "k_skin_normals"):
                    if k in row["Name"]:
                        out[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3}
    return out


def main():
    if sys.argv[1:2] == ["--frames"]:
        return frames()
    out_path = sys.argv[1]
    stats = sys.argv[sys.argv.index("--stats") + 1] if "--stats" in sys.argv else None
    r = {"scene": "BASELINE configs[2]: 20x20x250 PD beam (100 000 nodes, 539 334 elements); skin = its boundary, %d x %d squares per lattice face" % (PER_UNIT, PER_UNIT)}

    # ---- bind times (host only) ----
    h = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=capi.DEVICE_NONE)
    W, H, D = scenes.L100K
    h.create_tet_box(W, H, D, translation=(0.0, 2.0, 0.0), w=1.0, volume=False, triangles=False)
    v, tri, tets, md = beam_skin(h)
    t0 = time.perf_counter()
    h.add_skin(v, tets, tri, max_distance=md)
    r["skin_vertices"], r["skin_triangles"], r["elements"] = len(v), len(tri), len(tets)
    r["bind_s"] = round(time.perf_counter() - t0, 3)
    h.close()
    h = capi.Solver(capi.Options(solver=capi.PD, iterations=10), device=capi.DEVICE_NONE)
    W, H, D = scenes.L500K
    h.create_tet_box(W, H, D, translation=(0.0, 2.0, 0.0), w=1.0, volume=False, triangles=False)
    big = h.ids(capi.TET)[:500000]
    p = h.positions
    rng = np.random.default_rng(7)
    cells = big[rng.integers(0, len(big), 1000000)]  # a random point inside a random one of the 500k elements
    bary = rng.dirichlet(np.ones(4), len(cells)).astype(np.float32)
    pts = np.einsum("vk,vkj->vj", bary, p[cells]).astype(np.float32)
    t0 = time.perf_counter()
    h.add_skin(pts, big, None, max_distance=1e-4)
    r["bind_1m_vertices_500k_elements_s"] = round(time.perf_counter() - t0, 3)
    h.close()
    print("bind: %d vertices / %d elements %.2f s; 1M / 500k %.2f s" % (r["skin_vertices"], r["elements"], r["bind_s"],
                                                                        r["bind_1m_vertices_500k_elements_s"]), flush=True)

    # ---- frames per second with and without the skin (the same handle: first without) ----
    g = bench.pd_beam(scenes.L100K, 0)
    r["frames_per_s_without_skin"] = round(frame_rate(g, False), 1)
    v, tri, tets, md = beam_skin(g)
    g.add_skin(v, tets, tri, max_distance=md)
    r["frames_per_s_with_skin"] = round(frame_rate(g, True), 1)
    t0 = time.perf_counter()
    for _ in range(20):
        g.read_skin(0)
    r["read_skin_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
    g.close()
    print("frames/s: %.1f without, %.1f with the skin; read_skin %.2f ms" % (r["frames_per_s_without_skin"], r["frames_per_s_with_skin"],
                                                                            r["read_skin_ms"]), flush=True)

    # ---- kernel times and HBM fractions ----
    nv, nt = r["skin_vertices"], r["skin_triangles"]
    r["bytes_positions"] = nv * (32 + 64 + 12)
    # 4 B per CSR entry + 36 B of positions per incident triangle + 12 B out (+ on top: 12 B of triangle indices per incident
    # triangle and 8 B of row pointers per vertex, which the kernel reads as well)
    r["bytes_normals"] = 3 * nt * (4 + 36) + 12 * nv
    r["bytes_normals_with_indices"] = r["bytes_normals"] + 3 * nt * 12 + 8 * nv
    if stats:
        ks = kernel_stats(stats)
        for k, key in (("k_skin_positions", "bytes_positions"), ("k_skin_normals", "bytes_normals")):
            if k in ks:
                r[k + "_us"] = round(ks[k]["avg_us"], 2)
                r[k + "_calls"] = ks[k]["calls"]
                r[k + "_hbm_frac"] = round(r[key] / (ks[k]["avg_us"] * 1e-6) / 1e9 / bench.HBM_PEAK_GBS, 4)
        r["timing_source"] = "rocprofv3 --kernel-trace --stats over `probe_skin.py --frames` (100 frames)"
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)
    print(json.dumps(r))


if __name__ == "__main__":
    main()
