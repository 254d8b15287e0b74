"""pies_add_tri_mesh_volume at the sizes a host would use: an icosphere of 20 480 triangles at resolutions 16, 32 and 64.
Recorded, not gated:

  kernel_ms              k_winding alone, between two HIP events recorded around its launch on the solver's stream.  The events
                         exist in the diagnostic build only (python -m pies_amd.build --exp; select it with PIES_LIB); with
                         the product library the field is null
  voxelize_ms            the whole pies_voxelize_tri_mesh call on the body's lattice (uploads, kernel, copies out)
  add_ms                 the whole pies_add_tri_mesh_volume call (classification, lattice body, boundary rule, skin binding)
  solid_angles_per_s     samples x triangles / kernel time

    PIES_LIB=pies_amd/lib/libpies_hip_exp.so python tools/probe_trimesh.py profiles/trimesh_probe.json
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from pies_amd import capi  # noqa: E402
from test_trimesh import icosphere, lattice_of  # noqa: E402


def kernel_ms(L, g):
    """the handle's last k_winding launch (diagnostic library only)"""
    if not hasattr(L, "pies_exp_winding_ms"):
        return None
    L.pies_exp_winding_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    ms = C.c_float()
    return float(ms.value) if L.pies_exp_winding_ms(g._h, C.byref(ms)) == 0 and ms.value >= 0 else None


def main():
    out_path = sys.argv[1]
    v, tri = icosphere(5, 1.0, (0.0, 2.0, 0.0))
    r = {"mesh": "icosphere, %d triangles, %d vertices" % (len(tri), len(v)), "library": os.path.basename(capi.LIB_PATH), "runs": []}
    L = capi.load()
    for resolution in (16, 32, 64):
        g = capi.Solver(capi.Options(solver=capi.PD, iterations=10))
        origin, cell, dims = lattice_of(v, resolution)
        g.voxelize_tri_mesh(v, tri, origin, cell, dims)  # warm: code object load, first allocations
        best_kernel, best_call = None, None
        for _ in range(5):
            t0 = time.perf_counter()
            g.voxelize_tri_mesh(v, tri, origin, cell, dims)
            call = (time.perf_counter() - t0) * 1e3
            k = kernel_ms(L, g)
            best_call = call if best_call is None else min(best_call, call)
            best_kernel = k if best_kernel is None or (k is not None and k < best_kernel) else best_kernel
        t0 = time.perf_counter()
        _, nodes, tets, _ = g.add_tri_mesh_volume(v, tri, resolution)
        add = (time.perf_counter() - t0) * 1e3
        pairs = int(np.prod(dims, dtype=np.int64)) * len(tri)
        run = {"resolution": resolution, "dims": list(dims), "samples": int(np.prod(dims)), "solid_angles": pairs,
               "kernel_ms": None if best_kernel is None else round(best_kernel, 4), "voxelize_ms": round(best_call, 3),
               "add_ms": round(add, 2), "nodes": nodes, "elements": tets,
               "solid_angles_per_s": None if not best_kernel else round(pairs / (best_kernel * 1e-3), 0)}
        print(json.dumps(run), flush=True)
        r["runs"].append(run)
        g.close()
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
