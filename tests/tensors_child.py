"""Child process of tests/test_tensors_gpu.py: pies_amd.tensors needs torch imported before libpies_hip.so is loaded, which a
pytest process that has already loaded the library cannot offer.  Runs every check once and prints one JSON line."""
import json
import os
import sys

import torch  # first: the HIP runtime torch ships becomes the process's only one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import scenes  # noqa: E402
from pies_amd import capi, tensors  # noqa: E402

U = np.uint32


def same(t, a):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return bool(np.array_equal(np.ascontiguousarray(t, np.float32).reshape(-1).view(U),
                               np.ascontiguousarray(a, np.float32).reshape(-1).view(U)))


def beam(kind):
    if kind == "pd":
        g = capi.Solver(capi.Options(solver=capi.PD, iterations=10))
        g.create_tet_box(5, 5, 12, translation=(0.0, 0.02, 0.0), w=1.0, volume=True, triangles=True)
        g.add_position(np.array([12 * (j + 5 * i) for i in range(5) for j in range(5)], dtype=U), 2.0)
        scenes.perturb(g, 9, 0.03)
        g.set_prev_positions(g.positions)
        return g
    g = capi.Solver(scenes.pbd_options(capi, 4))
    scenes.build_beam(g, (5, 5, 12))
    scenes.perturb(g, 1, 0.05)
    g.set_flag(1, 0)
    g.set_schedule(capi.SCHEDULE_LAYERED)
    return g


def getters(out):
    g = beam("pbd")
    g.tick(2)
    io = tensors.Tensors(g)
    dev = torch.device("cuda", 0)
    out["getters"] = {
        "positions": same(io.positions(), g.positions), "prev_positions": same(io.prev_positions(), g.prev_positions),
        "velocities": same(io.velocities(), g.velocities), "radii": same(io.radii(), g.radii),
        "inv_masses": same(io.inv_masses(), g.inv_masses),
    }
    x4 = io.positions(stride=4)
    out["stride4"] = tuple(x4.shape) == (300, 4) and same(x4[:, :3].contiguous(), g.positions) and not bool(x4[:, 3].any())
    x, v = io.state()
    out["state"] = same(x, g.positions) and same(v, g.velocities) and bool(torch.equal(x, io.positions())) and bool(torch.equal(v, io.velocities()))
    buf = torch.full((300, 3), -1.0, device=dev)
    got = io.velocities(out=buf)
    out["out_reuse"] = got is buf and same(buf, g.velocities)
    g.tick_async()
    again = io.velocities(out=buf)
    out["out_reuse"] = out["out_reuse"] and again is buf and same(buf, g.velocities)
    refused = []
    for bad in (torch.zeros((300, 3), device=dev, requires_grad=True), torch.zeros((300, 3)), torch.zeros((299, 3), device=dev),
                torch.zeros((300, 3), device=dev, dtype=torch.float64)):
        try:
            io.positions(out=bad)
            refused.append(False)
        except capi.PiesError:
            refused.append(True)
    out["out_refused"] = refused
    # setters: whole arrays, rows by int32 and by int64 ids (converted on the device)
    new = torch.rand((300, 3), device=dev)
    io.set_positions(new)
    ok = same(g.positions, new.cpu().numpy()) and same(io.inv_masses(), g.inv_masses)
    ids64 = torch.tensor([0, 299, 7, 150], device=dev)
    rows = torch.rand((4, 4), device=dev)
    want = g.velocities
    want[ids64.cpu().numpy()] = rows[:, :3].cpu().numpy()
    io.set_velocities(rows, ids64)
    ok = ok and same(g.velocities, want)
    rows3 = torch.rand((4, 3), device=dev)
    want = g.prev_positions
    want[ids64.cpu().numpy()] = rows3.cpu().numpy()
    io.set_prev_positions(rows3, ids64.to(torch.int32))
    out["setters"] = ok and same(g.prev_positions, want)
    g.close()


def skins(out):
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=10))
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5), w=1.0, volume=True, triangles=True)
    tets = g.ids(capi.TET).reshape(-1, 4)
    p = g.positions
    verts = np.concatenate([p[tets[k]].mean(0, keepdims=True) for k in range(0, 48, 3)]).astype(np.float32)
    tri = np.array([[0, 1, 2], [2, 3, 4], [5, 6, 7]], U)
    g.add_skin(verts, tets, tri)
    scenes.perturb(g, 6, 0.04)
    g.set_prev_positions(g.positions)
    g.tick(2)
    io = tensors.Tensors(g)
    x, nr = io.skin(0)
    hx, hn = g.read_skin(0)
    out["skin"] = same(x, hx) and same(nr, hn) and same(io.skin(0, normals=False), hx)
    g.close()


def closed_loop(kind, through_tensors):
    """20 ticks of tick_async -> positions -> v = (x[ids] - target) * (-k) -> set_velocities(v, ids), no host synchronisation
    inside the loop when it runs through tensors; through the host getters and setters otherwise, with the same two torch
    operations on the device in both"""
    if kind == "pd":
        capi.set_tuning("PIES_PCG_BUDGET", "24")  # the host loop synchronises every tick: the captured CG budget must not follow that
    g = beam(kind)
    dev = torch.device("cuda", 0)
    ids_np = np.arange(3, 300, 12, dtype=np.int64)
    ids = torch.tensor(ids_np, device=dev)
    target = torch.tensor(g.positions[ids_np] + np.float32([0.0, 0.5, 0.0]), device=dev)
    k = 4.0
    io = tensors.Tensors(g)
    for _ in range(20):
        g.tick_async()
        if through_tensors:
            x = io.positions()
            v = (x[ids] - target) * (-k)
            io.set_velocities(v, ids)
        else:
            x = torch.tensor(g.positions, device=dev)
            v = (x[ids] - target) * (-k)
            vel = g.velocities
            vel[ids_np] = v.cpu().numpy()
            g.set_velocities(vel)
    state = [g.positions, g.prev_positions, g.velocities]
    failed = g.failed
    g.close()
    capi.set_tuning("PIES_PCG_BUDGET", None)
    return state, failed


def main():
    out = {"torch": torch.__version__, "runtimes": tensors.hip_runtimes()}
    getters(out)
    skins(out)
    for kind in ("pbd", "pd"):
        a, fa = closed_loop(kind, True)
        b, fb = closed_loop(kind, False)
        out["loop_" + kind] = {"equal": [same(x, y) for x, y in zip(a, b)], "failed": bool(fa or fb),
                               "finite": bool(all(np.isfinite(x).all() for x in a)),
                               "moved": float(np.abs(a[2]).max())}
    out["runtimes_after"] = tensors.hip_runtimes()
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
