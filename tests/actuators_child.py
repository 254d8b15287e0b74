"""Child process of tests/test_actuators_gpu.py: pies_amd.tensors needs torch imported before libpies_hip.so is loaded, which a
pytest process that has already loaded the library cannot offer (tests/tensors_child.py).  Tensors.drive_actuators against the
host-pointer form, bit for bit; runs every check once and prints one JSON line."""
import json
import os
import sys

import torch  # first: the HIP runtime torch ships becomes the process's only one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "benchlib"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from pies_amd import capi, tensors  # noqa: E402
from test_actuators import containers, lattice_and_sheet, random_set  # noqa: E402

F, U = np.float32, np.uint32
DEV = torch.device("cuda", 0)


def same(t, a):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return bool(np.array_equal(np.ascontiguousarray(t).reshape(-1).view(U), np.ascontiguousarray(a).reshape(-1).view(U)))


def body():
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4))
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
    lattice_and_sheet(g)
    g.finalize()
    ids, rest = containers(g)
    k = g.add_actuators(random_set(np.random.default_rng(5), {t: len(r) for t, r in rest.items()}, 200, 3), 3)
    return g, k


def outputs(out):
    A, ka = body()
    B, kb = body()
    activation = np.array([1.4, -0.7, 0.2], F)
    want = A.drive_actuators(ka, activation, per_actuator=True)
    io = tensors.Tensors(B)
    sums, live, per = torch.full((3, 2), -1.0, device=DEV), torch.full((3,), 9, device=DEV, dtype=torch.int32), torch.full((200, 2), -1.0, device=DEV)
    io.drive_actuators(kb, torch.tensor(activation, device=DEV), sums=sums, live=live, per_actuator=per)
    out["outputs"] = {"sums": same(sums, want[0]), "live": same(live, want[1]), "per_actuator": same(per, want[2]),
                      "rest": all(same(A.rest(t), B.rest(t)) for t in (capi.DISTANCE, capi.BEND))}
    # a NaN in the tensor: its channel's actuators are not live and their constraints keep their rests
    before = {t: B.rest(t) for t in (capi.DISTANCE, capi.BEND)}
    io.drive_actuators(kb, torch.tensor([float("nan")] * 3, device=DEV), live=live)
    out["nan"] = {"live": same(live, np.zeros(3, np.int32)), "rest": all(same(B.rest(t), before[t]) for t in before)}
    refused = []
    for bad in (dict(sums=torch.zeros((3, 2))), dict(sums=torch.zeros((2, 2), device=DEV)), dict(live=torch.zeros(3, device=DEV))):
        try:
            io.drive_actuators(kb, torch.tensor(activation, device=DEV), **bad)
            refused.append(False)
        except capi.PiesError:
            refused.append(True)
    out["refused"] = refused
    A.close()
    B.close()


def sheet():
    """a bend sheet under PD, two rows pinned, every bend constraint an actuator of one channel"""
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6))
    g.create_bend_sheet(6, 5, translation=(0.0, 3.0, 0.0), w=2.0)
    g.add_position(np.arange(0, 10, dtype=U), 5.0)
    g.set_prev_positions(g.positions)
    g.finalize()
    A = capi.Actuator.make
    k = g.add_actuators([A(capi.BEND, i, 0, -0.2, 1.5, 3.2) for i in range(g.count(capi.BEND))], 1)
    return g, k


def closed_loop(through_tensors):
    """12 ticks of tick_async -> positions -> u = a policy of the state, on the device -> drive; no host synchronisation inside the
    loop when it runs through tensors, through the host getters and the host-pointer form otherwise - the same torch operations"""
    capi.set_tuning("PIES_PCG_BUDGET", "24")  # the host loop synchronises every tick: the captured CG budget must not follow that
    g, k = sheet()
    io = tensors.Tensors(g)
    for t in range(12):
        g.tick_async()
        x = io.positions() if through_tensors else torch.tensor(g.positions, device=DEV)
        u = torch.sigmoid(x[:, 1].max() - 2.0).reshape(1) * (t / 12.0)
        if through_tensors:
            io.drive_actuators(k, u)
        else:
            g.drive_actuators(k, u.cpu().numpy(), sums=False)
    state = [g.positions, g.prev_positions, g.velocities]
    failed = g.failed
    rest = g.rest(capi.BEND)
    g.close()
    capi.set_tuning("PIES_PCG_BUDGET", None)
    return state, failed, rest


def main():
    out = {"torch": torch.__version__, "runtimes": tensors.hip_runtimes()}
    outputs(out)
    a, fa, ra = closed_loop(True)
    b, fb, rb = closed_loop(False)
    out["loop"] = {"equal": [same(x, y) for x, y in zip(a, b)] if same(ra, rb) else [False] * 3, "failed": bool(fa or fb),
                   "finite": bool(all(np.isfinite(x).all() for x in a)), "folded": float(np.pi - ra.min())}
    torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
