"""What it costs to get every tick's positions out of the library, form by form, at BASELINE config 2 (PBD, 20 x 20 x 250 = 100 000
particles, schedule LAYERED) and at the 300-node beam, and what the device-side node access (pies_read_nodes_device /
pies_write_nodes_device) costs per call.

  loops      ticks/s of a loop that delivers each tick's positions: `bare` (pies_tick_async, nothing delivered: the ceiling),
             `tick` (pies_tick: packed on the device, copied to the host mirror, host synchronised), `export` (pies_tick_begin /
             pies_export_acquire of the frame before: pinned host frames, two in flight), `device_read` (pies_tick_async +
             pies_read_nodes_device into the caller's device array on a stream of the caller's, no host synchronisation inside the
             window; `device_read_default`: the same on the default stream), `closed_loop`
             (tick -> read positions and velocities -> write the velocities back from the caller's array: a controller's shape
             without the controller).  Every form has a handle of its own on the same scene; the windows of WINDOW ticks alternate
             between the forms, so every form times the same ticks of the same collapse (the reads change nothing and the closed
             loop writes back what it read).  Host clock around a window that ends in a synchronisation; median, fastest and spread
             (max - min) over the windows after the warm-up.
  stores     microseconds per pies_read_nodes_device of the packed positions (stride 3) for each PIES_NODE_IO_VARIANT and for a
             destination that is 16-byte aligned or one float off, and for stride 4: CALLS calls queued back to back, then one
             synchronisation (host clock / CALLS: the sustained per-call cost, enqueue and event bracket included).
  writes     microseconds for replacing every velocity: pies_write_nodes + the upload it leaves to the next use (pies_finalize)
             against pies_write_nodes_device + pies_synchronize.

  kernels    `--calls` only issues CALLS packed reads and writes per variant at config 2, for a rocprofv3 --kernel-trace --stats run
             of its own: the kernels' names carry the variant (k_node_io_read<Gather, Staged>).

    python tools/probe_device_io.py [out.json]
    PIES_PROFILER_SAFE=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_device_io.py --calls
"""
import ctypes as C
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

WINDOW, WARM_WINDOWS, WINDOWS = 25, 1, 5
CALLS, REPEATS = 200, 7
FORMS = ("bare", "tick", "export", "device_read", "device_read_default", "closed_loop")


class Memory:
    """hipMalloc through the runtime the library is linked to"""

    def __init__(self):
        self.L = capi.load()
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipFree.argtypes = [C.c_void_p]
        self.L.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        self.held = []
        stream = C.c_void_p()
        assert self.L.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # hipStreamNonBlocking: the caller's own stream
        self.stream = stream.value

    def floats(self, count, offset=0):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), 4 * (count + 4)) == 0
        self.held.append(p.value)
        return p.value + 4 * offset

    def free(self):
        for p in self.held:
            self.L.hipFree(p)
        self.held = []


def scene(dims):
    g = bench.build_scene(capi, dims, 1234, schedule=capi.SCHEDULE_LAYERED, device=0)
    g.finalize()
    return g


def stats(values):
    v = sorted(values)
    return {"median": v[len(v) // 2], "best": v[-1], "spread": v[-1] - v[0]}


def window(form, g, mem, state):
    """WINDOW ticks of `form` on handle g, ending synchronised; returns seconds"""
    n = g.count(capi.NODES)
    t0 = time.perf_counter()
    if form == "bare":
        g.tick_async(WINDOW)
        g.synchronize()
    elif form == "tick":
        for _ in range(WINDOW):
            g.tick()
    elif form == "export":
        prev = None
        for _ in range(WINDOW):
            f = g.tick_begin()
            if prev is not None:
                g.export_acquire(prev)
                g.export_release(prev)
            prev = f
        g.export_acquire(prev)
        g.export_release(prev)
    elif form in ("device_read", "device_read_default"):
        stream = mem.stream if form == "device_read" else 0
        for _ in range(WINDOW):
            g.tick_async()
            g.read_nodes_device(position=state["pos"], n=n, stream=stream)
        g.synchronize()
    else:
        for _ in range(WINDOW):
            g.tick_async()
            g.read_nodes_device(position=state["pos"], velocity=state["vel"], n=n, stream=mem.stream)
            g.write_nodes_device(velocity=state["vel"], m=n, stream=mem.stream)
        g.synchronize()
    return time.perf_counter() - t0


def loops(dims, mem):
    handles = {form: scene(dims) for form in FORMS}
    n = handles["bare"].count(capi.NODES)
    state = {"pos": mem.floats(3 * n), "vel": mem.floats(3 * n)}
    rates = {form: [] for form in FORMS}
    for w in range(WARM_WINDOWS + WINDOWS):
        for form in FORMS:
            dt = window(form, handles[form], mem, state)
            if w >= WARM_WINDOWS:
                rates[form].append(WINDOW / dt)
    # every form has run the same ticks: the forms that only read end in the same positions
    ref = handles["bare"].positions
    same = {form: bool(np.array_equal(handles[form].positions, ref)) for form in FORMS}
    for g in handles.values():
        g.close()
    return {"nodes": n, "ticks_per_s": {form: stats(rates[form]) for form in FORMS}, "same_positions": same}


def per_call(call, sync):
    out = []
    for r in range(REPEATS + 1):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        sync()
        if r:
            out.append(1e6 * (time.perf_counter() - t0) / CALLS)
    v = sorted(out)
    return {"median_us": v[len(v) // 2], "best_us": v[0], "spread_us": v[-1] - v[0]}


def stores(dims, mem):
    g = scene(dims)
    g.tick_async(3)
    g.synchronize()
    n = g.count(capi.NODES)
    out = {"nodes": n}
    cases = [("stride3_%s_%s" % (variant, "aligned" if off == 0 else "offset"), variant, 3, off)
             for off in (0, 1) for variant in ("plain", "staged")] + [("stride4_aligned", None, 4, 0), ("stride4_offset", None, 4, 1)]
    results = {name: [] for name, *_ in cases}
    bufs = {off: mem.floats(4 * n, off) for off in (0, 1)}
    for _ in range(3):  # the cases alternate
        for name, variant, stride, off in cases:
            capi.set_tuning("PIES_NODE_IO_VARIANT", variant)
            results[name].append(per_call(lambda: g.read_nodes_device(position=bufs[off], stride=stride, n=n), g.synchronize))
    capi.set_tuning("PIES_NODE_IO_VARIANT", None)
    for name in results:
        r = results[name]
        out[name] = {"median_us": sorted(x["median_us"] for x in r)[1], "best_us": min(x["best_us"] for x in r),
                     "spread_us": max(x["median_us"] for x in r) - min(x["median_us"] for x in r)}
    g.close()
    return out


def writes(dims, mem):
    g = scene(dims)
    g.tick_async(3)
    g.synchronize()
    n = g.count(capi.NODES)
    v = g.velocities
    buf = mem.floats(3 * n)
    g.read_nodes_device(velocity=buf, n=n, flags=capi.IO_HOST_SYNC)
    host, dev = [], []
    for r in range(REPEATS + 2):
        t0 = time.perf_counter()
        g.set_velocities(v)
        g.finalize()  # the upload the write leaves to the next tick
        t1 = time.perf_counter()
        g.write_nodes_device(velocity=buf, m=n)
        g.synchronize()
        t2 = time.perf_counter()
        if r >= 2:
            host.append(1e6 * (t1 - t0))
            dev.append(1e6 * (t2 - t1))
    g.close()
    med = lambda a: sorted(a)[len(a) // 2]  # noqa: E731
    return {"nodes": n, "host_write_us": {"median": med(host), "best": min(host), "spread": max(host) - min(host)},
            "device_write_us": {"median": med(dev), "best": min(dev), "spread": max(dev) - min(dev)}}


def calls(mem):
    g = scene(scenes.L100K)
    g.tick_async(3)
    g.synchronize()
    n = g.count(capi.NODES)
    buf = mem.floats(3 * n)
    for variant in ("plain", "staged"):
        capi.set_tuning("PIES_NODE_IO_VARIANT", variant)
        for _ in range(CALLS):
            g.read_nodes_device(position=buf, n=n, stream=mem.stream)
        for _ in range(CALLS):
            g.write_nodes_device(position=buf, m=n, stream=mem.stream)
        g.synchronize()
    capi.set_tuning("PIES_NODE_IO_VARIANT", None)
    g.close()


def main():
    mem = Memory()
    if "--calls" in sys.argv:
        calls(mem)
        return
    out = {}
    for name, dims in (("beam_300", (5, 5, 12)), ("config2_100k", scenes.L100K)):
        out[name] = {"loops": loops(dims, mem), "stores": stores(dims, mem), "writes": writes(dims, mem)}
        mem.free()
        print(name, json.dumps(out[name]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
