"""pies_drive_actuators at the sizes the project is built for: createBox's 25 x 25 x 250 lattice (156 250 nodes, 1 029 321 distance
constraints) under PBD in schedule LAYERED without node-node collisions; sets of 1 000, 100 000 and 1 000 000 actuators (the first
constraints of the container, eight channels, scale and offset mode alternating), driven through the host-pointer form and through
the device form.  Beside each: the same edit through pies_set_rest and the tick that pays for its rebuild, on the same scene in
the same run - the path a host had before.

  host_us            host clock around pies_drive_actuators (the call ends in a stream synchronisation; the copy of the activations
                     in and of the outputs out are part of it), median of the repeats; min_us the fastest
  device_issue_us    host clock around pies_drive_actuators_device without PIES_IO_HOST_SYNC: what the caller's thread pays
  device_us          the device form's launches between two events on the caller's stream, per call over 20 queued calls (the two
                     event waits between the streams are inside)
  first_call_us      the first drive of a set: it builds the slot map and stages the device copy
  set_rest_tick_us   pies_set_rest over the same constraints with the same values + pies_tick (full rebuild + one tick), median
  tick_us            pies_tick alone on the built scene, median: what of the line above is not the rebuild

    python tools/probe_actuators.py profiles/actuators_probe.json
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
import scenes  # noqa: E402
from device_buffers import DevBuf, Hip  # noqa: E402
from pies_amd import capi  # noqa: E402

DIMS = (25, 25, 250)
SIZES = (1000, 100000, 1000000)
CHANNELS = 8
REPEATS, WARM = 15, 3
REBUILDS = 3
F = np.float32


def timed(call, repeats=REPEATS, warm=WARM):
    ts = []
    for k in range(warm + repeats):
        t0 = time.perf_counter()
        call()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e6)
    return {"us_per_call": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1)}


def actuator_set(count):
    """the first `count` distance constraints, as a ctypes array filled through numpy"""
    arr = (capi.Actuator * count)()
    a = np.frombuffer(arr, np.dtype([("type", "<i4"), ("index", "<u4"), ("channel", "<u4"), ("gain", "<f4"), ("lo", "<f4"), ("hi", "<f4"),
                                     ("base", "<f4"), ("flags", "<u4")]))
    i = np.arange(count, dtype=np.uint32)
    a["type"], a["index"], a["channel"], a["gain"], a["lo"], a["hi"], a["flags"] = capi.DISTANCE, i, i % CHANNELS, 0.05, 0.25, 4.0, i & 1
    return arr


def device_time(hip, g, k, act, outs, calls=20):
    L = hip.L
    for name, args in {"hipEventCreate": [C.POINTER(C.c_void_p)], "hipEventRecord": [C.c_void_p, C.c_void_p], "hipEventSynchronize": [C.c_void_p],
                       "hipEventElapsedTime": [C.POINTER(C.c_float), C.c_void_p, C.c_void_p], "hipEventDestroy": [C.c_void_p]}.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int
    e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_float()
    hip.ok(L.hipEventCreate(C.byref(e0)))
    hip.ok(L.hipEventCreate(C.byref(e1)))
    hip.ok(L.hipEventRecord(e0, None))
    for _ in range(calls):
        g.drive_actuators_device(k, CHANNELS, act.ptr, *outs)
    hip.ok(L.hipEventRecord(e1, None))
    hip.ok(L.hipEventSynchronize(e1))
    hip.ok(L.hipEventElapsedTime(C.byref(ms), e0, e1))
    hip.ok(L.hipEventDestroy(e0))
    hip.ok(L.hipEventDestroy(e1))
    return round(ms.value * 1e3 / calls, 2)


def main():
    out_path = sys.argv[1]
    hip = Hip()
    g = capi.Solver(scenes.pbd_options(capi, 4))
    g.set_flag(capi.FLAG_NODE_COLLISIONS, 0)
    g.set_schedule(capi.SCHEDULE_LAYERED)
    g.create_box(*DIMS, translation=(0.0, 2.0, 0.0), w=0.5, triangles=False)
    t0 = time.perf_counter()
    g.finalize()
    r = {"timing": "host clock, median (min) of %d calls after %d warm-up calls; rebuilds: median of %d" % (REPEATS, WARM, REBUILDS),
         "nodes": g.count(capi.NODES), "distance_constraints": g.count(capi.DISTANCE), "channels": CHANNELS, "schedule": "LAYERED",
         "first_finalize_us": round((time.perf_counter() - t0) * 1e6, 1), "sets": []}
    g.tick()
    r["tick_us"] = timed(g.tick, repeats=5, warm=1)
    print(json.dumps({k: v for k, v in r.items() if k != "sets"}), flush=True)
    rest0 = g.rest(capi.DISTANCE)
    activation = np.linspace(-1.0, 1.0, CHANNELS).astype(F)
    act = DevBuf(hip, CHANNELS, fill=activation)
    sums, live = DevBuf(hip, 2 * CHANNELS), DevBuf(hip, CHANNELS)
    for count in SIZES:
        k = g.add_actuators(actuator_set(count), CHANNELS)
        per = DevBuf(hip, 2 * count)
        t0 = time.perf_counter()
        counts = g.drive_actuators(k, activation)[1]
        row = {"actuators": count, "live": int(counts.sum()), "first_call_us": round((time.perf_counter() - t0) * 1e6, 1)}
        row["host_us"] = {"no_outputs": timed(lambda: g.drive_actuators(k, activation, sums=False)),
                          "sums": timed(lambda: g.drive_actuators(k, activation)),
                          "sums_and_per_actuator": timed(lambda: g.drive_actuators(k, activation, per_actuator=True))}
        row["device_issue_us"] = {"no_outputs": timed(lambda: g.drive_actuators_device(k, CHANNELS, act.ptr)),
                                  "sums": timed(lambda: g.drive_actuators_device(k, CHANNELS, act.ptr, sums.ptr, live.ptr))}
        g.synchronize()
        row["device_us"] = {"no_outputs": device_time(hip, g, k, act, ()), "sums": device_time(hip, g, k, act, (sums.ptr, live.ptr)),
                            "sums_and_per_actuator": device_time(hip, g, k, act, (sums.ptr, live.ptr, per.ptr))}
        # the same edit the old way: the values the drive left, written through pies_set_rest, and the tick that rebuilds
        driven = g.rest(capi.DISTANCE)[:count].copy()

        def rebuild():
            g.set_rest(capi.DISTANCE, driven, first=0)
            g.tick()
        row["set_rest_tick_us"] = timed(rebuild, repeats=REBUILDS, warm=1)
        r["sets"].append(row)
        print(json.dumps(row), flush=True)
        per.free()
        g.set_rest(capi.DISTANCE, rest0)
        g.tick()  # (the rebuild is paid here, not by the next set's first drive)
    assert np.isfinite(g.positions).all()
    for b in (act, sums, live):
        b.free()
    g.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
