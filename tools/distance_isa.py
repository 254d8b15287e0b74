#!/usr/bin/env python3
"""Static instruction counts of distance_core (pbd_project.h) in the gfx950 ISA hipcc emits for the product flags, stand-alone: one
lane loads two node records and a (rest, w) pair, projects, stores.  Two kernels: the body that divides three times with `/`
(distance_core<false>, what PIES_LAYER_DIST_FORM=0 selects in k_layer) and the body with the three quotients from one reciprocal
behind its per-lane range test (distance_core<true>).  For the second the path with every lane in range is counted as well: the
region with the fallback's division (v_div_scale), which a branch on the empty execution mask jumps over, left out.  Cross-compilation only: runs without a GPU.

Then the LDS instructions of a distance colour as k_layer's product build emits them, by width: the stretches between two workgroup
barriers of k_layer<512, 0, 1, true, 1, 1> that gather at most four and scatter at most two node records (tools/layer_isa.py
cuts the kernel; a colour has a path for its first 512 members and a loop for the rest).

usage: python tools/distance_isa.py [extra compiler flags for k_layer] > profiles/rNN_distance_isa.txt"""
import os
import re
import subprocess
import sys
import tempfile

import layer_isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = """#include "pbd_project.h"
template <bool SHARED> __global__ void k_probe(float4* p, const float4* q, const float2* rw) {
  const unsigned i = threadIdx.x;
  float4 a = p[i];
  pies::distance_core<SHARED>(a, q[i], rw[i]);
  p[i] = a;
}
template __global__ void k_probe<false>(float4*, const float4*, const float2*);
template __global__ void k_probe<true>(float4*, const float4*, const float2*);
"""
KINDS = ("v_div_scale", "v_div_fmas", "v_div_fixup", "v_rcp", "v_sqrt", "v_fma", "v_fmac", "v_mul", "v_cmp", "v_cndmask", "s_nop")


def in_range_path(lines):
    """the instructions a wavefront executes when every lane is in range: a region that a branch on an empty execution mask jumps over
    is left out when it holds the fallback's division"""
    ops, labels = [], {}
    for raw in lines:
        t = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = len(ops)
        elif t and not t.startswith((";", ".")):
            ops.append(t.split()[:2])
    path, i = [], 0
    while i < len(ops):
        op = ops[i]
        path.append(op[0])
        if op[0] == "s_cbranch_execz" and labels.get(op[1], 0) > i and any(o[0].startswith("v_div_") for o in ops[i + 1:labels[op[1]]]):
            i = labels[op[1]]
        else:
            i += 1
    return [o[0] for o in ops], path


def tally(ops):
    c = {"all": len(ops), "valu": sum(o.startswith("v_") for o in ops), "salu": sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop")) for o in ops)}
    for k in KINDS:
        c[k] = sum(o.startswith(k) for o in ops)
    return c


def show(title, c):
    print("%s: all %d, VALU %d, scalar %d; %s" % (title, c["all"], c["valu"], c["salu"], ", ".join("%s %d" % (k, c[k]) for k in KINDS if c[k])))


def main():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "probe.hip"), os.path.join(tmp, "probe.s")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.check_call([hipcc, "-S", src, "-o", out, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
                               "--cuda-device-only", "-I", os.path.join(ROOT, "pies_amd", "csrc"), "-I", os.path.join(ROOT, "include")], stderr=subprocess.DEVNULL)
        with open(out) as f:
            txt = f.read()
    res = {}
    for shared in (0, 1):
        m = re.search(r"^_Z7k_probeILb%dEE\S*:.*?s_endpgm" % shared, txt, re.S | re.M)
        every, path = in_range_path(m.group(0).splitlines()[1:])
        title = "distance_core<%s> + 3 loads, 1 store" % ("true" if shared else "false")
        show(title + ", whole kernel", tally(every))
        if shared:
            show(title + ", the path with every lane in range", tally(path))
            res[1] = tally(path)
        else:
            res[0] = tally(every)
    print("off the common path: %d instructions, of them VALU %d, s_nop %d; scalar %+d" %
          (res[0]["all"] - res[1]["all"], res[0]["valu"] - res[1]["valu"], res[0]["s_nop"] - res[1]["s_nop"], res[1]["salu"] - res[0]["salu"]))
    with tempfile.TemporaryDirectory() as tmp:
        txt = layer_isa.compile_isa(tmp, "layer.s", sys.argv[1:])
    lines = layer_isa.kernel_text(txt, "_ZN4pies7k_layerILi512ELi0ELi1ELb1ELi1ELi1EEE")[0]
    print("LDS instructions of a distance colour in k_layer<512, 0, 1, true, 1, 1> (product build, between two workgroup barriers):")
    for key, n in sorted(layer_isa.barrier_segments(lines).items(), key=lambda kv: -kv[1]):
        wide = dict(kv.rsplit(" ", 1) for kv in key.split(", "))
        reads = sum(int(v) for k, v in wide.items() if k in ("ds_read_b96", "ds_read_b128"))
        writes = sum(int(v) for k, v in wide.items() if k in ("ds_write_b96", "ds_write_b128"))
        if 0 < reads <= 4 and 0 < writes <= 2:
            print("  %3d x  %s" % (n, key))


if __name__ == "__main__":
    main()
