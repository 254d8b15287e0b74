#!/usr/bin/env python3
"""Static instruction counts of k_layer's MAIN tetrahedral colour loop in the gfx950 ISA hipcc emits for the product flags
(cross-compilation only: runs without a GPU), per basic block and summed along the path every element of BASELINE config 2 takes:
from the block after the barrier through the closed form, one rotation, the polish and one clean certifying snapshot to the
scatter and the barrier.

The main loop's gather and the rare paths (the start of an element with fewer than two pairs out of tolerance, the rotating sweeps, the completion
of a collapsed direction, the loop for classes larger than the workgroup) are told from the common one by a comment the
sources emit under -DPIES_PATH_NOTES (dev_math.h: PIES_MAIN_TET_PATH, PIES_RARE_PATH); the tool compiles once with and once without it and reports
both kernels' lengths, so that a difference made by the notes shows.  LDS instructions are reported by width: along the main loop's
product build only (the notes change which widths the compiler picks, so the path walk says nothing about them): over the whole
kernel and per stretch between two workgroup barriers - a colour step; the distance colours are the stretches with two gathers
and one scatter per path, the bend step the one with four 16-byte gathers and four 16-byte scatters.  --dump writes the instructions along the path of the
tet_rows.h kernel, block by block: where the moves of a source region stand.

usage: python tools/layer_isa.py [--block 512] [--streamed] [--json profiles/rNN_layer_critical_path.json] [--dump path.s] [extra compiler flags]
       > profiles/rNN_layer_isa.txt"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVES = ("v_mov_b32", "v_mov_b64", "v_pk_mov_b32", "v_accvgpr")
MEMORY = ("ds_", "global_", "buffer_", "flat_", "scratch_")


def take(argv, flag, default=None):
    if flag in argv:
        i = argv.index(flag)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


def compile_isa(tmp, name, flags):
    out = os.path.join(tmp, name)
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.check_call([hipcc, "-S", os.path.join(ROOT, "pies_amd/csrc/layer_kernels.hip"), "-o", out, "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fno-fast-math"] + flags + ["--offload-arch=gfx950", "--cuda-device-only", "-I", os.path.join(ROOT, "include")],
                          stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def kernel_text(txt, sym):
    m = re.search(r"^%s\S*:.*?s_endpgm" % sym, txt, re.S | re.M)
    meta = re.search(r"%s.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)" % sym, txt, re.S)
    return m.group(0).splitlines(), meta.groups()


def basic_blocks(lines):
    """true basic blocks: split at labels and after every branch.  name = the label, or label+k for the k-th piece after it"""
    blocks, cur, label, piece = [], None, "entry", 0

    def start(name):
        b = {"name": name, "ops": [], "text": [], "rare": False, "main": False, "branch": None}
        blocks.append(b)
        return b
    cur = start(label)
    for raw in lines:
        t = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            label, piece = m.group(1), 0
            cur = start(label)
            continue
        if "pies-rare-path" in t:
            cur["rare"] = True
        if "pies-main-tet-path" in t:
            cur["main"] = True
        if not t or t.startswith((";", ".")):
            continue
        op = t.split()[0]
        cur["ops"].append(op)
        cur["text"].append(t)
        if op.startswith(("s_cbranch", "s_branch")):
            cur["branch"] = (op, t.split()[1])
            piece += 1
            cur = start("%s+%d" % (label, piece))
    return blocks


def counts(b):
    ops = b["ops"]
    valu = [o for o in ops if o.startswith("v_")]
    return {"all": len(ops), "valu": len(valu), "moves": sum(o.startswith(MOVES) for o in valu),
            "packed": sum(o.startswith("v_pk_") and not o.startswith("v_pk_mov") for o in valu),
            "waits": sum(o.startswith("s_waitcnt") for o in ops),
            "scalar": sum(o.startswith("s_") and not o.startswith("s_waitcnt") for o in ops),
            "memory": sum(o.startswith(MEMORY) for o in ops)}


def lds_widths(ops):
    """LDS instructions by mnemonic (the width is part of it): 'ds_read_b128 4, ds_write_b96 4'"""
    tally = {}
    for o in ops:
        if o.startswith("ds_"):
            tally[o] = tally.get(o, 0) + 1
    return ", ".join("%s %d" % kv for kv in sorted(tally.items())) or "none"


def barrier_segments(lines):
    """the product build's kernel cut at its workgroup barriers, in the order of the text: a colour step is what stands between
    two barriers.  Returns {LDS instructions of a segment, by width: number of such segments} for the segments that gather or
    scatter node records (12 or 16 bytes wide): the tetrahedral steps (four gathers, four scatters, with the dictionary the rest
    table's rows), the distance colours (two gathers, one scatter), the prologue and the per-node steps."""
    found, ops = {}, []
    for raw in list(lines) + ["s_barrier"]:
        t = raw.strip()
        if not t or t.startswith((";", ".")):
            continue
        op = t.split()[0]
        if op == "s_barrier":
            if any(o.endswith(("_b96", "_b128")) for o in ops if o.startswith("ds_")):
                key = lds_widths(ops)
                found[key] = found.get(key, 0) + 1
            ops = []
        else:
            ops.append(op)
    return found


def main_loop_path(blocks):
    index = {b["name"]: i for i, b in enumerate(blocks)}
    marked = [i for i, b in enumerate(blocks) if b["main"]]
    if len(marked) != 1:
        raise SystemExit("the main tetrahedral colour loop's note was found %d times" % len(marked))
    header = back = marked[0]

    def rare(i, depth=0):
        b = blocks[i]
        if b["rare"]:
            return True
        only_jump = all(o.startswith(("s_branch", "s_or_b64", "s_mov_b64", "s_nop")) for o in b["ops"])
        if only_jump and depth < 4:
            if b["branch"] and b["branch"][0] == "s_branch":
                return rare(index[b["branch"][1]], depth + 1)
        return False
    def succ(i):
        b = blocks[i]
        if not b["branch"]:
            return [i + 1] if i + 1 < len(blocks) else []
        op, target = b["branch"]
        return [index[target]] if op == "s_branch" else [index[target], i + 1]

    def distance_home(i):  # blocks from i back to the loop's gather, not through a rare path
        seen, front, d = {i}, [i], 0
        while front and d < 200:
            if header in front:
                return d
            front = [j for k in front for j in succ(k) if j not in seen and not rare(j) and not seen.add(j)]
            d += 1
        return 1 << 30
    path, i, notes = [], header, []
    while True:
        b = blocks[i]
        if i == header and path:
            break
        path.append(i)
        if len(path) > 400:
            raise SystemExit("the walk does not come back to the loop's gather: " + " ".join(blocks[k]["name"] for k in path[:60]))
        if not b["branch"]:
            i += 1
            continue
        op, target = b["branch"]
        t, f = index[target], i + 1
        if op == "s_branch":
            i = t
        elif rare(f) and not rare(t):
            i = t
        elif rare(t):
            i = f
        elif op == "s_cbranch_execz":
            i = f  # (lanes are active: the guarded region runs)
        elif op == "s_cbranch_execnz":
            i = t
        else:  # a scalar condition (the loop's own tests): the way that stays in the loop
            i = t if distance_home(t) < distance_home(f) else f
        other = t if i == f else f
        if i in path and i != header and other not in path and not rare(other):  # an inner loop (the sweeps) is left after its first, clean pass
            i = other
    return header, back, path, notes


def report(txt, sym, title, dump=None):
    lines, (vgprs, scratch, occupancy) = kernel_text(txt, sym)
    blocks = basic_blocks(lines)
    header, back, path, notes = main_loop_path(blocks)
    print("%s: %d lines of ISA, %s VGPRs, scratch %s bytes, occupancy %s" % (title, len(lines), vgprs, scratch, occupancy))
    print("main tetrahedral colour loop (gather in block %s); * = on the path of a config-2 element" % blocks[header]["name"])
    total = dict.fromkeys(("all", "valu", "moves", "packed", "scalar", "waits", "memory"), 0)
    lo, hi = min(path), max(path)
    for i in range(lo, hi + 1):
        c = counts(blocks[i])
        if not c["all"]:
            continue
        on = i in path
        if on:
            for k in total:
                total[k] += c[k]
        print(" %s %-16s all %4d  VALU %4d (moves %3d, packed %3d)  scalar %3d  waits %2d  memory %2d%s" %
              ("*" if on else " ", blocks[i]["name"], c["all"], c["valu"], c["moves"], c["packed"], c["scalar"], c["waits"], c["memory"],
               "  [rare]" if blocks[i]["rare"] else ""))
    for n in notes:
        print("  note: " + n)
    print("per colour step along the path: all %(all)d, VALU %(valu)d (moves %(moves)d, packed %(packed)d), scalar %(scalar)d, waits %(waits)d, memory %(memory)d"
          % total)
    print()
    if dump:  # the instructions along the path, block by block: where the moves of a source region stand
        with open(dump, "w") as f:
            for i in path:
                f.write("%s:\n" % blocks[i]["name"])
                f.writelines("  %s\n" % t for t in blocks[i]["text"])
    return total, len(lines), (vgprs, scratch)


def main():
    argv = sys.argv[1:]
    block = int(take(argv, "--block", "512"))
    json_out = take(argv, "--json")
    dump = take(argv, "--dump")
    dict_ = 0 if "--streamed" in argv else 1
    argv = [a for a in argv if a != "--streamed"]
    with tempfile.TemporaryDirectory() as tmp:
        noted = compile_isa(tmp, "noted.s", ["-DPIES_PATH_NOTES"] + argv)
        plain = compile_isa(tmp, "plain.s", argv)
    out = {}
    for form, what in ((0, "tet_core (the form before tet_rows.h)"), (1, "tet_rows.h")):
        sym = "_ZN4pies7k_layerILi%dELi0ELi1ELb%dELi%dELi1EEE" % (block, dict_, form)  # (DIST = 1: the distance projection's product form)
        title = "k_layer<%d, 0, 1, %s, %d>, %s" % (block, "true" if dict_ else "false", form, what)
        total, n_noted, regs = report(noted, sym, title, dump if form == 1 else None)
        n_plain = len(kernel_text(plain, sym)[0])
        vg, sc = kernel_text(plain, sym)[1][:2]
        print("  (the product build of this kernel, without the notes: %d lines of ISA against %d with them; %s VGPRs, scratch %s)\n" % (n_plain, n_noted, vg, sc))
        lines = kernel_text(plain, sym)[0]
        print("  LDS instructions of the product build of this kernel: " + lds_widths(t.split()[0] for t in map(str.strip, lines) if t))
        print("  between two workgroup barriers of it (segments that gather or scatter node records; a distance colour: two gathers, one scatter):")
        for key, n in sorted(barrier_segments(lines).items(), key=lambda kv: -kv[1]):
            print("    %3d x  %s" % (n, key))
        print()
        out[form] = total
    print("registers of every instantiation (product flags):")
    for m in re.finditer(r"^(_ZN4pies7k_layerI\S+):.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)", plain, re.S | re.M):
        print("  %-48s VGPRs %3s  scratch %s" % (m.group(1), m.group(2), m.group(3)))
    if json_out:
        with open(os.path.join(ROOT, "profiles", "r06_layer_critical_path.json")) as f:
            base = json.load(f)
        base["what"] = ("VALU instructions the busiest wavefront of a k_layer tile executes in one launch of BASELINE config 2, as in "
                        "r06_layer_critical_path.json; tet_colour_valu recounted by tools/layer_isa.py along the config-2 path of the main loop of "
                        "k_layer<%d, 0, 1, true, 1> (tet_rows.h); the distance and load/store figures are r06's." % block)
        base["tet_colour_valu"] = out[1]["valu"]
        base["tet_colour_all_instructions"] = out[1]["all"]
        base["tet_colour_valu_tet_core_form"] = out[0]["valu"]
        base["tet_colour_all_instructions_tet_core_form"] = out[0]["all"]
        base.pop("cross_check", None)
        with open(json_out, "w") as f:
            json.dump(base, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
