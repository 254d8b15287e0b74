"""The resource ledger (pies_amd/csrc/resource_ledger.{h,cpp}, pies_resource_counts) counts every HIP resource the library creates
or destroys - as long as every call goes through it.  This check reads the sources: outside the ledger's two files no file of
pies_amd/csrc/ may name a HIP function that creates or destroys a device allocation, a pinned allocation, a stream, an event, a
graph or an executable graph.  Comments and string literals are not code and are skipped.  tests/test_handle_lifetime_gpu.py holds
the counts themselves to their contract on a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pies_amd", "csrc")
LEDGER = ("resource_ledger.h", "resource_ledger.cpp")

# the calls the ledger wraps ...
WRAPPED = ["hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipStreamCreateWithFlags", "hipStreamDestroy", "hipEventCreate",
           "hipEventCreateWithFlags", "hipEventDestroy", "hipStreamEndCapture", "hipGraphDestroy", "hipGraphInstantiate",
           "hipGraphExecDestroy"]
# ... and the runtime's other ways to the same eight kinds of resource, which the ledger would not see
UNCOUNTED = ["hipMallocAsync", "hipFreeAsync", "hipMallocFromPoolAsync", "hipMallocManaged", "hipMallocPitch", "hipMalloc3D",
             "hipExtMallocWithFlags", "hipMallocHost", "hipHostAlloc", "hipFreeHost", "hipHostRegister", "hipHostUnregister",
             "hipStreamCreate", "hipStreamCreateWithPriority", "hipGraphCreate", "hipGraphClone", "hipGraphInstantiateWithFlags",
             "hipGraphInstantiateWithParams", "hipMemPoolCreate", "hipMemPoolDestroy"]
RAW = re.compile(r"\b(%s)\b" % "|".join(WRAPPED + UNCOUNTED))
# comments, string and character literals (one alternation: whichever starts first wins, so a quote inside a comment opens nothing)
NOT_CODE = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', re.S)


def code_of(text):
    """text with comments and literals blanked, line numbers kept"""
    return NOT_CODE.sub(lambda m: re.sub(r"[^\n]", " ", m.group(0)), text)


def raw_calls(text):
    return [(text.count("\n", 0, m.start()) + 1, m.group(1)) for m in RAW.finditer(code_of(text))]


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".cpp", ".hip")) and f not in LEDGER)


def test_the_check_sees_a_raw_call_and_only_code():
    assert raw_calls("int f() {\n  return hipMalloc(&p, 4);\n}\n") == [(2, "hipMalloc")]
    assert raw_calls("auto fn = &hipFree;") == [(1, "hipFree")]  # a function pointer is a way round too
    assert raw_calls("hipEventCreateWithFlags (&e, 0); hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);") == \
        [(1, "hipEventCreateWithFlags"), (1, "hipGraphInstantiate")]
    assert raw_calls("hipMallocAsync(&p, 4, st);") == [(1, "hipMallocAsync")]
    assert raw_calls('// hipMalloc(&p, 4)\n/* hipFree(p)\n hipFree(q) */ fail(s, "hipStreamEndCapture: it\'s" + x); char c = \'"\';') == []
    assert raw_calls("ledger::dev_malloc(&p, 4); hipMemcpyAsync(a, b, n, k, st); hipMallocator(); my_hipFree(p);") == []


def test_sources_are_found():
    names = sources()
    assert len(names) >= 60 and "capi.cpp" in names and "device_util.h" in names and "layer_kernels.hip" in names


@pytest.mark.parametrize("name", sources())
def test_no_raw_resource_call_outside_the_ledger(name):
    with open(os.path.join(CSRC, name)) as f:
        found = raw_calls(f.read())
    assert not found, "%s: HIP resource calls that bypass resource_ledger.h (line, call): %s" % (name, found)


def test_the_ledger_wraps_every_listed_call():
    with open(os.path.join(CSRC, "resource_ledger.cpp")) as f:
        named = {call for _, call in raw_calls(f.read())}
    assert named == set(WRAPPED)


def test_counts_without_a_device():
    """the entry point takes no handle and needs no device: NULL is refused, sixteen words come back, and a host-only handle
    moves none of them (it creates nothing on a device)"""
    from pies_amd import capi
    L = capi.load()
    assert L.pies_resource_counts(None) == capi.ERR_INVALID
    before = capi.resource_counts()
    assert list(before) == ["live", "created"] and all(tuple(before[k]) == capi.RESOURCE_KINDS for k in before)
    assert all(before["live"][k] <= before["created"][k] for k in capi.RESOURCE_KINDS), before
    g = capi.Solver(capi.Options(solver=capi.PBD), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3)
    g.set_schedule(capi.SCHEDULE_LAYERED)
    g.finalize()
    assert capi.resource_counts() == before
    g.close()
    assert capi.resource_counts() == before
    raw = (ctypes.c_uint64 * 16)(*([7] * 16))
    assert L.pies_resource_counts(raw) == capi.OK
    assert list(raw) == [before[half][k] for half in ("live", "created") for k in capi.RESOURCE_KINDS]
