"""pies_amd.tensors: node state and skins as torch tensors on the solver's device.  The module needs torch imported BEFORE
libpies_hip.so is loaded (one HIP runtime per process), which this pytest process - its other tests have loaded the library long
ago - cannot offer: tests/tensors_child.py runs once per session in a fresh process and the tests assert on the JSON line it
prints.  Every comparison the child makes is bit for bit against the numpy getters and setters of pies_amd.capi."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tensors_child.py")


@pytest.fixture(scope="session")
def child():
    out = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-800:], out.stderr[-1600:])
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout[-800:]
    return json.loads(lines[0])


def test_one_runtime_is_mapped(child):
    """the two-runtime guard: with torch imported first the library runs on torch's runtime and no second one is mapped"""
    assert len(child["runtimes"]) == 1 and child["runtimes_after"] == child["runtimes"], child["runtimes_after"]


def test_getters_equal_the_numpy_getters(child):
    assert all(child["getters"].values()) and len(child["getters"]) == 5, child["getters"]
    assert child["stride4"]


def test_state_equals_the_two_single_reads(child):
    assert child["state"]


def test_out_reuse(child):
    assert child["out_reuse"]
    assert child["out_refused"] == [True, True, True, True]  # requires_grad, a CPU tensor, a wrong shape, a wrong dtype


def test_setters(child):
    assert child["setters"]


def test_skin(child):
    assert child["skin"]


@pytest.mark.parametrize("kind", ["pbd", "pd"])
def test_closed_loop_equals_the_host_loop(child, kind):
    """20 ticks of tick_async -> positions() -> two torch operations -> set_velocities(v, ids) without a host synchronisation end
    in exactly the state of the same loop through g.positions / g.set_velocities"""
    r = child["loop_" + kind]
    assert r["equal"] == [True, True, True] and r["finite"] and not r["failed"], r
    assert r["moved"] > 0.0
