"""Solver::measureElements / measureNodes through the C++ drop-in class: tests/cpp/measure_example.cpp, built like
tests/test_dropin_cpp.py builds its host programs.  The summary and the node sums the program prints are compared bit for bit with
the numpy restatements of the two rules (tests/test_measure.py) on the same body, built here on a host-only handle."""
import os
import subprocess

import numpy as np
import pytest

from pies_amd import capi
from test_dropin_cpp import build_example
from test_measure import F, measure_elements, measure_nodes, node_sums_matrix, summary_words

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "measure_example.cpp")


def test_measure_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


def expected():
    """the program's body, stretch, velocity and ranges, restated: (summary, node sums)"""
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    g.create_tet_box(3, 3, 3, translation=(0.25, 1.5, 0.5), scale=1.0, w=1.0, mass=1.0)
    pos = g.positions.copy()
    pos[:, 0] *= F(1.25)
    n = len(pos)
    vel = np.broadcast_to(np.array([0.5, -0.25, 2.0], F), pos.shape)
    _, summary = measure_elements(pos, g.ids(capi.TET), g.rest(capi.TET), F(0.8), F(1.0))
    about = np.array([(1.0, 2.0, 0.5), (0.0, 0.0, 0.0), (1.0, 2.0, 0.5)], F)
    return summary, measure_nodes(pos, vel, g.inv_masses, [(0, n), (n // 2, 7), (n, 0)], about), g.count(capi.TET)


def test_the_restated_body_is_the_programs():
    summary, sums, tets = expected()
    assert summary["over"] == tets > 0 and summary["under"] == summary["inverted"] == summary["nonfinite"] == 0
    assert abs(summary["max_stretch"] - 1.25) < 1e-5 and sums["dynamic"][0] + sums["fixed"][0] == 27 and sums["mass"][2] == 0
    assert abs(sums["momentum"][0][2] - 2 * sums["mass"][0]) < 1e-4 * sums["mass"][0]


@pytest.mark.gpu
def test_measure_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "measure ok" in out.stdout
    summary, sums, _ = expected()
    line = [x for x in out.stdout.splitlines() if x.startswith("summary ")][0].split()[1:]
    got = np.array([float(x) for x in line[:6]], F).view(np.uint32).tolist() + [int(x) for x in line[6:]]  # (nine digits carry an fp32 exactly)
    assert got == summary_words(summary)
    rows = [x.split()[1:] for x in out.stdout.splitlines() if x.startswith("sums ")]
    assert [int(r[0]) for r in rows] == [0, 1, 2]
    floats = np.array([[float(x) for x in r[1:12]] for r in rows], F)
    assert np.array_equal(floats.view(np.uint32), node_sums_matrix(sums).view(np.uint32))
    assert [[int(r[12]), int(r[13])] for r in rows] == [[int(a), int(b)] for a, b in zip(sums["dynamic"], sums["fixed"])]
