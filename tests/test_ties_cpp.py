"""Solver::addTies and Solver::applyTies through the C++ drop-in class: tests/cpp/ties_example.cpp, built like
tests/test_dropin_cpp.py builds its host programs.  The reaction the program prints is compared bit for bit with the numpy
restatement of the rule (tests/test_ties.py) on the same two sheets, built here on a host-only handle through the Python binding's
Tie.on_triangle - so the two bindings compute the same weights.  Its companion is tests/test_anchors_cpp.py."""
import os
import subprocess

import numpy as np
import pytest

from pies_amd import capi
from test_dropin_cpp import build_example
from test_ties import F, apply_ties

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "ties_example.cpp")


def test_ties_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


def expected_reaction():
    """the program's scene, set and groups, restated"""
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    g.create_sheet(20, 20, translation=(0.5, 3.0, 0.25), scale=1.0, mass=2.0, w=1.0)
    g.create_sheet(20, 20, translation=(0.5, 3.125, 0.25), scale=1.0, mass=2.0, w=1.0)
    pos, vel, w = g.positions, g.velocities, g.inv_masses
    ties = [capi.Tie.on_triangle(400 + i, (i, i + 1, i + 20), 0.25, 0.25, stiffness=600.0, damping=2.0, group=0) for i in range(20)]
    ties += [capi.Tie.make(420 + i, 20 + i, stiffness=300.0, damping=1.0, group=1) for i in range(5)]
    groups = [capi.TieGroup.make(pos[0]), capi.TieGroup.make(pos[20], break_stretch=0.1)]
    return apply_ties(pos, vel, w, ties, groups, F(1.0 / 64.0), 4)


def test_the_restated_scene_is_the_programs():
    out = expected_reaction()
    assert out[3].tolist() == [20, 0] and out[1][0][1] < 0 and not out[1][1].any()
    assert out[5].tolist() == [0] * 20 + [1] * 5 and np.abs(out[4][20:, 3] - F(0.125)).max() < 1e-5


@pytest.mark.gpu
def test_ties_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "ties ok" in out.stdout
    rows = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("reaction ")]
    assert [int(r[0]) for r in rows] == [0, 1]
    got = np.array([[float(x) for x in r[1:7]] for r in rows], F)  # (nine digits carry an fp32 exactly)
    want = expected_reaction()
    for k in range(2):
        assert np.array_equal(got[k, :3].view(np.uint32), want[1][k].view(np.uint32)), (k, got[k], want[1])
        assert np.array_equal(got[k, 3:].view(np.uint32), want[2][k].view(np.uint32)), (k, got[k], want[2])
        assert int(rows[k][7]) == int(want[3][k])
