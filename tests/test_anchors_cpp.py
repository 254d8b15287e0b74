"""Solver::addAnchorsHere and Solver::applyAnchors through the C++ drop-in class: tests/cpp/anchors_example.cpp, built like
tests/test_dropin_cpp.py builds its host programs.  The reaction the program prints is compared bit for bit with the numpy
restatement of the rule (tests/test_anchors.py) on the same sheet, built here on a host-only handle through the Python binding's
Anchor.at - so the two bindings compute the same local coordinates."""
import os
import subprocess

import numpy as np
import pytest

from pies_amd import capi
from test_anchors import F, apply_anchors
from test_dropin_cpp import build_example

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "anchors_example.cpp")


def test_anchors_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


def expected_reactions():
    """the program's scene, sets and frames, restated: the springs' call, then the pin's on the state the first left"""
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    g.create_sheet(20, 20, translation=(0.5, 3.0, 0.25), scale=1.0, mass=2.0, w=1.0)
    pos, vel, w = g.positions, g.velocities, g.inv_masses
    n, dt = len(pos), F(1.0 / 64.0)
    bar = pos[0]
    held = [capi.Anchor.at(i, 0, capi.AnchorFrame.make(bar), pos[i], stiffness=600.0, damping=2.0) for i in range(20)]
    up = (bar[0], bar[1] + F(0.125), bar[2])
    lifted = capi.AnchorFrame.make(up, velocity=(0.0, 2.0, 0.5), angular=(0.0, 1.5, 0.0), pivot=up)
    first = apply_anchors(pos, vel, w, held, [lifted], dt)
    corner = [capi.Anchor.make(n - 1, 0, (0.25, 0.0, -0.5), pin=True)]
    post = capi.AnchorFrame.make((pos[n - 1][0], pos[n - 1][1] + F(0.5), pos[n - 1][2]), velocity=(0.0, 1.0, 0.0), pivot=(0.0, 0.0, 0.0))
    second = apply_anchors(first[0], first[2], w, corner, [post], dt, prev=first[1])
    return first, second


def test_the_restated_scene_is_the_programs():
    first, second = expected_reactions()
    assert first[5].tolist() == [20] and first[3][0][1] > 0 and np.abs(first[6][:, 3] - F(0.125)).max() < 1e-5
    assert second[5].tolist() == [1] and second[3][0][1] == 2.0  # the corner (mass 2, at rest) takes the post's velocity (0, 1, 0)


@pytest.mark.gpu
def test_anchors_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "anchors ok" in out.stdout
    rows = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("reaction ")]
    assert [int(r[0]) for r in rows] == [0, 1]
    got = np.array([[float(x) for x in r[1:7]] for r in rows], F)  # (nine digits carry an fp32 exactly)
    for k, want in enumerate(expected_reactions()):
        assert np.array_equal(got[k, :3].view(np.uint32), want[3][0].view(np.uint32)), (k, got[k], want[3])
        assert np.array_equal(got[k, 3:].view(np.uint32), want[4][0].view(np.uint32)), (k, got[k], want[4])
        assert int(rows[k][7]) == int(want[5][0])
