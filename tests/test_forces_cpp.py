"""Solver::applyForces through the C++ drop-in class: tests/cpp/forces_example.cpp, built like tests/test_dropin_cpp.py builds its
host programs.  The reaction the program prints is compared bit for bit with the numpy restatement of the rule
(tests/test_forces.py) on the same sheet, built here on a host-only handle."""
import os
import subprocess

import numpy as np
import pytest

from pies_amd import capi
from test_dropin_cpp import build_example
from test_forces import F, apply_forces

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "forces_example.cpp")


def test_forces_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


def expected_reaction():
    """the program's scene and forces, restated"""
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    g.create_sheet(20, 20, translation=(0.5, 3.0, 0.25), scale=1.0, mass=2.0, w=1.0)
    pos = g.positions
    middle = pos[len(pos) // 2 + 10]
    forces = [capi.Force.wind((1.0, 2.0, 6.0), 1.5, shear=0.25).within((middle[0] + F(0.015625), middle[1], middle[2]), 4.03125, capi.FALLOFF_LINEAR),
              capi.Force.drag(8.0, velocity=(0.0, -1.0, 0.0))]
    return apply_forces(pos, g.velocities, g.inv_masses, forces, F(1.0 / 64.0), g.ids(capi.TRIANGLES))


def test_the_restated_scene_is_the_programs():
    vel, impulse, torque, nodes = expected_reaction()
    assert 0 < nodes[0] < nodes[1] == 400 and impulse[1][1] == -100.0 and np.dot(impulse[0], [1.0, 2.0, 6.0]) > 0


@pytest.mark.gpu
def test_forces_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "forces ok" in out.stdout
    rows = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("reaction ")]
    assert [int(r[0]) for r in rows] == [0, 1]
    got = np.array([[float(x) for x in r[1:7]] for r in rows], F)  # (nine digits carry an fp32 exactly)
    vel, impulse, torque, nodes = expected_reaction()
    assert np.array_equal(got[:, :3].view(np.uint32), impulse.view(np.uint32))
    assert np.array_equal(got[:, 3:].view(np.uint32), torque.view(np.uint32))
    assert [int(r[7]) for r in rows] == nodes.tolist()
