"""Solver::applySurfaceLoads through the C++ drop-in class: tests/cpp/loads_example.cpp, built like tests/test_dropin_cpp.py builds
its host programs.  Reaction, volume and area the program prints are compared bit for bit with the numpy restatement of the rule
(tests/test_loads.py) on the same box, built here on a host-only handle."""
import os
import subprocess

import numpy as np
import pytest

from pies_amd import capi
from test_dropin_cpp import build_example
from test_loads import F, apply_surface_loads

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "loads_example.cpp")
W, H, D = 3, 4, 3


def test_loads_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


def boundary_of(verts, tets):
    """addTetMeshVolume's boundary (include/Pies/Solver.h): the faces that belong to one element, elements in order, faces opposite
    vertex 0, 1, 2, 3, each wound so that its normal points away from the element's fourth vertex"""
    k_face = ((1, 2, 3), (0, 3, 2), (0, 1, 3), (0, 2, 1))
    seen = {}
    for t in tets:
        for f in k_face:
            key = tuple(sorted(int(t[i]) for i in f))
            seen[key] = seen.get(key, 0) + 1
    out = []
    for t in tets:
        for opposite, f in enumerate(k_face):
            a, b, c = (int(t[i]) for i in f)
            if seen[tuple(sorted((a, b, c)))] != 1:
                continue
            u, v = verts[b] - verts[a], verts[c] - verts[a]
            normal = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], F)
            to_fourth = verts[int(t[opposite])] - verts[a]
            if normal[0] * to_fourth[0] + normal[1] * to_fourth[1] + normal[2] * to_fourth[2] > 0:
                b, c = c, b
            out.append([a, b, c])
    return np.array(out, np.uint32)


def expected_reaction():
    """the program's box and loads, restated"""
    origin = F([0.5, 2.0, 0.25])
    lattice = lambda x, y, z: z + D * (y + H * x)
    verts = np.array([origin + F(0.5) * F([x, y, z]) for x in range(W) for y in range(H) for z in range(D)], F)
    tets = []
    for x in range(W - 1):
        for y in range(H - 1):
            for z in range(D - 1):
                for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                    c = [x, y, z]
                    tet = [lattice(*c)]
                    for k in p:
                        c[k] += 1
                        tet.append(lattice(*c))
                    tets.append(tet)
    tris = boundary_of(verts, np.array(tets))
    g = capi.Solver(capi.Options(solver=capi.PD, iterations=6), device=capi.DEVICE_NONE)
    n = len(verts)
    g.add_nodes_raw(verts, vel=np.tile(F([0.0, -1.0, 0.0]), (n, 1)), radius=np.full(n, 0.5, F), invMass=np.full(n, F(1.0) / F(2.0), F))
    g.add_triangles(tris)
    centre = origin + F([0.5, 0.75, 0.5])
    level = float(origin[1] + F(0.75) + F(0.0078125))
    loads = [capi.SurfaceLoad.gas(1.5, 2.0, about=centre), capi.SurfaceLoad.fluid(9.8125, (0.0, level, 0.0)).with_drag(0.5, (0.25, 0.0, 0.0))]
    return apply_surface_loads(g.positions, g.velocities, g.inv_masses, g.ids(capi.TRIANGLES), loads, F(1.0 / 64.0))


def test_the_restated_scene_is_the_programs():
    vel, impulse, torque, nodes, volume, area = expected_reaction()
    boundary = W * H * D - (W - 2) * (H - 2) * (D - 2)
    assert nodes[0] == boundary and 0 < nodes[1] < boundary and np.allclose(volume, 1.5, rtol=1e-6) and np.allclose(area, 8.0, rtol=1e-6)
    lift = 9.8125 * 0.75 / 64
    assert 0.5 * lift < impulse[1][1] < 1.5 * lift and np.abs(impulse[0]).max() < 1e-5


@pytest.mark.gpu
def test_loads_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "loads ok" in out.stdout
    rows = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("reaction ")]
    assert [int(r[0]) for r in rows] == [0, 1]
    got = np.array([[float(x) for x in r[1:7] + r[8:10]] for r in rows], F)  # (nine digits carry an fp32 exactly)
    vel, impulse, torque, nodes, volume, area = expected_reaction()
    assert np.array_equal(got[:, :3].view(np.uint32), impulse.view(np.uint32))
    assert np.array_equal(got[:, 3:6].view(np.uint32), torque.view(np.uint32))
    assert [int(r[7]) for r in rows] == nodes.tolist()
    assert np.array_equal(got[:, 6].view(np.uint32), volume.view(np.uint32)) and np.array_equal(got[:, 7].view(np.uint32), area.view(np.uint32))
