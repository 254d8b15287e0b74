"""pies_amd/csrc/actuator_rule.h compiled for the host (tests/cpp/actuator_rule_host.cpp: the functions the kernel calls, bit for bit
against the numpy restatement of tests/test_actuators.py on the same vectors), and Solver::addActuators / actuators /
driveActuators through the C++ drop-in class (tests/cpp/actuators_example.cpp, built like tests/test_dropin_cpp.py builds its host
programs; the channel sums the program prints are compared bit for bit with the restatement on the same lattice)."""
import os
import subprocess

import numpy as np
import pytest

from pies_amd import capi
from test_actuators import F, U, bits, containers, drive_actuators, lattice_and_sheet, random_set, with_base
from test_dropin_cpp import build_example

HERE = os.path.dirname(os.path.abspath(__file__))
RULE = os.path.join(HERE, "cpp", "actuator_rule_host.cpp")
SRC = os.path.join(HERE, "cpp", "actuators_example.cpp")


def words(values):
    return " ".join("%08x" % w for w in bits(values))


def test_rule_header_gives_the_restatements_bits_on_the_host(tmp_path):
    """every actuator of a random set over the lattice and the sheet, each asked three ways: the rest with a finite activation, the
    rest with a non-finite one (live or not), and its measured value from the positions"""
    exe = build_example(tmp_path, RULE)
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    lattice_and_sheet(g, seed=5)
    ids, rest = containers(g)
    rng = np.random.default_rng(5)
    acts = with_base(random_set(rng, {t: len(r) for t, r in rest.items()}, 120, 4), rest)
    activation = np.array([1.4, -0.9, np.nan, -np.inf], F)
    pos = g.positions
    new, per, sums, live = drive_actuators(pos, ids, rest, acts, activation)
    finite = np.array([1.4, -0.9, 0.3, -1.1], F)
    per_finite = drive_actuators(pos, ids, rest, acts, finite)[1]
    lines = []
    for a in acts:
        for u in (activation[a.channel], finite[a.channel]):
            lines.append("R %s %08x %s" % (words([a.base, a.gain, a.lo, a.hi]), a.flags, words([u])))
        nodes = np.asarray(ids[a.type]).reshape(len(rest[a.type]), -1)[a.index]
        lines.append("%s %s" % ("D" if a.type == capi.DISTANCE else "B", words(pos[nodes])))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-400:])
    got = out.stdout.split("\n")
    assert len(got) == 3 * len(acts) + 1
    seen_dead = 0
    for i, a in enumerate(acts):
        is_live = bool(np.isfinite(activation[a.channel]))
        alive, r = got[3 * i].split()
        assert int(alive) == int(is_live)
        if is_live:
            assert int(r, 16) == int(bits(per[i, 0])[0]), (i, r)
        seen_dead += not is_live
        alive, r = got[3 * i + 1].split()
        assert int(alive) == 1 and int(r, 16) == int(bits(per_finite[i, 0])[0]), (i, r)
        assert int(got[3 * i + 2], 16) == int(bits(per[i, 1])[0]), (i, a.type, got[3 * i + 2])
    assert 0 < seen_dead < len(acts) and {a.type for a in acts} == {capi.DISTANCE, capi.BEND}
    assert live.sum() == len(acts) - seen_dead
    g.close()


def test_actuators_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


def expected_channels():
    """the program's lattice, set and activations, restated"""
    g = capi.Solver(capi.Options(solver=capi.PBD, iterations=4), device=capi.DEVICE_NONE)
    g.create_box(5, 5, 5, translation=(0.5, 3.0, 0.25), scale=1.0, w=0.5)
    A = capi.Actuator.make
    acts = [A(capi.DISTANCE, i, 0, -0.5, 0.25, 4.0) for i in range(40)] + [A(capi.DISTANCE, i, 1, 0.25, 0.25, 4.0, offset=True) for i in range(40, 60)]
    k = g.add_actuators(acts, 2)
    ids, rest = containers(g)
    out = drive_actuators(g.positions, ids, rest, g.get_actuators(k)[0], np.array([0.5, 1.0], F))
    g.close()
    return out


def test_the_restated_scene_is_the_programs():
    new, per, sums, live = expected_channels()
    assert live.tolist() == [40, 20] and (per[:40, 0] < per[:40, 1]).all() and (per[40:, 0] > per[40:, 1]).all()


@pytest.mark.gpu
def test_actuators_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "actuators ok" in out.stdout
    rows = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("channel ")]
    assert [int(r[0]) for r in rows] == [0, 1]
    got = np.array([[float(x) for x in r[1:3]] for r in rows], F)  # (nine digits carry an fp32 exactly)
    new, per, sums, live = expected_channels()
    assert np.array_equal(got.view(U), sums.view(U)), (got, sums)
    assert [int(r[3]) for r in rows] == live.tolist()
