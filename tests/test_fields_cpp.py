"""Solver::addField, addFieldFromTriMesh and collideFieldProps through the C++ drop-in class: tests/cpp/fields_example.cpp, built
like tests/test_dropin_cpp.py builds its host programs."""
import os
import subprocess

import pytest

from test_dropin_cpp import build_example

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "fields_example.cpp")


def test_fields_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_example(tmp_path, SRC))


@pytest.mark.gpu
def test_fields_host_program(tmp_path):
    out = subprocess.run([build_example(tmp_path, SRC)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "fields ok" in out.stdout
