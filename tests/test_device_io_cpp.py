"""Solver::readNodesDevice / writeNodesDevice through the C++ drop-in class: tests/cpp/device_io_example.cpp.  The program owns
device memory and a stream (hipMalloc, hipStreamCreate), so it is built with hipcc here - build_example of
tests/test_dropin_cpp.py uses g++, which does not know the HIP runtime's headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "pies_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "device_io_example.cpp")


def build_hip_example(tmp_path, src=SRC):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / os.path.splitext(os.path.basename(src))[0])
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), src, "-o", exe, "-L", LIBDIR, "-lpies_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_device_io_program_compiles_and_links(tmp_path):
    assert os.path.exists(build_hip_example(tmp_path))


@pytest.mark.gpu
def test_device_io_host_program(tmp_path):
    out = subprocess.run([build_hip_example(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-400:], out.stderr[-400:])
    assert "device io ok" in out.stdout
