"""The arithmetic of tet_rows.h (pies_amd/csrc: the tetrahedral projection of k_layer on row pairs, rare paths behind uniform tests)
compiled for the host and compared bit for bit with the oracle's svd3 + svd3_recompose, clamp, flip and blend on 120 000 seeded
inputs that take every path of the decomposition: a stand-alone program, built plainly and once more under ASan + UBSan (CPU only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tet_rows_example.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_tet_rows(tmp_path, sanitize):
    exe = str(tmp_path / "tet_rows_example")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "pies_amd", "csrc"),
                           "-I", os.path.join(ROOT, "oracle"), SRC, "-o", exe] + extra)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tet rows ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
