"""layer_rest_set6 against layer_rest_set (every set below the cap of 64, over the id patterns of test_pack_round_trip) and a rest
table row in pair order read back as tet_rows.h reads it against rest_of on the plain row: a stand-alone host program
(tests/cpp/layer_rest_row_example.cpp), built plainly and once more under ASan + UBSan (CPU only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "layer_rest_row_example.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_layer_rest_row(tmp_path, sanitize):
    exe = str(tmp_path / "layer_rest_row_example")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "pies_amd", "csrc"),
                           SRC, "-o", exe] + extra)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "layer rest row ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
