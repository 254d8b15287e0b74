"""The three quotients of distance_core from one reciprocal (pies_amd/csrc/distance_quotient.h) compiled for the host and compared
bit for bit with `/` and sqrtf (tests/cpp/distance_quotient_example.cpp): 1.2e7 seeded operand triples inside the range of the
per-lane test, each with the float nearest to 1/d and both its neighbours as the reciprocal seed; both sides of every boundary of
the range; zeros of either sign, dist around the 1e-5 threshold, subnormal and overflowing sums of squares, infinities and NaN, for
which the fallback must be taken.  A stand-alone program, built plainly and once more under ASan + UBSan (CPU only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "distance_quotient_example.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_distance_quotient(tmp_path, sanitize):
    exe = str(tmp_path / "distance_quotient_example")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "pies_amd", "csrc"),
                           SRC, "-o", exe] + extra)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "distance quotient ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
