"""follow() (pies_amd/csrc/follow_rule.h), the rule by which captured launch counts follow the scene: a stand-alone host program,
built plainly and once more under ASan + UBSan (CPU only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "follow_rule_example.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_follow_rule(tmp_path, sanitize):
    exe = str(tmp_path / "follow_rule_example")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pies_amd", "csrc"), SRC, "-o", exe] + extra)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "follow rule ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
