"""CPU: compiles and runs tests/cpp/test_tc_core_plan.cpp against gms_amd/csrc/host/tc_core_plan.hpp — the rule that sizes the dense core of the
triangle count (GMSX_TC_CORE = -1) and the bookkeeping of its blocks (pure C++, no HIP): the hand-derived cases and the property loop live
in the C++ file."""
import os
import subprocess

from conftest import ROOT


def test_tc_core_plan(tmp_path):
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gms_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cpp", "test_tc_core_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tc core plan ok" in r.stdout, r.stdout + r.stderr
