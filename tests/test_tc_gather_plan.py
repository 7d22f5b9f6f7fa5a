"""CPU: compiles and runs tests/cpp/test_tc_gather_plan.cpp against gms_amd/csrc/host/tc_gather_plan.hpp — the rule that says which trailing
16-byte units of a stream row move to the receiver's gathered row (GMSX_TC_GATHER; pure C++, no HIP): the exhaustive loop over position in
the line, units, form and limit, and the hand-derived cases live in the C++ file."""
import os
import subprocess

from conftest import ROOT


def test_tc_gather_plan(tmp_path):
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gms_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cpp", "test_tc_gather_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tc gather plan ok" in r.stdout, r.stdout + r.stderr
