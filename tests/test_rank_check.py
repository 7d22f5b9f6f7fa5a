"""CPU: compiles and runs tests/cpp/test_rank_check.cpp against gms_amd/csrc/host/rank_check.hpp, the one host-side validation of a caller's
rank array (gmsx_bk_partial, gmsx_bk_list; pure C++, no HIP): the cases live in the C++ file."""
import os
import subprocess

from conftest import ROOT


def test_rank_check(tmp_path):
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gms_amd", "csrc", "host"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_rank_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rank check ok" in r.stdout, r.stdout + r.stderr
