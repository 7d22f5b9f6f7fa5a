"""CPU: compiles and runs tests/cpp/test_list_key.cpp against gms_amd/csrc/host/list_key.hpp, the key of the cached pass 1 of the listing calls
(gmsx_bk_list, gmsx_kclique_star_list, gmsx_subgraph_match; pure C++, no HIP): the cases live in the C++ file."""
import os
import subprocess

from conftest import ROOT


def test_list_key(tmp_path):
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gms_amd", "csrc", "host"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_list_key.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "list key ok" in r.stdout, r.stdout + r.stderr
