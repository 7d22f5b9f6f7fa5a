"""CPU: compiles and runs tests/cpp/test_kc_bin_plan.cpp against gms_amd/csrc/host/kc_bin_plan.hpp — the one table of the k-clique bins
(pure C++, no HIP) that the driver of kclique.hip resolves and launches from: for every k = 3 … 10, with and without the per-vertex counts and the
triangular layout, and a range of width limits, the plan against tables written out by hand, and the properties every plan has (the bins tile
(0, max_d], at most KcBins::kN of them, every dynamic-LDS size within its kernel's limit, which bins a k = 4 count may export).  The cases live in
the C++ file."""
import os
import subprocess

from conftest import ROOT


def test_kc_bin_plan(tmp_path):
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gms_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cpp", "test_kc_bin_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "kc bin plan ok" in r.stdout, r.stdout + r.stderr
