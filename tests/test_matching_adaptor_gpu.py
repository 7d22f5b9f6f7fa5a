"""GPU: the C++ adaptor of the matching (gmsx::greedy_matching / gmsx::matching_verify, include/gmsx_set_graph.hpp) through
tests/cpp/test_matching_adaptor.cpp, and `gmsx_driver matching [--weighted] -v`."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_matching_golden_cpu import record

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def labels_of(out):
    return {ln.split(":")[0]: ln.split(":")[1].strip() for ln in out.splitlines() if ":" in ln}


def test_matching_adaptor(gpu, tmp_path):
    exe = tmp_path / "matching_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_matching_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    for key, args in (("wel_two_parts_a", ["file", os.path.join(GOLDEN, "sssp", "two_parts_a.wel")]), ("kronecker_10_16", ["kron", "10"])):
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = {ln.split()[1]: ln.split()[2:] for ln in out.splitlines() if ln.startswith("matching ")}
        assert sorted(lines) == ["unit", "weighted"]
        for which, weighted in (("unit", False), ("weighted", True)):
            rec = record(key, weighted)
            assert lines[which] == [str(rec["pairs"]), str(rec["total_weight"]), str(rec["free_vertices"]), str(rec["rounds"]), rec["fnv"], "1"]


def test_driver_matching(gpu):
    runs = [(["-g", "kronecker", "10"], "kronecker_10_16"), (["-f", os.path.join(GOLDEN, "sssp", "two_parts_b.wel")], "wel_two_parts_b")]
    for where, key in runs:
        for extra, weighted in (([], False), (["--weighted"], True)):
            rec = record(key, weighted)
            r = subprocess.run([DRIVER, "matching"] + where + ["-n", "2", "-v"] + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            out = r.stdout
            assert out.count("Trial Time:") == 2 and out.count("@@@ matching " + ("weighted" if weighted else "unweighted")) == 2
            assert "Average Time:" in out and out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
            label = labels_of(out)
            assert (int(label["Pairs"]), int(label["Total Weight"]), int(label["Free"]), int(label["Rounds"])) == (
                rec["pairs"], rec["total_weight"], rec["free_vertices"], rec["rounds"])
    # --weighted belongs to communities and matching alone; a matching is global
    assert subprocess.run([DRIVER, "cc", "-g", "kronecker", "8", "--weighted"], capture_output=True, text=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "matching", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
