"""GPU: the C++ adaptor of the spanning forest (gmsx::min_spanning_forest / gmsx::msf_arc_mask, include/gmsx_set_graph.hpp) through
tests/cpp/test_msf_adaptor.cpp, and `gmsx_driver msf [--max] -v`."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_msf_golden_cpu import record

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def test_msf_adaptor(gpu, tmp_path):
    exe = tmp_path / "msf_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_msf_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    for key, args in (("file_two_parts_a", ["file", os.path.join(GOLDEN, "sssp", "two_parts_a.wel")]), ("kronecker_10_16", ["kron", "10"])):
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = {ln.split()[1]: ln.split()[2:] for ln in out.splitlines() if ln.startswith("msf ")}
        assert sorted(lines) == ["max", "min"]
        for which, maximum in (("min", False), ("max", True)):
            rec = record(key, maximum)
            assert lines[which] == [str(rec["edges"]), str(rec["total_weight"]), str(rec["trees"]), str(rec["rounds"]), rec["fnv"], str(2 * rec["edges"])]


def test_driver_msf(gpu):
    for extra, maximum in (([], False), (["--max"], True)):
        rec = record("kronecker_10_16", maximum)
        r = subprocess.run([DRIVER, "msf", "-g", "kronecker", "10", "-n", "2", "-v"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout
        assert out.count("Trial Time:") == 2 and out.count("@@@ msf " + ("maximum" if maximum else "minimum")) == 2 and "Average Time:" in out
        assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
        label = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in out.splitlines() if ":" in ln}
        assert (int(label["Trees"]), int(label["Edges"]), int(label["Total Weight"])) == (rec["trees"], rec["edges"], rec["total_weight"])
    path = os.path.join(GOLDEN, "sssp", "two_parts_b.wel")
    r = subprocess.run([DRIVER, "msf", "-f", path, "-n", "1", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout
    label = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in r.stdout.splitlines() if ":" in ln}
    assert int(label["Total Weight"]) == record("file_two_parts_b", False)["total_weight"]
    # --max belongs to msf alone; a forest is global
    assert subprocess.run([DRIVER, "cc", "-g", "kronecker", "8", "--max"], capture_output=True, text=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "msf", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
