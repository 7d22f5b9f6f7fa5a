"""GPU: the C++ adaptor of the biconnected components (gmsx::biconnected_components / gmsx::articulation_points / gmsx::bridges,
include/gmsx_set_graph.hpp) through tests/cpp/test_bicc_adaptor.cpp, and `gmsx_driver bicc -v`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_bicc_golden_cpu import golden_bicc, rec_of

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def fnv_of(a):
    """FNV-1a over the bytes of an int32 array: what the C++ adaptor test prints"""
    x = 1469598103934665603
    for b in np.ascontiguousarray(a, dtype="<i4").tobytes():
        x = ((x ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return x


def test_bicc_adaptor(gpu, tmp_path):
    exe = tmp_path / "bicc_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_bicc_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    for key, args in (("file_eppsteinExample", ["file", os.path.join(GOLDEN, "testGraphs", "eppsteinExample.el")]),
                      ("file_tomitaExample", ["file", os.path.join(GOLDEN, "testGraphs", "tomitaExample.el")]),
                      ("kronecker_10_16", ["kron", "10", "16"]), ("kronecker_12_2", ["kron", "12", "2"])):
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split()[1:] for ln in out.splitlines() if ln.startswith("bicc ")]
        rec = rec_of(key)
        block, blocks_at, _, _ = golden_bicc(gpu, key)
        assert lines == [[str(rec["blocks"]), str(rec["bridges"]), str(rec["articulation_points"]), str(rec["levels"]), str(fnv_of(block)),
                          str(fnv_of(blocks_at))]], key


def test_driver_bicc(gpu):
    rec = rec_of("kronecker_10_16")
    r = subprocess.run([DRIVER, "bicc", "-g", "kronecker", "10", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ biconnected components") == 2 and "Average Time:" in out
    assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
    label = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in out.splitlines() if ":" in ln}
    assert (int(label["Blocks"]), int(label["Bridges"]), int(label["Articulation Points"]), int(label["Components"]), int(label["Levels"])) == \
        (rec["blocks"], rec["bridges"], rec["articulation_points"], rec["components"], rec["levels"])
    path = os.path.join(GOLDEN, "testGraphs", "tomitaExample.el")
    r = subprocess.run([DRIVER, "bicc", "-f", path, "-n", "1", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout
    label = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in r.stdout.splitlines() if ":" in ln}
    assert int(label["Blocks"]) == rec_of("file_tomitaExample")["blocks"]
    # the blocks are global and have no metric
    assert subprocess.run([DRIVER, "bicc", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "bicc", "-g", "kronecker", "8", "--metric", "jaccard"], capture_output=True, text=True, timeout=60).returncode == 100
