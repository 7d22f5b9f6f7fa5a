"""GPU: the C++ adaptor of the motif census (gmsx::cycle4_count / gmsx::motif_census4, include/gmsx_set_graph.hpp) through
tests/cpp/test_motifs_adaptor.cpp, and `gmsx_driver motifs -v`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_motifs_golden_cpu import MOTIFS, RECS, census_np

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def test_motifs_adaptor(gpu, tmp_path):
    exe = tmp_path / "motifs_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_motifs_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    names = sorted(f for f in os.listdir(os.path.join(GOLDEN, "testGraphs")) if f.endswith(".el"))
    assert len(names) == 6
    for name in names:
        path = os.path.join(GOLDEN, "testGraphs", name)
        csr = gpu.HostCSR.load(path)   # (the adaptor test loads it the same way: relabelled where the loader finds it worth it)
        want = census_np(np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32))
        out = subprocess.run([str(exe), path], check=True, capture_output=True, text=True, timeout=120).stdout
        lines = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()}
        assert lines["cycle4"] == [want["subgraphs"]["cycle4"]]
        assert np.array_equal(lines["at_vertex"], want["at_vertex"])
        assert lines["subgraphs"] == [want["subgraphs"][k] for k in MOTIFS] and lines["induced"] == [want["induced"][k] for k in MOTIFS]
        assert lines["walked"] == [want["wedges_walked"], want["max_codegree"]]


def test_driver_motifs(gpu):
    rec = RECS["kronecker_10_16"]
    r = subprocess.run([DRIVER, "motifs", "-g", "kronecker", "10", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ motif census") == 2 and "Average Time:" in out
    assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
    label = {ln.split(":")[0]: ln.split(":")[1].split() for ln in out.splitlines() if ":" in ln}
    for k in MOTIFS:
        assert label[k] == [str(rec["subgraphs"][k]), "induced", str(rec["induced"][k])], k
    assert label["Wedges Walked"] == [str(rec["wedges_walked"])] and label["Max Codegree"] == [str(rec["max_codegree"])]
    assert subprocess.run([DRIVER, "motifs", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
