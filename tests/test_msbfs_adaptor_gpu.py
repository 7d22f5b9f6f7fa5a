"""GPU: the C++ adaptor of the batched multi-source BFS (gmsx::bfs_multi / closeness, include/gmsx_set_graph.hpp) through
tests/cpp/test_msbfs_adaptor.cpp on tomitaExample.el and kronecker_10_16 against the goldens, and `gmsx_driver closeness`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_msbfs_golden_cpu import ARR, GRAPHS, INT_KEYS, golden_per_source, harmonic_bound

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def test_msbfs_adaptor(gpu, tmp_path):
    exe = tmp_path / "msbfs_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_msbfs_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    for key, argv in (("file_tomitaExample", [os.path.join(GOLDEN, "testGraphs", "tomitaExample.el")]), ("kronecker_10_16", ["kronecker", "10"])):
        out = subprocess.run([str(exe)] + argv, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split() for ln in out.splitlines()]
        want = golden_per_source(key)
        rows = [ln for ln in lines if ln[0] == "source"]
        assert [int(ln[1]) for ln in rows] == list(range(GRAPHS[key]["n"]))
        for j, k in enumerate(INT_KEYS):
            assert np.array_equal([int(ln[2 + j]) for ln in rows], want[k]), k
        close, harm = np.array([float.fromhex(ln[6]) for ln in rows]), np.array([float.fromhex(ln[7]) for ln in rows])
        assert close.tobytes() == want["closeness"].tobytes()
        bound = np.array([harmonic_bound(int(lv)) for lv in want["levels"]])
        assert np.all(np.abs(harm - want["harmonic"]) <= bound * want["harmonic"])
        for name in ("dist_sum", "reach", "far"):
            assert np.array_equal([int(x) for x in next(ln for ln in lines if ln[0] == name)[1:]], ARR[name + "_" + key]), name
        top = next(ln for ln in lines if ln[0] == "top")
        assert float.fromhex(top[1]) == close.max() and float.fromhex(top[2]) == harm.max()


def labels(out):
    return [tuple(x.strip() for x in ln.split(":", 1)) for ln in out.splitlines() if ":" in ln]


def test_driver_closeness(gpu):
    from gms_amd import capi
    from test_traversal_golden_cpu import golden_csr
    r = subprocess.run([DRIVER, "closeness", "-g", "kronecker", "10", "-i", "70", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ closeness") == 2 and "Average Time:" in out
    assert out.count("Verification:") == 2 and "Verification:" in out and "PASS" in out and "FAIL" not in out
    assert [v for k, v in labels(out) if k == "Verification"] == ["PASS", "PASS"]
    # the second trial's sources are picks 70 .. 139 (the picker runs on); the goldens hold every vertex of this graph as a source
    picks = golden_csr(capi, "kronecker_10_16").pick_sources(140).tolist()[70:]
    want = golden_per_source("kronecker_10_16")["closeness"][picks]
    order = np.lexsort((np.arange(want.size), -want))[:5]   # ties: the earlier source
    at = len(out.splitlines()) - 1 - out.splitlines()[::-1].index("@@@ closeness")
    top = [ln.split(":") for ln in out.splitlines()[at + 1: at + 6]]
    assert [int(t[0]) for t in top] == [picks[i] for i in order]
    assert np.allclose([float(t[1]) for t in top], want[order], rtol=1e-5, atol=0)   # (six significant digits are printed)
    assert float([v for k, v in labels(out) if k == "Max Score"][-1]) == pytest.approx(want.max(), rel=1e-5)
    r = subprocess.run([DRIVER, "closeness", "-g", "kronecker", "8", "-r", "3", "-n", "1", "-v"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Verification" in r.stdout and "PASS" in r.stdout and r.stdout.splitlines()[-2].startswith("3:")
    # not sharded; no metric, no threshold
    for bad in (["--gpus", "2"], ["--threshold", "1"], ["--metric", "jaccard"]):
        assert subprocess.run([DRIVER, "closeness", "-g", "kronecker", "8"] + bad, capture_output=True, text=True, timeout=60).returncode == 100, bad
