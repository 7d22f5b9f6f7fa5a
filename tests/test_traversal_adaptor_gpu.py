"""GPU: the C++ adaptor of the traversals (gmsx::bfs / betweenness / pick_sources, include/gmsx_set_graph.hpp) through
tests/cpp/test_traversal_adaptor.cpp on the six .el graphs against the goldens, and `gmsx_driver bfs` / `gmsx_driver bc`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_traversal_golden_cpu import ARR, BC, BFS, GRAPHS, bc_bound

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def test_traversal_adaptor(gpu, tmp_path):
    exe = tmp_path / "traversal_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_traversal_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    keys = [k for k, g in GRAPHS.items() if g["source"]["kind"] == "file"]
    assert len(keys) == 6
    for key in keys:
        g = GRAPHS[key]
        path = os.path.join(GOLDEN, "testGraphs", g["source"]["name"])
        out = subprocess.run([str(exe), path] + [str(s) for s in g["bfs_sources"]], check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split() for ln in out.splitlines()]
        assert [int(x) for x in next(ln for ln in lines if ln[0] == "picks")[1:]] == g["picks"]
        for rec in (r for r in BFS if r["graph"] == key):
            parent = next(ln for ln in lines if ln[0] == "parent" and int(ln[1]) == rec["source"])
            depth = next(ln for ln in lines if ln[0] == "depth" and int(ln[1]) == rec["source"])
            assert int(parent[2]) == rec["reached"] and int(depth[2]) == rec["levels"]
            assert np.array_equal([int(x) for x in parent[3:]], ARR["parent_%s_%d" % (key, rec["source"])])
            assert np.array_equal([int(x) for x in depth[3:]], ARR["depth_%s_%d" % (key, rec["source"])])
        for rec in (r for r in BC if r["graph"] == key and r["sources"] != "all"):
            flags = (1 if rec["exclude_source"] else 0) | (2 if rec["normalize"] else 0)
            got = next(ln for ln in lines if ln[0] == "bc" and ln[1] == rec["sources"] and int(ln[2]) == flags)
            scores, want = np.array([float(x) for x in got[4:]]), ARR[rec["array"]]
            assert np.all(np.abs(scores - want) <= bc_bound(want, rec["max_levels"], g["max_degree"], rec["n_sources"]))


def labels(out):
    return [tuple(x.strip() for x in ln.split(":", 1)) for ln in out.splitlines() if ":" in ln]


def test_driver_bfs_and_bc(gpu):
    g = GRAPHS["kronecker_10_16"]
    r = subprocess.run([DRIVER, "bfs", "-g", "kronecker", "10", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ bfs") == 2 and "Average Time:" in out
    assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
    recs = [next(b for b in BFS if b["graph"] == "kronecker_10_16" and b["source"] == s) for s in g["picks"][:2]]
    assert [int(v) for k, v in labels(out) if k == "Source"] == g["picks"][:2]   # trial t starts from the t-th pick
    assert [int(v) for k, v in labels(out) if k == "Levels"] == [b["levels"] for b in recs]
    assert [int(v) for k, v in labels(out) if k == "Bottom-up Levels"] == [b["bottom_up_levels"] for b in recs]
    assert "BFS Tree has %d nodes and %d edges" % (recs[1]["reached"], recs[1]["reached_arcs"]) in out
    r = subprocess.run([DRIVER, "bfs", "-g", "kronecker", "10", "-n", "1", "-r", "0"], capture_output=True, text=True, timeout=300)
    hub = next(b for b in BFS if b["graph"] == "kronecker_10_16" and b["source"] == 0)
    assert r.returncode == 0 and "BFS Tree has %d nodes and %d edges" % (hub["reached"], hub["reached_arcs"]) in r.stdout

    r = subprocess.run([DRIVER, "bc", "-g", "kronecker", "10", "-i", "4", "-n", "1", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 1 and out.count("@@@ betweenness") == 1 and "Average Time:" in out
    assert out.count("Verification:") == 1 and "PASS" in out and "FAIL" not in out
    rec = next(b for b in BC if b["graph"] == "kronecker_10_16" and b["sources"] == "4" and not b["exclude_source"])
    raw = ARR[rec["array"]]
    want = raw / raw.max()
    order = np.lexsort((np.arange(want.size), -want))[:5]   # ties: the smaller id
    at = out.splitlines().index("@@@ betweenness")
    top = [ln.split(":") for ln in out.splitlines()[at + 1: at + 6]]
    assert [int(t[0]) for t in top] == order.tolist()
    assert np.allclose([float(t[1]) for t in top], want[order], rtol=1e-5, atol=0)   # (six significant digits are printed)
    assert float(next(v for k, v in labels(out) if k == "Max Score")) == pytest.approx(raw.max(), rel=1e-5)
    # a traversal is global and has neither a metric nor a threshold; -i belongs to bc
    for bad in (["bfs", "--gpus", "2"], ["bc", "--gpus", "2"], ["bfs", "--threshold", "1"], ["bc", "--threshold", "1"], ["bfs", "--metric", "jaccard"],
                ["bc", "--metric", "common"], ["bfs", "-i", "2"], ["cc", "-r", "1"]):
        assert subprocess.run([DRIVER, bad[0], "-g", "kronecker", "8"] + bad[1:], capture_output=True, text=True, timeout=60).returncode == 100, bad
    r = subprocess.run([DRIVER, "bfs", "-g", "kronecker", "8", "-n", "0"], capture_output=True, text=True, timeout=60)  # no trial: no statistics
    assert r.returncode == 0 and "Average Time:" in r.stdout and "BFS Tree" not in r.stdout
