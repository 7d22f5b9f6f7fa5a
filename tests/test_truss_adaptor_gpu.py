"""GPU: the C++ adaptor of the truss decomposition (gmsx::edge_support / truss_numbers / ktruss_edges, include/gmsx_set_graph.hpp) through
tests/cpp/test_truss_adaptor.cpp, and `gmsx_driver truss -v`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph
from test_truss_golden_cpu import ARR, TRUSS, edge_ids, truss_np

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def test_truss_adaptor(gpu, tmp_path):
    exe = tmp_path / "truss_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_truss_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    keys = [k for k, r in TRUSS.items() if r["source"]["kind"] == "file"]
    assert len(keys) == 6
    for key in keys:
        rec = TRUSS[key]
        path = os.path.join(GOLDEN, "testGraphs", rec["source"]["name"])
        csr = gpu.HostCSR.load(path)
        off, adj = csr.offsets(), csr.neighbors()
        out = subprocess.run([str(exe), path], check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split() for ln in out.splitlines()]
        want_truss, _, rounds, levels, want_sup = truss_np(off, adj)
        info = [int(x) for x in next(ln for ln in lines if ln[0] == "info")[1:]]
        assert info == [rec["max_truss"], levels, rounds, rec["max_support"], rec["top_edges"], rec["triangles"]] and levels == rec["levels"]
        support = np.array(next(ln for ln in lines if ln[0] == "support")[1:], dtype=np.int64)
        truss = np.array(next(ln for ln in lines if ln[0] == "truss")[1:], dtype=np.int64)
        assert np.array_equal(support, ARR["support_" + key]) and np.array_equal(support, want_sup)
        assert np.array_equal(truss, ARR["truss_" + key]) and np.array_equal(truss, want_truss)
        src = edge_ids(off, adj)[0]
        ktruss = {int(ln[1]): [int(x) for x in ln[2:]] for ln in lines if ln[0] == "ktruss"}
        assert sorted(ktruss) == list(range(2, rec["max_truss"] + 1))
        for k, flat in ktruss.items():
            keep = (src < adj) & (truss >= k)
            assert flat == np.stack([src[keep], np.asarray(adj)[keep]], axis=1).reshape(-1).tolist(), k


def test_driver_truss(gpu):
    rec = TRUSS["kronecker_10_16"]
    r = subprocess.run([DRIVER, "truss", "-g", "kronecker", "10", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ truss decomposition") == 2 and "Average Time:" in out
    label = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in out.splitlines() if ":" in ln}
    assert int(label["Max Truss"]) == rec["max_truss"] and int(label["Levels"]) == rec["levels"] and int(label["Triangles"]) == rec["triangles"]
    csr = host_graph(gpu, "kronecker", 10, 16, True)  # what `-g kronecker 10` loads
    assert (csr.num_nodes, csr.num_edges) == (rec["n"], rec["m"])
    assert int(label["Rounds"]) == truss_np(csr.offsets(), csr.neighbors())[2] and label["Verification"] == "PASS" and "FAIL" not in out
    hist = {ln.split()[1].rstrip(":"): int(ln.split()[2]) for ln in out.splitlines() if ln.startswith("truss ")}
    assert hist == rec["hist"]
    r = subprocess.run([DRIVER, "truss", "-g", "kronecker", "8", "-n", "0"], capture_output=True, text=True, timeout=60)  # no trial: no histogram
    assert r.returncode == 0 and "Average Time:" in r.stdout and not any(ln.startswith("truss ") for ln in r.stdout.splitlines())
    assert subprocess.run([DRIVER, "truss", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
