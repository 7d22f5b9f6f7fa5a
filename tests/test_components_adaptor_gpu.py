"""GPU: the C++ adaptor of the components (gmsx::connected_components / jarvis_patrick / ktruss_components, include/gmsx_set_graph.hpp) through
tests/cpp/test_components_adaptor.cpp, and `gmsx_driver cc` / `gmsx_driver jp -v`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_components_golden_cpu import ARR, CC, JP, components_np, jarvis_patrick_np
from test_truss_golden_cpu import ARR as TRUSS_ARR
from test_truss_golden_cpu import TRUSS

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def test_components_adaptor(gpu, tmp_path):
    exe = tmp_path / "components_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_components_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    keys = [k for k, r in CC.items() if r["source"]["kind"] == "file"]
    assert len(keys) == 6
    for key in keys:
        rec = CC[key]
        path = os.path.join(GOLDEN, "testGraphs", rec["source"]["name"])
        csr = gpu.HostCSR.load(path)
        off, adj = csr.offsets(), csr.neighbors()
        max_k = TRUSS[key]["max_truss"] + 1   # one past the top truss: nothing is kept
        out = subprocess.run([str(exe), path, "4", "1", str(max_k)], check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split() for ln in out.splitlines()]
        cc = [int(x) for x in next(ln for ln in lines if ln[0] == "cc")[1:]]
        assert cc[0] == rec["components"] and np.array_equal(cc[1:], ARR["label_" + key])
        jp = [int(x) for x in next(ln for ln in lines if ln[0] == "jp")[1:]]
        want, info, _ = jarvis_patrick_np(off, adj, "common_neighbors", 1.0)
        assert jp[:2] == [info["components"], info["kept_edges"]] and np.array_equal(jp[2:], want)
        ktruss = {int(ln[1]): [int(x) for x in ln[2:]] for ln in lines if ln[0] == "ktruss"}
        assert sorted(ktruss) == list(range(2, max_k + 1))
        for k, got in ktruss.items():
            want, info = components_np(off, adj, (TRUSS_ARR["truss_" + key] >= k).astype(np.uint8))
            assert got[:2] == [info["components"], info["kept_edges"]] and np.array_equal(got[2:], want), k
        assert ktruss[max_k][:2] == [rec["n"], 0] and ktruss[2][0] == rec["components"]


def comp_stats(out):
    """(the 'label:size' lines, the component count) of PrintCompStats' output"""
    lines = out.splitlines()
    at = next(i for i, ln in enumerate(lines) if ln.endswith("biggest clusters"))
    k = int(lines[at].split()[0])
    return [tuple(int(x) for x in ln.split(":")) for ln in lines[at + 1: at + 1 + k]], int(lines[at + 1 + k].split()[2])


def top5(label):
    roots, sizes = np.unique(label, return_counts=True)
    order = np.lexsort((roots, -sizes))[:5]
    return [(int(roots[i]), int(sizes[i])) for i in order]


def test_driver_cc_and_jp(gpu):
    rec = CC["kronecker_10_16"]
    r = subprocess.run([DRIVER, "cc", "-g", "kronecker", "10", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ connected components") == 2 and "Average Time:" in out
    assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
    top, count = comp_stats(out)
    assert count == rec["components"] and top == top5(ARR["label_kronecker_10_16"]) and top[0] == (rec["largest_label"], rec["largest"])
    jrec = next(j for j in JP if (j["graph"], j["metric"], float.fromhex(j["threshold"])) == ("kronecker_10_16", "common_neighbors", 2.0))
    r = subprocess.run([DRIVER, "jp", "-g", "kronecker", "10", "-n", "1", "-v", "--metric", "common", "--threshold", "2"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("@@@ jarvis-patrick common 2") == 1 and "PASS" in out and "FAIL" not in out
    label = {ln.split(":")[0]: ln.split(":")[1].strip() for ln in out.splitlines() if ":" in ln}
    assert int(label["Kept Edges"]) == jrec["kept_edges"] and int(label["Components"]) == jrec["components"]
    top, count = comp_stats(out)
    assert count == jrec["components"] and top == top5(ARR[jrec["array"]])
    # the threshold is required for jp and refused elsewhere; a component is global
    assert subprocess.run([DRIVER, "jp", "-g", "kronecker", "8"], capture_output=True, text=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "cc", "-g", "kronecker", "8", "--threshold", "1"], capture_output=True, text=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "cc", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
    r = subprocess.run([DRIVER, "cc", "-g", "kronecker", "8", "-n", "0"], capture_output=True, text=True, timeout=60)  # no trial: no statistics
    assert r.returncode == 0 and "Average Time:" in r.stdout and "biggest clusters" not in r.stdout
