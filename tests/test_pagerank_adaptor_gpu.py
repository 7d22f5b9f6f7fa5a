"""GPU: the C++ adaptor of PageRank (gmsx::pagerank / pagerank_residual / top_scores, include/gmsx_set_graph.hpp) through
tests/cpp/test_pagerank_adaptor.cpp on tomitaExample.el and kronecker 10 against the goldens, and `gmsx_driver pr`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_pagerank_golden_cpu import ARR, GRAPHS, RECORDS, golden_csr, pagerank_np, record_bound, scalar_bound, top_five

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def golden(key, flags):
    return next(r for r in RECORDS if r["graph"] == key and r["flags"] == flags and r["teleport"] == "uniform" and r["tolerance"] == 1e-4)


def test_pagerank_adaptor(gpu, tmp_path):
    exe = tmp_path / "pagerank_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_pagerank_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    assert subprocess.run([str(exe), "--host"], capture_output=True, text=True, timeout=60).returncode == 0
    for key, args in (("file_tomitaExample", [os.path.join(GOLDEN, "testGraphs", "tomitaExample.el")]), ("kronecker_10_16", ["kronecker", "10"])):
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split() for ln in out.splitlines()]
        n = GRAPHS[key]["n"]
        for flags in (0, 1, 2):
            rec = golden(key, flags)
            run = next(ln for ln in lines if ln[0] == "run" and int(ln[1]) == flags)
            assert [int(x) for x in run[2:5]] == [rec["iterations"], rec["converged"], rec["argmax"]]
            scores = np.array([float.fromhex(x) for x in next(ln for ln in lines if ln[0] == "scores" and int(ln[1]) == flags)[2:]])
            bound = record_bound(rec)
            dist = float(np.abs(scores - ARR[rec["array"]]).sum())
            print(f"{key} flags {flags}: L1 distance {dist:.3e}, distance / bound {dist / bound:.3f}")
            assert scores.size == n and dist <= bound
            assert abs(float.fromhex(run[5]) - rec["error"]) <= scalar_bound(bound, n, rec["error"])
            assert abs(float.fromhex(run[6]) - rec["sum"]) <= scalar_bound(bound, n, rec["sum"])
            assert 0.0 <= float.fromhex(run[7]) < 1e-4   # PRVerifier's rule at the record's tolerance
            top = [kv.split(":") for kv in next(ln for ln in lines if ln[0] == "top" and int(ln[1]) == flags)[2:]]
            assert [int(t[0]) for t in top] == rec["top"] == top_five(scores) and [float.fromhex(t[1]) for t in top] == scores[rec["top"]].tolist()


def labels(out):
    return [tuple(x.strip() for x in ln.split(":", 1)) for ln in out.splitlines() if ":" in ln]


def test_driver_pr(gpu):
    rec = golden("kronecker_10_16", 0)
    want = ARR[rec["array"]]
    r = subprocess.run([DRIVER, "pr", "-g", "kronecker", "10", "-n", "2", "-v"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.count("Trial Time:") == 2 and out.count("@@@ pagerank") == 2 and "Average Time:" in out
    assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
    assert [int(v) for k, v in labels(out) if k == "Iterations"] == [rec["iterations"]] * 2
    assert float(next(v for k, v in labels(out) if k == "Error")) == pytest.approx(rec["error"], rel=1e-5)   # (six significant digits are printed)
    at = len(out.splitlines()) - 1 - out.splitlines()[::-1].index("@@@ pagerank")
    top = [ln.split(":") for ln in out.splitlines()[at + 1: at + 6]]
    assert [int(t[0]) for t in top] == rec["top"]
    assert np.allclose([float(t[1]) for t in top], want[rec["top"]], rtol=1e-5, atol=0)
    # -i and -t are the reference's: -t 0 runs every one of the -i sweeps, and a loose tolerance stops early
    short = next(x for x in RECORDS if x["graph"] == "kronecker_10_16" and x["tolerance"] == 0.0)
    r = subprocess.run([DRIVER, "pr", "-g", "kronecker", "10", "-n", "1", "-i", str(short["max_iters"]), "-t", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [int(v) for k, v in labels(r.stdout) if k == "Iterations"] == [short["max_iters"]]
    assert float(next(v for k, v in labels(r.stdout) if k == "Error")) == pytest.approx(short["error"], rel=1e-5)
    r = subprocess.run([DRIVER, "pr", "-g", "kronecker", "10", "-n", "1", "-t", "0.5"], capture_output=True, text=True, timeout=300)
    csr = golden_csr(gpu, "kronecker_10_16")
    loose = pagerank_np(np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int64), tolerance=0.5)[1]["iterations"]
    assert r.returncode == 0 and 1 <= loose < rec["iterations"] and [int(v) for k, v in labels(r.stdout) if k == "Iterations"] == [loose]
    # PageRank is global and has neither a source nor a metric nor a threshold
    for bad in (["--gpus", "2"], ["-r", "1"], ["--metric", "jaccard"], ["--threshold", "1"], ["-t", "-1"], ["-i", "0"]):
        assert subprocess.run([DRIVER, "pr", "-g", "kronecker", "8"] + bad, capture_output=True, text=True, timeout=60).returncode == 100, bad
    r = subprocess.run([DRIVER, "pr", "-g", "kronecker", "8", "-n", "0"], capture_output=True, text=True, timeout=60)   # no trial: no scores
    assert r.returncode == 0 and "Average Time:" in r.stdout and "@@@" not in r.stdout
