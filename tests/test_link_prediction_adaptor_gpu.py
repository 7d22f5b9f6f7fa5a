"""GPU: the C++ adaptor of link prediction (gmsx::link_prediction / link_prediction_shard / merge_link_predictions /
link_prediction_precision, include/gmsx_set_graph.hpp) through tests/cpp/test_link_prediction_adaptor.cpp — the padded result equals the
golden verbatim, the nothing-qualifies case, merge — and one `gmsx_driver lp --list` run parsed back."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_link_prediction_golden_cpu import LP, METRICS, RECORDS, check_against_record

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def parse_blocks(text):
    """[(metric, q, u, v, scores)] of the "R" / "E" lines, padding included"""
    out = []
    for ln in text.splitlines():
        t = ln.split()
        if t and t[0] == "R":
            out.append([int(t[1]), int(t[2]), [], [], [], int(t[3])])
        elif t and t[0] == "E":
            out[-1][2].append(int(t[1]))
            out[-1][3].append(int(t[2]))
            out[-1][4].append(float.fromhex(t[3]))
    for b in out:
        assert len(b[2]) == b[5]
    return [(b[0], b[1], np.array(b[2], np.int32), np.array(b[3], np.int32), np.array(b[4], np.float64)) for b in out]


def check_padded(rec, u, v, s):
    pad = rec["padding"]
    assert u.size == pad + rec["found"] == (rec["q"] if rec["found"] else 1)
    assert np.all(u[:pad] == 0) and np.all(v[:pad] == 0) and np.all(s[:pad] == -1.0)
    check_against_record(rec, (u[pad:], v[pad:], s[pad:]))


def test_link_prediction_adaptor(gpu, tmp_path):
    exe = tmp_path / "lp_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_link_prediction_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    keys = [k for k, r in LP["graphs"].items() if r["source"]["kind"] == "file"]
    assert len(keys) == 6
    seen_empty = False
    for key in keys:
        path = os.path.join(GOLDEN, "testGraphs", LP["graphs"][key]["source"]["name"])
        recs = [r for r in RECORDS if r["graph"] == key]
        args = ["%d:%d" % (METRICS.index(r["metric"]), r["q"]) for r in recs]
        out = subprocess.run([str(exe), path, *args], check=True, capture_output=True, text=True, timeout=120).stdout
        blocks = parse_blocks(out)
        assert len(blocks) == len(recs)
        for rec, (m, q, u, v, s) in zip(recs, blocks):
            assert (METRICS[m], q) == (rec["metric"], rec["q"])
            check_padded(rec, u, v, s)
            seen_empty |= rec["found"] == 0
        k5 = [ln.split() for ln in out.splitlines() if ln.startswith("K5 ")]
        assert len(k5) == 7 and all(t[2:5] == ["1", "0", "0"] and float.fromhex(t[5]) == -1.0 and t[6] == "0" for t in k5), k5
        p = [ln.split() for ln in out.splitlines() if ln.startswith("P ")][0]
        assert (int(p[1]), int(p[2]), float.fromhex(p[3]), float.fromhex(p[4])) == (10, 10, 10 / 11.0, 1.0)
    assert seen_empty  # a golden graph without a non-edge: one padded entry, verbatim


def test_driver_lp_list(gpu, tmp_path):
    path = os.path.join(GOLDEN, "testGraphs", "smallRandom1.el")
    recs = {(r["metric"], r["q"]): r for r in RECORDS if r["graph"] == "file_smallRandom1"}
    for metric, q in (("common", 7), ("jaccard", 100)):
        lst = tmp_path / ("lp_%s.txt" % metric)
        r = subprocess.run([DRIVER, "lp", "-f", path, "--metric", metric, "-q", str(q), "-n", "2", "-v", "--list", str(lst)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        rec = recs[(metric, q)]
        assert r.stdout.count("predicted links: %d of %d requested (%s)" % (rec["found"], q, metric)) == 2
        marks = [ln for ln in r.stdout.splitlines() if ln.startswith("@@@ ")]
        assert len(marks) == 2 and all(" PASS " in ln for ln in marks), r.stdout
        rows = [ln.split() for ln in open(lst).read().splitlines()]
        u, v = np.array([int(t[0]) for t in rows], np.int32), np.array([int(t[1]) for t in rows], np.int32)
        s = np.array([float.fromhex(t[2]) for t in rows], np.float64)
        check_padded(rec, u, v, s)
    assert subprocess.run([DRIVER, "lp", "-f", path, "--metric", "cosine", "-q", "3"], capture_output=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "tc", "-f", path, "--list", str(tmp_path / "x")], capture_output=True, timeout=60).returncode == 100
