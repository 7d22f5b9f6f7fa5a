"""GPU: the C++ adaptor of the colouring (gmsx::coloring / coloring_order / coloring_check, include/gmsx_set_graph.hpp) through
tests/cpp/test_coloring_adaptor.cpp on kronecker 10 against the goldens, and `gmsx_driver color`."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_coloring_golden_cpu import COL, COL_ARR, golden_rank
from test_core_golden_cpu import CORE

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")
KEY = "kronecker_10_16"


def test_coloring_adaptor(gpu, tmp_path):
    exe = tmp_path / "coloring_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_coloring_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    files = []
    for order in ("matula", "random"):
        path = tmp_path / (order + ".bin")
        golden_rank(KEY, order).astype("<i4").tofile(path)
        files.append(str(path))
    out = subprocess.run([str(exe), "10", *files], check=True, capture_output=True, text=True, timeout=120).stdout
    lines = {" ".join(ln.split()[:2]): ln.split()[2:] for ln in out.splitlines()}
    rec = COL[KEY]["orders"]
    max_degree = None
    for tag, order in (("file0", "matula"), ("file1", "random"), ("id", "id"), ("ff", "ff"), ("lf", "degree")):
        want = COL_ARR["color_%s_%s" % (order, KEY)]
        assert np.array_equal(np.array(lines["color " + tag], dtype=np.int64), want), tag
        assert [int(x) for x in lines["info " + tag]] == [rec[order][f] for f in ("colors", "rounds", "max_pred", "first_round")], tag
        chk = [int(x) for x in lines["check " + tag]]
        assert chk[:4] == [0, 0, rec[order]["colors"], rec[order]["colors"]], tag
        max_degree = chk[4]
    assert max_degree >= rec["id"]["max_pred"]
    degeneracy = CORE[KEY]["degeneracy"]
    sl = [int(x) for x in lines["info sl"]]
    assert sl[0] <= degeneracy + 1 and sl[2] == degeneracy and [int(x) for x in lines["check sl"]][:4] == [0, 0, sl[0], sl[0]]
    adg = [int(x) for x in lines["info adg"]]
    assert adg[0] <= adg[2] + 1 and [int(x) for x in lines["check adg"]][:4] == [0, 0, adg[0], adg[0]]


def run_driver(*args):
    return subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=300)


def labels(stdout, label):
    return [ln.split(":", 1)[1].strip() for ln in stdout.splitlines() if ln.startswith(label + ":")]


def test_driver_color(gpu):
    want = COL[KEY]["orders"]["id"]["colors"]  # what the reference's JonesV3 gives on this CSR under getSimpleIdOrdering
    r = run_driver("color", "-g", "kronecker", "10", "--deg", "16", "--order", "id", "-v", "-n", "2")
    assert r.returncode == 0, r.stderr
    assert labels(r.stdout, "Colors") == [str(want)] * 2 and labels(r.stdout, "Verification") == ["PASS"] * 2, r.stdout
    assert len(labels(r.stdout, "Preprocess Time")) == 2 and len(labels(r.stdout, "Trial Time")) == 2
    assert len(labels(r.stdout, "Average Time")) == 1 and len(labels(r.stdout, "Average pp Time")) == 1
    assert float(labels(r.stdout, "Average colors")[0]) == float(want)
    default = run_driver("color", "-g", "kronecker", "10", "-n", "1")  # --order defaults to id, the reference's
    assert default.returncode == 0 and labels(default.stdout, "Colors") == [str(want)] and not labels(default.stdout, "Verification")
    for order, golden in (("ff", "ff"), ("lf", "degree")):
        r = run_driver("color", "-g", "kronecker", "10", "--order", order, "-v", "-n", "1")
        assert r.returncode == 0 and labels(r.stdout, "Colors") == [str(COL[KEY]["orders"][golden]["colors"])] and labels(r.stdout, "Verification") == ["PASS"]
    for order in ("sl", "adg"):
        r = run_driver("color", "-g", "kronecker", "10", "--order", order, "--eps", "0.001", "-v", "-n", "1")
        assert r.returncode == 0 and labels(r.stdout, "Verification") == ["PASS"], r.stdout
        assert int(labels(r.stdout, "Colors")[0]) <= (CORE[KEY]["degeneracy"] + 1 if order == "sl" else COL[KEY]["orders"]["degree"]["max_pred"] + 1)


def test_driver_color_refusals(gpu):
    assert run_driver("color", "-g", "kronecker", "8", "--gpus", "2").returncode == 100  # a colouring is global: single process only
    assert run_driver("color", "-g", "kronecker", "8", "--order", "dgr").returncode == 100
    assert run_driver("color", "-g", "kronecker", "8", "--order").returncode == 100
    assert run_driver("tc", "-g", "kronecker", "8", "--order", "sl").returncode == 100
    assert run_driver("bk", "-g", "kronecker", "8", "--order", "lf").returncode == 100
