"""GPU: the C++ adaptor of the core decomposition (gmsx::core_numbers / degeneracy_order / degree_order / order_quality,
include/gmsx_set_graph.hpp) through tests/cpp/test_core_adaptor.cpp, and `gmsx_driver bk --order adg|deg|dgr`."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_core_golden_cpu import ARR, CORE, later_np, peel_np, quality_np

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")
GRAPHS = load_golden("graphs.json")


def test_core_adaptor(gpu, tmp_path):
    exe = tmp_path / "core_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_core_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    keys = [k for k, r in CORE.items() if r["source"]["kind"] == "file"]
    assert len(keys) == 6
    for key in keys:
        rec = CORE[key]
        path = os.path.join(GOLDEN, "testGraphs", rec["source"]["name"])
        csr = gpu.HostCSR.load(path)
        off, adj = csr.offsets(), csr.neighbors()
        n = off.size - 1
        out = subprocess.run([str(exe), path], check=True, capture_output=True, text=True, timeout=120).stdout
        lines = {ln.split()[0] + (" " + ln.split()[1] if ln.startswith("quality") else ""): ln.split() for ln in out.splitlines()}
        want_core, rnd, rounds, levels = peel_np(off, adj)
        assert [int(x) for x in lines["degeneracy"][1::2]] == [rec["degeneracy"], levels, rounds, rec["top_core"]]
        core = np.array(lines["core"][1:], dtype=np.int64)
        assert np.array_equal(core, ARR["core_" + key]) and np.array_equal(core, want_core)
        order = np.array(lines["order"][1:], dtype=np.int64)
        assert np.array_equal(order, np.lexsort((np.arange(n), rnd)))
        degrank = np.array(lines["degrank"][1:], dtype=np.int64)
        assert np.array_equal(degrank, ARR["degrank_" + key])
        q = quality_np(later_np(off, adj, degrank), rec["degeneracy"], n)
        assert [int(x) for x in lines["quality degree"][2:]] == [q["max_later"], q["core_number"], q["faulty"], q["excess"]]
        assert [int(x) for x in lines["quality exact"][2:]] == [rec["degeneracy"], rec["degeneracy"], 0, 0]
        assert int(lines["quality adg"][2]) <= q["max_later"]


def run_driver(*args):
    return subprocess.run([DRIVER, *args], capture_output=True, text=True, timeout=300)


def test_driver_bk_order(gpu):
    want = GRAPHS["kronecker-10-16-relabel"]["bk"]
    outs = {}
    for order in ("deg", "dgr", "adg", None):
        extra = ["--order", order] if order else []
        r = run_driver("bk", "-g", "kronecker", "10", "-n", "2", "-v", *extra)
        assert r.returncode == 0, r.stderr
        assert f"The Number of maximal clique counted: {want}" in r.stdout, r.stdout
        assert r.stdout.count("Preprocess Time:") == 2 and r.stdout.count("Trial Time:") == 2
        marks = [ln for ln in r.stdout.splitlines() if ln.startswith("@@@ ")]
        assert len(marks) == 2 and all(" PASS " in ln for ln in marks), r.stdout
        outs[order] = r.stdout
    # without --order the driver prints what it always printed: the ADG run's lines, the times aside
    def strip(s):  # the "@@@" lines carry only times (and PASS, checked above)
        return re.sub(r"\d+\.\d+", "#", "\n".join(ln for ln in s.splitlines() if not ln.startswith("@@@ ")))
    assert strip(outs[None]) == strip(outs["adg"])
    assert strip(outs[None]) == strip(outs["deg"]) == strip(outs["dgr"])  # the label lines do not name the preprocessor


def test_driver_refuses_order_elsewhere(gpu):
    assert run_driver("tc", "-g", "kronecker", "8", "--order", "deg").returncode == 100
    assert run_driver("kclique", "-g", "kronecker", "8", "--order", "dgr").returncode == 100
    assert run_driver("bk", "-g", "kronecker", "8", "--order", "matula").returncode == 100
    assert run_driver("bk", "-g", "kronecker", "8", "--order").returncode == 100
