"""GPU: the C++ adaptor of subgraph matching (gmsx::subgraph_isomorphism — the reference's Result::isomorphism shape, target -> pattern — and
gmsx::subgraph_isomorphisms, include/gmsx_set_graph.hpp) through tests/cpp/test_subgraph_adaptor.cpp, against the goldens."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu
GOLD = load_golden("subgraph.json")
NAMES = ["K2", "K3", "P4_r1", "claw", "C5", "house_r2", "K5"]


def test_subgraph_adaptor(gpu, tmp_path):
    exe = tmp_path / "subgraph_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_subgraph_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    files = []
    for name in NAMES:
        files.append(str(tmp_path / (name + ".el")))
        with open(files[-1], "w") as f:
            f.write("".join(f"{a} {b}\n" for a, b in GOLD["patterns"][name]))
    keys = [k for k, s in GOLD["graphs"].items() if s["kind"] == "file" and s["n"] >= 5]
    assert len(keys) == 4
    found = 0
    for key in keys:
        path = os.path.join(GOLDEN, "testGraphs", GOLD["graphs"][key]["name"])
        out = subprocess.run([str(exe), path] + files, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = [ln.split() for ln in out.splitlines()]
        for i, name in enumerate(NAMES):
            rec = next(r for r in GOLD["records"] if r["graph"] == key and r["pattern"] == name)
            iso = next(ln for ln in lines if ln[0] == "iso" and int(ln[1]) == i)[2:]
            got = {int(x.split(":")[0]): int(x.split(":")[1]) for x in iso}
            assert got == ({} if rec["ref"] is None else {t: p for p, t in enumerate(rec["ref"])}), (key, name)
            assert [int(x.split(":")[0]) for x in iso] == sorted(got)
            found += bool(got)
            for mode in ("induced", "mono"):
                ln = next(ln for ln in lines if ln[0] == mode and int(ln[1]) == i)
                k = int(ln[2])
                rows = np.array(ln[3:], dtype=np.int32).reshape(-1, k)
                assert rows.shape[0] == rec[mode]["count"], (key, name, mode)
                assert hashlib.sha256(np.ascontiguousarray(rows, dtype="<i4").tobytes()).hexdigest() == rec[mode]["sha256"]
    assert found >= 10
