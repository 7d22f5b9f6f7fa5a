"""GPU: the C++ adaptors of the communities (gmsx::label_propagation / gmsx::modularity, include/gmsx_set_graph.hpp) through
tests/cpp/test_communities_adaptor.cpp, and `gmsx_driver communities [-i MAX_SWEEPS] [--weighted] -v`, against the golden records."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from test_communities_golden_cpu import J, coloring_of, fnv_of, graph_arrays, lp_np, mod_np

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")


def record(weighted, key, coloring="default"):
    return next(r for r in J["records"] if r["weighted"] == weighted and r["graph"] == key and r["coloring"] == coloring)


def line_of(info, fnv, mod):
    return [str(info[k]) for k in ("communities", "largest", "singletons", "changes", "sweeps", "colors", "converged")] + [
        str(fnv), str(mod["total_weight"]), str(mod["intra_weight"]), str(int(mod["sumsq"]) >> 64), str(int(mod["sumsq"]) & (2 ** 64 - 1)),
        str(mod["unstable"])]


def test_communities_adaptor(gpu, tmp_path):
    exe = tmp_path / "communities_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_communities_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    for key, args in (("file_two_parts_a", ["file", os.path.join(GOLDEN, "sssp", "two_parts_a.wel")]), ("kronecker_10_16", ["kron", "10"])):
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True, timeout=120).stdout
        lines = {ln.split()[1]: ln.split()[2:] for ln in out.splitlines() if ln.startswith("lp ")}
        assert sorted(lines) == ["u", "w"]
        rec = record(True, key)
        assert lines["w"] == line_of(rec, rec["fnv"], rec["mod"])
        # the same structure without its weights: the restatement
        off, adj, _ = graph_arrays(gpu, "w", key)
        label, info, _ = lp_np(off, adj, None, coloring_of(off, adj, "default"))
        assert lines["u"] == line_of(info, fnv_of(label), mod_np(off, adj, None, label))


def labels_of(out):
    return {ln.split(":")[0]: ln.split(":")[1].strip() for ln in out.splitlines() if ":" in ln}


def test_driver_communities(gpu):
    for extra, rec in (([], record(False, "kronecker_10_16")), (["--weighted"], record(True, "kronecker_10_16"))):
        r = subprocess.run([DRIVER, "communities", "-g", "kronecker", "10", "-n", "2", "-v"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout
        assert out.count("Trial Time:") == 2 and out.count("@@@ communities " + ("weighted" if extra else "unweighted")) == 2 and "Average Time:" in out
        assert out.count("Verification:") == 2 and "PASS" in out and "FAIL" not in out
        label = labels_of(out)
        assert (int(label["Communities"]), int(label["Sweeps"])) == (rec["communities"], rec["sweeps"])
        assert label["Modularity"] == "%.6f" % float.fromhex(rec["mod"]["modularity"])
    path = os.path.join(GOLDEN, "sssp", "two_parts_b.wel")
    rec = record(True, "file_two_parts_b")
    r = subprocess.run([DRIVER, "communities", "-f", path, "-n", "1", "-v", "--weighted"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout and "FAIL" not in r.stdout
    label = labels_of(r.stdout)
    assert (int(label["Communities"]), int(label["Sweeps"])) == (rec["communities"], rec["sweeps"])
    # a sweep cap: fewer sweeps, still the host's labels
    r = subprocess.run([DRIVER, "communities", "-f", path, "-n", "1", "-v", "--weighted", "-i", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS" in r.stdout and int(labels_of(r.stdout)["Sweeps"]) == 2
    # --weighted belongs to communities alone; communities are global
    assert subprocess.run([DRIVER, "cc", "-g", "kronecker", "8", "--weighted"], capture_output=True, text=True, timeout=60).returncode == 100
    assert subprocess.run([DRIVER, "communities", "-g", "kronecker", "8", "--gpus", "2"], capture_output=True, text=True, timeout=60).returncode == 100
