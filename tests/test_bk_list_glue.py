"""CPU tests of the opt-in listing route of include/gmsx_gms_glue.hpp (GMSX_GLUE_BK_LIST): compiled against the reference tree, it
specialises BkEppsteinPar::mceBench<HipSetGraph / HipRoaringGraph> in a listing build (-DMINEBENCH_TEST) to return the device's list; without
the macro the listing build keeps the reference's host template.  Skips without the reference tree."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def _build(tmp_path, defs, name):
    from oracle.ref_drivers import LIBDIR, REF
    if not os.path.isdir(os.path.join(REF, "gms")):
        pytest.skip("reference tree not present")
    roaring = os.path.join(ROOT, "oracle", "_ref", "roaring.o")
    if not os.path.exists(roaring):
        pytest.skip("oracle/_ref/roaring.o not built")
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-march=x86-64-v3", "-fopenmp", "-w", "-DNOPAPIW"] + defs +
                   ["-I", os.path.join(ROOT, "include"), "-I", REF, os.path.join(ROOT, "tests", "cpp", "test_glue_bk_list.cpp"), roaring,
                    "-L", LIBDIR, "-lgmsx", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("count", [False, True])
def test_glue_bk_list_routed_fails_loudly_without_device(tmp_path, count):
    defs = ["-DMINEBENCH_TEST", "-DGMSX_GLUE_BK_LIST", "-DEXPECT_ROUTED=1"] + (["-DBK_COUNT"] if count else [])
    exe = _build(tmp_path, defs, "glue_bk_list")  # the static_assert pins GMSX_GLUE_BK_LIST_ROUTED == 1
    if _have_gpu():
        pytest.skip("a device is present: the routed binary is run by the GPU tests' adaptor checks instead")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0, r.stdout[-2000:]
    assert "no HIP device" in (r.stdout + r.stderr), r.stdout[-2000:] + r.stderr[-2000:]
    assert "listed" not in r.stdout  # never an (empty) list


@pytest.mark.parametrize("count", [False, True])
def test_glue_bk_list_not_routed_without_opt_in(tmp_path, count):
    defs = ["-DMINEBENCH_TEST", "-DEXPECT_ROUTED=0"] + (["-DBK_COUNT"] if count else [])
    exe = _build(tmp_path, defs, "glue_bk_host")  # the static_assert pins GMSX_GLUE_BK_LIST_ROUTED == 0
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "routed 0 listed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
