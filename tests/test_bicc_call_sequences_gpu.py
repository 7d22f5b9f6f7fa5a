"""GPU: gmsx_biconnected_components between other calls on ONE handle — bicc, gmsx_connected_components, bicc, gmsx_bfs, bicc.  The call keeps
its state in buffers of its own and does not modify the handle: the three results are the same bytes, and the calls between them still give
their own goldens (tests/golden/components.json, traversal.json)."""
import numpy as np
import pytest

from test_bicc_golden_cpu import INFO_KEYS, J, golden_bicc
from test_components_golden_cpu import CC
from test_components_golden_cpu import golden_csr as cc_golden_csr
from test_components_golden_cpu import sha as cc_sha
from test_traversal_golden_cpu import BFS
from test_traversal_golden_cpu import INFO_KEYS as BFS_KEYS
from test_traversal_golden_cpu import sha as bfs_sha

pytestmark = pytest.mark.gpu

GRAPH = "kronecker_10_16_raw"   # of components.json and traversal.json: the unrelabelled kronecker_10_16 of bicc.json


def test_bicc_between_components_and_bfs(gpu):
    g = gpu.DeviceGraph.from_csr(cc_golden_csr(gpu, GRAPH))
    want = golden_bicc(gpu, "kronecker_10_16")
    rec = next(r for r in J["records"] if r["graph"] == "kronecker_10_16")
    before = g.device_bytes

    def bicc():
        block, at, keep, info = g.biconnected_components(want_mask=True)
        assert info == want[3] == {k: rec[k] for k in INFO_KEYS}
        assert (block.tobytes(), at.tobytes(), keep.tobytes()) == (want[0].tobytes(), want[1].tobytes(), want[2].tobytes())
        assert g.device_bytes == before

    bicc()
    label, info = g.connected_components()
    assert cc_sha(label) == CC[GRAPH]["label_sha256"] and info["components"] == CC[GRAPH]["components"] == rec["components"]
    bicc()
    b = next(r for r in BFS if r["graph"] == GRAPH and r["kind"] == "hub")
    depth, parent, info = g.bfs(b["source"])
    assert bfs_sha(depth) == b["depth_sha256"] and bfs_sha(parent) == b["parent_sha256"] and {k: info[k] for k in BFS_KEYS} == {k: b[k] for k in BFS_KEYS}
    bicc()
    g.free()
