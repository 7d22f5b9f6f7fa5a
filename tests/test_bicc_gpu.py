"""GPU: gmsx_biconnected_components through the C-ABI against the goldens (tests/golden/bicc.{json,npz}) and the restatement of
tests/test_bicc_golden_cpu.py (bicc_np).  All results are integers: every comparison is exact.

  goldens       every record: block, blocks_at, arc_keep and info; want_* all False gives the same info
  deep forest   a path of 4096: 4095 bridges, levels 4096, the same bytes under BCC_WG_LEVEL 0 and the default, and under the default no more
                launches than on a path of 512 (+ 8: the flatten rounds of the two union-finds)
  cycle         a 4096-cycle: one block; a single non-tree edge closes it
  hub           stars with 1 500 and 40 000 leaves at both ends of BCC_WAVE_ROW / BCC_WG_ROW: all bridges, the centre in every block
  windmill      500 triangles sharing vertex 0: rule (i) alone joins the sibling subtrees
  dense         K_64 and the 64 x 64 grid: one block each
  clique chain  K_5's alternately sharing a vertex and joined by a bridge; a vertex in three blocks
  root cases    P3 with the middle vertex as id 0; a triangle with a pendant on a non-root
  many roots    the disjoint union of 200 seeded random graphs under a seeded permutation of all ids
  renumbering   kronecker 12 under a seeded permutation
  extremes      n = 1; edgeless with n = 5; two components plus isolated vertices
  consistency   arc_keep into gmsx_connected_components gives components + bridges; the three identities on every graph above
  same bytes    on the many-roots graph and kronecker 12: three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, a second
                handle, every corner of the four options: one tobytes() value for each output
  contract      NULL info, unknown flag bits: ERR_INVALID, arrays untouched"""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_bicc_golden_cpu import (ARR, ARRAY_MAX_N, INFO_KEYS, J, MANY_ROOTS, bicc_np, clique_chain_edges, clique_edges, cycle_edges, golden_arrays,
                                  golden_bicc, golden_csr, grid_edges, identities_hold, many_roots_edges, p3_middle_root, path_edges, permuted, sha,
                                  star_edges, triangle_with_pendant, two_components_and_isolated, windmill_edges)
from test_components_golden_cpu import csr_of

pytestmark = pytest.mark.gpu

HUGE = 2 ** 31 - 1
BINS = ((1, 1), (1, HUGE), (HUGE, HUGE))   # BCC_WAVE_ROW, BCC_WG_ROW: every row a workgroup's / a wave's / a lane's or a group's


def check(gpu, g, off, adj, want=None):
    """every output of one call against the restatement, the identities, and arc_keep through gmsx_connected_components; returns
    (block, blocks_at, arc_keep, info, stats)"""
    block, at, keep, info, st = g.biconnected_components(want_mask=True, stats=True)
    wb, wa, wk, wi = want or bicc_np(off, adj)
    assert info == wi
    assert np.array_equal(block, wb) and np.array_equal(at, wa) and np.array_equal(keep, wk)
    assert identities_hold(off, adj, block, at, keep, info)
    if len(adj):
        assert g.connected_components(arc_keep=keep)[1]["components"] == info["components"] + info["bridges"]
    assert st["units"] == info["blocks"] and st["probes"] == info["levels"] and (st["launches"] >= 20) == (len(adj) > 0)
    return block, at, keep, info, st


def shape_graph(gpu, edges_n):
    off, adj = csr_of(*edges_n)
    return gpu.DeviceGraph.upload(off, adj), off, adj


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", J["records"], ids=lambda r: r["graph"])
def test_bicc_equals_the_golden(gpu, rec):
    key = rec["graph"]
    off, adj = golden_arrays(gpu, key)
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    block, at, keep, info, st = check(gpu, g, off, adj, want=golden_bicc(gpu, key))
    assert info == {k: rec[k] for k in INFO_KEYS} and sha(block) == rec["sha256_block"] and sha(at) == rec["sha256_blocks_at"]
    if off.size - 1 <= ARRAY_MAX_N:
        assert np.array_equal(block, ARR["block_" + key]) and np.array_equal(at, ARR["blocks_at_" + key])
    none = g.biconnected_components(want_block=False, want_blocks_at=False)
    assert none[:3] == (None, None, None) and none[3] == info
    g.free()


# ---- 2. deep forest -------------------------------------------------------------------------------------------------------------------
def test_deep_forest(gpu):
    g, off, adj = shape_graph(gpu, path_edges(4096))
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert (info["blocks"], info["bridges"], info["levels"]) == (4095, 4095, 4096) and np.all(at[1:-1] == 2) and not keep.any()
    with gpu.options(BCC_WG_LEVEL=0):
        b0, a0, k0, i0, s0 = g.biconnected_components(want_mask=True, stats=True)
    assert (b0.tobytes(), a0.tobytes(), k0.tobytes(), i0) == (block.tobytes(), at.tobytes(), keep.tobytes(), info)
    assert s0["launches"] > st["launches"] + 3 * 4000   # every level of the three sweeps a launch of its own
    g.free()
    g, off, adj = shape_graph(gpu, path_edges(512))
    short = check(gpu, g, off, adj)[4]
    assert st["launches"] <= short["launches"] + 8   # independent of the depth
    g.free()


# ---- 3. cycle -------------------------------------------------------------------------------------------------------------------------
def test_cycle(gpu):
    g, off, adj = shape_graph(gpu, cycle_edges(4096))
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert (info["blocks"], info["bridges"], info["articulation_points"], info["largest_block_vertices"]) == (1, 0, 0, 4096) and keep.all()
    g.free()


# ---- 4. hub ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1500, 40000])
def test_hub(gpu, leaves):
    g, off, adj = shape_graph(gpu, star_edges(leaves))
    want = bicc_np(off, adj)
    for wave_row, wg_row in BINS:
        with gpu.options(BCC_WAVE_ROW=wave_row, BCC_WG_ROW=wg_row):
            block, at, keep, info, st = check(gpu, g, off, adj, want=want)
        assert (info["blocks"], info["bridges"], info["max_blocks_at"], int(at[0])) == (leaves, leaves, leaves, leaves)
    g.free()


# ---- 5. windmill, dense, clique chain, root cases ---------------------------------------------------------------------------------------
def test_windmill(gpu):
    g, off, adj = shape_graph(gpu, windmill_edges(500))
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert (info["blocks"], info["bridges"], int(at[0]), info["articulation_points"]) == (500, 0, 500, 1)
    g.free()


def test_dense(gpu):
    for edges_n, edges in (((clique_edges(64), 64), 2016), (grid_edges(64), 2 * 64 * 63)):
        g, off, adj = shape_graph(gpu, edges_n)
        info = check(gpu, g, off, adj)[3]
        assert (info["blocks"], info["largest_block_edges"], info["articulation_points"]) == (1, edges, 0)
        g.free()


def test_clique_chain(gpu):
    g, off, adj = shape_graph(gpu, clique_chain_edges(6))
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert (info["blocks"], info["bridges"], info["largest_block"]) == (8, 2, 0) and [int(at[v]) for v in (4, 8, 9, 13)] == [2, 2, 2, 2]
    g.free()
    e = np.concatenate([clique_edges(5, 0), clique_edges(5, 4), np.array([(4, 9)], dtype=np.int64)])   # vertex 4 in two K_5's and a bridge
    g, off, adj = shape_graph(gpu, (e, 10))
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert int(at[4]) == 3 and info["max_blocks_at"] == 3
    g.free()


def test_root_cases(gpu):
    g, off, adj = shape_graph(gpu, p3_middle_root())
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert at.tolist() == [2, 1, 1] and block.tolist() == [0, 1, 0, 1]
    g.free()
    g, off, adj = shape_graph(gpu, triangle_with_pendant())
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert at.tolist() == [1, 1, 2, 1] and keep.tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    g.free()


# ---- 6. many roots, renumbering, extremes -----------------------------------------------------------------------------------------------
_MANY = {}


def many_roots(gpu):
    if not _MANY:
        off, adj = csr_of(*many_roots_edges())
        _MANY["g"] = (off, adj, bicc_np(off, adj))
    return _MANY["g"]


def test_many_roots(gpu):
    off, adj, want = many_roots(gpu)
    g = gpu.DeviceGraph.upload(off, adj)
    info = check(gpu, g, off, adj, want=want)[3]
    assert dict({k: info[k] for k in MANY_ROOTS if k != "n"}, n=off.size - 1) == MANY_ROOTS
    g.free()


def test_renumbering(gpu):
    off, adj = permuted(*golden_arrays(gpu, "kronecker_12_16"), seed=12)
    g = gpu.DeviceGraph.upload(off, adj)
    info = check(gpu, g, off, adj)[3]
    rec = next(r for r in J["records"] if r["graph"] == "kronecker_12_16")
    for k in ("blocks", "bridges", "articulation_points", "largest_block_edges", "largest_block_vertices", "components", "isolated", "max_blocks_at"):
        assert info[k] == rec[k], k   # (what a renumbering keeps)
    g.free()


def test_extremes(gpu):
    zeros = dict.fromkeys(INFO_KEYS, 0)
    g = gpu.DeviceGraph.upload(np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32))
    block, at, keep, info, st = g.biconnected_components(want_mask=True, stats=True)
    assert info == dict(zeros, components=1, isolated=1) and at.tolist() == [0] and block.size == 0 and keep.size == 0 and st["launches"] == 0
    g.free()
    g = gpu.DeviceGraph.upload(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32))
    block, at, keep, info = g.biconnected_components(want_mask=True)
    assert info == dict(zeros, components=5, isolated=5) and at.tolist() == [0] * 5
    g.free()
    g, off, adj = shape_graph(gpu, two_components_and_isolated())
    block, at, keep, info, st = check(gpu, g, off, adj)
    assert (info["components"], info["isolated"], info["blocks"], info["bridges"]) == (5, 3, 3, 1) and int(at[4]) == 2 and int(at[0]) == 0
    g.free()


# ---- 7. same bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["many_roots", "kronecker_12_16"])
def test_same_bytes(gpu, which):
    if which == "many_roots":
        off, adj, want = many_roots(gpu)
        csr = gpu.HostCSR.from_arrays(off, adj)
    else:
        csr, want = golden_csr(gpu, which), golden_bicc(gpu, which)
    wanted = (want[0].tobytes(), want[1].tobytes(), want[2].tobytes(), want[3])

    def same(r):
        assert (r[0].tobytes(), r[1].tobytes(), r[2].tobytes(), r[3]) == wanted

    base = gpu.DeviceGraph.from_csr(csr)
    for _ in range(3):
        same(base.biconnected_components(want_mask=True))
    for flags, shard in ((gpu.UPLOAD_TRUSTED, None), (64 << 8, None), (0, (1, 2)), (0, None)):
        g = gpu.DeviceGraph.from_csr(csr, flags, shard=shard)
        same(g.biconnected_components(want_mask=True))
        g.free()
    for (wave_row, wg_row), wg_frontier, wg_level in itertools.product(BINS, (0, HUGE), (0, HUGE)):
        with gpu.options(BCC_WAVE_ROW=wave_row, BCC_WG_ROW=wg_row, BCC_WG_FRONTIER=wg_frontier, BCC_WG_LEVEL=wg_level):
            same(base.biconnected_components(want_mask=True))
    base.free()


# ---- 8. contract --------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    g, off, adj = shape_graph(gpu, triangle_with_pendant())
    L = gpu.lib()
    block, at, keep = np.full(8, 77, dtype=np.int32), np.full(4, 77, dtype=np.int32), np.full(8, 77, dtype=np.uint8)
    pb, pa, pk = (a.ctypes.data_as(C.c_void_p) for a in (block, at, keep))
    info = gpu.BiccInfo()

    def untouched():
        return bool(np.all(block == 77) and np.all(at == 77) and np.all(keep == 77))

    before = g.device_bytes
    for flags in (1, 2, 1 << 31):
        assert L.gmsx_biconnected_components(g._h, flags, pb, pa, pk, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_biconnected_components(g._h, 0, pb, pa, pk, None, None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_biconnected_components(None, 0, pb, pa, pk, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_biconnected_components(g._h, 0, pb, pa, pk, C.byref(info), None) == gpu.OK and not untouched()
    assert (info.blocks, info.bridges, info.articulation_points) == (2, 1, 1) and block.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    assert g.device_bytes == before
    g.free()
