"""GPU: gmsx_edge_support and gmsx_truss_decomposition through the C-ABI, bit for bit against the goldens of this project's serial bucket peel
(tests/golden/truss.{json,npz}) and the numpy restatement of the level-synchronous peel kept in tests/test_truss_golden_cpu.py:

  goldens     arrays or sha256 plus info up to kronecker 14; round_of, rounds and levels against truss_np up to kronecker 12; edge_support against
              gmsx_intersect_count_batch on the same arcs; Σ support / 3 against gmsx_tc_total
  shapes      no vertex, isolated vertices, one edge, triangle, K5, C6, two K5 sharing an edge, the square of a path, K6 plus a strip, the
              triangulated cylinder of 501 rounds at both ends of TRUSS_WG_FRONTIER, the book graph above the parking and the hand-back bound,
              a seeded G(300, 4000) with a planted K14 (37 rounds, 29 of them in one level)
  no cliffs   kronecker 16 against its golden sha256; the k-truss re-uploaded as a graph keeps every edge at >= k on the device itself
  same bytes  a second call, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, the un-relabelled graph
  contract    NULL info and NULL support are GMSX_ERR_INVALID and write nothing; stats.units == m, stats.probes == rounds"""
import ctypes as C

import numpy as np
import pytest

from conftest import edges_to_csr, host_graph
from test_truss_golden_cpu import (ARR, PLANTED, SHAPES, TRUSS, edge_ids, golden_csr, info_of, k6_plus_strip, planted, rounds_per_level, sha, truss_np)

pytestmark = pytest.mark.gpu
KEYS = sorted(k for k in TRUSS if TRUSS[k]["m"] <= 250000)          # up to kronecker 14 (kronecker 16 has its own test below)
NP_KEYS = sorted(k for k in TRUSS if TRUSS[k]["m"] <= 70000)        # up to kronecker 12: the restatement's triangle list stays small
WG_ALL, WG_NONE = 2 ** 31 - 1, 0
_NP = {}


def restated(key, off, adj):
    """truss_np of a golden graph, computed once and shared"""
    if key not in _NP:
        _NP[key] = truss_np(off, adj)
    return _NP[key]


def check_against_restatement(g, off, adj, want=None):
    """truss, round_of, info, support and stats of one device graph against truss_np; returns (truss, round_of, info)"""
    want_truss, want_rnd, rounds, levels, want_sup = want if want is not None else truss_np(off, adj)
    src = edge_ids(off, adj)[0]
    truss, rnd, info, st = g.truss_decomposition(rounds=True, stats=True)
    sup, tri = g.edge_support()
    assert np.array_equal(sup, want_sup) and np.array_equal(truss, want_truss) and np.array_equal(rnd, want_rnd)
    want_info = dict(info_of(want_truss, want_sup, src, adj), rounds=rounds, levels=levels)
    assert info == want_info and tri == want_info["triangles"]
    assert st["units"] == adj.size // 2 and st["probes"] == rounds and (adj.size == 0 or st["launches"] >= 3)
    only, info2 = g.truss_decomposition()
    assert np.array_equal(only, truss) and info2 == info
    return truss, rnd, info


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_truss_equals_the_golden(gpu, key):
    rec, csr = TRUSS[key], golden_csr(gpu, key)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    truss, info, st = g.truss_decomposition(stats=True)
    sup, tri = g.edge_support()
    assert sha(truss) == rec["truss_sha256"] and sha(sup) == rec["support_sha256"]
    if rec["literal"]:
        assert np.array_equal(truss, ARR["truss_" + key]) and np.array_equal(sup, ARR["support_" + key])
    for f in ("max_truss", "levels", "top_edges", "max_support", "triangles"):
        assert info[f] == rec[f], f
    assert tri == rec["triangles"] == g.tc_total()                    # Σ support / 3
    assert st["units"] == rec["m"] and st["probes"] == info["rounds"] >= info["levels"]
    src = edge_ids(off, adj)[0]
    up = src < adj
    assert {str(int(v)): int(c) for v, c in zip(*np.unique(truss[up], return_counts=True))} == rec["hist"]
    # the same numbers by today's route: one intersect_count per arc
    assert np.array_equal(g.intersect_count_batch(src.astype(np.int32), adj).astype(np.int32), sup)
    if key in NP_KEYS:
        check_against_restatement(g, off, adj, restated(key, off, adj))
    g.free()


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------------------
def test_graph_without_vertices_and_without_edges(gpu):
    zero = {"max_truss": 0, "levels": 0, "rounds": 0, "max_support": 0, "top_edges": 0, "triangles": 0}
    for csr in (gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)), edges_to_csr(gpu, [], n=5)):
        g = gpu.DeviceGraph.from_csr(csr)
        truss, rnd, info, st = g.truss_decomposition(rounds=True, stats=True)
        sup, tri = g.edge_support()
        assert truss.size == rnd.size == sup.size == 0 and info == zero and tri == 0 and st["units"] == 0 and st["probes"] == 0
        g.free()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(gpu, name):
    edges, n, hist, rounds, levels = SHAPES[name]
    csr = edges_to_csr(gpu, edges, n=n)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    truss, rnd, info = check_against_restatement(g, off, adj)
    src = edge_ids(off, adj)[0]
    up = src < adj
    assert {int(v): int(c) for v, c in zip(*np.unique(truss[up], return_counts=True))} == hist
    assert info["levels"] == levels and (rounds is None or info["rounds"] == rounds) and info["max_truss"] == max(hist)
    if name == "book of 1500 with a K6":
        assert info["max_support"] == 1504 and truss[(src == 0) & (adj == 1)].tolist() == [6]
    for wg in (WG_NONE, WG_ALL):
        with gpu.options(TRUSS_WG_FRONTIER=wg):
            t2, r2, i2 = g.truss_decomposition(rounds=True)
        assert t2.tobytes() == truss.tobytes() and r2.tobytes() == rnd.tobytes() and i2 == info, wg
    g.free()


def test_k6_plus_strip(gpu):
    e = k6_plus_strip()
    csr = edges_to_csr(gpu, e)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    truss, rnd, info = check_against_restatement(g, off, adj)
    up = edge_ids(off, adj)[0] < adj
    assert {int(v): int(c) for v, c in zip(*np.unique(truss[up], return_counts=True))} == {3: 40, 6: 15} and info["levels"] == 2
    assert info["max_truss"] == 6 and info["top_edges"] == 15
    g.free()


def test_planted_clique_in_a_random_graph(gpu):
    csr = edges_to_csr(gpu, planted(), n=300)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    truss, rnd, info = check_against_restatement(g, off, adj)
    assert {k: info[k] for k in ("rounds", "levels", "max_truss", "top_edges")} == {k: PLANTED[k] for k in ("rounds", "levels", "max_truss", "top_edges")}
    assert max(rounds_per_level(truss, rnd).values()) == PLANTED["most_rounds_in_a_level"]  # 29 of the 37 rounds in one level
    for wg in (WG_NONE, WG_ALL, 3):
        with gpu.options(TRUSS_WG_FRONTIER=wg):
            t2, r2, i2 = g.truss_decomposition(rounds=True)
        assert t2.tobytes() == truss.tobytes() and r2.tobytes() == rnd.tobytes() and i2 == info, wg
    g.free()


# ---- 3. no cliffs ---------------------------------------------------------------------------------------------------------------------
def subgraph(gpu, src, adj, keep, n):
    """the undirected edges `keep` (a mask over the arcs) as a host CSR on the same vertex ids"""
    return gpu.HostCSR.from_edges(src[keep].astype(np.int32), np.asarray(adj)[keep].astype(np.int32), num_nodes=n)


def test_kronecker_16_and_its_trusses_on_the_device(gpu):
    rec = TRUSS["kronecker_16_16"]
    csr = golden_csr(gpu, "kronecker_16_16")
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    truss, info = g.truss_decomposition()
    sup, tri = g.edge_support()
    assert sha(truss) == rec["truss_sha256"] and sha(sup) == rec["support_sha256"] and tri == rec["triangles"] == g.tc_total()
    for f in ("max_truss", "levels", "top_edges", "max_support", "triangles"):
        assert info[f] == rec[f], f
    src = edge_ids(off, adj)[0]
    for k in (info["max_truss"], (info["max_truss"] + 2) // 2):  # the top truss and one in the middle
        u, v = g.ktruss_edges(k, truss=truss)                      # the CSR the graph was uploaded from, still held here
        u2, v2 = g.ktruss_edges(k, off, adj, truss=truss)
        assert np.array_equal(u, u2) and np.array_equal(v, v2)
        keep = (src < adj) & (truss >= k)
        assert np.array_equal(u, src[keep]) and np.array_equal(v, np.asarray(adj)[keep]) and u.size > 0
        sub = subgraph(gpu, src, adj, keep, off.size - 1)
        h = gpu.DeviceGraph.from_csr(sub)
        s2, _ = h.edge_support()
        t2, i2 = h.truss_decomposition()
        assert s2.size == 2 * u.size and s2.min() >= k - 2 and t2.min() >= k
        if k == info["max_truss"]:
            assert np.all(t2 == k) and i2["levels"] == 1 and i2["top_edges"] == rec["top_edges"]
        h.free()
    g.free()


# ---- 4. same bytes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["kronecker_12_16", "kronecker_10_8_raw"])
def test_same_bytes_whatever_the_upload_and_the_kernel_mix(gpu, key):
    csr = golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    truss, rnd, info = g.truss_decomposition(rounds=True)
    sup, tri = g.edge_support()
    assert sha(truss) == TRUSS[key]["truss_sha256"]
    variants = [("second call", g, None), ("trusted", gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_TRUSTED), None),
                ("hub limit 64", gpu.DeviceGraph.from_csr(csr, flags=64 << 8), None), ("shard 1 of 3", gpu.DeviceGraph.from_csr(csr, shard=(1, 3)), None),
                ("every round a kernel boundary", g, WG_NONE), ("every round in one workgroup", g, WG_ALL), ("tiny threshold", g, 3)]
    for name, h, wg in variants:
        if wg is None:
            t2, r2, i2 = h.truss_decomposition(rounds=True)
        else:
            with gpu.options(TRUSS_WG_FRONTIER=wg):
                t2, r2, i2 = h.truss_decomposition(rounds=True)
        s2, tri2 = h.edge_support()
        assert t2.tobytes() == truss.tobytes() and r2.tobytes() == rnd.tobytes() and i2 == info and s2.tobytes() == sup.tobytes() and tri2 == tri, name
        if h is not g:
            h.free()
    g.free()


# ---- 5. contract ----------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = golden_csr(gpu, "kronecker_8_16")
    nnz = csr.nnz
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    a, b = np.full(nnz, -77, dtype=np.int32), np.full(nnz, -77, dtype=np.int32)
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    info, tri = gpu.TrussInfo(), C.c_uint64(123)
    assert L.gmsx_truss_decomposition(g._h, pa, pb, None, None) == gpu.ERR_INVALID
    assert L.gmsx_truss_decomposition(None, pa, pb, C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_edge_support(g._h, None, C.byref(tri), None) == gpu.ERR_INVALID
    assert L.gmsx_edge_support(None, pa, C.byref(tri), None) == gpu.ERR_INVALID
    assert np.all(a == -77) and np.all(b == -77) and info.max_truss == 0 and info.rounds == 0 and tri.value == 123
    st = gpu.Stats()
    assert L.gmsx_truss_decomposition(g._h, None, None, C.byref(info), C.byref(st)) == gpu.OK  # both arrays may be NULL: only *info is filled
    assert info.max_truss == TRUSS["kronecker_8_16"]["max_truss"] and st.units == nnz // 2 and st.probes == info.rounds
    assert L.gmsx_edge_support(g._h, pa, None, None) == gpu.OK and np.array_equal(a, ARR["support_kronecker_8_16"])  # triangles may be NULL
    g.free()
