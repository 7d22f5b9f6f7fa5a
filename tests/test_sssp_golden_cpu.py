"""CPU: the goldens of gmsx_sssp (tests/golden/sssp.json, sssp.npz, fixtures under tests/golden/sssp/; tools/make_golden_sssp.py) against a
restatement in plain Python / numpy, which is also what tests/test_sssp_gpu.py holds the device to:
  * dijkstra_np — a binary-heap Dijkstra: dist[v], -1 = unreachable;
  * parent_np — the first tight entry of the ascending row: the SMALLEST-id neighbour u with dist[u] + w(u, v) == dist[v];
  * verify_np — gmsx_sssp_verify's four numbers; info_np — the integers of gmsx_sssp_info that are facts about (graph, weights, source, delta).
The recorded distances are the reference's DeltaStep (delta 1 and 16, one and four OpenMP threads: all equal, accepted by its SSSPVerifier)."""
import heapq
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

J = load_golden("sssp.json")
ARR = np.load(os.path.join(GOLDEN, "sssp.npz"))
TRAV = load_golden("traversal.json")
TRAV_ARR = np.load(os.path.join(GOLDEN, "traversal.npz"))
DELTAS = (1, 16, 0, 2 ** 31 - 1)  # what the GPU test runs every record under; 0 = the library's choice


def dijkstra_np(off, adj, w, source):
    n = len(off) - 1
    off, adj, w = [int(x) for x in off], [int(x) for x in adj], [int(x) for x in w]
    dist = [-1] * n
    dist[source] = 0
    heap = [(0, source)]
    while heap:
        d, u = heapq.heappop(heap)
        if d != dist[u]:
            continue
        for j in range(off[u], off[u + 1]):
            v, nd = adj[j], d + w[j]
            if dist[v] < 0 or nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, v))
    return np.array(dist, dtype=np.int64)


def _rows(off):
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))


def parent_np(off, adj, w, source, dist):
    """The first tight entry of every reached vertex's ascending row (np.minimum.at over the tight arcs: the smallest id)."""
    n = len(off) - 1
    adj, w, dist = np.asarray(adj, dtype=np.int64), np.asarray(w, dtype=np.int64), np.asarray(dist, dtype=np.int64)
    row = _rows(off)
    tight = (dist[row] >= 0) & (dist[adj] >= 0) & (dist[adj] + w == dist[row])
    parent = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(parent, row[tight], adj[tight])
    parent[parent == np.iinfo(np.int64).max] = -1
    parent[dist < 0] = -1
    if dist[source] >= 0:
        parent[source] = source
    return parent.astype(np.int32)


def verify_np(off, adj, w, source, dist):
    n = len(off) - 1
    adj, w, dist = np.asarray(adj, dtype=np.int64), np.asarray(w, dtype=np.int64), np.asarray(dist, dtype=np.int64)
    row = _rows(off)  # arc u -> v is met in v's row: row = v, adj = u
    dv, du = dist[row], dist[adj]
    both = (dv >= 0) & (du >= 0)
    has_tight = np.zeros(n, dtype=bool)
    has_tight[row[both & (dv == du + w)]] = True
    has_reached = np.zeros(n, dtype=bool)
    has_reached[row[du >= 0]] = True
    reached = dist >= 0
    not_source = np.arange(n) != source
    return {"violated_arcs": int((both & (dv > du + w)).sum()), "untight": int((reached & not_source & ~has_tight).sum()),
            "wrong_unreached": int((~reached & has_reached).sum()), "source_ok": int(dist[source] == 0)}


def info_np(off, dist, delta=None):
    dist = np.asarray(dist, dtype=np.int64)
    reached = dist >= 0
    mx = int(dist[reached].max())
    out = {"reached": int(reached.sum()), "reached_arcs": int(np.diff(off)[reached].sum()), "dist_sum": int(dist[reached].sum()), "max_dist": mx,
           "far_vertex": int(np.flatnonzero(dist == mx)[0])}
    if delta:
        out["buckets"] = int(np.unique(dist[reached] // delta).size)
    return out


def golden_csr(capi, key):
    """The weighted host CSR of a golden graph."""
    src = J["graphs"][key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load_weighted(os.path.join(GOLDEN, "sssp", src["name"]), symmetrize=True, relabel=capi.RELABEL_NEVER)
    return capi.HostCSR.generate_weighted(src["generator"], src["scale"], src["degree"], capi.RELABEL_ALWAYS if src["relabel"] else capi.RELABEL_NEVER)


_CSR = {}


def golden_arrays(capi, key):
    if key not in _CSR:
        c = golden_csr(capi, key)
        _CSR[key] = (np.array(c.offsets(), dtype=np.int64), np.array(c.neighbors(), dtype=np.int32), np.array(c.weights(), dtype=np.int32))
    return _CSR[key]


def rec_id(r):
    return "%s-s%d" % (r["graph"], r["source"])


def test_goldens_are_complete():
    keys = set(J["graphs"])
    assert {"kronecker_10_16", "kronecker_12_16", "uniform_10_16", "kronecker_10_16_relabelled"} <= keys
    files = [k for k in keys if J["graphs"][k]["source"]["kind"] == "file"]
    assert len(files) >= 2 and all(J["graphs"][k]["n"] <= 64 for k in files)
    for k in keys:
        recs = [r for r in J["records"] if r["graph"] == k]
        assert len({r["source"] for r in recs}) >= 2 and any(r["source"] == 0 for r in recs), k
        for r in recs:
            assert r["reference_deltas"] == [1, 16] and r["reference_threads"] == [1, 4] and r["reference_verified"]
    assert os.path.getsize(os.path.join(GOLDEN, "sssp.npz")) < 1 << 20


@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_restatement_reproduces_the_golden(capi, rec):
    off, adj, w = golden_arrays(capi, rec["graph"])
    gold = ARR["dist_" + rec_id(rec)].astype(np.int64)
    dist = dijkstra_np(off, adj, w, rec["source"])
    assert np.array_equal(dist, gold)
    info = info_np(off, dist)
    for k in ("reached", "dist_sum", "max_dist", "far_vertex"):
        assert info[k] == rec[k], k
    parent = parent_np(off, adj, w, rec["source"], dist)
    assert np.array_equal(parent, ARR["parent_" + rec_id(rec)])
    assert verify_np(off, adj, w, rec["source"], dist) == {"violated_arcs": 0, "untight": 0, "wrong_unreached": 0, "source_ok": 1}
    for delta in (1, 16, 2 ** 31 - 1):
        assert info_np(off, dist, delta)["buckets"] == len(set(int(d) // delta for d in dist if d >= 0))
    # dist strictly falls along parents: parent is a tree
    reached = np.flatnonzero((dist >= 0) & (np.arange(dist.size) != rec["source"]))
    assert np.all(dist[parent[reached]] < dist[reached])


@pytest.mark.parametrize("key", sorted(J["graphs"]))
def test_scipy_agrees_on_the_golden_graphs(capi, key):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    off, adj, w = golden_arrays(capi, key)
    n = off.size - 1
    m = sp.csr_matrix((w.astype(np.float64), adj, off), shape=(n, n))
    for rec in [r for r in J["records"] if r["graph"] == key]:
        d = dijkstra(m, directed=True, indices=rec["source"])
        want = np.where(np.isinf(d), -1, d).astype(np.int64)
        assert np.array_equal(want, ARR["dist_" + rec_id(rec)].astype(np.int64))


def test_unit_weights_are_breadth_first_search(capi):
    """With all weights 1 on the existing testGraphs, dist and parent equal the recorded depths and parents of gmsx_bfs."""
    seen = 0
    for rec in TRAV["bfs"]:
        src = TRAV["graphs"][rec["graph"]]["source"]
        name = "depth_%s_%d" % (rec["graph"], rec["source"])
        if src["kind"] != "file" or name not in TRAV_ARR.files:
            continue
        c = capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
        off, adj = np.array(c.offsets(), dtype=np.int64), np.array(c.neighbors(), dtype=np.int32)
        w = np.ones(adj.size, dtype=np.int32)
        dist = dijkstra_np(off, adj, w, rec["source"])
        assert np.array_equal(dist, TRAV_ARR[name].astype(np.int64))
        assert np.array_equal(parent_np(off, adj, w, rec["source"], dist), TRAV_ARR["parent_%s_%d" % (rec["graph"], rec["source"])])
        seen += 1
    assert seen >= 6


def test_verify_np_counts_what_it_says():
    # a path 0 - 1 - 2 with weights 2, 3 and an isolated vertex 3
    off, adj, w = np.array([0, 1, 3, 4, 4]), np.array([1, 0, 2, 1]), np.array([2, 2, 3, 3])
    dist = dijkstra_np(off, adj, w, 0)
    assert dist.tolist() == [0, 2, 5, -1]
    assert verify_np(off, adj, w, 0, dist) == {"violated_arcs": 0, "untight": 0, "wrong_unreached": 0, "source_ok": 1}
    assert verify_np(off, adj, w, 0, [0, 2, 6, -1]) == {"violated_arcs": 1, "untight": 1, "wrong_unreached": 0, "source_ok": 1}
    assert verify_np(off, adj, w, 0, [0, 2, 4, -1]) == {"violated_arcs": 0, "untight": 1, "wrong_unreached": 0, "source_ok": 1}
    assert verify_np(off, adj, w, 0, [0, 2, -1, -1]) == {"violated_arcs": 0, "untight": 0, "wrong_unreached": 1, "source_ok": 1}
    assert verify_np(off, adj, w, 0, [1, 2, 5, -1])["source_ok"] == 0


def test_new_symbols_declared_and_exported(capi):
    import ctypes
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in ("gmsx_csr_weights", "gmsx_csr_generate_weighted", "gmsx_csr_from_weighted_edges", "gmsx_csr_load_weighted", "gmsx_csr_save_wsg",
                 "gmsx_csr_from_arrays_weighted", "gmsx_graph_set_weights", "gmsx_graph_has_weights", "gmsx_sssp", "gmsx_sssp_verify"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    for opt in ("SSSP_WG_FRONTIER", "SSSP_WIDE", "SSSP_DELTA_AUTO"):
        assert opt in capi.option_names()
    assert ctypes.sizeof(capi.SsspInfo) == 72 and ctypes.sizeof(capi.SsspCheck) == 32
