"""CPU: the goldens of gmsx_min_spanning_forest (tests/golden/msf.json, msf.npz; tools/make_golden_msf.py) against two restatements in plain
Python / numpy, which are also what tests/test_msf_gpu.py holds the device to:
  * kruskal_np — Kruskal over the edges sorted by the order of include/gmsx.h: key (w, lo, hi), the maximum with the heavier edge first and
    ties still by the smaller (lo, hi); returns the forest's (u, v, w), u < v, ascending by (u, v);
  * boruvka_np — full Borůvka rounds under the same order (every component that has a crossing edge picks its first one, all picks are
    applied): the same edge set and `rounds`, the number of rounds that added an edge;
  * info_np — the integers of gmsx_msf_info; labels_np — the smallest vertex id of every vertex's tree.
The reference has no spanning forest; scipy.sparse.csgraph agrees on the total weight, the edge count and the number of trees."""
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_sssp_golden_cpu import J as SSSP_J
from test_sssp_golden_cpu import golden_csr as sssp_golden_csr

J = load_golden("msf.json")
ARR = np.load(os.path.join(GOLDEN, "msf.npz"))
EXTRA = {"kronecker_14_16": ("kronecker", 14, 16)}   # beside the six graphs of sssp.json
INFO_KEYS = ("edges", "total_weight", "trees", "isolated", "largest_tree", "min_weight", "max_weight", "rounds")
ARRAY_MAX_N = 1 << 12   # graphs up to scale 12 keep their edge arrays in msf.npz


def graph_keys():
    return sorted(SSSP_J["graphs"]) + sorted(EXTRA)


def golden_csr(capi, key):
    """The weighted host CSR of a golden graph: the files and generator settings of sssp.json, plus kronecker_14_16."""
    if key in EXTRA:
        kind, scale, deg = EXTRA[key]
        return capi.HostCSR.generate_weighted(kind, scale, deg, capi.RELABEL_NEVER)
    return sssp_golden_csr(capi, key)


_CSR = {}


def golden_arrays(capi, key):
    if key not in _CSR:
        c = golden_csr(capi, key)
        _CSR[key] = (np.array(c.offsets(), dtype=np.int64), np.array(c.neighbors(), dtype=np.int32), np.array(c.weights(), dtype=np.int32))
    return _CSR[key]


def _upper_edges(off, adj, w):
    """(lo, hi, w) of the u < v arcs, in CSR order"""
    off, adj, w = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64), np.asarray(w, dtype=np.int64)
    row = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
    up = row < adj
    return row[up], adj[up], w[up]


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _as_edges(lo, hi, w, take):
    take = np.asarray(sorted(take), dtype=np.int64)   # positions in CSR order of the u < v arcs: ascending by (u, v)
    return lo[take].astype(np.int32), hi[take].astype(np.int32), w[take].astype(np.int32)


def kruskal_np(off, adj, w, maximum=False):
    lo, hi, ww = _upper_edges(off, adj, w)
    order = np.lexsort((hi, lo, -ww if maximum else ww))
    parent = list(range(len(off) - 1))
    take = []
    for e, a, b in zip(order.tolist(), lo[order].tolist(), hi[order].tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            take.append(e)
    return _as_edges(lo, hi, ww, take)


def boruvka_np(off, adj, w, maximum=False):
    """((u, v, w), rounds)"""
    n = len(off) - 1
    lo, hi, ww = _upper_edges(off, adj, w)
    k0 = -ww if maximum else ww
    comp = np.arange(n, dtype=np.int64)
    take, rounds = set(), 0
    while True:
        ca, cb = comp[lo], comp[hi]
        cross = np.flatnonzero(ca != cb)
        if cross.size == 0:
            break
        # every crossing edge is offered to both of its components; the first of a component in the order is its pick
        e = np.concatenate([cross, cross])
        c = np.concatenate([ca[cross], cb[cross]])
        order = np.lexsort((hi[e], lo[e], k0[e], c))
        first = np.ones(order.size, dtype=bool)
        first[1:] = c[order][1:] != c[order][:-1]
        picks = np.unique(e[order][first])
        take.update(picks.tolist())
        rounds += 1
        parent = list(range(n))
        for a, b in zip(comp[lo[picks]].tolist(), comp[hi[picks]].tolist()):
            ra, rb = _find(parent, a), _find(parent, b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        root = np.array([_find(parent, x) for x in range(n)], dtype=np.int64)
        comp = root[comp]
    return _as_edges(lo, hi, ww, take), rounds


def labels_np(n, u, v):
    """the smallest vertex id of every vertex's tree"""
    parent = list(range(n))
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([_find(parent, x) for x in range(n)], dtype=np.int32)


def info_np(off, u, v, w, rounds):
    n = len(off) - 1
    label = labels_np(n, u, v)
    sizes = np.bincount(label, minlength=max(n, 1))[:n]
    w = np.asarray(w, dtype=np.int64)
    return {"edges": int(w.size), "total_weight": int(w.sum()), "trees": int((sizes > 0).sum()), "isolated": int((np.diff(off) == 0).sum()),
            "largest_tree": int(sizes.max()) if n else 0, "min_weight": int(w.min()) if w.size else 0, "max_weight": int(w.max()) if w.size else 0,
            "rounds": int(rounds)}


def mask_np(off, adj, u, v):
    """1 on both arcs of every listed edge"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    keys = set((np.asarray(u, dtype=np.int64) * n + np.asarray(v, dtype=np.int64)).tolist())
    code = np.minimum(row, adj) * n + np.maximum(row, adj)
    return np.fromiter((c in keys for c in code.tolist()), dtype=np.uint8, count=code.size)


def sha_of(u, v, w):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype="<i4").tobytes() for a in (u, v, w))).hexdigest()


def fnv_of(u, v, w):
    """FNV-1a over the same bytes: what the C++ adaptor test prints"""
    x = 1469598103934665603
    for b in b"".join(np.ascontiguousarray(a, dtype="<i4").tobytes() for a in (u, v, w)):
        x = ((x ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return x


def rec_id(r):
    return "%s-%s" % (r["graph"], "max" if r["maximum"] else "min")


def record(key, maximum):
    return next(r for r in J["records"] if r["graph"] == key and r["maximum"] == maximum)


_FOREST = {}


def forest(capi, key, maximum):
    """kruskal_np of a golden graph, computed once"""
    if (key, maximum) not in _FOREST:
        _FOREST[(key, maximum)] = kruskal_np(*golden_arrays(capi, key), maximum)
    return _FOREST[(key, maximum)]


def test_goldens_are_complete():
    assert sorted(J["graphs"]) == sorted(graph_keys()) and len(J["graphs"]) == 7
    for key in J["graphs"]:
        recs = [r for r in J["records"] if r["graph"] == key]
        assert sorted(r["maximum"] for r in recs) == [False, True], key
        for r in recs:
            assert set(INFO_KEYS) <= set(r) and len(r["sha256"]) == 64
            has = all(("%s_%s" % (a, rec_id(r))) in ARR.files for a in "uvw")
            assert has == (J["graphs"][key]["n"] <= ARRAY_MAX_N), rec_id(r)
    assert len(J["records"]) == 14
    assert os.path.getsize(os.path.join(GOLDEN, "msf.npz")) < 1 << 20


@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_kruskal_reproduces_the_golden(capi, rec):
    off, adj, w = golden_arrays(capi, rec["graph"])
    u, v, ww = forest(capi, rec["graph"], rec["maximum"])
    assert np.all(u < v) and np.all(np.diff(u.astype(np.int64) * off.size + v) > 0)   # ascending by (u, v)
    assert sha_of(u, v, ww) == rec["sha256"] and str(fnv_of(u, v, ww)) == rec["fnv"]
    assert info_np(off, u, v, ww, rec["rounds"]) == {k: rec[k] for k in INFO_KEYS}
    assert rec["edges"] == off.size - 1 - rec["trees"]
    assert rec["rounds"] <= int(np.floor(np.log2(max(rec["largest_tree"], 1))))
    if J["graphs"][rec["graph"]]["n"] <= ARRAY_MAX_N:
        for name, a in zip("uvw", (u, v, ww)):
            assert np.array_equal(ARR["%s_%s" % (name, rec_id(rec))], a)


@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_boruvka_gives_the_same_forest_and_the_recorded_rounds(capi, rec):
    off, adj, w = golden_arrays(capi, rec["graph"])
    (u, v, ww), rounds = boruvka_np(off, adj, w, rec["maximum"])
    assert sha_of(u, v, ww) == rec["sha256"] and rounds == rec["rounds"]


@pytest.mark.parametrize("key", graph_keys())
def test_scipy_agrees_on_the_golden_graphs(capi, key):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
    off, adj, w = golden_arrays(capi, key)
    n = off.size - 1
    wmax = int(w.max())
    for maximum in (False, True):
        rec = record(key, maximum)
        vals = (wmax + 1 - w.astype(np.int64)) if maximum else w.astype(np.int64)
        t = minimum_spanning_tree(sp.csr_matrix((vals.astype(np.float64), adj, off), shape=(n, n)))
        assert t.nnz == rec["edges"]
        total = int(round(t.sum()))
        assert (rec["edges"] * (wmax + 1) - total if maximum else total) == rec["total_weight"]
        u, v, _ = forest(capi, key, maximum)
        trees, _ = connected_components(sp.csr_matrix((np.ones(u.size), (u, v)), shape=(n, n)), directed=False)
        assert trees == rec["trees"]
    assert record(key, True)["total_weight"] >= record(key, False)["total_weight"]


def test_the_order_breaks_ties_by_the_ids():
    # a 4-cycle 0 - 1 - 2 - 3 - 0 of unit weights: (0,1), (0,3), (1,2) come first; with weights the heavier edge leaves (minimum) or stays
    off, adj = np.array([0, 2, 4, 6, 8]), np.array([1, 3, 0, 2, 1, 3, 0, 2])
    u, v, w = kruskal_np(off, adj, np.ones(8, dtype=np.int32))
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 3), (1, 2)]
    (bu, bv, bw), rounds = boruvka_np(off, adj, np.ones(8, dtype=np.int32))
    assert (bu.tolist(), bv.tolist(), rounds) == (u.tolist(), v.tolist(), 1)   # 0 and 1 pick (0,1), 2 picks (1,2), 3 picks (0,3)
    wt = np.array([5, 2, 5, 7, 7, 2, 2, 2], dtype=np.int32)   # w(0,1) = 5, w(0,3) = 2, w(1,2) = 7, w(2,3) = 2
    u, v, w = kruskal_np(off, adj, wt)
    assert list(zip(u.tolist(), v.tolist(), w.tolist())) == [(0, 1, 5), (0, 3, 2), (2, 3, 2)]
    u, v, w = kruskal_np(off, adj, wt, maximum=True)
    assert list(zip(u.tolist(), v.tolist(), w.tolist())) == [(0, 1, 5), (0, 3, 2), (1, 2, 7)]   # ties among the weight 2: the smaller (lo, hi)
    assert info_np(off, u, v, w, 1) == {"edges": 3, "total_weight": 14, "trees": 1, "isolated": 0, "largest_tree": 4, "min_weight": 2,
                                        "max_weight": 7, "rounds": 1}
    assert mask_np(off, adj, u, v).tolist() == [1, 1, 1, 1, 1, 0, 1, 0]


def test_new_symbol_declared_exported_and_documented(capi):
    import ctypes
    L = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(L, "gmsx_min_spanning_forest") and "gmsx_min_spanning_forest" in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    assert re.search(r"\bint gmsx_min_spanning_forest\(", hdr) and "GMSX_MSF_MAXIMUM = 1u" in hdr and "} gmsx_msf_info;" in hdr
    for opt in ("MSF_WAVE_ROW", "MSF_WG_ROW", "MSF_PRUNE"):
        assert opt in capi.option_names() and re.search(r"\b%s\b" % opt, hdr), opt
    assert ctypes.sizeof(capi.MsfInfo) == 56 and capi.MSF_MAXIMUM == 1
    assert capi.lib().gmsx_version() == 320
