"""CPU: the goldens of connected components and Jarvis–Patrick clustering (tests/golden/components.{json,npz}, written by
tools/make_golden_components.py: the component labels are what the REFERENCE's ShiloachVishkin returns, log_graph/cc.cc:40-72; the
Jarvis–Patrick records come from the restatement below, there is no reference code) agree with the definitions of include/gmsx.h restated in
numpy / scipy:

  * components_np (scipy.sparse.csgraph.connected_components relabelled to the smallest id) reproduces every component record: info, the
    literal label array up to 2^16 vertices, the sha256 beyond;
  * jarvis_patrick_np (a score per edge from sparse row products, a threshold, components_np over what is kept) reproduces every
    Jarvis–Patrick record, and no record keeps nothing or everything;
  * the restatement gives the values of the issue on the shapes tests/test_components_gpu.py runs on the device;
  * both entry points are in capi.SYMBOLS and exported, the three options are enumerated, and without a GPU the calls return GMSX_ERR_NO_DEVICE.

components_np, jarvis_patrick_np and the shape builders are what tests/test_components_gpu.py checks the device against."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components as scipy_cc

from conftest import GOLDEN, ROOT, host_graph, load_golden

COMP = load_golden("components.json")
ARR = np.load(os.path.join(GOLDEN, "components.npz"))
CC = COMP["cc"]
JP = COMP["jp"]
METRIC_IDS = {"jaccard": 0, "overlap": 1, "adamic_adar": 2, "resource": 3, "common_neighbors": 4, "total_neighbors": 5, "pref_attachment": 6}
INFO_KEYS = ("components", "singletons", "largest", "largest_label", "kept_edges")
LITERAL_MAX_N = 1 << 16
CC_WAVE_ROW, CC_WG_ROW = 256, 4096  # the defaults of components.hip (gmsx.h, OPTIONS)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def sources(off):
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))


def info_np(label, kept_edges):
    """the gmsx_components_info integers of a label array (passes is a diagnostic and not a fact about the graph)"""
    label = np.asarray(label, dtype=np.int64)
    if label.size == 0:
        return dict.fromkeys(INFO_KEYS, 0)
    roots, sizes = np.unique(label, return_counts=True)
    top = int(np.flatnonzero(sizes == sizes.max())[0])  # np.unique ascends: the first maximum is the smallest label
    return {"components": int(roots.size), "singletons": int((sizes == 1).sum()), "largest": int(sizes[top]), "largest_label": int(roots[top]),
            "kept_edges": int(kept_edges)}


def components_np(off, adj, arc_keep=None):
    """(label, info): label[v] = the smallest vertex id of v's component over the arcs whose byte in arc_keep is non-zero (None: all); an edge
    is kept if either of its arcs is, and kept_edges counts it once."""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    if n == 0:
        return np.zeros(0, dtype=np.int32), info_np([], 0)
    src = sources(off)
    keep = np.ones(adj.size, dtype=bool) if arc_keep is None else np.asarray(arc_keep) != 0
    a, b = np.minimum(src[keep], adj[keep]), np.maximum(src[keep], adj[keep])
    edges = np.unique(a * n + b)
    a, b = edges // n, edges % n
    m = sp.coo_matrix((np.ones(a.size, dtype=np.int8), (a, b)), shape=(n, n)).tocsr()
    _, comp = scipy_cc(m, directed=False)
    smallest = np.full(int(comp.max()) + 1, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n, dtype=np.int64))
    label = smallest[comp].astype(np.int32)
    return label, info_np(label, edges.size)


def edge_counts_np(off, adj, weights=None, chunk=1 << 15):
    """(eu, ev, cnt, wsum): for every edge u < v in CSR order |N(u) ∩ N(v)| and, with weights, the sum of weights[w] over the common neighbours w"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    src = sources(off)
    up = src < adj
    eu, ev = src[up], adj[up]
    A = sp.csr_matrix((np.ones(adj.size, dtype=np.float64), adj, off), shape=(n, n))
    cnt, wsum = np.zeros(eu.size), np.zeros(eu.size)
    for i in range(0, eu.size, chunk):
        X = A[eu[i:i + chunk]].multiply(A[ev[i:i + chunk]]).tocsr()
        cnt[i:i + chunk] = np.asarray(X.sum(axis=1)).ravel()
        if weights is not None:
            X.data = weights[X.indices]
            wsum[i:i + chunk] = np.asarray(X.sum(axis=1)).ravel()
    return eu, ev, cnt, wsum


def edge_scores_np(off, adj, metric, counts=None):
    """(eu, ev, score): the metric of include/gmsx.h (gmsx_vertex_similarity_batch) on the full rows for every edge u < v, in CSR order.  The
    count-based scores are the device's bits (one IEEE operation on exact integers); the Adamic-Adar / Resource sums agree to the last bits
    only.  counts: edge_counts_np of the graph (without weights), for the count-based metrics."""
    deg = np.diff(np.asarray(off, dtype=np.int64)).astype(np.float64)
    with np.errstate(divide="ignore"):
        w = {"adamic_adar": 1.0 / np.log(deg), "resource": 1.0 / deg}.get(metric)
    eu, ev, cnt, wsum = counts if counts is not None and w is None else edge_counts_np(off, adj, w)
    da, db = deg[eu], deg[ev]
    score = {"jaccard": lambda: cnt / (da + db + cnt), "overlap": lambda: cnt / np.minimum(da, db), "adamic_adar": lambda: wsum,
             "resource": lambda: wsum, "common_neighbors": lambda: cnt, "total_neighbors": lambda: da + db - cnt,
             "pref_attachment": lambda: da * db}[metric]()
    return eu, ev, score


def mask_of_edges(off, adj, eu, ev):
    """the symmetric 0 / 1 byte per arc of the edges (eu[i], ev[i])"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    src = sources(off)
    keys = np.unique(np.minimum(eu, ev) * n + np.maximum(eu, ev))
    arc = np.minimum(src, adj) * n + np.maximum(src, adj)
    at = np.minimum(np.searchsorted(keys, arc), max(keys.size - 1, 0))
    return (keys[at] == arc).astype(np.uint8) if keys.size else np.zeros(adj.size, dtype=np.uint8)


def jarvis_patrick_np(off, adj, metric, threshold, scores=None):
    """(label, info, mask): keep {u, v} iff score >= threshold (never a NaN score); the components of what is kept"""
    eu, ev, score = scores if scores is not None else edge_scores_np(off, adj, metric)
    with np.errstate(invalid="ignore"):
        keep = score >= threshold
    mask = mask_of_edges(off, adj, eu[keep], ev[keep])
    label, info = components_np(off, adj, mask)
    assert info["kept_edges"] == int(keep.sum())
    return label, info, mask


def golden_csr(capi, key):
    src = CC[key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def csr_of(edges, n):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = np.concatenate([e, e[:, ::-1]])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    return np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]).astype(np.int64), e[:, 1].astype(np.int32)


# ---- the shapes of the issue (tests/test_components_gpu.py runs the same on the device) ---------------------------------------------------------
def path_edges(n, numbering):
    """a path on n vertices: numbered along it, in reverse, or by a seeded random permutation"""
    ids = {"along": np.arange(n), "reverse": np.arange(n)[::-1], "random": np.random.RandomState(4096).permutation(n)}[numbering]
    return np.stack([ids[:-1], ids[1:]], axis=1)


def star_edges(leaves):
    return np.stack([np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1)], axis=1)


def bins_graph(degrees):
    """one star per wanted degree, the hubs first (vertex i has degree degrees[i]); returns (edges, n): len(degrees) components"""
    hubs, at, e = len(degrees), len(degrees), []
    for h, d in enumerate(degrees):
        e.append(np.stack([np.full(d, h, dtype=np.int64), np.arange(at, at + d)], axis=1))
        at += d
    return np.concatenate(e), at


BIN_DEGREES = [1, 15, 16, 17, 63, 64, 65, CC_WAVE_ROW - 1, CC_WAVE_ROW, CC_WAVE_ROW + 1, CC_WG_ROW - 1, CC_WG_ROW, CC_WG_ROW + 1]


def matching_edges(pairs, seed=65536):
    """a perfect matching on 2 * pairs vertices, partners by a seeded permutation"""
    p = np.random.RandomState(seed).permutation(2 * pairs)
    return np.stack([p[:pairs], p[pairs:]], axis=1)


def giant_plus_triangles(giant=3000, triangles=500, seed=7):
    """one large component (a seeded random tree plus chords, ids shuffled) and `triangles` separate triangles; returns (edges, n)"""
    rng = np.random.RandomState(seed)
    n = giant + 3 * triangles
    ids = rng.permutation(n)
    tree = [(ids[i], ids[rng.randint(0, i)]) for i in range(1, giant)]
    chords = [(ids[a], ids[b]) for a, b in rng.randint(0, giant, (2 * giant, 2)) if a != b]
    tri = []
    for t in range(triangles):
        a, b, c = ids[giant + 3 * t: giant + 3 * t + 3]
        tri += [(a, b), (b, c), (a, c)]
    return np.array(tree + chords + tri, dtype=np.int64), n


def two_k8_and_a_bridge():
    k8 = [(i, j) for i in range(8) for j in range(i)]
    return np.array(k8 + [(a + 8, b + 8) for a, b in k8] + [(7, 8)], dtype=np.int64), 16


# ---- the goldens ------------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_complete():
    want = {"file_eppsteinExample", "file_micro", "file_smallRandom1", "file_tomitaExample", "file_triangles_1", "file_triangles_3",
            "kronecker_10_16", "kronecker_12_16", "kronecker_16_16", "kronecker_20_16", "uniform_10_16", "uniform_16_16", "kronecker_10_16_raw"}
    assert set(CC) == want
    for key, rec in CC.items():
        assert rec["literal"] == (rec["n"] <= LITERAL_MAX_N) == ("label_" + key in ARR)
        assert 1 <= rec["components"] <= rec["n"] and rec["singletons"] <= rec["components"] and rec["largest"] >= 1
    assert any(not r["literal"] for r in CC.values())
    assert CC["kronecker_16_16"]["singletons"] > 1000  # the Kronecker graphs have many isolated vertices
    got = {(r["graph"], r["metric"]) for r in JP}
    for g in ("kronecker_10_16", "kronecker_12_16", "kronecker_16_16"):
        assert {(g, "common_neighbors"), (g, "jaccard"), (g, "overlap")} <= got
        assert sorted(float.fromhex(r["threshold"]) for r in JP if (r["graph"], r["metric"]) == (g, "common_neighbors")) == [1.0, 2.0, 5.0, 20.0]
        for metric in ("jaccard", "overlap"):
            assert sum((r["graph"], r["metric"]) == (g, metric) for r in JP) == 2
    assert sum(r["metric"] == "adamic_adar" for r in JP) >= 2 and {r["graph"] for r in JP if r["metric"] == "adamic_adar"} == {"kronecker_10_16", "kronecker_12_16"}
    for r in JP:  # a record that keeps nothing or everything tests nothing
        assert 0 < r["kept_edges"] < CC[r["graph"]]["nnz"] // 2, r


@pytest.mark.parametrize("key", sorted(CC))
def test_components_restatement_reproduces_the_reference(capi, key):
    rec, csr = CC[key], golden_csr(capi, key)
    off, adj = csr.offsets(), csr.neighbors()
    assert (off.size - 1, adj.size) == (rec["n"], rec["nnz"])
    label, info = components_np(off, adj)
    assert sha(label) == rec["label_sha256"]
    if rec["literal"]:
        assert np.array_equal(label, ARR["label_" + key])
    assert info == dict({k: rec[k] for k in INFO_KEYS if k != "kept_edges"}, kept_edges=rec["nnz"] // 2)
    assert np.all(label <= np.arange(rec["n"])) and np.array_equal(label[label], label)


_COUNTS, _SCORES = {}, {}


def scores_of(capi, graph, metric):
    """the per-edge scores of a golden graph: the common-neighbour counts once per graph, the scores once per (graph, metric)"""
    if (graph, metric) not in _SCORES:
        csr = golden_csr(capi, graph)
        if graph not in _COUNTS:
            _COUNTS[graph] = edge_counts_np(csr.offsets(), csr.neighbors())
        _SCORES[(graph, metric)] = edge_scores_np(csr.offsets(), csr.neighbors(), metric, _COUNTS[graph])
    return _SCORES[(graph, metric)]


def jp_id(r):
    return "%s-%s-%s" % (r["graph"], r["metric"], float.fromhex(r["threshold"]))


@pytest.mark.parametrize("rec", JP, ids=jp_id)
def test_jarvis_patrick_restatement_reproduces_the_golden(capi, rec):
    csr = golden_csr(capi, rec["graph"])
    off, adj = csr.offsets(), csr.neighbors()
    label, info, mask = jarvis_patrick_np(off, adj, rec["metric"], float.fromhex(rec["threshold"]), scores_of(capi, rec["graph"], rec["metric"]))
    assert info == {k: rec[k] for k in INFO_KEYS}
    assert sha(label) == rec["label_sha256"]
    if rec["literal"]:
        assert np.array_equal(label, ARR[rec["array"]])
    assert int(mask.sum()) == 2 * rec["kept_edges"]


# ---- the shapes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["along", "reverse", "random"])
def test_restatement_on_paths(numbering):
    off, adj = csr_of(path_edges(4096, numbering), 4096)
    label, info = components_np(off, adj)
    assert not label.any() and info == {"components": 1, "singletons": 0, "largest": 4096, "largest_label": 0, "kept_edges": 4095}


def test_restatement_on_the_other_shapes():
    off, adj = csr_of(star_edges(70000), 70001)
    assert components_np(off, adj)[1] == {"components": 1, "singletons": 0, "largest": 70001, "largest_label": 0, "kept_edges": 70000}
    e, n = bins_graph(BIN_DEGREES)
    off, adj = csr_of(e, n)
    assert np.diff(off)[:len(BIN_DEGREES)].tolist() == BIN_DEGREES
    label, info = components_np(off, adj)
    assert info["components"] == len(BIN_DEGREES) and info["largest"] == CC_WG_ROW + 2 and info["largest_label"] == len(BIN_DEGREES) - 1
    assert np.array_equal(label[:len(BIN_DEGREES)], np.arange(len(BIN_DEGREES)))
    e = matching_edges(1 << 15)
    off, adj = csr_of(e, (1 << 16) + 1000)
    label, info = components_np(off, adj)
    assert info == {"components": 32768 + 1000, "singletons": 1000, "largest": 2, "largest_label": 0, "kept_edges": 32768}
    assert np.array_equal(label[e[:, 0]], e.min(axis=1)) and np.array_equal(label[e[:, 1]], e.min(axis=1))
    e, n = giant_plus_triangles()
    info = components_np(*csr_of(e, n))[1]
    assert info["components"] == 501 and info["largest"] == 3000 and info["singletons"] == 0


def test_restatement_on_two_k8_and_a_bridge():
    e, n = two_k8_and_a_bridge()
    off, adj = csr_of(e, n)
    label, info, mask = jarvis_patrick_np(off, adj, "common_neighbors", 1)  # the bridge's endpoints share nobody
    assert info == {"components": 2, "singletons": 0, "largest": 8, "largest_label": 0, "kept_edges": 56} and label.tolist() == [0] * 8 + [8] * 8
    assert jarvis_patrick_np(off, adj, "common_neighbors", 0)[1] == {"components": 1, "singletons": 0, "largest": 16, "largest_label": 0, "kept_edges": 57}
    assert jarvis_patrick_np(off, adj, "common_neighbors", 7)[1] == {"components": 16, "singletons": 16, "largest": 1, "largest_label": 0, "kept_edges": 0}
    # a one-sided mask means the same as the symmetric one
    src = sources(off)
    for side in (src < adj, src > adj):
        l2, i2 = components_np(off, adj, mask * side)
        assert np.array_equal(l2, label) and i2 == info


def test_clusters_groups_by_label(capi):
    got = capi.clusters(np.array([0, 1, 0, 3, 1, 0], dtype=np.int32))
    assert [c.tolist() for c in got] == [[0, 2, 5], [1, 4], [3]] and all(c.dtype == np.int32 for c in got)
    assert capi.clusters(np.zeros(0, dtype=np.int32)) == []


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_connected_components", "gmsx_jarvis_patrick"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    for name in ("CC_SAMPLE", "CC_WAVE_ROW", "CC_WG_ROW"):
        assert name in capi.option_names()
    assert ctypes.sizeof(capi.ComponentsInfo) == 40
    assert capi.lib().gmsx_version() == 320


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_entry_points_fail_loudly_without_gpu(capi):
    L = capi.lib()
    label = np.full(4, -77, dtype=np.int32)
    info = capi.ComponentsInfo()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(1 << 16)))  # never read: both calls check the device before they read the handle
    assert L.gmsx_connected_components(fake, None, label.ctypes.data_as(ctypes.c_void_p), ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_jarvis_patrick(fake, 4, 2.0, label.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_connected_components(None, None, None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_jarvis_patrick(fake, 7, 2.0, None, None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_jarvis_patrick(fake, 4, float("nan"), None, None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert np.all(label == -77)
