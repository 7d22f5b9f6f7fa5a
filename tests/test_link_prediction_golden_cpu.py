"""CPU: the goldens of link prediction (tests/golden/link_prediction.json, written by tools/make_golden_link_prediction.py from the compiled
reference) agree with the rule gmsx_link_prediction is specified by (include/gmsx.h), restated here in numpy from a numpy restatement of the
seven scores:

  candidates  the non-edges u < v whose score is not NaN
  order       decreasing score, ties by ascending (u, v)
  result      the first min(q, candidates), worst first; the reference pads q - found leading (-1.0, (0,0)) entries, one when nothing qualifies

Jaccard, Overlap, CommonNeighbors, TotalNeighbors and PrefAttachment: pairs and scores exactly.  Adamic-Adar and Resource sum their terms in
another order here than in the reference, so they follow the tolerance rule (compare_tolerant): positional scores within 1e-12 relative, pairs
equal as sets inside each run of golden positions whose scores lie within 1e-9 relative of one another — the generator asserted that the q-th
and (q+1)-th reference scores and all distinct kept scores are further apart than that.

all_scores_np / rule_np / compare_tolerant / decode / digest are what tests/test_link_prediction_gpu.py checks the device against."""
import base64
import ctypes
import hashlib
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

LP = load_golden("link_prediction.json")
RECORDS = LP["records"]
METRICS = ["jaccard", "overlap", "adamic_adar", "resource", "common", "total", "prefatt"]
TOLERANT = ("adamic_adar", "resource")
GRAPH_KEYS = sorted(LP["graphs"])


def golden_csr(capi, key):
    src = LP["graphs"][key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    from conftest import host_graph
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def digest(u, v, s):
    return hashlib.sha256(np.ascontiguousarray(u, dtype="<i4").tobytes() + np.ascontiguousarray(v, dtype="<i4").tobytes() +
                          np.ascontiguousarray(s, dtype="<f8").tobytes()).hexdigest()


def decode(rec):
    """(u, v, scores) of a record's real entries, worst first; None for a record that carries its sha256 only"""
    if rec["form"] == "literal":
        s = [float.fromhex(h) for h, c in rec["scores_rle"] for _ in range(c)]
        return np.array(rec["u"], dtype=np.int32), np.array(rec["v"], dtype=np.int32), np.array(s, dtype=np.float64)
    if rec["form"] == "packed":
        e = np.frombuffer(zlib.decompress(base64.b64decode(rec["edges_z"])), dtype="<i4").reshape(-1, 2)
        img = np.cumsum(np.frombuffer(zlib.decompress(base64.b64decode(rec["scores_z"])), dtype="<u8"), dtype=np.uint64)
        bits = np.where(img >> np.uint64(63), img & ~np.uint64(1 << 63), ~img)
        return e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), bits.astype("<u8").view("<f8").copy()
    return None


def all_scores_np(off, adj, metric):
    """S[u, v] = the reference's vertex_similarity<metric>(u, v) (vertex_similarity.h:30-222) for every pair, float64, dense; and the
    adjacency matrix.  n <= a few thousand."""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    deg = np.diff(off).astype(np.float64)
    A = np.zeros((n, n), dtype=np.float64)
    A[np.repeat(np.arange(n), np.diff(off)), adj] = 1.0
    metric = METRICS[metric] if not isinstance(metric, str) else metric
    da, db = deg[:, None], deg[None, :]
    if metric in TOLERANT:
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(deg >= 2, 1.0 / np.log(deg) if metric == "adamic_adar" else 1.0 / deg, 0.0)  # a common neighbour has degree >= 2
        S = A @ (w[:, None] * A)
    else:
        c = np.rint(A @ A)
        with np.errstate(divide="ignore", invalid="ignore"):
            if metric == "jaccard":
                S = np.where((da == 0) & (db == 0), 1.0, c / (da + db + c))
            elif metric == "overlap":
                S = c / np.minimum(da, db)
            elif metric == "common":
                S = c
            elif metric == "total":
                S = da + db - c
            else:
                S = da * db
    return S, A


def rule_from_pairs(u, v, s, q):
    """the rule on candidate arrays: NaN out, decreasing score, ties by ascending (u, v), the first q, worst first"""
    ok = ~np.isnan(s)
    u, v, s = u[ok], v[ok], s[ok]
    order = np.lexsort((v, u, -s))[:q][::-1]
    return u[order].astype(np.int32), v[order].astype(np.int32), s[order].astype(np.float64)


def nonedges(A, part=0, nparts=1):
    n = A.shape[0]
    u, v = np.triu_indices(n, 1)
    keep = (A[u, v] == 0) & (u % nparts == part)
    return u[keep], v[keep]


def rule_np(off, adj, metric, q, part=0, nparts=1):
    S, A = all_scores_np(off, adj, metric)
    u, v = nonedges(A, part, nparts)
    return rule_from_pairs(u, v, S[u, v], q)


def compare_tolerant(gold, got):
    """the Adamic-Adar / Resource rule: `gold` and `got` are (u, v, scores), worst first"""
    gu, gv, gs = gold
    u, v, s = got
    assert len(s) == len(gs)
    assert np.all(np.abs(np.asarray(s) - gs) <= 1e-12 * np.abs(gs)), float(np.max(np.abs(np.asarray(s) - gs) / np.maximum(np.abs(gs), 1e-300)))
    i = 0
    while i < len(gs):
        j = i + 1
        while j < len(gs) and abs(gs[j] - gs[j - 1]) <= 1e-9 * abs(gs[j]):
            j += 1
        assert set(zip(gu[i:j].tolist(), gv[i:j].tolist())) == set(zip(np.asarray(u[i:j]).tolist(), np.asarray(v[i:j]).tolist())), (i, j)
        i = j


def check_against_record(rec, got):
    """`got` = (u, v, scores) of the rule with q = rec["q"]: exact for the count-based metrics, the tolerance rule for the other two"""
    u, v, s = got
    assert len(s) == rec["found"]
    assert rec["padding"] == (rec["q"] - rec["found"] if rec["found"] else 1)
    gold = decode(rec)
    if rec["metric"] in TOLERANT:
        compare_tolerant(gold, got)
    else:
        if gold is not None:
            assert np.array_equal(gold[0], u) and np.array_equal(gold[1], v)
            assert np.array_equal(gold[2].view(np.uint64), np.asarray(s, dtype=np.float64).view(np.uint64))
        assert digest(u, v, s) == rec["sha256"]


def test_goldens_are_complete():
    assert len(GRAPH_KEYS) == 9 and {"kronecker_8_4", "kronecker_10_8", "uniform_8_4"} <= set(GRAPH_KEYS)
    seen = {(r["graph"], r["metric"], r["q_requested"]) for r in RECORDS}
    assert seen == {(g, m, q) for g in GRAPH_KEYS for m in METRICS for q in (1, 7, 100, 2000)}
    for r in RECORDS:
        assert r["metric"] in TOLERANT or r["q"] == r["q_requested"]
        gold = decode(r)
        assert (gold is None) == (r["form"] == "sha256") and (r["form"] != "sha256" or r["metric"] not in TOLERANT)
        if gold is not None:
            assert len(gold[2]) == r["found"] and digest(*gold) == r["sha256"]
            assert np.all(gold[0] < gold[1]) and np.all(np.diff(gold[2]) >= 0)
    assert os.path.getsize(os.path.join(GOLDEN, "link_prediction.json")) <= 200 * 1024
    # the classes are live: isolated vertices in the two kronecker graphs (Jaccard's 1.0 pairs, Overlap's excluded ones)
    assert any(r["metric"] == "jaccard" and r["graph"].startswith("kronecker") and r["form"] == "literal" and r["scores_rle"][-1][0] == (1.0).hex()
               for r in RECORDS)
    assert any(r["found"] == 0 and r["padding"] == 1 for r in RECORDS) and any(0 < r["found"] < r["q"] for r in RECORDS)


@pytest.mark.parametrize("key", GRAPH_KEYS)
def test_rule_restatement_reproduces_the_reference(capi, key):
    csr = golden_csr(capi, key)
    off, adj = csr.offsets(), csr.neighbors()
    assert (off.size - 1, adj.size) == (LP["graphs"][key]["n"], LP["graphs"][key]["nnz"])
    for mi, metric in enumerate(METRICS):
        S, A = all_scores_np(off, adj, mi)
        u, v = nonedges(A)
        s = S[u, v]
        for rec in (r for r in RECORDS if r["graph"] == key and r["metric"] == metric):
            check_against_record(rec, rule_from_pairs(u, v, s, rec["q"]))


def test_precision_golden_restated(capi):
    from conftest import host_graph
    for p in LP["precision"]:
        csr = host_graph(capi, p["generator"], p["scale"], p["degree"], p["relabel"])
        train, test_u, test_v = split_np(capi, csr, p["seed"], p["test_fraction"])
        assert test_u.size == p["true_count"] == p["q"]
        u, v, s = rule_np(train.offsets(), train.neighbors(), p["metric"], p["q"])
        assert digest(u, v, s) == p["prediction_sha256"]
        tp = len(set(zip(u.tolist(), v.tolist())) & set(zip(test_u.tolist(), test_v.tolist())))
        assert tp == p["true_positives"]
        assert float.fromhex(p["precision"]) == tp / float(p["q"]) and float.fromhex(p["recall"]) == tp / float(p["true_count"])
    assert any(p["true_positives"] > 0 for p in LP["precision"])


def split_np(capi, csr, seed, fraction):
    """the fixed split of the generator: a seeded permutation of the undirected edges; returns (train HostCSR, test u, test v)"""
    off, adj = np.array(csr.offsets()), np.array(csr.neighbors())
    n = off.size - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    keep = src < adj
    eu, ev = src[keep].astype(np.int32), adj[keep].astype(np.int32)
    perm = np.random.RandomState(seed).permutation(eu.size)
    n_test = int(fraction * eu.size)
    te, tr = perm[:n_test], perm[n_test:]
    return capi.HostCSR.from_edges(eu[tr], ev[tr], num_nodes=n), eu[te], ev[te]


def test_rule_restatement_on_shapes():
    def csr_of(edges, n):
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        e = np.concatenate([e, e[:, ::-1]])
        e = e[np.lexsort((e[:, 1], e[:, 0]))]
        return np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]), e[:, 1]
    # five isolated vertices: Jaccard ranks all ten pairs at 1.0, lexicographic (worst first = reversed); Overlap has no candidate
    off, adj = csr_of([], 5)
    u, v, s = rule_np(off, adj, "jaccard", 100)
    assert list(zip(u.tolist(), v.tolist())) == [(a, b) for a in range(5) for b in range(a + 1, 5)][::-1] and np.all(s == 1.0)
    assert rule_np(off, adj, "overlap", 100)[0].size == 0
    # K5: no non-edge
    assert rule_np(*csr_of([(a, b) for a in range(5) for b in range(a)], 5), "common", 3)[0].size == 0
    # two triangles and two isolated vertices, Jaccard: the isolated pair first, then the ZERO pairs lexicographically
    off, adj = csr_of([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)], 8)
    u, v, s = rule_np(off, adj, "jaccard", 3)
    assert list(zip(u.tolist(), v.tolist(), s.tolist())) == [(0, 4, 0.0), (0, 3, 0.0), (6, 7, 1.0)]


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_link_prediction", "gmsx_link_prediction_precision"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert {"LP_LDS_MAXN", "LP_SLAB_MB"} <= set(capi.option_names())
    assert ctypes.sizeof(capi.LinkPredictionInfo) == 32
    assert callable(capi.merge_link_predictions)
    if not _have_gpu():  # no host path: both refuse with "no HIP device" before they look at the graph
        fake = ctypes.create_string_buffer(1 << 16)
        out = (ctypes.c_int32 * 4)()
        sc = (ctypes.c_double * 4)()
        info = capi.LinkPredictionInfo()
        rc = capi.lib().gmsx_link_prediction(ctypes.cast(fake, ctypes.c_void_p), 0, 4, 0, 1, ctypes.cast(out, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p),
                                             ctypes.cast(sc, ctypes.c_void_p), 4, ctypes.byref(info), None)
        assert rc == capi.ERR_NO_DEVICE
        rc = capi.lib().gmsx_link_prediction_precision(ctypes.cast(fake, ctypes.c_void_p), 0, None, None, None, None, None, None, None)
        assert rc == capi.ERR_NO_DEVICE


def test_merge_link_predictions(capi):
    u = np.array([5, 0, 2], dtype=np.int32)
    v = np.array([6, 3, 9], dtype=np.int32)
    s = np.array([0.0, 0.5, 0.5])
    w = (np.array([1, 0], dtype=np.int32), np.array([2, 1], dtype=np.int32), np.array([0.0, 0.5]))
    mu, mv, ms = capi.merge_link_predictions([(u, v, s), w], 4)
    assert list(zip(mu.tolist(), mv.tolist(), ms.tolist())) == [(1, 2, 0.0), (2, 9, 0.5), (0, 3, 0.5), (0, 1, 0.5)]
