"""The goldens of gmsx_cycle4_count / gmsx_motif_census4 (tests/golden/motifs.json, motifs.npz; tools/make_golden_motifs.py) against three
statements that share no code with the device and none with each other:
  enumerator   every 3- and 4-subset of the vertices, literally (graphs of at most 40 vertices)
  census_np    the sparse A·A restatement: 4-cycles = ½ Σ_{u<w} C((A²)_uw, 2), the other motifs from their definitions
  closed forms K_n, K_{a,b}, Q_4, the 8×8 grid, Petersen, C_n
and the induced / non-induced identities of include/gmsx.h, Σ at_vertex = 4 · cycle4, and the rule's own diagnostics (wedges_walked,
max_codegree) restated in rank ids.  No GPU."""
import hashlib
import itertools
import json
import os
from math import comb

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, edges_to_csr, host_graph

MOTIFS = ("wedge", "triangle", "star3", "path4", "paw", "cycle4", "diamond", "clique4")
AUT = {"star3": 6, "path4": 2, "paw": 2, "cycle4": 8, "diamond": 4, "clique4": 24}
# the connected 4-vertex motifs as edge lists on the vertices 0 .. 3 (patterns of gmsx_subgraph_match in the GPU tests)
PATTERNS = {"star3": [(0, 1), (0, 2), (0, 3)], "path4": [(0, 1), (1, 2), (2, 3)], "paw": [(0, 1), (1, 2), (0, 2), (2, 3)],
            "cycle4": [(0, 1), (1, 2), (2, 3), (3, 0)], "diamond": [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)],
            "clique4": [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i8").tobytes()).hexdigest()


def load():
    path = os.path.join(GOLDEN, "motifs.json")
    if not os.path.exists(path):
        return {}, {}
    with open(path) as f:
        recs = json.load(f)
    return recs, np.load(os.path.join(GOLDEN, "motifs.npz"))


RECS, ARR = load()


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------------
def complete(n):
    return n, [(i, j) for i in range(n) for j in range(i + 1, n)]


def bipartite(a, b):
    return a + b, [(i, a + j) for i in range(a) for j in range(b)]


def cycle(n):
    return n, [(i, (i + 1) % n) for i in range(n)]


def hypercube(d):
    return 1 << d, [(v, v ^ (1 << b)) for v in range(1 << d) for b in range(d) if v < v ^ (1 << b)]


def grid(r, c):
    e = [(i * c + j, i * c + j + 1) for i in range(r) for j in range(c - 1)] + [(i * c + j, (i + 1) * c + j) for i in range(r - 1) for j in range(c)]
    return r * c, e


def petersen():
    return 10, [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]


def wheel(rim):
    return rim + 1, [(0, 1 + i) for i in range(rim)] + [(1 + i, 1 + (i + 1) % rim) for i in range(rim)]


def friendship(k):
    return 2 * k + 1, [e for i in range(k) for e in ((0, 2 * i + 1), (0, 2 * i + 2), (2 * i + 1, 2 * i + 2))]


CLOSED = {"K_4": complete(4), "K_5": complete(5), "K_33": complete(33), "K_65": complete(65), "K_2_2": bipartite(2, 2), "K_3_64": bipartite(3, 64),
          "K_65_130": bipartite(65, 130), "C_4": cycle(4), "C_5": cycle(5), "C_64": cycle(64), "Q_4": hypercube(4), "grid_8x8": grid(8, 8),
          "petersen": petersen(), "star_300": bipartite(1, 300), "wheel_7": wheel(7), "friendship_40": friendship(40)}
GENERATED = {"kronecker_8_8": ("kronecker", 8, 8, True), "kronecker_10_16": ("kronecker", 10, 16, True), "kronecker_10_16_raw": ("kronecker", 10, 16, False),
             "uniform_10_8": ("uniform", 10, 8, True), "kronecker_12_16": ("kronecker", 12, 16, True)}
CLOSED_C4 = {"K_4": 3 * comb(4, 4), "K_5": 3 * comb(5, 4), "K_33": 3 * comb(33, 4), "K_65": 3 * comb(65, 4), "K_2_2": 1, "K_3_64": comb(3, 2) * comb(64, 2),
             "K_65_130": comb(65, 2) * comb(130, 2), "C_4": 1, "C_5": 0, "C_64": 0, "Q_4": 24, "grid_8x8": 49, "petersen": 0, "star_300": 0}


def variant(n, edges, how):
    """the graph itself, with 7 isolated vertices appended, or as two disjoint copies"""
    if how == "isolated":
        return n + 7, list(edges)
    if how == "twice":
        return 2 * n, list(edges) + [(a + n, b + n) for a, b in edges]
    return n, list(edges)


def arrays_of(n, edges):
    """(off int64[n + 1], adj int32[nnz]) of the symmetric CSR of an edge list, rows ascending"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    a = sp.coo_matrix((np.ones(2 * len(e), dtype=np.int64), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n)).tocsr()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int32)


def golden_csr(capi, key):
    if key in CLOSED:
        return edges_to_csr(capi, CLOSED[key][1], n=CLOSED[key][0])
    kind, scale, deg, relabel = GENERATED[key]
    return host_graph(capi, kind, scale, deg, relabel)


# ---- the restatements -----------------------------------------------------------------------------------------------------------------------
def induced_from(sub):
    """the induced counts the identities of include/gmsx.h derive from the non-induced ones"""
    ind = {"clique4": sub["clique4"]}
    ind["diamond"] = sub["diamond"] - 6 * ind["clique4"]
    ind["cycle4"] = sub["cycle4"] - ind["diamond"] - 3 * ind["clique4"]
    ind["paw"] = sub["paw"] - 4 * ind["diamond"] - 12 * ind["clique4"]
    ind["star3"] = sub["star3"] - ind["paw"] - 2 * ind["diamond"] - 4 * ind["clique4"]
    ind["path4"] = sub["path4"] - 2 * ind["paw"] - 4 * ind["cycle4"] - 6 * ind["diamond"] - 12 * ind["clique4"]
    ind["triangle"] = sub["triangle"]
    ind["wedge"] = sub["wedge"] - 3 * sub["triangle"]
    return ind


def rank_ids(off):
    """rank[v]: position of v by decreasing (degree, id) — the device's rank ids"""
    deg = np.diff(off)
    order = np.lexsort((-np.arange(deg.size), -deg))
    rank = np.empty(deg.size, dtype=np.int64)
    rank[order] = np.arange(deg.size)
    return rank


def census_np(off, adj):
    """{subgraphs, induced, at_vertex, wedges_walked, max_codegree} by sparse matrix products and the definitions; Python integers throughout"""
    n = off.size - 1
    deg = np.diff(off).astype(np.int64)
    a = sp.csr_matrix((np.ones(adj.size, dtype=np.int64), adj.astype(np.int64), off), shape=(n, n))
    a2 = (a @ a).tocsr()
    a2.setdiag(0)
    a2.eliminate_zeros()
    pairs = sp.csr_matrix(((a2.data * (a2.data - 1)) // 2, a2.indices, a2.indptr), shape=(n, n))
    at_vertex = np.asarray(pairs.sum(axis=1)).ravel().astype(np.int64)   # Σ_{w != v} C((A²)_vw, 2)
    ordered = int(at_vertex.astype(object).sum())   # every cycle at its four vertices = ½ Σ_{u<w} C((A²)_uw, 2) four times
    assert ordered % 4 == 0
    sup_m = a.multiply(a2).tocoo()   # support of every arc
    src = np.repeat(np.arange(n), deg)
    sup = np.zeros(adj.size, dtype=np.int64)
    lookup = {}
    if sup_m.nnz:
        key = sup_m.row.astype(np.int64) * n + sup_m.col
        lookup = dict(zip(key.tolist(), sup_m.data.tolist()))
    for j in range(adj.size):
        sup[j] = lookup.get(int(src[j]) * n + int(adj[j]), 0)
    up = src < adj
    eu, ev, es = src[up], adj[up].astype(np.int64), sup[up]
    tri3 = int(es.astype(object).sum()) if es.size else 0
    assert tri3 % 3 == 0
    t = tri3 // 3
    t_v = np.bincount(src, weights=sup, minlength=n).astype(np.int64) // 2   # triangles at every vertex
    sub = {"wedge": sum(comb(int(d), 2) for d in deg), "star3": sum(comb(int(d), 3) for d in deg), "triangle": t,
           "path4": sum((int(deg[u]) - 1) * (int(deg[v]) - 1) for u, v in zip(eu, ev)) - 3 * t,
           "paw": sum(int(tv) * (int(d) - 2) for tv, d in zip(t_v, deg)),
           "cycle4": ordered // 4, "diamond": sum(comb(int(s), 2) for s in es)}
    # 4-cliques from the definition: the edges inside the common neighbourhood of every edge, each clique met at its six edges
    rows = [set(adj[off[v]:off[v + 1]].tolist()) for v in range(n)]
    k4 = 0
    for u, v, s in zip(eu, ev, es):
        if s < 2:
            continue
        common = sorted(rows[u] & rows[v])
        k4 += sum(1 for i, p in enumerate(common) for q in common[i + 1:] if q in rows[p])
    assert k4 % 6 == 0
    sub["clique4"] = k4 // 6
    # the rule's diagnostics, in rank ids: F = arcs to a later vertex, W = F A restricted to later opposite vertices
    rank = rank_ids(off)
    ar = sp.csr_matrix((np.ones(adj.size, dtype=np.int64), (rank[src], rank[adj])), shape=(n, n))
    f = sp.triu(ar, k=1).tocsr()
    walked = np.asarray(f.sum(axis=1)).ravel() >= 2   # sources with at least two later neighbours
    w = sp.triu(sp.diags(walked.astype(np.int64)) @ f @ ar, k=1).tocsr()
    wedges = int(w.data.astype(object).sum()) if w.nnz else 0
    assert sum(int(c) * (int(c) - 1) // 2 for c in w.data) == sub["cycle4"]   # the rule counts every cycle once
    return {"subgraphs": sub, "induced": induced_from(sub), "at_vertex": at_vertex, "wedges_walked": wedges,
            "max_codegree": int(w.data.max()) if w.nnz else 0}


def _classify(mask, pairs):
    """the connected spanning motif that the edges of `mask` form on four vertices, or None"""
    degs = [0, 0, 0, 0]
    m = 0
    for b, (i, j) in enumerate(pairs):
        if mask >> b & 1:
            degs[i] += 1
            degs[j] += 1
            m += 1
    degs.sort()
    return {(3, (1, 1, 1, 3)): "star3", (3, (1, 1, 2, 2)): "path4", (4, (1, 2, 2, 3)): "paw", (4, (2, 2, 2, 2)): "cycle4",
            (5, (2, 2, 3, 3)): "diamond", (6, (3, 3, 3, 3)): "clique4"}.get((m, tuple(degs)))


def enumerate_literally(n, edges):
    """(subgraphs, induced) by visiting every 3-subset and every 4-subset of the vertices and, inside a 4-subset, every subset of its edges"""
    adjm = np.zeros((n, n), dtype=bool)
    for a, b in edges:
        adjm[a, b] = adjm[b, a] = True
    pairs = list(itertools.combinations(range(4), 2))
    table = []
    for mask in range(64):
        copies = dict.fromkeys(AUT, 0)
        for subm in range(64):
            if subm & ~mask == 0 and _classify(subm, pairs):
                copies[_classify(subm, pairs)] += 1
        table.append((copies, _classify(mask, pairs)))
    sub, ind = dict.fromkeys(MOTIFS, 0), dict.fromkeys(MOTIFS, 0)
    for q in itertools.combinations(range(n), 4):
        mask = sum(1 << b for b, (i, j) in enumerate(pairs) if adjm[q[i], q[j]])
        copies, kind = table[mask]
        for k, c in copies.items():
            sub[k] += c
        if kind:
            ind[kind] += 1
    for q in itertools.combinations(range(n), 3):
        e = int(adjm[q[0], q[1]]) + int(adjm[q[0], q[2]]) + int(adjm[q[1], q[2]])
        sub["wedge"] += {2: 1, 3: 3}.get(e, 0)
        ind["wedge"] += e == 2
        sub["triangle"] += e == 3
        ind["triangle"] += e == 3
    return sub, ind


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_complete():
    assert set(RECS) == set(CLOSED) | set(GENERATED)


@pytest.mark.parametrize("key", sorted(CLOSED))
def test_closed_form_records(key):
    rec = RECS[key]
    n, edges = CLOSED[key]
    off, adj = arrays_of(n, edges)
    got = census_np(off, adj)
    assert got["subgraphs"] == rec["subgraphs"] and got["induced"] == rec["induced"]
    assert (got["wedges_walked"], got["max_codegree"]) == (rec["wedges_walked"], rec["max_codegree"])
    assert sha(got["at_vertex"]) == rec["at_vertex_sha256"] and np.array_equal(ARR["at_" + key], got["at_vertex"])
    assert int(got["at_vertex"].sum()) == 4 * rec["subgraphs"]["cycle4"]
    assert induced_from(rec["subgraphs"]) == rec["induced"] and all(v >= 0 for v in rec["induced"].values())
    if key in CLOSED_C4:
        assert rec["subgraphs"]["cycle4"] == CLOSED_C4[key]
    if n <= 40:
        assert rec["enumerated"]
        sub, ind = enumerate_literally(n, edges)
        assert sub == rec["subgraphs"] and ind == rec["induced"]


@pytest.mark.parametrize("n", range(3, 12))
def test_cycles_have_a_four_cycle_only_at_four(n):
    off, adj = arrays_of(*cycle(n))
    assert census_np(off, adj)["subgraphs"]["cycle4"] == (1 if n == 4 else 0)


@pytest.mark.parametrize("how", ["isolated", "twice"])
@pytest.mark.parametrize("key", ["K_5", "K_2_2", "wheel_7", "petersen", "friendship_40"])
def test_variants_scale_as_expected(key, how):
    """what the GPU tests assume of the two variants of every closed-form graph"""
    rec, f = RECS[key], 2 if how == "twice" else 1
    got = census_np(*arrays_of(*variant(*CLOSED[key], how)))
    assert got["subgraphs"] == {k: f * v for k, v in rec["subgraphs"].items()} and got["induced"] == {k: f * v for k, v in rec["induced"].items()}
    assert (got["wedges_walked"], got["max_codegree"]) == (f * rec["wedges_walked"], rec["max_codegree"])


@pytest.mark.parametrize("key", sorted(GENERATED))
def test_generated_records(capi, key):
    rec, csr = RECS[key], golden_csr(capi, key)
    off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32)
    assert (off.size - 1, adj.size) == (rec["n"], rec["nnz"])
    assert induced_from(rec["subgraphs"]) == rec["induced"] and all(v >= 0 for v in rec["induced"].values())
    at = ARR["at_" + key]
    assert sha(at) == rec["at_vertex_sha256"] and int(at.sum()) == 4 * rec["subgraphs"]["cycle4"]
    if rec["n"] <= 1024:   # the restatement again, where it takes a second or two
        got = census_np(off, adj)
        assert got["subgraphs"] == rec["subgraphs"] and np.array_equal(got["at_vertex"], at)
        assert (got["wedges_walked"], got["max_codegree"]) == (rec["wedges_walked"], rec["max_codegree"])


def test_random_graphs_enumerator_against_restatement():
    rng = np.random.default_rng(4)
    for n, p in ((6, 0.5), (9, 0.3), (11, 0.7), (12, 1.0)):
        edges = [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < p]
        got = census_np(*arrays_of(n, edges))
        sub, ind = enumerate_literally(n, edges)
        assert got["subgraphs"] == sub and got["induced"] == ind


def test_bindings_and_options(capi):
    assert capi.MOTIFS == MOTIFS
    assert {"C4_LDS_SPAN", "C4_SLAB_MB", "C4_SPLIT_WEDGES"} <= set(capi.option_names())
    import ctypes as C
    assert C.sizeof(capi.MotifInfo) == 8 * 8 * 2 + 8 + 4 + 4
    for name in ("gmsx_cycle4_count", "gmsx_cycle4_partial", "gmsx_motif_census4"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
