"""CPU: the goldens of the truss decomposition (tests/golden/truss.{json,npz}, written by tools/make_golden_truss.py from this project's own
serial bucket peel) agree with the level-synchronous peel gmsx_truss_decomposition is specified by (include/gmsx.h), restated here in numpy
over a triangle list with per-round masks:

  * the restatement reproduces every literal golden (support and trussness per arc, histogram, levels, top edges) bit for bit;
  * the triangles of each golden equal the compiled reference's count in tests/golden/graphs.json / testgraphs.json wherever both record the graph;
  * networkx.k_truss(G, k) equals the golden's {truss >= k} edge set on the six file graphs (skipped where networkx is missing);
  * the restatement gives the values of the issue on the shapes tests/test_truss_gpu.py runs on the device;
  * both entry points are in capi.SYMBOLS and exported, and without a GPU they return GMSX_ERR_NO_DEVICE.

truss_np is what tests/test_truss_gpu.py checks the device against."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph, load_golden

TRUSS = load_golden("truss.json")
ARR = np.load(os.path.join(GOLDEN, "truss.npz"))
GRAPHS = load_golden("graphs.json")
FILES = load_golden("testgraphs.json")
LITERAL = sorted(k for k, r in TRUSS.items() if r["literal"])
FILE_KEYS = sorted(k for k, r in TRUSS.items() if r["source"]["kind"] == "file")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def edge_ids(off, adj):
    """(src per arc, eid per arc, eu, ev): edge ids are the u < v arcs in CSR order, carried by both arcs"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    up = src < adj
    eu, ev = src[up], adj[up]
    keys = eu * n + ev  # ascending: CSR order with ascending rows
    eid = np.searchsorted(keys, np.minimum(src, adj) * n + np.maximum(src, adj))
    assert eid.size == 0 or np.array_equal(keys[eid], np.minimum(src, adj) * n + np.maximum(src, adj))
    return src, eid, eu, ev


def triangles_np(off, adj):
    """the triangles u < v < w as three columns of edge ids: (u,v), (u,w), (v,w)"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    src, eid, eu, ev = edge_ids(off, adj)
    m = eu.size
    keys = eu * n + ev
    # for every edge (u, v) the entries w of row v above v; kept where (u, w) is an edge
    lens = off[ev + 1] - off[ev]
    total = int(lens.sum())
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    e_uv = np.repeat(np.arange(m, dtype=np.int64), lens)
    j = np.repeat(off[ev] - starts, lens) + np.arange(total, dtype=np.int64)
    w = adj[j]
    above = w > ev[e_uv]
    e_uv, j, w = e_uv[above], j[above], w[above]
    k_uw = eu[e_uv] * n + w
    at = np.minimum(np.searchsorted(keys, k_uw), max(m - 1, 0))
    hit = keys[at] == k_uw if m else np.zeros(0, dtype=bool)
    return e_uv[hit], at[hit], eid[j[hit]]


def truss_np(off, adj):
    """The peel of include/gmsx.h: l rises to the smallest remaining support; then rounds until none applies — in a round every remaining
    edge of remaining support <= l leaves at once (trussness l + 2, round = running index); a triangle whose three edges were all remaining
    at the start of the round and of which at least one leaves is destroyed, and each of its edges that stays loses one.
    Returns (truss, round_of, rounds, levels, support): the arrays per ARC, parallel to adj."""
    src, eid, eu, ev = edge_ids(off, adj)
    m = eu.size
    t = triangles_np(off, adj)
    sup = sum(np.bincount(c, minlength=m) for c in t).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    support = sup.copy()
    truss, rnd = np.zeros(m, dtype=np.int32), np.full(m, -1, dtype=np.int32)
    alive, tri_alive = np.ones(m, dtype=bool), np.ones(t[0].size, dtype=bool)
    left, r, l, levels = m, 0, 0, 0
    while left:
        l = max(l, int(sup[alive].min()))
        levels += 1
        while True:
            f = alive & (sup <= l)
            nf = int(f.sum())
            if nf == 0:
                break
            truss[f], rnd[f] = l + 2, r
            r += 1
            live = np.flatnonzero(tri_alive)
            cols = [c[live] for c in t]
            hit = f[cols[0]] | f[cols[1]] | f[cols[2]]
            for c in cols:
                stay = hit & ~f[c]
                sup -= np.bincount(c[stay], minlength=m)
            tri_alive[live[hit]] = False
            alive &= ~f
            left -= nf
    return truss[eid], rnd[eid], r, levels, support[eid].astype(np.int32)


def golden_csr(capi, key):
    src = TRUSS[key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def info_of(truss, support, src, adj):
    """the gmsx_truss_info integers that follow from the per-arc arrays (rounds and levels come from the peel)"""
    up = src < adj
    vals, counts = np.unique(truss[up], return_counts=True)
    return {"max_truss": int(vals.max()) if vals.size else 0, "levels": int(vals.size), "top_edges": int(counts[-1]) if vals.size else 0,
            "max_support": int(support.max()) if support.size else 0, "triangles": int(support.sum()) // 6}


def csr_of(edges, n):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = np.concatenate([e, e[:, ::-1]])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    return np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]).astype(np.int64), e[:, 1].astype(np.int32)


# ---- the shapes of the issue (tests/test_truss_gpu.py runs the same on the device) -------------------------------------------------------------
def clique(ids):
    ids = list(ids)
    return [(ids[i], ids[j]) for i in range(len(ids)) for j in range(i)]


def cylinder(L):
    """triangulated cylinder, rings of 4: (r, j) joined to (r, j+1), (r+1, j), (r+1, j+1)"""
    e = []
    for r in range(L):
        for j in range(4):
            e.append((4 * r + j, 4 * r + (j + 1) % 4))
            if r + 1 < L:
                e += [(4 * r + j, 4 * (r + 1) + j), (4 * r + j, 4 * (r + 1) + (j + 1) % 4)]
    return e


def book(P, k6=False):
    """edge (0, 1) plus P pages adjacent to both; with k6 a K6 on 0, 1 and four more vertices"""
    e = [(0, 1)] + [(a, 2 + i) for i in range(P) for a in (0, 1)]
    if k6:
        ids = [0, 1] + list(range(2 + P, 6 + P))
        e += [p for p in clique(ids) if set(p) != {0, 1}]
    return e


def k6_plus_strip():
    """a K6 and, hanging off one of its edges, a strip of 20 triangles: 15 edges of truss 6, 40 of truss 3"""
    e = clique(range(6))
    a, b = 0, 1
    for x in range(6, 26):  # each new vertex closes one triangle over the strip's last edge
        e += [(a, x), (b, x)]
        a, b = b, x
    return e


PLANTED = {"rounds": 37, "levels": 5, "most_rounds_in_a_level": 29, "max_truss": 14, "top_edges": 91}  # of planted(): the issue's figures


def rounds_per_level(truss, rnd):
    """{trussness: rounds in which edges of that trussness leave}"""
    return {int(t): int(np.unique(rnd[truss == t]).size) for t in np.unique(truss)}


def planted(seed=20, n=300, m=4000, k=14):
    """a seeded G(n, m) with a planted K_k (seed 20: 37 rounds, 29 of them in one level, max truss 14)"""
    rng = np.random.RandomState(seed)
    pairs = set()
    while len(pairs) < m:
        a, b = rng.randint(0, n, 2)
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    ids = rng.choice(n, k, replace=False)
    pairs |= {(min(a, b), max(a, b)) for a, b in clique(ids)}
    return sorted(pairs)


SHAPES = {
    # name: (edges, n, expected histogram {truss: edges}, rounds, levels)
    "one edge": ([(0, 1)], 2, {2: 1}, 1, 1),
    "triangle": (clique(range(3)), 3, {3: 3}, 1, 1),
    "K5": (clique(range(5)), 5, {5: 10}, 1, 1),
    "C6": ([(i, (i + 1) % 6) for i in range(6)], 6, {2: 6}, 1, 1),
    "two K5 sharing an edge": (clique(range(5)) + [p for p in clique([0, 1, 5, 6, 7]) if set(p) != {0, 1}], 8, {5: 19}, 2, 1),
    "square of a path on 41": ([(i, i + 1) for i in range(40)] + [(i, i + 2) for i in range(39)], 41, {3: 79}, 2, 1),
    "cylinder of 501 rings": (cylinder(501), 4 * 501, {3: 12 * 501 - 8}, 501, 1),
    "book of 1500": (book(1500), 1502, {3: 3001}, 2, 1),
    "book of 1500 with a K6": (book(1500, k6=True), 1506, {3: 3000, 6: 15}, None, 2),
    "book of 40000": (book(40000), 40002, {3: 80001}, 2, 1),
}


def test_goldens_are_complete():
    want = {"file_eppsteinExample", "file_micro", "file_smallRandom1", "file_tomitaExample", "file_triangles_1", "file_triangles_3",
            "kronecker_8_16", "kronecker_10_16", "kronecker_12_16", "kronecker_14_16", "kronecker_16_16", "kronecker_12_4", "kronecker_10_8_raw",
            "uniform_10_16", "uniform_12_16", "rmat_12_38"}
    assert set(TRUSS) == want
    for key, rec in TRUSS.items():
        assert rec["literal"] == (rec["m"] <= 50000) == ("truss_" + key in ARR) == ("support_" + key in ARR)
        assert sum(rec["hist"].values()) == rec["m"] and len(rec["hist"]) == rec["levels"] and rec["max_truss"] >= 2
        assert rec["hist"][str(rec["max_truss"])] == rec["top_edges"] and min(int(k) for k in rec["hist"]) >= 2
    assert any(not r["literal"] for r in TRUSS.values())


@pytest.mark.parametrize("key", sorted(TRUSS))
def test_triangles_equal_the_compiled_reference(key):
    rec = TRUSS[key]
    checked = 0
    if rec["graphs_key"] and "triangles" in GRAPHS[rec["graphs_key"]]:
        g = GRAPHS[rec["graphs_key"]]
        assert (g["n"], g["m"], g["triangles"]) == (rec["n"], rec["m"], rec["triangles"])
        checked += 1
    if rec["source"]["kind"] == "file":
        g = FILES[rec["source"]["name"]]
        assert (g["n"], g["m"], g["triangles"]) == (rec["n"], rec["m"], rec["triangles"])
        checked += 1
    if not checked:
        assert rec["graphs_key"] is None or "triangles" not in GRAPHS[rec["graphs_key"]]  # (nothing recorded to compare with)


@pytest.mark.parametrize("key", LITERAL)
def test_peel_restatement_reproduces_the_golden(capi, key):
    rec, csr = TRUSS[key], golden_csr(capi, key)
    off, adj = csr.offsets(), csr.neighbors()
    assert (off.size - 1, adj.size) == (rec["n"], rec["nnz"])
    truss, rnd, rounds, levels, support = truss_np(off, adj)
    assert np.array_equal(truss, ARR["truss_" + key]) and np.array_equal(support, ARR["support_" + key])
    assert sha(truss) == rec["truss_sha256"] and sha(support) == rec["support_sha256"]
    src = edge_ids(off, adj)[0]
    info = info_of(truss, support, src, adj)
    assert info == {k: rec[k] for k in info} and levels == rec["levels"]
    up = src < adj
    assert {str(int(v)): int(c) for v, c in zip(*np.unique(truss[up], return_counts=True))} == rec["hist"]
    assert rounds == int(rnd.max()) + 1 and rnd.min() == 0 and rounds >= levels
    # both arcs of an edge carry the same values
    _, eid, _, _ = edge_ids(off, adj)
    for a in (truss, rnd, support):
        first = np.zeros(rec["m"], dtype=a.dtype)
        first[eid[up]] = a[up]
        assert np.array_equal(first[eid], a)


@pytest.mark.parametrize("key", FILE_KEYS)
def test_networkx_k_truss_equals_the_golden(capi, key):
    nx = pytest.importorskip("networkx")
    rec, csr = TRUSS[key], golden_csr(capi, key)
    off, adj = csr.offsets(), csr.neighbors()
    truss = ARR["truss_" + key]
    src = edge_ids(off, adj)[0]
    up = src < adj
    G = nx.Graph()
    G.add_nodes_from(range(rec["n"]))
    G.add_edges_from(zip(src[up].tolist(), np.asarray(adj)[up].tolist()))
    for k in range(2, rec["max_truss"] + 2):
        want = {(min(a, b), max(a, b)) for a, b in nx.k_truss(G, k).edges()}
        keep = up & (truss >= k)
        assert want == set(zip(src[keep].tolist(), np.asarray(adj)[keep].tolist())), k


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_peel_restatement_on_shapes(name):
    edges, n, hist, rounds, levels = SHAPES[name]
    off, adj = csr_of(edges, n)
    truss, rnd, got_rounds, got_levels, support = truss_np(off, adj)
    src = edge_ids(off, adj)[0]
    up = src < adj
    assert {int(v): int(c) for v, c in zip(*np.unique(truss[up], return_counts=True))} == hist
    assert got_levels == levels and (rounds is None or got_rounds == rounds)
    if name == "cylinder of 501 rings":
        assert int(support.sum()) // 6 == 8 * 500 and set(np.bincount(rnd[up]).tolist()) == {4, 8, 16}  # tiny frontiers throughout
    if name == "book of 1500 with a K6":
        assert int(support.max()) == 1504 and truss[(src == 0) & (adj == 1)].tolist() == [6]


def test_peel_restatement_on_k6_plus_strip_and_planted_clique():
    e = k6_plus_strip()
    off, adj = csr_of(e, max(max(p) for p in e) + 1)
    truss, rnd, rounds, levels, _ = truss_np(off, adj)
    up = edge_ids(off, adj)[0] < adj
    assert {int(v): int(c) for v, c in zip(*np.unique(truss[up], return_counts=True))} == {3: 40, 6: 15} and levels == 2
    e = planted()
    off, adj = csr_of(e, 300)
    truss, rnd, rounds, levels, _ = truss_np(off, adj)
    per_level = rounds_per_level(truss, rnd)
    up = edge_ids(off, adj)[0] < adj
    assert {"rounds": rounds, "levels": levels, "most_rounds_in_a_level": max(per_level.values()), "max_truss": int(truss.max()),
            "top_edges": int((truss[up] == truss.max()).sum())} == PLANTED
    assert rounds == int(rnd.max()) + 1 == sum(per_level.values()) and len(per_level) == levels


def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_edge_support", "gmsx_truss_decomposition"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert "TRUSS_WG_FRONTIER" in capi.option_names()
    assert ctypes.sizeof(capi.TrussInfo) == 32


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_entry_points_fail_loudly_without_gpu(capi):
    L = capi.lib()
    sup = np.full(4, -77, dtype=np.int32)
    info = capi.TrussInfo()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(1 << 16)))  # never read: both calls check the device before they read the handle
    assert L.gmsx_edge_support(fake, sup.ctypes.data_as(ctypes.c_void_p), None, None) == capi.ERR_NO_DEVICE
    assert L.gmsx_truss_decomposition(fake, sup.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert np.all(sup == -77) and info.max_truss == 0
