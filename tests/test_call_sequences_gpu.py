"""GPU: SEQUENCES of calls — what one call leaves behind for the next.  Every other GPU test uploads a graph, calls one family of entry points on
the fresh handle and frees it; here handles are freed and re-uploaded, two handles are live at once, options and ranks change between the two
calls of a listing, the lazy containers are built in every order, weights are attached, replaced and detached, and one seeded random
sequence mixes all of it.  Every result is held to a table that is built ONCE per graph on the host: the C oracle's counts, plain-Python
enumerations (maximal cliques, triangles) and the numpy restatements and checkers the suite already has.

The graphs (fixed seeds, ~100 vertices): A = G(96, 0.12) plus 5 isolated vertices; B = A after double edge swaps that keep every degree, hence
the offsets array, every vertex's rank id and d+ — the same n, nnz and shapes, other cliques; H = the hub with three cliques of
test_random_gpu.py.  pair_ab() asserts those properties on the host before any device call (test_graph_preconditions runs it without a device).

  a  a FILL call without a sizing call on a handle that was uploaded after another one was freed: the cached pass 1 of the freed handle
     (same address, same arrays, same n and nnz — host/list_key.hpp) must not be used
  b  two live handles, and two shards of one handle, through the one-entry cache
  c  an option set between sizing and fill      d  a rank given to the fill only
  e  the lazy triangle-count containers in six orders under four kinds of upload
  f  weights attached, replaced, detached, attached again
  g  80 seeded random operations over at most two live handles per graph
  h  a handle gives back what it took: free device memory over eight cycles of upload, build, count, free, and over eight refused builds
"""
import ctypes as C

import numpy as np
import pytest

import test_bk_list_gpu as bkl
from conftest import host_graph
import test_kcstar_list_gpu as kcs
import test_subgraph_gpu as sgm
from test_coloring_golden_cpu import jp_np
from test_core_golden_cpu import peel_np
from test_msf_golden_cpu import kruskal_np, labels_np
from test_pagerank_golden_cpu import EPS, pagerank_np, pr_bound
from test_random_gpu import _graphs as random_graphs
from test_sssp_golden_cpu import dijkstra_np, parent_np
from test_traversal_golden_cpu import bfs_np

gpu_test = pytest.mark.gpu

TRIANGLE = [(0, 1), (1, 2), (0, 2)]
PATH3 = [(0, 1), (1, 2)]
PR_ITERS = 5


# ---- the graphs, on the host ----------------------------------------------------------------------------------------------------------
def csr_of(n, edges):
    """(off int64[n + 1], adj int32[nnz]) of the symmetric graph over the u < v pairs `edges`, rows ascending"""
    e = np.asarray(sorted(set((min(a, b), max(a, b)) for a, b in edges)), dtype=np.int64).reshape(-1, 2)
    assert np.all(e[:, 0] < e[:, 1])
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    order = np.lexsort((dst, src))
    off = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    return off, dst[order].astype(np.int32)


def edges_of(off, adj):
    src = np.repeat(np.arange(off.size - 1), np.diff(off))
    return [(int(a), int(b)) for a, b in zip(src, adj) if a < b]


def device_rank(deg):
    """rank id of every vertex in the device's numbering: the vertices by decreasing (degree, id), rank id 0 the biggest hub"""
    n = deg.size
    order = np.lexsort((-np.arange(n), -deg))
    r = np.empty(n, dtype=np.int64)
    r[order] = np.arange(n)
    return r


def dplus_of(off, adj, r):
    src = np.repeat(np.arange(off.size - 1), np.diff(off))
    return np.bincount(src[r[adj] < r[src]], minlength=off.size - 1)


def gnp_isolated(n, p, isolated, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    return n + isolated, list(zip(iu[keep].tolist(), ju[keep].tolist()))


def degree_keeping_swaps(n, edges, swaps, seed):
    """`swaps` double edge swaps (a,b),(c,d) -> (a,d),(c,b) with max(r(a), r(c)) < min(r(b), r(d)) in the device's rank ids and both new edges
    absent.  a and c trade a neighbour of a higher rank id for another one, b and d one of a lower rank id: every degree, every rank id and
    every d+ stays.  The pairs are chosen with deg(a), deg(c) > deg(b), deg(d) strictly, so the condition holds however ties are ranked."""
    deg = np.bincount(np.asarray(edges).reshape(-1), minlength=n)
    r = device_rank(deg)
    es = set(edges)
    rng = np.random.default_rng(seed)
    done = 0
    for _ in range(100000):
        if done == swaps:
            break
        cur = sorted(es)
        (a, b), (c, d) = cur[int(rng.integers(len(cur)))], cur[int(rng.integers(len(cur)))]
        if r[a] > r[b]:
            a, b = b, a
        if r[c] > r[d]:
            c, d = d, c
        if len({a, b, c, d}) < 4 or min(deg[a], deg[c]) <= max(deg[b], deg[d]):
            continue
        assert max(r[a], r[c]) < min(r[b], r[d])
        new1, new2 = (min(a, d), max(a, d)), (min(c, b), max(c, b))
        if new1 in es or new2 in es:
            continue
        es -= {(min(a, b), max(a, b)), (min(c, d), max(c, d))}
        es |= {new1, new2}
        done += 1
    assert done == swaps
    return sorted(es)


def maximal_cliques(off, adj):
    """Bron–Kerbosch with a pivot over Python sets: the maximal cliques as a set of ascending tuples (an isolated vertex is the clique {v})"""
    n = off.size - 1
    nb = [set(adj[off[v]:off[v + 1]].tolist()) for v in range(n)]
    out = set()

    def expand(r, p, x):
        if not p and not x:
            out.add(tuple(sorted(r)))
            return
        pivot = max(p | x, key=lambda u: len(nb[u] & p))
        for v in sorted(p - nb[pivot]):
            expand(r + [v], p & nb[v], x & nb[v])
            p = p - {v}
            x = x | {v}

    expand([], set(range(n)), set())
    return out


def triangles(off, adj):
    """the triangles as a sorted list of ascending triples"""
    n = off.size - 1
    nb = [set(adj[off[v]:off[v + 1]].tolist()) for v in range(n)]
    return sorted((u, v, w) for u in range(n) for v in nb[u] if v > u for w in nb[u] & nb[v] if w > v)


_TABLES = {}


def table(name, n, edges, oracle):
    """every expected value of one graph, computed once on the host and never changed"""
    if name in _TABLES:
        return _TABLES[name]
    off, adj = csr_of(n, edges)
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), np.diff(off)), adj] = True
    deg = np.diff(off)
    tri = triangles(off, adj)
    T = len(tri)
    assert oracle.tc_total(off, adj) == T == int(np.trace(A.astype(np.int64) @ A @ A)) // 6
    cliques = maximal_cliques(off, adj)
    X = {"name": name, "n": n, "off": off, "adj": adj, "A": A, "edges": edges_of(off, adj), "T": T, "triangles": tri,
         "k": {k: oracle.kclique(off, adj, k) for k in (3, 4, 5)}, "bk": oracle.bk_count(off, adj), "cliques": cliques,
         "vc2": oracle.tc_vertex_count2(off, adj), "dmax": int(deg.max()), "ind_p3": int((deg * (deg - 1)).sum()) - 6 * T}
    # (the oracle's k-clique count is the reference's: every clique once per order of its members, as gmsx_kclique_count's first output)
    assert X["k"][3] == 6 * T and X["k"][4] % 24 == 0 and X["bk"] == len(cliques)
    X["star3"] = oracle.kclique_star_count(off, adj, 3)
    assert X["star3"] == (T, 4 * (X["k"][4] // 24))
    core, rnd, rounds, levels = peel_np(off, adj)
    order = np.lexsort((np.arange(n), rnd)).astype(np.int32)
    rank = np.empty(n, dtype=np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    dg = int(core.max())
    X["core"] = (core, rank, {"degeneracy": dg, "levels": levels, "rounds": rounds, "top_core": int((core == dg).sum())})
    e = np.asarray(X["edges"]).reshape(-1, 2)
    X["label"] = labels_np(n, e[:, 0], e[:, 1])
    X["bfs0"] = {d: bfs_np(off, adj, 0, direction=d) for d in (0, 1)}
    scores, info, errors = pagerank_np(off, adj, max_iters=PR_ITERS)
    # the iteration count is a fact: no sweep's error of the restatement is near the tolerance (the bound is ~1e-13)
    assert info["iterations"] == PR_ITERS and all(err > 1e-3 for err in errors), errors
    X["pr"] = (scores, info, pr_bound(PR_ITERS, 0.85, X["dmax"], EPS))
    X["jp"] = jp_np(off, adj, np.arange(n))
    _TABLES[name] = X
    return X


AB_SEED, AB_SWAPS = 11, 12


def pair_ab(oracle):
    """The tables of A and B, with the properties the sequence tests rest on asserted on the host."""
    n, ea = gnp_isolated(96, 0.12, 5, AB_SEED)
    eb = degree_keeping_swaps(n, ea, AB_SWAPS, AB_SEED + 1)
    a, b = table("A", n, ea, oracle), table("B", n, eb, oracle)
    assert np.array_equal(a["off"], b["off"]) and a["adj"].size == b["adj"].size and not np.array_equal(a["adj"], b["adj"])
    assert int((np.diff(a["off"]) == 0).sum()) >= 5
    r = device_rank(np.diff(a["off"]))
    assert np.array_equal(dplus_of(a["off"], a["adj"], r), dplus_of(b["off"], b["adj"], r))
    assert len(set(ea) ^ set(eb)) >= 2 * AB_SWAPS   # (4 per swap, unless a later swap undoes half of an earlier one)
    assert a["cliques"] != b["cliques"] and a["triangles"] != b["triangles"]
    # info.cliques of the three listings: maximal cliques; k = 3 cliques (with and without stars); triangle and induced 3-path embeddings
    assert a["bk"] != b["bk"] and a["T"] != b["T"] and a["ind_p3"] != b["ind_p3"]
    return a, b


def hub_table(oracle):
    name, n, edges = next(g for g in random_graphs(np.random.default_rng(2026)) if g[0] == "hub-cliques")
    return table("H", n, [tuple(int(x) for x in e) for e in edges], oracle)


def test_graph_preconditions(oracle):
    """CPU: A and B have equal offsets, other maximal cliques, other triangles and other counts in every listing; H is what it says."""
    a, b = pair_ab(oracle)
    h = hub_table(oracle)
    print(f"A: n {a['n']} nnz {a['adj'].size} bk {a['bk']} T {a['T']} ind_p3 {a['ind_p3']}; B: bk {b['bk']} T {b['T']} ind_p3 {b['ind_p3']}; "
          f"H: n {h['n']} nnz {h['adj'].size} bk {h['bk']} T {h['T']}")
    assert a["n"] == b["n"] == 101 and h["n"] <= 101
    assert max(len(c) for c in h["cliques"]) == 35 and h["T"] == sum(s * (s + 1) * (s - 1) // 6 for s in (5, 12, 34))


@pytest.fixture(scope="module")
def tabs(oracle):
    a, b = pair_ab(oracle)
    return {"A": a, "B": b, "H": hub_table(oracle)}


# ---- the three listings behind one interface ------------------------------------------------------------------------------------------
def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Listing:
    """raw(gpu, g, fill, ...) is ONE call of the C entry point — (status, info dict, arrays or None, stats dict); a fill gets arrays of `caps`
    entries, ample for every graph of this file, pre-filled with -7, and checks that nothing behind the list was written.  wrapper() is the
    binding's sizing + fill.  check() holds (info, arrays) of the WHOLE graph to the table."""

    def wrapper_bytes(self, arrays):
        return [None if a is None else a.tobytes() for a in arrays]

    def same(self, x, y):
        return self.wrapper_bytes(x) == self.wrapper_bytes(y)


class BkList(Listing):
    name = "bk_list"
    caps = (1 << 12, 1 << 14)

    def raw(self, gpu, g, fill, part=0, nparts=1, rank=None):
        info, st = gpu.BkListInfo(), gpu.Stats()
        rp = None if rank is None else ptr(rank)
        if not fill:
            rc = gpu.lib().gmsx_bk_list(g._h, rp, part, nparts, None, None, 0, 0, C.byref(info), C.byref(st))
            return rc, info.as_dict(), None, st.as_dict()
        off, mem = np.full(self.caps[0], -7, dtype=np.int64), np.full(self.caps[1], -7, dtype=np.int32)
        rc = gpu.lib().gmsx_bk_list(g._h, rp, part, nparts, ptr(off), ptr(mem), off.size, mem.size, C.byref(info), C.byref(st))
        d = info.as_dict()
        if rc != gpu.OK:
            return rc, d, None, st.as_dict()
        nc, nm = d["cliques"], d["members"]
        assert np.all(off[nc + 1:] == -7) and np.all(mem[nm:] == -7)
        return rc, d, (off[:nc + 1].copy(), mem[:nm].copy()), st.as_dict()

    def wrapper(self, g, part=0, nparts=1):
        return g.bk_list(part=part, nparts=nparts)

    def as_set(self, arrays):
        off, mem = arrays
        return [tuple(int(x) for x in c) for c in bkl.cliques_of(off, mem)]

    def check(self, X, info, arrays):
        off, mem = arrays
        assert info == bkl.info_of(off, mem) and info["cliques"] == X["bk"]
        bkl.check_cliques(X["off"], X["adj"], off, mem)
        got = self.as_set(arrays)
        assert len(got) == len(set(got)) and set(got) == X["cliques"]

    def want(self, X):
        return X["bk"]


class StarList(Listing):
    k = 3
    caps = (1 << 13, 1 << 18)   # cliques, star members

    def __init__(self, only):
        self.only = only
        self.name = "kclique_star_list(3, CLIQUES_ONLY)" if only else "kclique_star_list(3)"

    def raw(self, gpu, g, fill, part=0, nparts=1, rank=None):
        info, st = gpu.KcliqueStarListInfo(), gpu.Stats()
        flags = gpu.KCSTAR_CLIQUES_ONLY if self.only else gpu.KCSTAR_DEFAULT
        f = gpu.lib().gmsx_kclique_star_list
        if not fill:
            rc = f(g._h, self.k, flags, part, nparts, None, None, None, 0, 0, C.byref(info), C.byref(st))
            return rc, info.as_dict(), None, st.as_dict()
        cl = np.full(self.caps[0] * self.k, -7, dtype=np.int32)
        soff, mem = np.full(self.caps[0] + 1, -7, dtype=np.int64), np.full(self.caps[1], -7, dtype=np.int32)
        rc = f(g._h, self.k, flags, part, nparts, ptr(cl), None if self.only else ptr(soff), None if self.only else ptr(mem), self.caps[0],
               0 if self.only else self.caps[1], C.byref(info), C.byref(st))
        d = info.as_dict()
        if rc != gpu.OK:
            return rc, d, None, st.as_dict()
        nc, nm = d["cliques"], d["star_members"]
        assert np.all(cl[nc * self.k:] == -7)
        if self.only:
            assert nm == 0 and np.all(soff == -7) and np.all(mem == -7)
            return rc, d, (cl[:nc * self.k].reshape(nc, self.k).copy(), None, None), st.as_dict()
        assert np.all(soff[nc + 1:] == -7) and np.all(mem[nm:] == -7)
        return rc, d, (cl[:nc * self.k].reshape(nc, self.k).copy(), soff[:nc + 1].copy(), mem[:nm].copy()), st.as_dict()

    def wrapper(self, g, part=0, nparts=1):
        return g.kclique_star_list(self.k, cliques_only=self.only, part=part, nparts=nparts)

    def as_set(self, arrays):
        return [tuple(int(x) for x in row) for row in arrays[0]]

    def check(self, X, info, arrays):
        cl, soff, mem = arrays
        assert info == kcs.info_of(cl, soff, mem, self.k) and info["cliques"] == X["T"]
        assert info["star_members"] == (0 if self.only else X["star3"][1])
        kcs.check_pairs(X["off"], X["adj"], self.k, cl, soff, mem)
        assert sorted(self.as_set(arrays)) == X["triangles"]

    def want(self, X):
        return X["T"]


class Match(Listing):
    def __init__(self, name, pattern):
        self.name, self.pattern = name, pattern
        self.k = 3
        self.caps = (1 << 16,)   # embeddings

    def raw(self, gpu, g, fill, part=0, nparts=1, rank=None):
        po, pn = gpu.pattern_arrays(self.pattern)
        info, st = gpu.SubgraphInfo(), gpu.Stats()
        f = gpu.lib().gmsx_subgraph_match
        if not fill:
            rc = f(g._h, self.k, ptr(po), ptr(pn), gpu.SGM_INDUCED, part, nparts, None, 0, C.byref(info), C.byref(st))
            return rc, info.as_dict(), None, st.as_dict()
        maps = np.full(self.caps[0] * self.k, -7, dtype=np.int32)
        rc = f(g._h, self.k, ptr(po), ptr(pn), gpu.SGM_INDUCED, part, nparts, ptr(maps), self.caps[0], C.byref(info), C.byref(st))
        d = info.as_dict()
        if rc != gpu.OK:
            return rc, d, None, st.as_dict()
        ne = d["embeddings"]
        assert np.all(maps[ne * self.k:] == -7)
        return rc, d, (maps[:ne * self.k].reshape(ne, self.k).copy(),), st.as_dict()

    def wrapper(self, g, part=0, nparts=1):
        return (g.subgraph_match(self.pattern, induced=True, part=part, nparts=nparts),)

    def as_set(self, arrays):
        return [tuple(int(x) for x in row) for row in arrays[0]]

    def want(self, X):
        return 6 * X["T"] if self.pattern is TRIANGLE else X["ind_p3"]

    def check(self, X, info, arrays):
        rows = arrays[0]
        assert info["embeddings"] == rows.shape[0] == self.want(X) and info["k"] == self.k
        sgm.check_list(X["A"], self.pattern, info["order"], rows, True)


LISTINGS = [BkList(), StarList(False), StarList(True), Match("subgraph_match(triangle)", TRIANGLE), Match("subgraph_match(induced 3-path)", PATH3)]
LISTING_IDS = ["bk_list", "kcstar", "kcstar_cliques_only", "sgm_triangle", "sgm_path3"]


def info_count(L, info):
    return info["embeddings"] if isinstance(L, Match) else info["cliques"]


def upload(gpu, X, flags=0):
    return gpu.DeviceGraph.upload(X["off"], X["adj"], flags)


def test_caps_are_ample(oracle):
    """CPU: the capacities of the fill-only calls hold every list of this file"""
    a, b = pair_ab(oracle)
    for X in (a, b, hub_table(oracle)):
        assert X["bk"] + 1 <= BkList.caps[0] and sum(len(c) for c in X["cliques"]) <= BkList.caps[1]
        assert X["T"] <= StarList.caps[0] and X["star3"][1] <= StarList.caps[1]
        assert max(6 * X["T"], X["ind_p3"]) <= LISTINGS[3].caps[0]


# ---- a. fill without sizing after free and re-upload ----------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("L", LISTINGS, ids=LISTING_IDS)
def test_fill_without_sizing_after_free_and_reupload(gpu, tabs, L):
    """A, B, A, B: each uploaded after the one before it was freed, which left ITS pass 1 in the cache.  From the second turn on the first
    call on the new handle is a fill — legal (gmsx.h: a fill whose capacity is too small returns the sizes) — and must be X's list."""
    addresses = []
    for turn, name in enumerate("ABAB"):
        X = tabs[name]
        g = upload(gpu, X)
        try:
            addresses.append(int(g._h.value))
            first = None
            if turn >= 1:
                rc, info, first, _ = L.raw(gpu, g, fill=True)
                assert rc == gpu.OK, (L.name, turn, name, rc)
                freed = tabs["B" if name == "A" else "A"]
                assert info_count(L, info) == L.want(X), (L.name, turn, name, "the freed graph's count" if info_count(L, info) == L.want(freed) else "")
                L.check(X, info, first)
            got = L.wrapper(g)   # sizing + fill: leaves X in the cache
            rc, info, _, _ = L.raw(gpu, g, fill=False)
            assert rc == gpu.OK
            L.check(X, info, got)
            if first is not None:
                assert L.same(first, got), (L.name, turn, name)
        finally:
            g.free()
    repeats = sum(a in addresses[:i] for i, a in enumerate(addresses))
    print(f"{L.name}: the handle address repeated in {repeats} of {len(addresses) - 1} re-uploads")


# ---- b. two live handles, two shards --------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("L", LISTINGS, ids=LISTING_IDS)
def test_two_live_handles_through_the_one_entry_cache(gpu, tabs, L):
    ga, gb = upload(gpu, tabs["A"]), upload(gpu, tabs["B"])
    try:
        rc, ia, _, sa = L.raw(gpu, ga, fill=False)
        assert rc == gpu.OK and info_count(L, ia) == L.want(tabs["A"])
        rc, ib, _, _ = L.raw(gpu, gb, fill=False)   # evicts A's pass 1
        assert rc == gpu.OK and info_count(L, ib) == L.want(tabs["B"])
        rc, ia2, la, fa = L.raw(gpu, ga, fill=True)  # searches again, then fills
        assert rc == gpu.OK and ia2 == ia
        L.check(tabs["A"], ia2, la)
        assert fa["launches"] >= sa["launches"], (fa, sa)
        rc, ib2, lb, _ = L.raw(gpu, gb, fill=True)   # … and evicted B's
        assert rc == gpu.OK and ib2 == ib
        L.check(tabs["B"], ib2, lb)
        assert L.same(la, L.wrapper(ga)) and L.same(lb, L.wrapper(gb))
    finally:
        ga.free()
        gb.free()


@gpu_test
@pytest.mark.parametrize("L", LISTINGS, ids=LISTING_IDS)
def test_sizing_one_shard_then_filling_another(gpu, tabs, L):
    """size shard (0, 2), fill shard (1, 2): the result is shard 1's list — the two shards are disjoint and together the whole list"""
    X = tabs["A"]
    g = upload(gpu, X)
    try:
        rc, i0, _, _ = L.raw(gpu, g, fill=False, part=0, nparts=2)
        assert rc == gpu.OK
        rc, i1, l1, _ = L.raw(gpu, g, fill=True, part=1, nparts=2)
        assert rc == gpu.OK
        w1, w0 = L.wrapper(g, part=1, nparts=2), L.wrapper(g, part=0, nparts=2)
        assert L.same(l1, w1)
        s0, s1 = L.as_set(w0), L.as_set(l1)
        assert info_count(L, i0) == len(s0) and info_count(L, i1) == len(s1) and len(s0) + len(s1) == L.want(X) and s0 and s1
        assert not set(s0) & set(s1)
        rc, info, whole, _ = L.raw(gpu, g, fill=True)
        assert rc == gpu.OK and sorted(L.as_set(whole)) == sorted(s0 + s1)
        L.check(X, info, whole)
    finally:
        g.free()


@gpu_test
def test_sizing_with_one_parameter_then_filling_with_another(gpu, tabs):
    """The call's own parameters belong to the key: the flags of gmsx_kclique_star_list (a sizing call with CLIQUES_ONLY, a fill with stars, and
    the other way round), and the pattern of gmsx_subgraph_match — triangle and 3-path have the same k and flags, the pattern is compared in full."""
    X = tabs["A"]
    g = upload(gpu, X)
    try:
        for sized, filled in ((LISTINGS[2], LISTINGS[1]), (LISTINGS[1], LISTINGS[2]), (LISTINGS[3], LISTINGS[4]), (LISTINGS[4], LISTINGS[3])):
            rc, info, _, _ = sized.raw(gpu, g, fill=False)
            assert rc == gpu.OK and info_count(sized, info) == sized.want(X)
            rc, info, got, _ = filled.raw(gpu, g, fill=True)
            assert rc == gpu.OK, (sized.name, filled.name)
            filled.check(X, info, got)
    finally:
        g.free()


# ---- c. an option set between sizing and fill -----------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("L,option,value", [(LISTINGS[0], "BK_LIST_ARENA_MB", 1), (LISTINGS[1], "KCSTAR_SLAB_MB", 1), (LISTINGS[2], "KCSTAR_SLAB_MB", 1),
                                            (LISTINGS[3], "SGM_LAUNCH_TASKS", 7), (LISTINGS[4], "SGM_LAUNCH_TASKS", 7)], ids=LISTING_IDS)
def test_option_set_between_sizing_and_fill(gpu, tabs, L, option, value):
    """The fill plans its launches over the cached slab offsets under the option of ITS call: the bytes do not change.  (1 MB, the smallest value
    of the two arena options, still holds every slab of these graphs in one launch — the launches are printed; SGM_LAUNCH_TASKS does split.)"""
    for name in ("A", "H"):
        X = tabs[name]
        g = upload(gpu, X)
        try:
            rc, info, plain, _ = L.raw(gpu, g, fill=True)
            assert rc == gpu.OK
            L.check(X, info, plain)
            rc, info1, _, s1 = L.raw(gpu, g, fill=False)
            assert rc == gpu.OK and info1 == info
            try:
                gpu.set_option(option, value)
                rc, info2, got, s2 = L.raw(gpu, g, fill=True)   # the cached pass 1, planned under the other option
            finally:
                gpu.set_option(option, None)
            assert rc == gpu.OK and info2 == info and L.same(got, plain), (L.name, name)
            print(f"{L.name} on {name}: launches sizing {s1['launches']}, fill under {option}={value} {s2['launches']}")
            if option == "SGM_LAUNCH_TASKS":
                assert s2["launches"] > s1["launches"]
        finally:
            g.free()


# ---- d. rank between the two calls ----------------------------------------------------------------------------------------------------
@gpu_test
def test_bk_list_rank_given_to_the_fill_only(gpu, tabs):
    L = LISTINGS[0]
    for name in ("A", "H"):
        X = tabs[name]
        g = upload(gpu, X)
        try:
            rc, info, plain, _ = L.raw(gpu, g, fill=True)
            assert rc == gpu.OK
            L.check(X, info, plain)
            rc, info1, _, s1 = L.raw(gpu, g, fill=False, rank=None)
            rank = np.arange(X["n"] - 1, -1, -1, dtype=np.int32)
            rc2, info2, got, s2 = L.raw(gpu, g, fill=True, rank=rank)
            assert rc == gpu.OK and rc2 == gpu.OK and info1 == info2 == info and L.same(got, plain)
            bad = rank.copy()
            bad[0] = bad[1]
            rc, _, _, _ = L.raw(gpu, g, fill=True, rank=bad)   # … but it IS validated, on a fill from the cache as well
            assert rc == gpu.ERR_INVALID
            rc, info3, again, _ = L.raw(gpu, g, fill=True)
            assert rc == gpu.OK and info3 == info and L.same(again, plain)
        finally:
            g.free()


# ---- e. lazy triangle containers in any order -----------------------------------------------------------------------------------------
TC_OPS = ["kclique_count(4)", "tc_partial(1,3)", "tc_total()", "prepare()", "tc_total(TC_FULL)", "tc_vertex_count2()", "bk_count()", "tc_partial(0,2)"]


def status_of(gpu, call):
    try:
        call()
    except gpu.GmsxError as e:
        return e.status
    return gpu.OK


@gpu_test
@pytest.mark.parametrize("kind", ["default", "for_tc", "hub_limit_9", "shard_1_of_3"])
def test_lazy_triangle_containers_in_any_order(gpu, tabs, kind):
    X = tabs["H"]
    T = X["T"]
    csr = gpu.HostCSR.from_arrays(X["off"], X["adj"])
    flags = {"default": 0, "for_tc": gpu.UPLOAD_FOR_TC, "hub_limit_9": 9 << 8, "shard_1_of_3": 0}[kind]
    sharded = kind == "shard_1_of_3"
    own = None
    if sharded:  # what shard 1 of 3 must count: the shards are disjoint and cover, so the triangles the two other ranks do not count
        others = []
        for p in (0, 2):
            g = gpu.DeviceGraph.from_csr(csr, shard=(p, 3))
            others.append(g.tc_partial(p, 3))
            g.free()
        own = T - sum(others)
        assert own >= 0
    seen_partial = {}
    for shuffle in range(6):
        ops = [TC_OPS[i] for i in np.random.default_rng(100 + shuffle).permutation(len(TC_OPS))]
        g = gpu.DeviceGraph.from_csr(csr, flags=flags, shard=(1, 3) if sharded else None)
        tc_used = kind == "for_tc"
        log = []
        try:
            for op in ops:
                log.append(op)
                passes = g.tc_passes
                assert (passes >= 1) if tc_used else (passes == 0), (kind, log, passes)
                if op == "kclique_count(4)":
                    assert g.kclique_count(4)[0] == X["k"][4], (kind, log)
                elif op == "bk_count()":
                    assert g.bk_count() == X["bk"], (kind, log)
                elif op == "tc_vertex_count2()":
                    assert np.array_equal(g.tc_vertex_count2(), X["vc2"]), (kind, log)
                elif op == "tc_total(TC_FULL)":
                    assert g.tc_total(gpu.TC_FULL) == T, (kind, log)
                elif op == "prepare()":
                    g.prepare()
                    tc_used = True
                elif op == "tc_total()":
                    if sharded:  # = shard (0, 1): a sharded upload counts its own shard only
                        assert status_of(gpu, g.tc_total) == gpu.ERR_INVALID, (kind, log)
                    else:
                        assert g.tc_total() == T, (kind, log)
                        tc_used = True
                else:
                    part, nparts = (1, 3) if op == "tc_partial(1,3)" else (0, 2)
                    if sharded and (part, nparts) != (1, 3):
                        assert status_of(gpu, lambda: g.tc_partial(part, nparts)) == gpu.ERR_INVALID, (kind, log)
                        full = [g.tc_partial(p, nparts, gpu.TC_FULL) for p in range(nparts)]   # … except with TC_FULL
                        assert sum(full) == 3 * T, (kind, log, full)
                    elif sharded:
                        assert g.tc_partial(1, 3) == own, (kind, log)
                        tc_used = True
                    else:  # the asked shard first, then the others: disjoint and covering
                        parts = [g.tc_partial((part + i) % nparts, nparts) for i in range(nparts)]
                        assert sum(parts) == T, (kind, log, parts)
                        assert seen_partial.setdefault((part, nparts), parts[0]) == parts[0], (kind, log, parts)   # whatever ran before it
                        tc_used = True
            assert g.tc_passes >= 1
        finally:
            g.free()


# ---- f. weights attached, replaced, detached ------------------------------------------------------------------------------------------
def edge_weights(X, seed):
    """int32[nnz], both arcs of an edge alike, 1 … 40"""
    n = X["n"]
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(X["off"]))
    code = np.minimum(src, X["adj"]) * n + np.maximum(src, X["adj"])
    uniq, inv = np.unique(code, return_inverse=True)
    return np.random.default_rng(seed).integers(1, 41, uniq.size).astype(np.int32)[inv]


@gpu_test
def test_weights_attached_replaced_detached(gpu, tabs):
    X = tabs["A"]
    off, adj = X["off"], X["adj"]
    w1, w2 = edge_weights(X, 1), edge_weights(X, 2)
    want = {}
    for key, w in (("w1", w1), ("w2", w2)):
        dist = dijkstra_np(off, adj, w, 0)
        want[key] = (dist, parent_np(off, adj, w, 0, dist), kruskal_np(off, adj, w))
    assert not np.array_equal(want["w1"][0], want["w2"][0]) and int(want["w1"][2][2].sum()) != int(want["w2"][2][2].sum())
    depth, parent, _ = X["bfs0"][0]

    def follows(g, key):
        dist, par, _ = g.sssp(0)
        u, v, w, _, _, info = g.min_spanning_forest()
        assert np.array_equal(dist, want[key][0]) and np.array_equal(par, want[key][1]), key
        fu, fv, fw = want[key][2]
        assert np.array_equal(u, fu) and np.array_equal(v, fv) and np.array_equal(w, fw) and info["total_weight"] == int(fw.sum()), key
        return b"".join(a.tobytes() for a in (dist, par, u, v, w))

    g = upload(gpu, X)
    try:
        assert not g.has_weights
        g.set_weights(w1)
        first = follows(g, "w1")
        g.set_weights(w2)   # a second attach replaces the first
        follows(g, "w2")
        g.set_weights(None)
        assert not g.has_weights
        assert status_of(gpu, lambda: g.sssp(0)) == gpu.ERR_INVALID   # gmsx.h: no weights attached -> GMSX_ERR_INVALID, nothing written
        assert status_of(gpu, g.min_spanning_forest) == gpu.ERR_INVALID
        d, p, _ = g.bfs(0)
        assert np.array_equal(d, depth) and np.array_equal(p, parent)
        g.set_weights(w1)
        assert g.has_weights and follows(g, "w1") == first
    finally:
        g.free()


# ---- g. one random sequence -----------------------------------------------------------------------------------------------------------
SEQ_OPTIONS = {"BK_GROUPS": 0, "KC_MFMA": 0, "KC_STREAMS": 1, "CC_SAMPLE": 0, "BFS_DIRECTION": 1}
SEQ_MENU = ["upload", "free", "tc_total", "kclique_count", "bk_count", "bk_list", "kclique_star_list", "subgraph_match", "core_decomposition",
            "connected_components", "bfs", "pagerank", "coloring_jp", "option"]


def run_listing(gpu, g, X, L, mode):
    if mode == "sizing":
        rc, info, _, _ = L.raw(gpu, g, fill=False)
        assert rc == gpu.OK and info_count(L, info) == L.want(X)
    elif mode == "fill":
        rc, info, got, _ = L.raw(gpu, g, fill=True)
        assert rc == gpu.OK
        L.check(X, info, got)
    else:
        got = L.wrapper(g)
        assert len(L.as_set(got)) == L.want(X)
        rc, info, _, _ = L.raw(gpu, g, fill=False)
        assert rc == gpu.OK
        L.check(X, info, got)


def run_op(gpu, g, X, op, arg, options):
    if op == "tc_total":
        assert g.tc_total() == X["T"]
    elif op == "kclique_count":
        assert g.kclique_count(arg)[0] == X["k"][arg]
    elif op == "bk_count":
        assert g.bk_count() == X["bk"]
    elif op in ("bk_list", "kclique_star_list", "subgraph_match"):
        run_listing(gpu, g, X, *arg)
    elif op == "core_decomposition":
        core, rank, info = g.core_decomposition()
        assert np.array_equal(core, X["core"][0]) and np.array_equal(rank, X["core"][1]) and info == X["core"][2]
    elif op == "connected_components":
        label, info = g.connected_components()
        assert np.array_equal(label, X["label"])
        roots, sizes = np.unique(X["label"], return_counts=True)
        assert (info["components"], info["singletons"], info["largest"], info["kept_edges"]) == (roots.size, int((sizes == 1).sum()), int(sizes.max()), len(X["edges"]))
    elif op == "bfs":
        want_d, want_p, want_i = X["bfs0"][1 if "BFS_DIRECTION" in options else 0]
        d, p, info = g.bfs(0)
        assert np.array_equal(d, want_d) and np.array_equal(p, want_p) and info == want_i
    elif op == "pagerank":
        want, winfo, bound = X["pr"]
        scores, info = g.pagerank(max_iters=PR_ITERS)
        assert float(np.abs(scores - want).sum()) <= bound, (float(np.abs(scores - want).sum()), bound)
        assert (info["iterations"], info["converged"], info["argmax"], info["isolated"]) == (PR_ITERS, 0, winfo["argmax"], winfo["isolated"])
    elif op == "coloring_jp":
        want_c, _, want_i = X["jp"]
        col, info = g.coloring_jp()
        assert np.array_equal(col, want_c) and info == want_i
        chk = g.coloring_verify(col)
        assert (chk["conflicts"], chk["invalid"], chk["max_color"], chk["distinct"]) == (0, 0, want_i["colors"], want_i["colors"])
    else:
        raise AssertionError(op)


@gpu_test
def test_one_random_sequence(gpu, tabs):
    rng = np.random.default_rng(2026)
    live = {name: [] for name in tabs}   # at most two handles per graph
    options, log = set(), []
    flag_names = {0: "0", gpu.UPLOAD_TRUSTED: "TRUSTED", gpu.UPLOAD_FOR_TC: "FOR_TC", 9 << 8: "HUB_LIMIT(9)"}
    try:
        for i in range(80):
            op = SEQ_MENU[int(rng.integers(len(SEQ_MENU)))]
            name = sorted(tabs)[int(rng.integers(len(tabs)))]
            flags = list(flag_names)[int(rng.integers(4))]
            slot, k, variant, mode = int(rng.integers(2)), int(rng.integers(3, 6)), int(rng.integers(2)), ("sizing", "fill", "wrapper")[int(rng.integers(3))]
            option = sorted(SEQ_OPTIONS)[int(rng.integers(len(SEQ_OPTIONS)))]
            X, hs = tabs[name], live[name]
            if op not in ("upload", "option") and not hs:
                op = "upload"   # nothing to call it on
            elif op == "upload" and len(hs) == 2:
                op = "free"
            arg = None
            if op == "kclique_count":
                arg = k
            elif op == "bk_list":
                arg = (LISTINGS[0], mode)
            elif op == "kclique_star_list":
                arg = (LISTINGS[1 + variant], mode)
            elif op == "subgraph_match":
                arg = (LISTINGS[3 + variant], mode)
            h = slot % len(hs) if hs else 0
            try:
                if op == "upload":
                    log.append(f"{i}: upload {name} flags={flag_names[flags]}")
                    hs.append(upload(gpu, X, flags))
                elif op == "free":
                    log.append(f"{i}: free {name}[{h}]")
                    hs.pop(h).free()
                elif op == "option":
                    if option in options:
                        log.append(f"{i}: reset {option}")
                        gpu.set_option(option, None)
                        options.discard(option)
                    else:
                        log.append(f"{i}: set {option}={SEQ_OPTIONS[option]}")
                        gpu.set_option(option, SEQ_OPTIONS[option])
                        options.add(option)
                else:
                    what = "" if arg is None else (str(arg) if isinstance(arg, int) else f"{arg[0].name}, {arg[1]}")
                    log.append(f"{i}: {op}({what}) on {name}[{h}]")
                    run_op(gpu, hs[h], X, op, arg, options)
            except (AssertionError, gpu.GmsxError) as e:
                raise AssertionError(f"operation {i} failed: {e!r}\noptions set: {sorted(options)}\noperations so far:\n  " + "\n  ".join(log)) from e
        print("\n".join(log))
    finally:
        gpu.reset_options()
        for hs in live.values():
            for g in hs:
                g.free()


# ---- h. a handle gives back what it took ----------------------------------------------------------------------------------------------
LEAK_MARGIN = 0   # bytes: the largest drop of free memory over cycles 2 … 8 measured with the parent commit's library (see the docstring)


@gpu_test
def test_a_handle_gives_back_what_it_took(gpu, oracle):
    """Free device memory (torch.cuda.mem_get_info: the whole process, the library's hipMalloc calls included) after every cycle of
    upload, prepare, tc_total, kclique_count(4), pagerank (3 iterations), two sharded calls that fill and replace the shard index cache, free
    — and after every round of refused and fallback builds: an upload refused after the CSR is on the device (an id out of range), a
    container budget too small for one pass (GMSX_ERR_DEVICE_MEM, the base layout stays usable), and a budget of half the containers (the
    passes fallback: every call frees and rebuilds the containers shard by shard).  Free memory after cycle 8 is not below free memory after
    cycle 2 (the first cycles pay for the k-clique pool, which only grows, and for code objects).

    Graph: kronecker scale 15, degree 16 — adj is about 4 MB, every nnz-sized array and both pools are above the allocator's granule.
    Margin: the same test against the parent commit's library (hand-kept free lists) dropped by 0 bytes over cycles 2 … 8 of both loops, so
    LEAK_MARGIN = 0.  What the test cannot see: an array smaller than the granule of the device allocator, which may be carved
    out of a block that stays mapped — the scratch words, the per-class tables, an empty graph's arrays."""
    import torch
    csr = host_graph(gpu, "kronecker", 15)
    off, adj = csr.offsets().copy(), csr.neighbors().copy()
    T = oracle.tc_total(off, adj)
    free = lambda: int(torch.cuda.mem_get_info()[0])
    free()
    seen, after = {}, []
    for cycle in range(1, 9):
        g = gpu.DeviceGraph.from_csr(csr)
        try:
            g.prepare()
            got = {"T": g.tc_total(), "k4": g.kclique_count(4)[0], "pr": g.pagerank(max_iters=3, tolerance=0.0)[1]["iterations"],
                   "parts": sum(g.tc_partial(p, 3) for p in range(3)) + g.tc_partial(0, 2) + g.tc_partial(1, 2), "bytes": g.device_bytes}
        finally:
            g.free()
        assert got["T"] == T and got["parts"] == 2 * T and got["pr"] == 3 and seen.setdefault("cycle", got) == got, (cycle, got, seen)
        after.append(free())
        print(f"cycle {cycle}: free {after[-1]} ({after[-1] - after[0]:+d} against cycle 1), device_bytes {got['bytes']}")
    assert after[7] >= after[1] - LEAK_MARGIN, after

    bad = adj.copy()
    bad[bad.size // 2] = off.size - 1   # an id = n: found by the validation kernel, after off, adj, scratch and acc were allocated
    g = gpu.DeviceGraph.from_csr(csr)
    base = g.device_bytes
    g.prepare()
    half_mb = max(1, (g.device_bytes - base) // 2 >> 20)
    g.free()
    after = []
    try:
        for turn in range(1, 9):
            assert status_of(gpu, lambda: gpu.DeviceGraph.upload(off, bad)) == gpu.ERR_NOT_CANONICAL
            gpu.set_option("TC_MEM_LIMIT_MB", 1)
            g = gpu.DeviceGraph.from_csr(csr)
            try:
                assert status_of(gpu, g.tc_total) == gpu.ERR_DEVICE_MEM and g.tc_passes == 0 and g.device_bytes == base
                assert g.tc_total(gpu.TC_FULL) == T
            finally:
                g.free()
            gpu.set_option("TC_MEM_LIMIT_MB", half_mb)
            g = gpu.DeviceGraph.from_csr(csr)
            try:
                assert g.tc_total() == T and g.tc_passes >= 2 and sum(g.tc_partial(p, 3) for p in range(3)) == T
                passes = g.tc_passes
            finally:
                g.free()
            gpu.set_option("TC_MEM_LIMIT_MB", None)
            after.append(free())
            print(f"refused round {turn}: free {after[-1]} ({after[-1] - after[0]:+d} against round 1), budget {half_mb} MB -> {passes} passes")
    finally:
        gpu.reset_options()
    assert after[7] >= after[1] - LEAK_MARGIN, after
