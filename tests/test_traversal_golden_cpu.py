"""CPU: the goldens of breadth-first search and betweenness centrality (tests/golden/traversal.{json,npz}, written by
tools/make_golden_traversal.py) agree with the definitions of include/gmsx.h restated here:

  * bfs_np: depth, the smallest-id parent, the gmsx_bfs_info integers and the replay of the reference's switching rule (bfs.cc:142-188) that
    gives bottom_up_levels; it reproduces every BFS record bit for bit.  The tool asserted before it wrote a record that the REFERENCE's DOBFS
    parents give the same depths and that the reference's BFSVerifier accepts both its own parents and the smallest-id ones;
  * betweenness_np: Brandes in double, math.fsum per row; it reproduces every BC record — the scores of betweenness_exact (integers for
    sigma, fractions for delta, rounded once) — within the derived bound bc_bound;
  * HostCSR.pick_sources equals the recorded picks of the reference's SourcePicker on every golden graph;
  * the closed forms of the issue.

bfs_np, betweenness_np, betweenness_exact, bc_bound and the shape builders are what tests/test_traversal_gpu.py checks the device against."""
import ctypes
import hashlib
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph, load_golden
from test_components_golden_cpu import csr_of, path_edges, star_edges  # noqa: F401  (the GPU tests take them from here)

TRAV = load_golden("traversal.json")
ARR = np.load(os.path.join(GOLDEN, "traversal.npz"))
GRAPHS = TRAV["graphs"]
BFS = TRAV["bfs"]
BC = TRAV["bc"]
INFO_KEYS = ("reached", "reached_arcs", "depth_sum", "widest", "levels", "widest_level")
LITERAL_MAX_N = 1 << 16
PARENT_LITERAL_MAX_N = 1 << 12  # (parent arrays do not compress: those of the 65 536-vertex graphs would not fit a committed file; the sha256 covers them)
EPS = 2.0 ** -53
ALPHA, BETA, BU_PROBE = 15, 18, 16  # the defaults of traversal.hip (gmsx.h, OPTIONS)
K_LONG_ROW = 1024                   # frontier_rounds.hpp


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def _rows(off, front):
    """(arc positions, their source) of the rows of the vertices in `front`"""
    lens = off[front + 1] - off[front]
    total = int(lens.sum())
    before = np.concatenate([[0], np.cumsum(lens)[:-1]]) if front.size else np.zeros(0, dtype=np.int64)
    pos = np.repeat(off[front] - before, lens) + np.arange(total, dtype=np.int64)
    return pos, np.repeat(front, lens)


def _cdiv(a, b):
    """C++'s integer division (towards zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def replay_bottom_up_levels(n, nnz, counts, degs, alpha=ALPHA, beta=BETA, direction=0):
    """bottom_up_levels by the reference's rule (bfs.cc:142-188) from the level sizes and the levels' degree sums: a fact about them"""
    levels = len(counts)
    if direction == 1:
        return 0
    if direction == 2:
        return levels - 1
    size = lambda d: counts[d] if d < levels else 0  # noqa: E731
    etc, scout, d, bu = nnz, degs[0], 0, 0
    while size(d) > 0:
        if scout > _cdiv(etc, alpha):
            awake = size(d)
            while True:
                old, d = awake, d + 1
                awake = size(d)
                bu += awake > 0
                if not (awake >= old or awake > n // beta):
                    break
            scout = 1
        else:
            etc -= scout
            d += 1
            scout = degs[d] if d < levels else 0
    return bu


def bfs_np(off, adj, source, alpha=ALPHA, beta=BETA, direction=0):
    """(depth, parent, info): parent[v] = the smallest-id neighbour of v one level up, parent[source] = source, -1 = unreachable"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    depth, parent = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    depth[source], parent[source] = 0, source
    front, d = np.array([source], dtype=np.int64), 0
    while front.size:
        pos, src = _rows(off, front)
        w = adj[pos]
        new = depth[w] == -1
        w, src = w[new], src[new]
        best = np.full(n, n, dtype=np.int64)
        np.minimum.at(best, w, src)
        front = np.flatnonzero(best < n)
        d += 1
        depth[front], parent[front] = d, best[front]
    reached = depth >= 0
    counts = np.bincount(depth[reached]).tolist()
    deg = np.diff(off)
    degs = np.bincount(depth[reached], weights=deg[reached]).astype(np.int64).tolist()
    info = {"reached": int(reached.sum()), "reached_arcs": int(deg[reached].sum()), "depth_sum": int(depth[reached].sum()), "widest": int(max(counts)),
            "levels": len(counts), "widest_level": int(np.argmax(counts)),
            "bottom_up_levels": int(replay_bottom_up_levels(n, int(adj.size), counts, degs, alpha, beta, direction))}
    return depth.astype(np.int32), parent.astype(np.int32), info


def bfs_verifier_np(off, adj, source, parent):
    """BFSVerifier (bfs.cc:212-258): the source is its own parent, parent[v] is a neighbour one level up, exactly the reachable have one"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    depth = bfs_np(off, adj, source)[0].astype(np.int64)
    parent = np.asarray(parent, dtype=np.int64)
    for u in range(off.size - 1):
        if depth[u] != -1 and parent[u] != -1:
            if u == source:
                if parent[u] != u:
                    return False
                continue
            row = adj[off[u]:off[u + 1]]
            if parent[u] not in row or depth[parent[u]] != depth[u] - 1:
                return False
        elif depth[u] != parent[u]:
            return False
    return True


def _levels_of(depth):
    order = np.argsort(depth, kind="stable")
    order = order[depth[order] >= 0]
    cuts = np.flatnonzero(np.diff(depth[order])) + 1
    return np.split(order, cuts)


def betweenness_np(off, adj, sources, exclude_source=False, normalize=False, cache=None):
    """(scores float64[n], info): Brandes in double from the listed sources, every row's sum by math.fsum; the expression and the operand order of
    bc.cc:131-132.  cache (a dict of the caller's, per graph): the per-source sweeps are kept in it and not repeated."""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    scores = [0.0] * n
    info = {"sources": len(sources), "reached_total": 0, "max_levels": 0, "max_sigma": 0.0}
    adjl, offl = adj.tolist(), off.tolist()
    cache = {} if cache is None else cache
    for s in sources:
        if s not in cache:
            depth = bfs_np(off, adj, s)[0].tolist()
            levels = [lv.tolist() for lv in _levels_of(np.asarray(depth))]
            sigma, delta = [0.0] * n, [0.0] * n
            sigma[s] = 1.0
            for lv in levels[1:]:
                for v in lv:
                    sigma[v] = math.fsum(sigma[u] for u in adjl[offl[v]:offl[v + 1]] if depth[u] == depth[v] - 1)
            for lv in levels[-2::-1] if len(levels) > 1 else []:
                for u in lv:
                    delta[u] = math.fsum(sigma[u] / sigma[v] * (1.0 + delta[v]) for v in adjl[offl[u]:offl[u + 1]] if depth[v] == depth[u] + 1)
            cache[s] = ([(u, delta[u]) for lv in levels[:-1] for u in lv], sum(len(lv) for lv in levels), len(levels), max(sigma))
        terms, reached, nlevels, top_sigma = cache[s]
        for u, x in terms:  # (in the order of the levels, as the device adds delta(u) to scores[u] source after source)
            if not (exclude_source and u == s):
                scores[u] += x
        info["reached_total"] += reached
        info["max_levels"] = max(info["max_levels"], nlevels)
        info["max_sigma"] = max(info["max_sigma"], top_sigma)
    scores = np.array(scores, dtype=np.float64)
    info["max_score"] = float(scores.max()) if n else 0.0
    if normalize and info["max_score"] > 0:
        scores = scores / info["max_score"]
    return scores, info


def betweenness_exact(off, adj, sources, exclude_source=False, normalize=False):
    """(scores float64[n] — the exact rationals rounded ONCE —, max_sigma as a Python integer, max_levels).  Per source sigma is integers and, with
    D = lcm of the path counts and B(v) = D (1 + delta(v)) / sigma(v) = D / sigma(v) + Σ_{w below v} B(w) an integer,
    delta(u) = sigma(u) Σ_{v below u} B(v) / D."""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    adjl, offl = adj.tolist(), off.tolist()
    total = [Fraction(0)] * n
    max_sigma, max_levels = 0, 0
    cache = {}
    for s in sources:
        if s not in cache:
            depth = bfs_np(off, adj, s)[0].tolist()
            levels = [lv.tolist() for lv in _levels_of(np.asarray(depth))]
            sigma = [0] * n
            sigma[s] = 1
            for lv in levels[1:]:
                for v in lv:
                    sigma[v] = sum(sigma[u] for u in adjl[offl[v]:offl[v + 1]] if depth[u] == depth[v] - 1)
            D = 1
            for x in set(sigma[v] for lv in levels for v in lv):
                D = D * x // math.gcd(D, x)
            B, below = [0] * n, [0] * n
            for lv in levels[::-1]:
                for u in lv:
                    below[u] = sum(B[v] for v in adjl[offl[u]:offl[u + 1]] if depth[v] == depth[u] + 1)
                    B[u] = D // sigma[u] + below[u]
            cache[s] = ([(u, Fraction(sigma[u] * below[u], D)) for lv in levels for u in lv if below[u]], max(sigma), len(levels))
        terms, ms, nl = cache[s]
        for u, x in terms:
            if not (exclude_source and u == s):
                total[u] += x
        max_sigma, max_levels = max(max_sigma, ms), max(max_levels, nl)
    top = max(total) if n else Fraction(0)
    if normalize and top > 0:
        total = [x / top for x in total]
    return np.array([float(x) for x in total], dtype=np.float64), max_sigma, max_levels


def bc_bound(want, levels, max_degree, n_sources, eps=EPS):
    """the derived bound of the issue while every path count is exact: one level adds at most (d + 2) eps to the relative error of delta, the sum
    over the sources S eps, the golden is rounded once; the factor 2 covers the second-order terms"""
    return 2.0 * eps * (levels * (max_degree + 2) + n_sources + 1) * np.asarray(want, dtype=np.float64)


def bc_bound_inexact(want, levels, max_degree, eps=EPS):
    """… and beyond 2^53, where sigma itself carries up to L d eps and enters a term twice"""
    return 2.0 * eps * levels * ((max_degree + 2) + 2 * levels * max_degree) * np.asarray(want, dtype=np.float64)


def golden_csr(capi, key):
    src = GRAPHS[key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def bc_sources(rec):
    g = GRAPHS[rec["graph"]]
    return list(range(g["n"])) if rec["sources"] == "all" else g["picks"][:int(rec["sources"])]


# ---- shapes the GPU tests run -------------------------------------------------------------------------------------------------------------------
def grid_edges(rows, cols):
    ids = np.arange(rows * cols).reshape(rows, cols)
    return np.concatenate([np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], axis=1), np.stack([ids[:-1].ravel(), ids[1:].ravel()], axis=1)])


PROBE_DEGREES = [1, 15, 16, 17, 63, 64, 65, K_LONG_ROW - 1, K_LONG_ROW, K_LONG_ROW + 1]


def probe_graph(where, probe):
    """(edges, n, hubs).  Vertex 0 is the source and the `anchor` its only neighbour, so level 1 is {anchor}.  Hub i has degree PROBE_DEGREES[i]:
    the anchor — its one neighbour of level 1 — and filler leaves of its own, whose ids lie below or above the anchor's so that the anchor is the
    first entry of the hub's ascending row ("first"), the last ("last"), or entry `probe`: just past the window of pass 1 of the bottom-up step
    ("past"; the last entry of a shorter row).  Levels: source, anchor, hubs, fillers."""
    degrees = PROBE_DEGREES
    before_of = lambda d: min({"first": 0, "last": d - 1, "past": probe}[where], d - 1)  # noqa: E731
    anchor = 1 + sum(before_of(d) for d in degrees)
    edges, hubs = [(0, anchor)], []
    at_low, at_high = 1, anchor + 1 + len(degrees)
    for i, d in enumerate(degrees):
        hub = anchor + 1 + i
        hubs.append(hub)
        edges.append((hub, anchor))
        for _ in range(before_of(d)):
            edges.append((hub, at_low))
            at_low += 1
        for _ in range(d - 1 - before_of(d)):
            edges.append((hub, at_high))
            at_high += 1
    assert at_low == anchor
    return np.array(edges, dtype=np.int64), at_high, hubs


# ---- the goldens ------------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_complete():
    want = {"file_eppsteinExample", "file_micro", "file_smallRandom1", "file_tomitaExample", "file_triangles_1", "file_triangles_3",
            "kronecker_10_16", "kronecker_12_16", "kronecker_16_16", "uniform_10_16", "uniform_16_16", "kronecker_10_16_raw"}
    assert set(GRAPHS) == want
    for key, g in GRAPHS.items():
        assert len(g["picks"]) == 16 and len(g["bfs_sources"]) >= (5 if g["n"] >= 1024 else 2)
        got = [r["source"] for r in BFS if r["graph"] == key]
        assert got == g["bfs_sources"]
    for r in BFS:
        assert r["literal"] == (GRAPHS[r["graph"]]["n"] <= LITERAL_MAX_N) and r["literal_parent"] == (GRAPHS[r["graph"]]["n"] <= PARENT_LITERAL_MAX_N)
    # an isolated source and one outside the largest component exist among the records
    assert {"pick", "hub", "isolated", "outside"} == {r["kind"] for r in BFS}
    assert all(r["reached"] == 1 for r in BFS if r["kind"] == "isolated")
    top = [r for r in BFS if r["graph"] == "kronecker_16_16" and r["source"] == 0]
    assert top and top[0]["bottom_up_levels"] >= 1  # the bottom-up step is on the default path of the GPU tests
    compared = {r["graph"] for r in BC if r["reference"]}
    assert {k for k in want if k.startswith("file_")} | {"kronecker_10_16"} <= compared
    for r in BC:
        assert int(r["max_sigma"]) < 2 ** 53 and (not r["reference"] or int(r["max_sigma"]) < 2 ** 31)


def bfs_id(r):
    return "%s-%d" % (r["graph"], r["source"])


_BFS_CACHE = {}


def bfs_of(capi, graph, source):
    if (graph, source) not in _BFS_CACHE:
        csr = golden_csr(capi, graph)
        _BFS_CACHE[(graph, source)] = bfs_np(csr.offsets(), csr.neighbors(), source)
    return _BFS_CACHE[(graph, source)]


@pytest.mark.parametrize("rec", BFS, ids=bfs_id)
def test_bfs_restatement_reproduces_the_golden(capi, rec):
    g = GRAPHS[rec["graph"]]
    csr = golden_csr(capi, rec["graph"])
    assert (csr.num_nodes, csr.nnz) == (g["n"], g["nnz"])
    depth, parent, info = bfs_of(capi, rec["graph"], rec["source"])
    assert info == {k: rec[k] for k in INFO_KEYS + ("bottom_up_levels",)}
    assert sha(depth) == rec["depth_sha256"] and sha(parent) == rec["parent_sha256"]
    if rec["literal"]:
        assert np.array_equal(depth, ARR["depth_%s_%d" % (rec["graph"], rec["source"])])
    if rec["literal_parent"]:
        assert np.array_equal(parent, ARR["parent_%s_%d" % (rec["graph"], rec["source"])])
    if g["n"] <= 4096:
        assert bfs_verifier_np(csr.offsets(), csr.neighbors(), rec["source"], parent)


def bc_id(r):
    return "%s-%s-%s" % (r["graph"], r["sources"], "xn" if r["exclude_source"] else "default")


_BC_CACHE = {}


@pytest.mark.parametrize("rec", BC, ids=bc_id)
def test_bc_restatement_reproduces_the_golden(capi, rec):
    csr = golden_csr(capi, rec["graph"])
    srcs = bc_sources(rec)
    got, info = betweenness_np(csr.offsets(), csr.neighbors(), srcs, rec["exclude_source"], rec["normalize"], _BC_CACHE.setdefault(rec["graph"], {}))
    want = ARR[rec["array"]]
    assert info["max_levels"] == rec["max_levels"] and info["max_sigma"] == float(int(rec["max_sigma"]))
    assert np.all(np.abs(got - want) <= bc_bound(want, rec["max_levels"], GRAPHS[rec["graph"]]["max_degree"], len(srcs)))


@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_pick_sources_equals_the_reference(capi, key):
    csr = golden_csr(capi, key)
    assert csr.pick_sources(16).tolist() == GRAPHS[key]["picks"]
    assert csr.pick_sources(3, given=1).tolist() == [1, 1, 1]
    assert csr.pick_sources(0).size == 0
    deg = np.diff(csr.offsets())
    assert np.all(deg[csr.pick_sources(16)] > 0)


def test_pick_sources_refuses_what_the_reference_cannot_do(capi):
    empty = capi.HostCSR.from_arrays(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32))
    with pytest.raises(capi.GmsxError) as ei:
        empty.pick_sources(4)
    assert ei.value.status == capi.ERR_INVALID
    assert empty.pick_sources(2, given=3).tolist() == [3, 3]
    for bad in (5, -2):
        with pytest.raises(capi.GmsxError) as ei:
            empty.pick_sources(1, given=bad)
        assert ei.value.status == capi.ERR_INVALID


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------------
def test_closed_forms_of_betweenness():
    n = 9
    off, adj = csr_of(path_edges(n, "along"), n)
    got, info = betweenness_np(off, adj, list(range(n)), exclude_source=True)
    assert got.tolist() == [2.0 * i * (n - 1 - i) for i in range(n)] and info["max_levels"] == n
    assert betweenness_exact(off, adj, list(range(n)), exclude_source=True)[0].tolist() == got.tolist()
    default = betweenness_np(off, adj, list(range(n)))[0]
    assert (default - got).tolist() == [float(n - 1)] * n  # reached(s) - 1 at every source
    off, adj = csr_of(star_edges(n - 1), n)
    got = betweenness_np(off, adj, list(range(n)), exclude_source=True)[0]
    assert got.tolist() == [float((n - 1) * (n - 2))] + [0.0] * (n - 1)
    assert betweenness_np(off, adj, list(range(n)), exclude_source=True, normalize=True)[0].tolist() == [1.0] + [0.0] * (n - 1)
    kn = [(i, j) for i in range(7) for j in range(i)]
    off, adj = csr_of(kn, 7)
    assert not betweenness_np(off, adj, list(range(7)), exclude_source=True)[0].any()
    assert betweenness_np(off, adj, [3, 3])[0].tolist() == [0.0, 0.0, 0.0, 12.0, 0.0, 0.0, 0.0]  # a source listed twice counts twice


def test_restatements_on_the_shapes_of_the_gpu_tests():
    off, adj = csr_of(path_edges(4096, "along"), 4096)
    depth, parent, info = bfs_np(off, adj, 0)
    assert info["levels"] == 4096 and depth.tolist() == list(range(4096)) and parent.tolist() == [0] + list(range(4095))
    assert bfs_np(off, adj, 2047)[2]["levels"] == 2049
    off, adj = csr_of(star_edges(70000), 70001)
    assert bfs_np(off, adj, 0)[2]["levels"] == 2 and bfs_np(off, adj, 5)[2]["levels"] == 3
    for where in ("first", "last", "past"):
        e, n, hubs = probe_graph(where, 16)
        off, adj = csr_of(e, n)
        assert np.diff(off)[hubs].tolist() == PROBE_DEGREES
        depth, parent, info = bfs_np(off, adj, 0)
        anchor = int(adj[off[0]])
        assert np.all(depth[hubs] == 2) and np.all(parent[hubs] == anchor) and info["levels"] == 4
        for hub, d in zip(hubs, PROBE_DEGREES):
            at = int(np.flatnonzero(adj[off[hub]:off[hub + 1]] == anchor)[0])
            assert at == {"first": 0, "last": d - 1, "past": min(16, d - 1)}[where]
    off, adj = csr_of(grid_edges(40, 40), 1600)
    _, max_sigma, levels = betweenness_exact(off, adj, [0])
    assert max_sigma == math.comb(78, 39) > 2 ** 64 and levels == 79


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_bfs", "gmsx_betweenness", "gmsx_csr_pick_sources"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    for name in ("BFS_DIRECTION", "BFS_ALPHA", "BFS_BETA", "BFS_BU_PROBE", "BFS_WG_FRONTIER"):
        assert name in capi.option_names() and name in hdr
    assert ctypes.sizeof(capi.BfsInfo) == 48 and ctypes.sizeof(capi.BcInfo) == 40
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
    out = np.full(4, -77, dtype=np.int32)
    scores = np.full(4, -77.0)
    src = np.zeros(1, dtype=np.int32)
    info, bc = capi.BfsInfo(), capi.BcInfo()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(1 << 16)))  # never read: the calls check the device before the handle
    assert L.gmsx_bfs(fake, 0, p(out), p(out), ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_betweenness(fake, 1, p(src), 0, p(scores), ctypes.byref(bc), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_bfs(None, 0, p(out), p(out), ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_bfs(fake, 0, p(out), p(out), None, None) == capi.ERR_INVALID
    assert L.gmsx_betweenness(fake, 1, p(src), 4, p(scores), ctypes.byref(bc), None) == capi.ERR_INVALID
    assert L.gmsx_betweenness(fake, 1, None, 0, p(scores), ctypes.byref(bc), None) == capi.ERR_INVALID
    assert np.all(out == -77) and np.all(scores == -77.0)
