"""CPU: the goldens of gmsx_biconnected_components (tests/golden/bicc.json, bicc.npz; tools/make_golden_bicc.py) against a restatement in plain
Python, which is also what tests/test_bicc_gpu.py holds the device to:
  * bicc_np(off, adj) -> (block, blocks_at, arc_keep, info) — an iterative Hopcroft–Tarjan (depth-first search with an edge stack), its
    blocks renumbered the way include/gmsx.h defines the ids: dense, ascending with each block's smallest `u < v` arc in CSR order;
    blocks_at[v] = the distinct blocks among v's arcs, arc_keep = 0 on both arcs of a block of one edge; info = the integers of gmsx_bicc_info
    (components from components_np of test_components_golden_cpu.py, levels from a breadth-first search rooted at every component's smallest
    id).
The reference has no biconnectivity; networkx agrees on the edge partition, the articulation points and the bridges (the goldens' generator
asserts it on every golden graph, this file on 200 seeded random graphs)."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph, load_golden
from test_components_golden_cpu import components_np, csr_of, sources

J = load_golden("bicc.json")
ARR = np.load(os.path.join(GOLDEN, "bicc.npz"))
FILES = ("eppsteinExample", "micro", "smallRandom1", "tomitaExample", "triangles_1", "triangles_3")
GENERATED = {"kronecker_10_16": ("kronecker", 10, 16), "kronecker_12_16": ("kronecker", 12, 16), "kronecker_14_16": ("kronecker", 14, 16),
             "uniform_12_16": ("uniform", 12, 16), "kronecker_12_2": ("kronecker", 12, 2)}
INFO_KEYS = ("blocks", "bridges", "articulation_points", "largest_block_edges", "largest_block_vertices", "components", "isolated",
             "largest_block", "max_blocks_at", "levels")
ARRAY_MAX_N = 1 << 12   # graphs up to 2^12 vertices keep their arrays in bicc.npz
BCC_OPTIONS = ("BCC_WAVE_ROW", "BCC_WG_ROW", "BCC_WG_FRONTIER", "BCC_WG_LEVEL")
MANY_ROOTS = {"n": 2661, "blocks": 834, "bridges": 660, "components": 481, "levels": 11}   # of many_roots_edges()


def graph_keys():
    return ["file_" + f for f in FILES] + sorted(GENERATED)


def golden_csr(capi, key):
    """The host CSR of a golden graph, never relabelled: the ids of the file / of the generator."""
    if key in GENERATED:
        kind, scale, deg = GENERATED[key]
        return host_graph(capi, kind, scale, deg, False)
    return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", key[len("file_"):] + ".el"), relabel=capi.RELABEL_NEVER)


_CSR = {}


def golden_arrays(capi, key):
    if key not in _CSR:
        c = golden_csr(capi, key)
        _CSR[key] = (np.array(c.offsets(), dtype=np.int64), np.array(c.neighbors(), dtype=np.int32))
    return _CSR[key]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def levels_np(off, adj, label):
    """non-empty levels of the breadth-first forest rooted at every vertex with label[v] == v"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    seen = np.asarray(label) == np.arange(n)
    front, levels = np.flatnonzero(seen), 0
    while front.size:
        levels += 1
        lo, deg = off[front], off[front + 1] - off[front]
        if deg.sum() == 0:
            break
        idx = np.repeat(lo - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg) + np.arange(int(deg.sum()))
        nxt = np.unique(adj[idx])
        front = nxt[~seen[nxt]]
        seen[front] = True
    return levels


def raw_blocks(off, adj):
    """Hopcroft–Tarjan, iterative: raw[j] = a block number for every arc j (both arcs of an edge the same), in the order the search closes
    the blocks"""
    off, adj = [int(x) for x in off], [int(x) for x in adj]
    n = len(off) - 1
    disc, low, raw = [-1] * n, [0] * n, [-1] * len(adj)
    of_edge, clock, nblocks = {}, 0, 0
    for root in range(n):
        if disc[root] >= 0:
            continue
        disc[root] = low[root] = clock
        clock += 1
        stack, edges = [(root, -1, off[root])], []   # (vertex, parent, next arc); the edge stack holds (lo, hi) keys
        while stack:
            v, p, j = stack[-1]
            if j < off[v + 1]:
                stack[-1] = (v, p, j + 1)
                w = adj[j]
                if w == p:
                    continue
                if disc[w] < 0:
                    edges.append((min(v, w), max(v, w)))
                    disc[w] = low[w] = clock
                    clock += 1
                    stack.append((w, v, off[w]))
                elif disc[w] < disc[v]:   # a back edge to an ancestor, met from its lower end only
                    edges.append((min(v, w), max(v, w)))
                    low[v] = min(low[v], disc[w])
            else:
                stack.pop()
                if p < 0:
                    continue
                low[p] = min(low[p], low[v])
                if low[v] >= disc[p]:   # p separates v's subtree: the edges above (p, v) on the stack are one block
                    key = (min(p, v), max(p, v))
                    while True:
                        e = edges.pop()
                        of_edge[e] = nblocks
                        if e == key:
                            break
                    nblocks += 1
    for u in range(n):
        for j in range(off[u], off[u + 1]):
            raw[j] = of_edge[(min(u, adj[j]), max(u, adj[j]))]
    return np.asarray(raw, dtype=np.int64), nblocks


def bicc_np(off, adj):
    """(block, blocks_at, arc_keep, info) as include/gmsx.h defines them"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n, nnz = off.size - 1, adj.size
    info = dict.fromkeys(INFO_KEYS, 0)
    info["components"] = info["isolated"] = n
    if nnz == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(0, dtype=np.uint8), info
    raw, nblocks = raw_blocks(off, adj)
    src = sources(off)
    up = np.flatnonzero(src < adj)   # the `u < v` arcs in CSR order
    _, first = np.unique(raw[up], return_index=True)   # per raw block (ascending) the position of its first `u < v` arc
    ids = np.empty(nblocks, dtype=np.int64)
    ids[np.argsort(first, kind="stable")] = np.arange(nblocks)
    block = ids[raw]
    edges_of = np.bincount(block[up], minlength=nblocks)
    pairs = np.unique(src * nblocks + block)   # (vertex, block) incidences
    blocks_at = np.bincount(pairs // nblocks, minlength=n)
    vertices_of = np.bincount(pairs % nblocks, minlength=nblocks)
    arc_keep = (edges_of[block] > 1).astype(np.uint8)
    label, cinfo = components_np(off, adj)
    largest = int(np.flatnonzero(edges_of == edges_of.max())[0])
    info.update(blocks=int(nblocks), bridges=int((edges_of == 1).sum()), articulation_points=int((blocks_at >= 2).sum()),
                largest_block_edges=int(edges_of[largest]), largest_block_vertices=int(vertices_of[largest]), components=int(cinfo["components"]),
                isolated=int((np.diff(off) == 0).sum()), largest_block=largest, max_blocks_at=int(blocks_at.max()), levels=levels_np(off, adj, label))
    return block.astype(np.int32), blocks_at.astype(np.int32), arc_keep, info


def identities_hold(off, adj, block, blocks_at, arc_keep, info):
    """the three identities of include/gmsx.h"""
    n = len(off) - 1
    if int(np.sum(blocks_at, dtype=np.int64)) != n - info["components"] + info["blocks"]:
        return False
    if len(adj) and components_np(off, adj, arc_keep)[1]["components"] != info["components"] + info["bridges"]:
        return False
    up = sources(off) < np.asarray(adj, dtype=np.int64)
    return int(np.bincount(np.asarray(block)[up], minlength=1).sum()) == len(adj) // 2 and (len(adj) == 0 or int(np.max(block)) == info["blocks"] - 1)


def against_networkx(off, adj, block, blocks_at, arc_keep):
    """the edge partition, the articulation points and the bridges of networkx 3.x"""
    import networkx as nx
    n = len(off) - 1
    src = sources(off)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(src.tolist(), np.asarray(adj).tolist()))
    mine = {}
    for u, v, b in zip(src.tolist(), np.asarray(adj).tolist(), np.asarray(block).tolist()):
        mine.setdefault(b, set()).add((min(u, v), max(u, v)))
    theirs = sorted(sorted((min(u, v), max(u, v)) for u, v in comp) for comp in nx.biconnected_component_edges(g))
    assert sorted(sorted(s) for s in mine.values()) == theirs
    assert set(np.flatnonzero(np.asarray(blocks_at) >= 2).tolist()) == set(nx.articulation_points(g))
    bridges = {(min(u, v), max(u, v)) for u, v in nx.bridges(g)}
    assert {(min(u, v), max(u, v)) for u, v, k in zip(src.tolist(), np.asarray(adj).tolist(), np.asarray(arc_keep).tolist()) if not k} == bridges
    # ids ascend with each block's smallest edge
    firsts = [min(mine[b]) for b in sorted(mine)]
    assert firsts == sorted(firsts) and sorted(mine) == list(range(len(mine)))


# ---- the shapes of the device tests (tests/test_bicc_gpu.py runs the same on the device) ----------------------------------------------------------
def path_edges(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), n


def cycle_edges(n):
    return np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1), n


def star_edges(leaves):
    return np.stack([np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1)], axis=1), leaves + 1


def windmill_edges(blades):
    """`blades` triangles that share vertex 0"""
    a, b = 1 + 2 * np.arange(blades), 2 + 2 * np.arange(blades)
    z = np.zeros(blades, dtype=np.int64)
    return np.concatenate([np.stack([z, a], axis=1), np.stack([z, b], axis=1), np.stack([a, b], axis=1)]), 2 * blades + 1


def clique_edges(k, base=0):
    return np.array([(base + i, base + j) for i in range(k) for j in range(i + 1, k)], dtype=np.int64)


def grid_edges(side):
    ids = np.arange(side * side).reshape(side, side)
    return np.concatenate([np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], axis=1), np.stack([ids[:-1].ravel(), ids[1:].ravel()], axis=1)]), side * side


def clique_chain_edges(cliques=6):
    """K_5's in a chain: clique i and i + 1 share a vertex when i is even and are joined by a bridge when i is odd"""
    e, base, last = [], 0, None
    for i in range(cliques):
        if i > 0 and i % 2 == 1:      # shares its first vertex with the last vertex of the clique before
            base = last
        elif i > 0:                    # a bridge from the last vertex of the clique before to its first vertex
            base = last + 1
            e.append(np.array([(last, base)], dtype=np.int64))
        e.append(clique_edges(5, base))
        last = base + 4
    return np.concatenate(e), last + 1


def p3_middle_root():
    return np.array([(0, 1), (0, 2)], dtype=np.int64), 3


def triangle_with_pendant():
    """a triangle 0 1 2 and a pendant 3 on vertex 2, which is no root"""
    return np.array([(0, 1), (0, 2), (1, 2), (2, 3)], dtype=np.int64), 4


def two_components_and_isolated():
    """a triangle with a tail, a 4-cycle, and three isolated vertices (two of them between the components' ids)"""
    return np.array([(1, 2), (1, 4), (2, 4), (4, 9), (5, 6), (6, 7), (7, 8), (5, 8)], dtype=np.int64), 11


def random_edges(rng, n, m):
    """up to m distinct edges on n vertices"""
    if n < 2 or m < 1:
        return np.zeros((0, 2), dtype=np.int64)
    e = rng.randint(0, n, (m, 2))
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.stack([e.min(axis=1), e.max(axis=1)], axis=1), axis=0) if e.size else e
    return e.astype(np.int64).reshape(-1, 2)


def many_roots_edges(graphs=200, seed=20261021):
    """the disjoint union of `graphs` seeded random graphs (2 … 24 vertices, 0.5 … 3 times as many edge draws) under a seeded permutation of
    all ids: hundreds of roots in one forest"""
    rng = np.random.RandomState(seed)
    parts, n = [], 0
    for _ in range(graphs):
        k = int(rng.randint(2, 25))
        m = int(round(k * rng.uniform(0.5, 3.0)))
        parts.append(random_edges(rng, k, m) + n)
        n += k
    perm = rng.permutation(n)
    return perm[np.concatenate(parts)], n


def permuted(off, adj, seed):
    """the same graph under a seeded permutation of its ids"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    perm = np.random.RandomState(seed).permutation(n)
    src = sources(off)
    up = src < adj
    return csr_of(np.stack([perm[src[up]], perm[adj[up]]], axis=1), n)


def rec_of(key):
    return next(r for r in J["records"] if r["graph"] == key)


_BICC = {}


def golden_bicc(capi, key):
    """bicc_np of a golden graph, computed once"""
    if key not in _BICC:
        _BICC[key] = bicc_np(*golden_arrays(capi, key))
    return _BICC[key]


# ---- the goldens ------------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_complete():
    assert sorted(J["graphs"]) == sorted(graph_keys()) and len(J["records"]) == len(J["graphs"]) == 11
    for r in J["records"]:
        assert set(INFO_KEYS) <= set(r) and len(r["sha256_block"]) == 64 and len(r["sha256_blocks_at"]) == 64
        has = all(("%s_%s" % (a, r["graph"])) in ARR.files for a in ("block", "blocks_at"))
        assert has == (J["graphs"][r["graph"]]["n"] <= ARRAY_MAX_N), r["graph"]
    assert os.path.getsize(os.path.join(GOLDEN, "bicc.npz")) < 1 << 19
    assert rec_of("kronecker_12_2")["bridges"] > 100 and rec_of("kronecker_12_2")["blocks"] > rec_of("kronecker_12_2")["bridges"]


@pytest.mark.parametrize("key", graph_keys())
def test_restatement_reproduces_the_golden(capi, key):
    off, adj = golden_arrays(capi, key)
    block, blocks_at, arc_keep, info = golden_bicc(capi, key)
    r = rec_of(key)
    assert (J["graphs"][key]["n"], J["graphs"][key]["nnz"]) == (off.size - 1, adj.size)
    assert info == {k: r[k] for k in INFO_KEYS}
    assert sha(block) == r["sha256_block"] and sha(blocks_at) == r["sha256_blocks_at"]
    assert identities_hold(off, adj, block, blocks_at, arc_keep, info)
    if off.size - 1 <= ARRAY_MAX_N:
        assert np.array_equal(ARR["block_" + key], block) and np.array_equal(ARR["blocks_at_" + key], blocks_at)


def test_restatement_against_networkx_on_random_graphs():
    pytest.importorskip("networkx")
    rng = np.random.RandomState(1985)
    for _ in range(200):
        n = int(rng.randint(1, 41))
        e = random_edges(rng, n, int(round(n * rng.uniform(0.5, 4.0))))
        off, adj = csr_of(e, n)
        block, blocks_at, arc_keep, info = bicc_np(off, adj)
        against_networkx(off, adj, block, blocks_at, arc_keep)
        assert identities_hold(off, adj, block, blocks_at, arc_keep, info)


def test_shapes_have_the_stated_values():
    def run(edges_n):
        off, adj = csr_of(*edges_n)
        return (off, adj) + bicc_np(off, adj)
    off, adj, block, at, keep, info = run(path_edges(4096))
    assert (info["blocks"], info["bridges"], info["levels"], info["articulation_points"]) == (4095, 4095, 4096, 4094)
    assert np.all(at[1:-1] == 2) and at[0] == at[-1] == 1 and not keep.any() and np.array_equal(block[sources(off) < adj], np.arange(4095))
    off, adj, block, at, keep, info = run(cycle_edges(4096))
    assert (info["blocks"], info["bridges"], info["articulation_points"], info["largest_block_edges"], info["levels"]) == (1, 0, 0, 4096, 2049)
    for leaves in (1500, 40000):
        off, adj, block, at, keep, info = run(star_edges(leaves))
        assert (info["blocks"], info["bridges"], info["articulation_points"], info["max_blocks_at"], at[0]) == (leaves, leaves, 1, leaves, leaves)
    off, adj, block, at, keep, info = run(windmill_edges(500))
    assert (info["blocks"], info["bridges"], at[0], info["articulation_points"], info["largest_block"]) == (500, 0, 500, 1, 0) and keep.all()
    for shape, edges in ((clique_edges(64), 64 * 63 // 2), (grid_edges(64)[0], 2 * 64 * 63)):
        off, adj, block, at, keep, info = run((shape, 64 if edges == 2016 else 4096))
        assert (info["blocks"], info["largest_block_edges"], info["articulation_points"]) == (1, edges, 0) and not block.any()
    off, adj, block, at, keep, info = run(clique_chain_edges(6))
    # K5 (0..4), K5 (4..8), bridge 8-9, K5 (9..13), K5 (13..17), bridge 17-18, K5 (18..22), K5 (22..26)
    assert (info["blocks"], info["bridges"], info["components"], info["largest_block_edges"], info["largest_block"]) == (8, 2, 1, 10, 0)
    assert at[4] == 2 and at[8] == 2 and at[9] == 2 and at[13] == 2 and at[0] == 1 and info["max_blocks_at"] == 2
    off, adj, block, at, keep, info = run(p3_middle_root())
    assert at.tolist() == [2, 1, 1] and block.tolist() == [0, 1, 0, 1] and info["bridges"] == 2
    off, adj, block, at, keep, info = run(triangle_with_pendant())
    assert at.tolist() == [1, 1, 2, 1] and block.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and keep.tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    off, adj, block, at, keep, info = run(two_components_and_isolated())
    assert (info["components"], info["isolated"], info["blocks"], info["bridges"], info["articulation_points"]) == (5, 3, 3, 1, 1) and at[4] == 2
    off, adj, block, at, keep, info = run(many_roots_edges())
    assert dict({k: info[k] for k in MANY_ROOTS if k != "n"}, n=off.size - 1) == MANY_ROOTS and identities_hold(off, adj, block, at, keep, info)
    off, adj = csr_of(np.zeros((0, 2), dtype=np.int64), 5)
    block, at, keep, info = bicc_np(off, adj)
    assert info == dict(dict.fromkeys(INFO_KEYS, 0), components=5, isolated=5) and at.tolist() == [0] * 5 and block.size == 0


def test_a_chain_of_three_cliques_shares_a_vertex_of_three_blocks():
    # vertex 4 in two K_5's and a bridge: blocks_at 3
    e = np.concatenate([clique_edges(5, 0), clique_edges(5, 4), np.array([(4, 9)], dtype=np.int64)])
    off, adj = csr_of(e, 10)
    block, at, keep, info = bicc_np(off, adj)
    assert at[4] == 3 and info["max_blocks_at"] == 3 and info["blocks"] == 3 and info["bridges"] == 1


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbol_declared_exported_and_documented(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(L, "gmsx_biconnected_components") and "gmsx_biconnected_components" in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    assert re.search(r"\bint gmsx_biconnected_components\(", hdr) and "} gmsx_bicc_info;" in hdr
    for opt in BCC_OPTIONS:
        assert opt in capi.option_names() and re.search(r"\b%s\b" % opt, hdr), opt
    assert ctypes.sizeof(capi.BiccInfo) == 72
    assert capi.lib().gmsx_version() == 320


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_entry_point_fails_loudly_without_gpu(capi):
    L = capi.lib()
    at = np.full(4, -77, dtype=np.int32)
    info = capi.BiccInfo()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(1 << 16)))  # never read: the call checks the device before it reads the handle
    assert L.gmsx_biconnected_components(fake, 0, None, at.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_biconnected_components(None, 0, None, None, None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_biconnected_components(fake, 0, None, None, None, None, None) == capi.ERR_INVALID
    assert L.gmsx_biconnected_components(fake, 2, None, at.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert np.all(at == -77)
