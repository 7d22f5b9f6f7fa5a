"""CPU: the goldens of gmsx_greedy_matching / gmsx_matching_verify (tests/golden/matching.json, matching.npz; tools/make_golden_matching.py)
against restatements in plain Python / numpy, which are also what tests/test_matching_gpu.py holds the device to:
  * mix_np      — the 32-bit mixer h(lo, hi) of include/gmsx.h;
  * greedy_np   — THE matching: the edges sorted by the key (heavier w first, h, lo, hi), then one scan that keeps an edge iff both ends are free;
  * rounds_np   — the locally dominant rounds the device runs: (mate, rounds), the same mate;
  * check_np    — the six integers of gmsx_matching_check for any mate array;
  * info_np     — the integers of gmsx_matching_info; pairs_np — the pairs (u, v, w), u < v, ascending by u.
w = None is the unweighted call (every edge weighs 1).  The reference has no matching; networkx's max_weight_matching bounds the total weight
from above by a factor of two."""
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

J = load_golden("matching.json")
ARR = np.load(os.path.join(GOLDEN, "matching.npz"))
INFO_KEYS = ("pairs", "total_weight", "free_vertices", "exposed", "min_weight", "max_weight", "rounds")
CHECK_KEYS = ("invalid", "pairs", "total_weight", "free_vertices", "augmentable", "undominated")
ARRAY_MAX_N = 1 << 12   # graphs up to scale 12 keep their mate array in matching.npz (the limit of the msf goldens)
# the golden graphs: every file of tests/golden/testGraphs (unit weights only), the two weighted files of tests/golden/sssp and kronecker 10 / 14
# with the loader's weights 1 … 255 (the last four both unweighted and weighted)
GRAPHS = {
    "el_eppsteinExample": {"kind": "el", "name": "eppsteinExample.el"}, "el_micro": {"kind": "el", "name": "micro.el"},
    "el_smallRandom1": {"kind": "el", "name": "smallRandom1.el"}, "el_tomitaExample": {"kind": "el", "name": "tomitaExample.el"},
    "el_triangles_1": {"kind": "el", "name": "triangles_1.el"}, "el_triangles_3": {"kind": "el", "name": "triangles_3.el"},
    "wel_two_parts_a": {"kind": "wel", "name": "two_parts_a.wel"}, "wel_two_parts_b": {"kind": "wel", "name": "two_parts_b.wel"},
    "kronecker_10_16": {"kind": "generated", "generator": "kronecker", "scale": 10, "degree": 16},
    "kronecker_14_16": {"kind": "generated", "generator": "kronecker", "scale": 14, "degree": 16},
}


def record_keys():
    """(graph, weighted) of every record, in the order of the file"""
    return [(k, wt) for k in sorted(GRAPHS) for wt in ((False,) if GRAPHS[k]["kind"] == "el" else (False, True))]


def golden_csr(capi, key):
    """The host CSR of a golden graph, never relabelled; the .el files carry no weights."""
    src = GRAPHS[key]
    if src["kind"] == "el":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]), symmetrize=True, relabel=capi.RELABEL_NEVER)
    if src["kind"] == "wel":
        return capi.HostCSR.load_weighted(os.path.join(GOLDEN, "sssp", src["name"]), symmetrize=True, relabel=capi.RELABEL_NEVER)
    return capi.HostCSR.generate_weighted(src["generator"], src["scale"], src["degree"], capi.RELABEL_NEVER)


_CSR = {}


def golden_arrays(capi, key):
    """(off, adj, w): w = None for the .el files"""
    if key not in _CSR:
        c = golden_csr(capi, key)
        w = None if GRAPHS[key]["kind"] == "el" else np.array(c.weights(), dtype=np.int32)
        _CSR[key] = (np.array(c.offsets(), dtype=np.int64), np.array(c.neighbors(), dtype=np.int32), w)
    return _CSR[key]


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def mix_np(lo, hi):
    lo, hi, m = np.asarray(lo).astype(np.uint64), np.asarray(hi).astype(np.uint64), np.uint64(0xFFFFFFFF)
    h = (lo * np.uint64(0x9E3779B1) + hi) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def upper_edges(off, adj, w=None):
    """(lo, hi, w) of the u < v arcs, in CSR order: ascending by (lo, hi); w = None: ones"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    row = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
    up = row < adj
    ww = np.ones(int(up.sum()), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)[up]
    return row[up], adj[up], ww


def order_np(lo, hi, w):
    """the edge indices in the order of gmsx.h: heavier first, then h, lo, hi"""
    return np.lexsort((hi, lo, mix_np(lo, hi), -w))


def greedy_np(off, adj, w=None):
    n = len(off) - 1
    lo, hi, ww = upper_edges(off, adj, w)
    order = order_np(lo, hi, ww)
    mate = [-1] * n
    for a, b in zip(lo[order].tolist(), hi[order].tolist()):
        if mate[a] < 0 and mate[b] < 0:
            mate[a], mate[b] = b, a
    return np.array(mate, dtype=np.int32)


def rounds_np(off, adj, w=None):
    """(mate, rounds): in every round the live edges (both ends free) that are the first live edge of both of their ends are matched"""
    n = len(off) - 1
    lo, hi, ww = upper_edges(off, adj, w)
    rank = np.empty(lo.size, dtype=np.int64)
    rank[order_np(lo, hi, ww)] = np.arange(lo.size)
    mate = -np.ones(n, dtype=np.int64)
    alive = np.ones(lo.size, dtype=bool)
    rounds = 0
    while True:
        alive &= (mate[lo] < 0) & (mate[hi] < 0)
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        best = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(best, lo[idx], rank[idx])
        np.minimum.at(best, hi[idx], rank[idx])
        dom = idx[(best[lo[idx]] == rank[idx]) & (best[hi[idx]] == rank[idx])]
        mate[lo[dom]] = hi[dom]
        mate[hi[dom]] = lo[dom]
        rounds += 1
    return mate.astype(np.int32), rounds


def _edge_index(n, lo, hi, a, b):
    """the index of the edge {a, b} among the u < v arcs, -1 if it is none (the codes lo * n + hi ascend)"""
    code = lo * n + hi
    want = np.minimum(a, b) * n + np.maximum(a, b)
    if code.size == 0:
        return -np.ones(want.shape, dtype=np.int64)
    at = np.minimum(np.searchsorted(code, want), code.size - 1)
    return np.where(code[at] == want, at, -1)


def check_np(off, adj, w, mate):
    """gmsx_matching_check: a vertex is invalid if its mate is outside [-1, n), is itself or no neighbour, or if its mate's mate is not the
    vertex; everything else treats the invalid vertices as free"""
    n = len(off) - 1
    lo, hi, ww = upper_edges(off, adj, w)
    mate = np.asarray(mate, dtype=np.int64)
    v = np.arange(n, dtype=np.int64)
    claims = mate != -1
    mutual = claims & (mate >= 0) & (mate < n) & (mate != v)
    mutual[mutual] = mate[mate[mutual]] == v[mutual]
    edge = -np.ones(n, dtype=np.int64)   # the index of v's matching edge
    edge[mutual] = _edge_index(n, lo, hi, v[mutual], mate[mutual])
    valid = edge >= 0
    rank = np.empty(lo.size, dtype=np.int64)
    rank[order_np(lo, hi, ww)] = np.arange(lo.size)
    mrank = np.full(n, np.iinfo(np.int64).max)   # the rank of v's matching edge in the order
    mrank[valid] = rank[edge[valid]]
    in_matching = np.zeros(lo.size, dtype=bool)
    in_matching[edge[valid]] = True
    others = ~in_matching
    pairs = int(in_matching.sum())
    return {"invalid": int((claims & ~valid).sum()), "pairs": pairs, "total_weight": int(ww[in_matching].sum()), "free_vertices": n - 2 * pairs,
            "augmentable": int((others & ~valid[lo] & ~valid[hi]).sum()),
            "undominated": int((others & (np.minimum(mrank[lo], mrank[hi]) > rank)).sum())}


def pairs_np(off, adj, w, mate):
    """(u, v, w) of the pairs with u < v, ascending by u"""
    n = len(off) - 1
    lo, hi, ww = upper_edges(off, adj, w)
    mate = np.asarray(mate, dtype=np.int64)
    u = np.flatnonzero(mate > np.arange(n))
    e = _edge_index(n, lo, hi, u, mate[u]) if u.size else np.zeros(0, dtype=np.int64)
    assert np.all(e >= 0)
    return u.astype(np.int32), mate[u].astype(np.int32), ww[e].astype(np.int32)


def info_np(off, adj, w, mate, rounds):
    u, v, ww = pairs_np(off, adj, w, mate)
    free = np.asarray(mate) < 0
    ww = ww.astype(np.int64)
    return {"pairs": int(u.size), "total_weight": int(ww.sum()), "free_vertices": int(free.sum()), "exposed": int((free & (np.diff(off) > 0)).sum()),
            "min_weight": int(ww.min()) if u.size else 0, "max_weight": int(ww.max()) if u.size else 0, "rounds": int(rounds)}


def csr_np(n, src, dst, w=None):
    """(off, adj, w) of an edge list without loops or repeats, rows ascending — the CSR the library builds from it"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    a, b = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.lexsort((b, a))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=off[1:])
    ww = None if w is None else np.concatenate([w, w])[order].astype(np.int32)
    return off, b[order].astype(np.int32), ww


def sha_of(mate):
    return hashlib.sha256(np.ascontiguousarray(mate, dtype="<i4").tobytes()).hexdigest()


def fnv_of(mate):
    """FNV-1a over the same bytes: what the C++ adaptor test prints"""
    x = 1469598103934665603
    for b in np.ascontiguousarray(mate, dtype="<i4").tobytes():
        x = ((x ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return x


def rec_id(r):
    return "%s-%s" % (r["graph"], "weighted" if r["weighted"] else "unit")


def record(key, weighted):
    return next(r for r in J["records"] if r["graph"] == key and r["weighted"] == weighted)


_MATCHING = {}


def matching(capi, key, weighted):
    """(mate, rounds) of a golden graph by greedy_np and rounds_np (which must agree), computed once"""
    if (key, weighted) not in _MATCHING:
        off, adj, w = golden_arrays(capi, key)
        mate = greedy_np(off, adj, w if weighted else None)
        other, rounds = rounds_np(off, adj, w if weighted else None)
        assert np.array_equal(mate, other), (key, weighted)
        _MATCHING[(key, weighted)] = (mate, rounds)
    return _MATCHING[(key, weighted)]


def random_graphs():
    """200 seeded graphs of 8 <= n <= 64 with weights drawn from {1}, 1 … 3 and 1 … 255 in turn: (n, off, adj, w)"""
    rng = np.random.RandomState(20261021)
    for i in range(200):
        n = int(rng.randint(8, 65))
        iu = np.triu_indices(n, 1)
        take = rng.rand(iu[0].size) < rng.uniform(0.05, 0.6)
        take[rng.randint(take.size)] = True   # at least one edge
        src, dst = iu[0][take], iu[1][take]
        w = rng.randint(1, (2, 4, 256)[i % 3], size=src.size)
        yield (n,) + csr_np(n, src, dst, w)


def path_edges(n):
    return np.arange(n - 1), np.arange(1, n)


def grid_edges(rows, cols):
    ids = np.arange(rows * cols).reshape(rows, cols)
    return np.concatenate([ids[:, :-1].ravel(), ids[:-1].ravel()]), np.concatenate([ids[:, 1:].ravel(), ids[1:].ravel()])


def complete_edges(n):
    iu = np.triu_indices(n, 1)
    return iu[0], iu[1]


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
def test_mixer_check_values():
    assert [int(mix_np(a, b)) for a, b in ((0, 1), (0, 2), (1, 2), (5, 7))] == [0x514e28b7, 0x30f4c306, 0x7e32275d, 0xc71f3556]
    assert int(mix_np(0, 50549)) == int(mix_np(50549, 62096)) == 0xe935fad8   # two arcs of the row of 50549 share h: the (lo, hi) tail decides
    # for a fixed end h is a bijection of the other end: no collision among the larger, nor among the smaller neighbours of one vertex
    assert np.unique(mix_np(np.full(1 << 16, 77), np.arange(1 << 16))).size == 1 << 16
    assert np.unique(mix_np(np.arange(1 << 16), np.full(1 << 16, 77))).size == 1 << 16


def test_goldens_are_complete():
    assert sorted(J["graphs"]) == sorted(GRAPHS) and [(r["graph"], r["weighted"]) for r in J["records"]] == record_keys() and len(J["records"]) == 14
    for r in J["records"]:
        assert set(INFO_KEYS) <= set(r) and len(r["sha256"]) == 64
        assert (("mate_" + rec_id(r)) in ARR.files) == (J["graphs"][r["graph"]]["n"] <= ARRAY_MAX_N), rec_id(r)
        assert 2 * r["pairs"] + r["free_vertices"] == J["graphs"][r["graph"]]["n"] and r["rounds"] <= r["pairs"]
    assert os.path.getsize(os.path.join(GOLDEN, "matching.npz")) < 1 << 17 and os.path.getsize(os.path.join(GOLDEN, "matching.json")) < 1 << 14


@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_restatements_reproduce_the_golden(capi, rec):
    off, adj, w = golden_arrays(capi, rec["graph"])
    w = w if rec["weighted"] else None
    mate, rounds = matching(capi, rec["graph"], rec["weighted"])   # greedy_np == rounds_np inside
    assert sha_of(mate) == rec["sha256"] and str(fnv_of(mate)) == rec["fnv"]
    assert info_np(off, adj, w, mate, rounds) == {k: rec[k] for k in INFO_KEYS}
    if off.size - 1 <= ARRAY_MAX_N:
        assert np.array_equal(ARR["mate_" + rec_id(rec)], mate)
    # the certificate: THE matching is valid, maximal and dominates every other edge
    c = check_np(off, adj, w, mate)
    assert c == {"invalid": 0, "pairs": rec["pairs"], "total_weight": rec["total_weight"], "free_vertices": rec["free_vertices"], "augmentable": 0,
                 "undominated": 0}
    if not rec["weighted"]:
        assert rec["total_weight"] == rec["pairs"] and (rec["min_weight"], rec["max_weight"]) == ((1, 1) if rec["pairs"] else (0, 0))


def test_restatements_agree_on_random_graphs_and_half_bound():
    nx = pytest.importorskip("networkx")
    seen_ties = 0
    for n, off, adj, w in random_graphs():
        mate = greedy_np(off, adj, w)
        other, rounds = rounds_np(off, adj, w)
        assert np.array_equal(mate, other)
        c = check_np(off, adj, w, mate)
        assert (c["invalid"], c["augmentable"], c["undominated"]) == (0, 0, 0) and 1 <= rounds <= c["pairs"] <= n // 2
        lo, hi, ww = upper_edges(off, adj, w)
        seen_ties += int(np.unique(ww).size < ww.size)
        g = nx.Graph()
        g.add_weighted_edges_from(zip(lo.tolist(), hi.tolist(), ww.tolist()))
        best = sum(g[a][b]["weight"] for a, b in nx.max_weight_matching(g))
        assert 2 * c["total_weight"] >= best >= c["total_weight"]
    assert seen_ties >= 150   # ties are frequent: every graph with weights from {1} or 1 … 3 and more than three edges has one


def test_a_maximal_matching_greedy_did_not_choose_is_not_certified():
    off, adj, _ = csr_np(4, *path_edges(4))   # 0 - 1 - 2 - 3, unit weights
    mate = greedy_np(off, adj)
    lo, hi, ww = upper_edges(off, adj)
    first = int(order_np(lo, hi, ww)[0])
    assert check_np(off, adj, None, mate) == {"invalid": 0, "pairs": int((mate >= 0).sum()) // 2, "total_weight": int((mate >= 0).sum()) // 2,
                                              "free_vertices": int((mate < 0).sum()), "augmentable": 0, "undominated": 0}
    # the other maximal matching: the middle edge alone, or the two outer edges
    other = np.array([-1, 2, 1, -1]) if mate[1] != 2 else np.array([1, 0, 3, 2])
    c = check_np(off, adj, None, other)
    assert c["invalid"] == 0 and c["augmentable"] == 0 and c["undominated"] > 0, (first, c)
    # perturbations of a mate array
    assert check_np(off, adj, None, np.array([2, -1, 0, -1]))["invalid"] == 2    # not a neighbour
    assert check_np(off, adj, None, np.array([1, 2, 1, -1]))["invalid"] == 1     # 0's mate's mate is someone else
    assert check_np(off, adj, None, np.array([7, -1, -2, 3]))["invalid"] == 3    # out of range, and itself
    assert check_np(off, adj, None, -np.ones(4)) == {"invalid": 0, "pairs": 0, "total_weight": 0, "free_vertices": 4, "augmentable": 3, "undominated": 3}


def test_the_hash_keeps_the_rounds_short():
    # measured with these restatements: 3, 5 and 7 rounds; without h in the order 2048, 95 and 32.  A cap, so that a lost hash shows.
    for n, (src, dst) in ((4096, path_edges(4096)), (4096, grid_edges(64, 64)), (64, complete_edges(64))):
        off, adj, _ = csr_np(n, src, dst)
        mate, rounds = rounds_np(off, adj)
        assert rounds <= 16 and np.array_equal(mate, greedy_np(off, adj))
    # strictly increasing weights along a path: one round per pair, inherent in the order
    off, adj, w = csr_np(256, *path_edges(256), w=np.arange(1, 256))
    mate, rounds = rounds_np(off, adj, w)
    assert rounds == 128 and np.array_equal(mate, np.arange(256) ^ 1)


def test_hash_tie_is_broken_by_the_ids():
    off, adj, w = csr_np(62097, [0, 50549], [50549, 62096], w=np.array([5, 5]))
    mate, rounds = rounds_np(off, adj, w)
    assert (mate[0], mate[50549], mate[62096], rounds) == (50549, 0, -1, 1) and np.array_equal(mate, greedy_np(off, adj, w))


def test_golden_files_equal_what_the_tool_regenerates(capi):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_matching", os.path.join(ROOT, "tools", "make_golden_matching.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    graphs, records, arrays = tool.build(capi)
    assert graphs == J["graphs"] and records == J["records"]
    assert sorted(arrays) == sorted(ARR.files) and all(np.array_equal(arrays[k], ARR[k]) and arrays[k].dtype == ARR[k].dtype for k in arrays)
    assert open(os.path.join(GOLDEN, "matching.json")).read() == tool.json_text(graphs, records)


def test_new_symbols_declared_exported_and_documented(capi):
    import ctypes
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_greedy_matching", "gmsx_matching_verify"):
        assert hasattr(L, name) and name in capi.SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
    assert "GMSX_MATCH_WEIGHTED = 1u" in hdr and "} gmsx_matching_info;" in hdr and "} gmsx_matching_check;" in hdr
    for opt in ("MATCH_WAVE_ROW", "MATCH_WG_ROW", "MATCH_KEEP"):
        assert opt in capi.option_names() and re.search(r"\b%s\b" % opt, hdr), opt
    assert ctypes.sizeof(capi.MatchingInfo) == 48 and ctypes.sizeof(capi.MatchingCheck) == 48 and capi.MATCH_WEIGHTED == 1
    assert capi.lib().gmsx_version() == 320
