"""CPU tests of subgraph matching: gmsx_subgraph_order (host only) against the golden orders and literal cases, its error codes, and a
pure-Python brute force over the tiny .el fixtures that reproduces the golden counts, hashes and row 0 — the goldens
(tools/make_golden_subgraph.py) proved against a second implementation."""
import ctypes as C
import hashlib
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

GOLD = load_golden("subgraph.json")


def arrays(capi, edges):
    off, neigh = capi.pattern_arrays(edges)
    return off, neigh


def order_rc(capi, k, off, neigh):
    off = np.ascontiguousarray(off, dtype=np.int64)
    neigh = np.ascontiguousarray(neigh if len(neigh) else [0], dtype=np.int32)
    out = np.full(40, -9, dtype=np.int32)
    rc = capi.lib().gmsx_subgraph_order(k, off.ctypes.data_as(C.c_void_p), neigh.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return rc, out


def test_subgraph_order_golden_and_literal(capi):
    for name, edges in GOLD["patterns"].items():
        want = next(r["order"] for r in GOLD["records"] if r["pattern"] == name)
        assert capi.subgraph_order(edges).tolist() == want, name
    assert capi.subgraph_order([(0, 1), (1, 2), (2, 3)]).tolist() == [0, 1, 2, 3]
    assert capi.subgraph_order([(0, 2), (2, 1), (1, 3)]).tolist() == [0, 2, 1, 3]
    assert capi.subgraph_order([(3, 0), (3, 1), (3, 2)]).tolist() == [0, 3, 1, 2]  # star centred at 3
    assert capi.subgraph_order((np.array([0, 0]), np.zeros(0, np.int32))).tolist() == [0]  # k = 1
    # the three pattern forms agree
    csr = capi.HostCSR.from_edges(np.array([2, 0, 3], np.int32), np.array([0, 3, 1], np.int32), num_nodes=4)
    pair = (np.array(csr.offsets()), np.array(csr.neighbors()))
    assert capi.subgraph_order(csr).tolist() == capi.subgraph_order(pair).tolist() == capi.subgraph_order([(2, 0), (0, 3), (3, 1)]).tolist() == [0, 2, 3, 1]


def test_subgraph_order_error_codes(capi):
    ok_off, ok_neigh = [0, 1, 3, 4], [1, 0, 2, 1]  # path 0-1-2
    assert order_rc(capi, 3, ok_off, ok_neigh)[0] == capi.OK
    assert order_rc(capi, 3, [0, 1, 3, 4], [1, 2, 0, 1])[0] == capi.ERR_NOT_CANONICAL    # row 1 not sorted
    assert order_rc(capi, 3, [0, 2, 4, 5], [0, 1, 0, 2, 1])[0] == capi.ERR_NOT_CANONICAL  # self loop at 0
    assert order_rc(capi, 3, [0, 1, 2, 3], [1, 0, 1])[0] == capi.ERR_NOT_CANONICAL       # arc 2 -> 1 without 1 -> 2
    assert order_rc(capi, 3, [0, 1, 3, 4], [1, 0, 3, 1])[0] == capi.ERR_NOT_CANONICAL    # id >= k
    assert order_rc(capi, 3, [0, 1, 3, 4], [1, 0, -1, 1])[0] == capi.ERR_NOT_CANONICAL   # negative id
    assert order_rc(capi, 3, [0, 3, 2, 4], [1, 0, 2, 1])[0] == capi.ERR_NOT_CANONICAL    # offsets not monotone
    assert order_rc(capi, 4, [0, 1, 2, 3, 4], [1, 0, 3, 2])[0] == capi.ERR_UNSUPPORTED   # two components
    assert order_rc(capi, 2, [0, 0, 0], [])[0] == capi.ERR_UNSUPPORTED                   # two isolated vertices
    assert order_rc(capi, 0, [0], [])[0] == capi.ERR_INVALID
    assert order_rc(capi, -1, [0], [])[0] == capi.ERR_INVALID
    path33 = [(i, i + 1) for i in range(32)]
    off, neigh = arrays(capi, path33)
    assert order_rc(capi, 33, off, neigh)[0] == capi.ERR_UNSUPPORTED
    off, neigh = arrays(capi, path33[:-1])
    rc, out = order_rc(capi, 32, off, neigh)
    assert rc == capi.OK and out[:32].tolist() == list(range(32)) and np.all(out[32:] == -9)
    lib = capi.lib()
    o = np.array(ok_off, np.int64)
    nb = np.array(ok_neigh, np.int32)
    out = np.zeros(3, np.int32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.gmsx_subgraph_order(3, None, vp(nb), vp(out)) == capi.ERR_INVALID
    assert lib.gmsx_subgraph_order(3, vp(o), None, vp(out)) == capi.ERR_INVALID
    assert lib.gmsx_subgraph_order(3, vp(o), vp(nb), None) == capi.ERR_INVALID
    assert "SGM_LAUNCH_TASKS" in capi.option_names()


def brute_force(n, tedges, k, pedges, order, induced):
    """every injective map by itertools, kept if it is an embedding, sorted in the list order: a second implementation of the goldens"""
    A = np.zeros((n, n), dtype=bool)
    for u, v in tedges:
        A[u, v] = A[v, u] = True
    P = np.zeros((k, k), dtype=bool)
    for a, b in pedges:
        P[a, b] = P[b, a] = True
    pairs = [(a, b) for a in range(k) for b in range(a + 1, k)]
    rows = []
    for f in itertools.permutations(range(n), k):
        if all((A[f[a], f[b]] == P[a, b]) if induced else (A[f[a], f[b]] or not P[a, b]) for a, b in pairs):
            rows.append(f)
    rows.sort(key=lambda f: [f[p] for p in order])
    return np.array(rows, dtype=np.int32).reshape(-1, k)


def test_subgraph_goldens_against_brute_force(capi):
    checked = 0
    for rec in GOLD["records"]:
        src = GOLD["graphs"][rec["graph"]]
        k = len(rec["order"])
        if src["kind"] != "file" or src["n"] > 12 or k > 5 or src["n"] ** k > 300000:
            continue
        csr = capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]), relabel=capi.RELABEL_NEVER)
        o, a = csr.offsets(), csr.neighbors()
        tedges = [(u, int(v)) for u in range(csr.num_nodes) for v in a[o[u]:o[u + 1]]]
        for mode, induced in (("induced", True), ("mono", False)):
            rows = brute_force(csr.num_nodes, tedges, k, GOLD["patterns"][rec["pattern"]], rec["order"], induced)
            ent = rec[mode]
            assert ent["count"] == rows.shape[0], (rec["graph"], rec["pattern"], mode)
            assert ent["row0"] == (rows[0].tolist() if rows.shape[0] else None)
            assert ent["sha256"] == hashlib.sha256(np.ascontiguousarray(rows, dtype="<i4").tobytes()).hexdigest()
            checked += 1
        assert rec["ref"] == rec["induced"]["row0"] and rec["ref_verified"] and rec["ref_parallel_found"] == (rec["ref"] is not None)
    assert checked >= 40


def test_subgraph_merge_and_device_calls_without_gpu(capi):
    order = [0, 2, 1]
    a = np.array([[5, 1, 0], [1, 9, 3]], np.int32)
    b = np.array([[1, 2, 3], [5, 0, 0]], np.int32)
    got = capi.merge_subgraph_matches([a, b], order)
    assert got.tolist() == [[1, 2, 3], [1, 9, 3], [5, 0, 0], [5, 1, 0]] and got.dtype == np.int32
    assert capi.merge_subgraph_matches([], order).shape == (0, 3)
    info = capi.SubgraphInfo()
    off, neigh = arrays(capi, [(0, 1)])
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert capi.lib().gmsx_subgraph_match(None, 2, vp(off), vp(neigh), 0, 0, 1, None, 0, C.byref(info), None) == capi.ERR_INVALID
