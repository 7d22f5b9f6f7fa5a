"""CPU: the goldens of the Jones–Plassmann colouring (tests/golden/coloring.{json,npz}, written by tools/make_golden_coloring.py from the
compiled reference's JonesV3::graph_coloring_jones) agree with the rule gmsx_coloring_jp is specified by (include/gmsx.h), restated here in
numpy as the level-synchronous rounds the device runs:

  * the restatement reproduces every golden colour array and every JSON integer (colors, rounds, max_pred, first_round);
  * colors <= max_pred + 1 for every order, and <= degeneracy + 1 for the Matula rank (the degeneracy of core_orders.json);
  * no gap in 1..colors;
  * the two entry points are in capi.SYMBOLS and exported by libgmsx.so, the option is registered.

jp_np / golden_rank are what tests/test_coloring_gpu.py checks the device against."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_core_golden_cpu import ARR as CORE_ARR, CORE, golden_csr, later_np, rows_of

COL = load_golden("coloring.json")
COL_ARR = np.load(os.path.join(GOLDEN, "coloring.npz"))
ORDERS = ("id", "ff", "degree", "matula", "random")
CASES = [(k, o) for k in sorted(COL) for o in ORDERS]


def golden_rank(key, order):
    """the rank vector of one golden (graph, order): the vertex of the highest position is coloured first"""
    n = COL[key]["n"]
    if order == "id":
        return np.arange(n, dtype=np.int32)
    if order == "ff":
        return np.arange(n - 1, -1, -1, dtype=np.int32)
    if order == "degree":
        return CORE_ARR["degrank_" + key].astype(np.int32)
    if order == "matula":
        return CORE_ARR["matula_" + key].astype(np.int32)
    return COL_ARR["perm_" + key].astype(np.int32)


def jp_np(off, adj, rank):
    """Jones–Plassmann in rounds: the frontier is every vertex whose predecessors (neighbours of higher rank) are all coloured; each takes the
    smallest colour >= 1 none of its coloured neighbours holds.  Returns (coloring, round_of, info dict)."""
    off, adj, rank = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64), np.asarray(rank, dtype=np.int64)
    n = off.size - 1
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), {"colors": 0, "rounds": 0, "max_pred": 0, "first_round": 0}
    pred = later_np(off, adj, rank)
    cnt = pred.copy()
    color, rnd = np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    frontier = np.flatnonzero(cnt == 0)
    first_round, r = int(frontier.size), 0
    while frontier.size:
        lens = off[frontier + 1] - off[frontier]
        owner = np.repeat(np.arange(frontier.size), lens)
        nb = adj[rows_of(off, frontier)]
        c = color[nb]
        held = c > 0  # the frontier is an independent set: a coloured neighbour is a predecessor, an uncoloured one a successor
        # smallest missing colour per frontier vertex: its held colours, unique and ascending, against 1, 2, 3, …
        key = np.unique(owner[held] * (n + 2) + c[held])
        o, cc = key // (n + 2), key % (n + 2)
        k = np.arange(key.size) - np.searchsorted(o, np.arange(frontier.size))[o]
        mex = np.bincount(o, minlength=frontier.size) + 1
        gap = cc != k + 1
        np.minimum.at(mex, o[gap], k[gap] + 1)
        color[frontier], rnd[frontier] = mex, r
        dec = np.bincount(nb[~held], minlength=n)
        cnt -= dec
        frontier = np.flatnonzero((cnt == 0) & (dec > 0))
        r += 1
    assert rnd.min() >= 0
    return color.astype(np.int32), rnd.astype(np.int32), {"colors": int(color.max()), "rounds": r, "max_pred": int(pred.max()), "first_round": first_round}


def test_goldens_are_complete():
    assert len(COL) == 12 and sum(r["source"]["kind"] == "file" for r in COL.values()) == 6
    for key, rec in COL.items():
        assert key in CORE and (rec["n"], rec["nnz"]) == (CORE[key]["n"], CORE[key]["nnz"]) and rec["n"] <= 1 << 14
        assert set(rec["orders"]) == set(ORDERS)
        perm = COL_ARR["perm_" + key]
        assert np.array_equal(np.sort(perm), np.arange(rec["n"]))
        for o in ORDERS:
            assert COL_ARR["color_%s_%s" % (o, key)].shape == (rec["n"],)
    for name in ("coloring.json", "coloring.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 656 * 1024


_JP = {}


def jp_golden(capi, key, order):
    """jp_np of one golden case, computed once per session (the GPU tests share it)"""
    if (key, order) not in _JP:
        csr = golden_csr(capi, key)
        _JP[(key, order)] = jp_np(csr.offsets(), csr.neighbors(), golden_rank(key, order))
    return _JP[(key, order)]


@pytest.mark.parametrize("key,order", CASES)
def test_restatement_reproduces_the_reference(capi, key, order):
    rec = COL[key]["orders"][order]
    color, rnd, info = jp_golden(capi, key, order)
    want = COL_ARR["color_%s_%s" % (order, key)]
    assert np.array_equal(color, want)
    assert info == {f: rec[f] for f in ("colors", "rounds", "max_pred", "first_round")}
    assert info["colors"] <= info["max_pred"] + 1
    assert np.array_equal(np.unique(want), np.arange(1, rec["colors"] + 1))  # no gap in 1..colors
    if order == "matula":
        assert rec["colors"] <= CORE[key]["degeneracy"] + 1 and rec["max_pred"] == CORE[key]["degeneracy"]
    # round_of is the depth in the priority DAG: 0 without predecessors, else 1 + the maximum over them
    csr = golden_csr(capi, key)
    off, adj, rank = csr.offsets().astype(np.int64), csr.neighbors().astype(np.int64), golden_rank(key, order).astype(np.int64)
    src = np.repeat(np.arange(off.size - 1), np.diff(off))
    arc = rank[adj] > rank[src]
    deepest = np.full(off.size - 1, -1, dtype=np.int64)
    np.maximum.at(deepest, src[arc], rnd[adj[arc]].astype(np.int64))
    assert np.array_equal(rnd, deepest + 1)


def test_restatement_on_shapes():
    def csr_of(edges, n):
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        e = np.concatenate([e, e[:, ::-1]])
        e = e[np.lexsort((e[:, 1], e[:, 0]))]
        return np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]), e[:, 1]
    color, rnd, info = jp_np(*csr_of([(i, j) for i in range(33) for j in range(i)], 33), np.arange(33))
    assert color.tolist() == list(range(33, 0, -1)) and info == {"colors": 33, "rounds": 33, "max_pred": 32, "first_round": 1}
    color, rnd, info = jp_np(*csr_of([(i, i + 1) for i in range(99)], 100), np.arange(100))
    assert info == {"colors": 2, "rounds": 100, "max_pred": 1, "first_round": 1} and rnd.tolist() == list(range(99, -1, -1))
    color, rnd, info = jp_np(np.zeros(8, dtype=np.int64), np.zeros(0, dtype=np.int64), np.arange(7))
    assert color.tolist() == [1] * 7 and info == {"colors": 1, "rounds": 1, "max_pred": 0, "first_round": 7}


def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_coloring_jp", "gmsx_coloring_verify"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert "COLOR_WG_FRONTIER" in capi.option_names()
    assert ctypes.sizeof(capi.ColoringInfo) == 24 and ctypes.sizeof(capi.ColoringCheck) == 32
