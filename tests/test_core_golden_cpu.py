"""CPU: the goldens of the core decomposition (tests/golden/core_orders.{json,npz}, written by tools/make_golden_core.py from the compiled
reference) agree with the peel gmsx_core_decomposition is specified by (include/gmsx.h), restated here in numpy:

  * the restatement reproduces the golden core numbers (the running maximum of the removal degrees along the reference's Matula order) and
    the golden degeneracies (CoreNumberEvaluator::getCoreNumberOfOrder; the naive DegeneracyOrderingVerifier::getDegeneracy where recorded);
  * the golden Matula rank is a permutation whose later-neighbour counts never exceed the golden core numbers;
  * the golden quality integers follow from the golden ranks;
  * the three entry points are in capi.SYMBOLS and exported by libgmsx.so.

peel_np / later_np / quality_np are what tests/test_core_gpu.py checks the device against."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden

CORE = load_golden("core_orders.json")
ARR = np.load(os.path.join(GOLDEN, "core_orders.npz"))
ORD = np.load(os.path.join(GOLDEN, "orderings.npz"))
LITERAL = sorted(k for k, r in CORE.items() if r["literal"])


def rows_of(off, vs):
    """indices into the adjacency array of all entries of the rows `vs`"""
    lens = (off[vs + 1] - off[vs]).astype(np.int64)
    total = int(lens.sum())
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    return np.repeat(off[vs].astype(np.int64) - starts, lens) + np.arange(total, dtype=np.int64)


def peel_np(off, adj):
    """The peel of include/gmsx.h: k rises to the smallest remaining degree; then rounds until none applies — in a round every remaining
    vertex of remaining degree <= k leaves at once (core number k, round = running index).  Returns (core, round_of, rounds, levels)."""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    deg = np.diff(off)
    core, rnd = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    left, r, k, levels = n, 0, 0, 0
    while left:
        k = max(k, int(deg[alive].min()))
        levels += 1
        while True:
            f = np.flatnonzero(alive & (deg <= k))
            if f.size == 0:
                break
            core[f], rnd[f], alive[f] = k, r, False
            left -= f.size
            r += 1
            if f.size * 64 < n:  # few rows: touch only their neighbours
                nb, c = np.unique(adj[rows_of(off, f)], return_counts=True)
                deg[nb] -= c
            else:
                deg -= np.bincount(adj[rows_of(off, f)], minlength=n)
    return core, rnd, r, levels


def later_np(off, adj, rank):
    """later[v] = |{w in N(v): rank[w] > rank[v]}|"""
    off, rank = np.asarray(off, dtype=np.int64), np.asarray(rank, dtype=np.int64)
    n = off.size - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    return np.bincount(src[rank[np.asarray(adj)] > rank[src]], minlength=n).astype(np.int64)


def quality_np(later, cn, n):
    """The integers and the three doubles of CoreNumberEvaluator::evaluateCoreNrAccuracy (core_number_evaluator.h:73-112)."""
    over = later > cn
    faulty, excess = int(over.sum()), int((later[over] - cn).sum())
    mx = int(later.max()) if later.size else 0
    q = {"max_later": mx, "core_number": int(cn), "core_number_of_order": max(int(cn), mx), "faulty": faulty, "excess": excess,
         "relative_error": 0.0, "fault_rate": 0.0, "relative_mean_difference": 0.0}
    if cn > 0:
        q["relative_error"] = (q["core_number_of_order"] - cn) / float(cn)
        q["fault_rate"] = float(faulty) / float(n)
        q["relative_mean_difference"] = 0.0 if faulty == 0 else (float(excess) / float(faulty)) / float(cn)
    return q


def golden_csr(capi, key):
    src = CORE[key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    from conftest import host_graph
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def test_goldens_are_complete():
    assert len(CORE) >= 14 and len(LITERAL) >= 12
    for key, rec in CORE.items():
        assert rec["degeneracy"] >= 1 and {"degree", "matula"} <= set(rec["quality"])
        assert rec["naive_degeneracy"] in (None, rec["degeneracy"])
        if rec["n"] <= 1 << 10:
            assert rec["naive_degeneracy"] == rec["degeneracy"]
        for kind in ("matula_", "core_", "degrank_"):
            assert (kind + key in ARR) == rec["literal"]
    assert any(not r["literal"] for r in CORE.values())  # the sha256-only graphs (kronecker 16 and up)


@pytest.mark.parametrize("key", LITERAL)
def test_peel_restatement_reproduces_the_reference(capi, key):
    rec, csr = CORE[key], golden_csr(capi, key)
    off, adj = csr.offsets(), csr.neighbors()
    n = off.size - 1
    assert (n, adj.size) == (rec["n"], rec["nnz"])
    core, rnd, rounds, levels = peel_np(off, adj)
    want = ARR["core_" + key]
    assert np.array_equal(core, want)
    assert hashlib.sha256(np.ascontiguousarray(core, dtype="<i4").tobytes()).hexdigest() == rec["core_sha256"]
    assert int(core.max()) == rec["degeneracy"] and levels == rec["levels"] == np.unique(want).size
    assert int((core == rec["degeneracy"]).sum()) == rec["top_core"]
    assert rounds == int(rnd.max()) + 1 and rnd.min() == 0
    # the (round, id) order is an exact degeneracy order: nobody has more than core[v] neighbours after it
    order = np.lexsort((np.arange(n), rnd))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    later = later_np(off, adj, rank)
    assert np.all(later <= core) and int(later.max()) == rec["degeneracy"]


@pytest.mark.parametrize("key", LITERAL)
def test_golden_matula_rank_and_quality_integers(capi, key):
    rec, csr = CORE[key], golden_csr(capi, key)
    off, adj = csr.offsets(), csr.neighbors()
    n = off.size - 1
    matula, degrank, core = ARR["matula_" + key], ARR["degrank_" + key], ARR["core_" + key]
    assert np.array_equal(np.sort(matula), np.arange(n)) and np.array_equal(np.sort(degrank), np.arange(n))
    later = later_np(off, adj, matula)
    assert np.all(later <= core)
    by = np.argsort(matula)
    assert np.array_equal(np.maximum.accumulate(later[by]), core[by])  # core = running maximum of the removal degrees
    # PpParallel::getDegreeOrdering: ascending (degree, id)
    assert np.array_equal(np.argsort(degrank), np.lexsort((np.arange(n), np.diff(off))))
    ranks = {"degree": degrank, "matula": matula}
    if "adg" in rec["quality"]:
        ranks["adg"] = ORD["adg_" + key]
    assert set(ranks) == set(rec["quality"])
    for tag, rank in ranks.items():
        assert quality_np(later_np(off, adj, rank), rec["degeneracy"], n) == rec["quality"][tag], (key, tag)
    assert rec["quality"]["matula"]["faulty"] == 0 and rec["quality"]["matula"]["max_later"] == rec["degeneracy"]
    if "adg" in rec["quality"]:  # the reference's ADG verifier (degeneracy_verifier.h:88-113)
        assert rec["quality"]["adg"]["max_later"] <= rec["quality"]["degree"]["max_later"]


def test_peel_restatement_on_shapes():
    def csr_of(edges, n):
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        e = np.concatenate([e, e[:, ::-1]])
        e = e[np.lexsort((e[:, 1], e[:, 0]))]
        return np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]), e[:, 1]
    core, rnd, rounds, levels = peel_np(*csr_of([(i, j) for i in range(70) for j in range(i)], 70))
    assert np.all(core == 69) and rounds == 1 and levels == 1
    core, rnd, rounds, levels = peel_np(*csr_of([(i, i + 1) for i in range(4000)], 4001))
    assert np.all(core == 1) and rounds == 2001 and levels == 1 and rnd[2000] == 2000
    core, rnd, rounds, levels = peel_np(*csr_of([(0, 1)], 5))
    assert core.tolist() == [1, 1, 0, 0, 0] and rnd.tolist() == [1, 1, 0, 0, 0] and (rounds, levels) == (2, 2)


def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_core_decomposition", "gmsx_degree_rank", "gmsx_order_quality"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert "CORE_WG_FRONTIER" in capi.option_names()
    assert ctypes.sizeof(capi.CoreInfo) == 24 and ctypes.sizeof(capi.OrderQualityInfo) == 56
