"""GPU: gmsx_core_decomposition, gmsx_degree_rank and gmsx_order_quality through the C-ABI, against the goldens of the compiled reference
(tests/golden/core_orders.{json,npz}) and the numpy restatement of the peel kept in tests/test_core_golden_cpu.py:

  goldens        core numbers (literal or sha256), degeneracy, levels, top core, rounds
  order          a permutation in both formats, sorted by (round, id), graded as exact, a valid Bron–Kerbosch rank
  degree_rank    the reference's rank bit for bit, both formats
  order_quality  the reference's integers and doubles for its Matula, degree and ADG ranks; later[] against numpy
  shapes         empty, one edge, star, clique, a path of 2 001 rounds, two cliques on a path, one row above every bin threshold, small frontiers too
                 heavy for the one-workgroup kernel
  no cliffs      kronecker 20; the same bytes with other upload flags, on a sharded upload, on a second call and at both ends of CORE_WG_FRONTIER
  contract       NULL info, a non-permutation and an out-of-range id are GMSX_ERR_INVALID and write nothing"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, edges_to_csr, host_graph, load_golden
from test_core_golden_cpu import ARR, CORE, ORD, golden_csr, later_np, peel_np, quality_np

pytestmark = pytest.mark.gpu
GRAPHS = load_golden("graphs.json")
KEYS = sorted(k for k in CORE if CORE[k]["n"] <= 1 << 18)  # (kronecker 20 has its own test below)
LITERAL = [k for k in KEYS if CORE[k]["literal"]]
WG_ALL, WG_NONE = 2 ** 31 - 1, 0
# the golden graphs of scale <= 12 whose maximal-clique count graphs.json records
BK_KEYS = {"kronecker_8_16": "kronecker-8-16-relabel", "kronecker_10_16": "kronecker-10-16-relabel", "kronecker_12_16": "kronecker-12-16-relabel",
           "kronecker_12_4": "kronecker-12-4-relabel"}
assert all(k in CORE and "bk" in GRAPHS[v] for k, v in BK_KEYS.items())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def order_from_rounds(rnd):
    n = rnd.size
    order = np.lexsort((np.arange(n), rnd)).astype(np.int32)
    rank = np.empty(n, dtype=np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    return rank, order


def check_against_restatement(gpu, g, off, adj):
    """core, both orderings and info of one device graph against peel_np; returns (core, rank, info)"""
    n = off.size - 1
    want_core, rnd, rounds, levels = peel_np(off, adj)
    core, rank, info, st = g.core_decomposition(stats=True)
    _, order, info2 = g.core_decomposition(rank_format=False)
    assert np.array_equal(core, want_core)
    degeneracy = int(want_core.max()) if n else 0
    assert info == info2 == {"degeneracy": degeneracy, "levels": levels, "rounds": rounds, "top_core": int((want_core == degeneracy).sum()) if n else 0}
    want_rank, want_order = order_from_rounds(rnd)
    assert np.array_equal(rank, want_rank) and np.array_equal(order, want_order)
    assert st["units"] == n and st["probes"] == rounds and (n == 0 or st["launches"] >= 3)
    only_info = g.core_decomposition(order=False)
    assert only_info[1] is None and only_info[2] == info and np.array_equal(only_info[0], core)
    return core, rank, info


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_core_numbers_equal_the_reference(gpu, key):
    rec, csr = CORE[key], golden_csr(gpu, key)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    core, rank, info = check_against_restatement(gpu, g, off, adj)
    assert sha(core) == rec["core_sha256"]
    if rec["literal"]:
        assert np.array_equal(core, ARR["core_" + key])
    assert info["degeneracy"] == rec["degeneracy"] and info["levels"] == rec["levels"] and info["top_core"] == rec["top_core"]
    g.free()


# ---- 2. the order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_order_is_an_exact_degeneracy_order(gpu, key):
    rec, csr = CORE[key], golden_csr(gpu, key)
    off, adj = csr.offsets(), csr.neighbors()
    n = off.size - 1
    g = gpu.DeviceGraph.from_csr(csr)
    core, rank, info = g.core_decomposition()
    _, order, _ = g.core_decomposition(rank_format=False)
    assert np.array_equal(np.sort(rank), np.arange(n)) and np.array_equal(order[rank], np.arange(n))
    q, later = g.order_quality(order, rank_format=False, later=True)
    assert q["max_later"] == rec["degeneracy"] == q["core_number"] and q["faulty"] == 0 and q["excess"] == 0
    assert np.all(later <= core) and np.array_equal(later, later_np(off, adj, rank))
    if key in BK_KEYS:  # what BK consumes (eppsteinPAR.h:41)
        assert g.bk_count(rank=rank) == GRAPHS[BK_KEYS[key]]["bk"]
    elif rec["n"] <= 1 << 12:  # no golden count for this graph: the count must not depend on the rank
        assert g.bk_count(rank=rank) == g.bk_count()
    g.free()


# ---- 3. degree_rank -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_degree_rank_is_the_reference_order(gpu, key):
    csr = golden_csr(gpu, key)
    off = csr.offsets()
    n = off.size - 1
    g = gpu.DeviceGraph.from_csr(csr)
    rank, order = g.degree_rank(), g.degree_rank(rank_format=False)
    want_order = np.lexsort((np.arange(n), np.diff(off)))
    assert np.array_equal(order, want_order) and np.array_equal(order[rank], np.arange(n))
    if CORE[key]["literal"]:
        assert np.array_equal(rank, ARR["degrank_" + key]) and np.array_equal(order, np.argsort(ARR["degrank_" + key]))
    g.free()


# ---- 4. order_quality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", LITERAL)
def test_order_quality_equals_the_reference(gpu, key):
    rec, csr = CORE[key], golden_csr(gpu, key)
    off, adj = csr.offsets(), csr.neighbors()
    n = off.size - 1
    g = gpu.DeviceGraph.from_csr(csr)
    ranks = {"matula": ARR["matula_" + key], "degree": ARR["degrank_" + key]}
    if "adg" in rec["quality"]:
        ranks["adg"] = ORD["adg_" + key]
    for tag, rank in ranks.items():
        want = rec["quality"][tag]
        got, later = g.order_quality(rank, core_number=rec["degeneracy"], later=True)
        for f in ("max_later", "core_number", "core_number_of_order", "faulty", "excess", "relative_error", "fault_rate", "relative_mean_difference"):
            assert got[f] == want[f], (key, tag, f, got[f], want[f])  # the doubles too: the same IEEE expressions on the same integers
        assert got == quality_np(later_np(off, adj, rank), rec["degeneracy"], n)
        assert np.array_equal(later, later_np(off, adj, rank))
        assert g.order_quality(rank) == got                                       # core_number=None: the degeneracy, computed on the device
        order = np.argsort(rank).astype(np.int32)
        assert g.order_quality(order, rank_format=False, core_number=rec["degeneracy"]) == got
    adg, _ = g.adg_rank()
    assert g.order_quality(adg)["max_later"] <= g.order_quality(g.degree_rank())["max_later"]  # degeneracyOrderingApproxVerifier (degeneracy_verifier.h:88-113)
    g.free()


# ---- 5. shapes ------------------------------------------------------------------------------------------------------------------------
def clique(lo, hi):
    return [(i, j) for i in range(lo, hi) for j in range(lo, i)]


def hubs(count, leaves):
    """`count` hubs that form a clique, each with `leaves` leaves of its own: the hubs leave together, in one round of `count` rows"""
    first = count
    e = clique(0, count)
    for h in range(count):
        e += [(h, first + h * leaves + i) for i in range(leaves)]
    return e


SHAPES = {
    "empty": ([], -1),
    "one edge among five": ([(0, 1)], 5),
    "star of 300": ([(0, i) for i in range(1, 300)], -1),
    "clique of 70": (clique(0, 70), -1),
    "path of 4001": ([(i, i + 1) for i in range(4000)], -1),
    "two cliques joined by a path": (clique(0, 40) + clique(100, 125) + [(39, 40)] + [(i, i + 1) for i in range(40, 100)], -1),
    "one row of 40000": ([(0, i) for i in range(1, 40001)] + clique(1, 12), -1),
    # a small frontier that is too heavy for the one-workgroup kernel: more long rows than its list parks / more entries than it may walk
    "300 hubs with long rows": (hubs(300, 1100), -1),
    "450 hubs above the work bound": (hubs(450, 500), -1),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(gpu, name):
    edges, n = SHAPES[name]
    if name == "empty":  # (an edge list without edges builds one isolated vertex: the graph without vertices comes from its arrays)
        csr = gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    else:
        csr = edges_to_csr(gpu, edges, n=n)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    core, rank, info = check_against_restatement(gpu, g, off, adj)
    if name == "empty":
        assert csr.num_nodes == 0 and info == {"degeneracy": 0, "levels": 0, "rounds": 0, "top_core": 0}
        q = g.order_quality(np.zeros(0, np.int32))
        assert q["max_later"] == 0 and q["relative_error"] == 0.0
        assert g.degree_rank().size == 0
    if name == "clique of 70":
        assert np.all(core == 69) and info["rounds"] == 1
    if name == "path of 4001":
        assert np.all(core == 1) and info["rounds"] == 2001  # the many-tiny-rounds path
    if name == "one edge among five":
        assert core.tolist() == [1, 1, 0, 0, 0] and rank.tolist() == [3, 4, 0, 1, 2]
    if csr.num_nodes:
        q, later = g.order_quality(rank, later=True)
        assert q["max_later"] == info["degeneracy"] and q["faulty"] == 0 and np.array_equal(later, later_np(off, adj, rank))
        for opt in (WG_NONE, WG_ALL):
            with gpu.options(CORE_WG_FRONTIER=opt):
                c2, r2, i2 = g.core_decomposition()
            assert np.array_equal(c2, core) and np.array_equal(r2, rank) and i2 == info
        n_ = csr.num_nodes
        assert np.array_equal(g.degree_rank(rank_format=False), np.lexsort((np.arange(n_), np.diff(off))))
        dq, dlater = g.order_quality(g.degree_rank(), core_number=info["degeneracy"], later=True)
        assert np.array_equal(dlater, later_np(off, adj, g.degree_rank())) and dq == quality_np(dlater.astype(np.int64), info["degeneracy"], n_)
    g.free()


def test_edgeless_graph_has_zero_doubles(gpu):
    csr = edges_to_csr(gpu, [], n=7)
    g = gpu.DeviceGraph.from_csr(csr)
    core, rank, info = g.core_decomposition()
    assert np.all(core == 0) and rank.tolist() == list(range(7)) and info == {"degeneracy": 0, "levels": 1, "rounds": 1, "top_core": 7}
    q = g.order_quality(rank)
    assert q == {"max_later": 0, "core_number": 0, "core_number_of_order": 0, "faulty": 0, "excess": 0, "relative_error": 0.0, "fault_rate": 0.0,
                 "relative_mean_difference": 0.0}
    g.free()


# ---- 6. no cliffs ---------------------------------------------------------------------------------------------------------------------
def test_kronecker_20(gpu):
    csr = host_graph(gpu, "kronecker", 20, 16, True)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    core, rank, info = check_against_restatement(gpu, g, off, adj)
    rec = CORE.get("kronecker_20_16")
    if rec:
        assert sha(core) == rec["core_sha256"] and info["degeneracy"] == rec["degeneracy"] and info["levels"] == rec["levels"]
        assert info["top_core"] == rec["top_core"]
        dq = g.order_quality(g.degree_rank(), core_number=rec["degeneracy"])
        for f, v in rec["quality"]["degree"].items():
            assert dq[f] == v, f
    q = g.order_quality(rank)
    assert q["max_later"] == info["degeneracy"] and q["faulty"] == 0
    g.free()


@pytest.mark.parametrize("spec", [("kronecker", 14, 16), ("uniform", 12, 16)])
def test_same_bytes_whatever_the_upload_and_the_kernel_mix(gpu, spec):
    csr = host_graph(gpu, *spec, True)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    core, rank, info = g.core_decomposition()
    drank = g.degree_rank()
    q, later = g.order_quality(rank, later=True)
    variants = [("second call", g, None), ("hub limit 256", gpu.DeviceGraph.from_csr(csr, flags=256 << 8), None),
                ("shard 1 of 4", gpu.DeviceGraph.from_csr(csr, shard=(1, 4)), None), ("every round a kernel boundary", g, WG_NONE),
                ("every round in one workgroup", g, WG_ALL), ("tiny threshold", g, 3)]
    for name, h, wg in variants:
        if wg is None:
            c2, r2, i2 = h.core_decomposition()
        else:
            with gpu.options(CORE_WG_FRONTIER=wg):
                c2, r2, i2 = h.core_decomposition()
        assert c2.tobytes() == core.tobytes() and r2.tobytes() == rank.tobytes() and i2 == info, name
        assert h.degree_rank().tobytes() == drank.tobytes(), name
        q2, l2 = h.order_quality(rank, later=True)
        assert q2 == q and l2.tobytes() == later.tobytes(), name
        if h is not g:
            h.free()
    g.free()


# ---- 7. contract ----------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = host_graph(gpu, "kronecker", 8, 16, True)
    n = csr.num_nodes
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    sentinel = np.full(n, -77, dtype=np.int32)
    core, order = sentinel.copy(), sentinel.copy()
    assert L.gmsx_core_decomposition(g._h, core.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), 1, None, None) == gpu.ERR_INVALID
    info = gpu.CoreInfo()
    assert L.gmsx_core_decomposition(None, core.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), 1, C.byref(info), None) == gpu.ERR_INVALID
    assert np.all(core == -77) and np.all(order == -77) and info.degeneracy == 0 and info.rounds == 0
    assert L.gmsx_degree_rank(None, 1, order, None) == gpu.ERR_INVALID and np.all(order == -77)
    good = g.degree_rank()
    qi = gpu.OrderQualityInfo()
    qi.max_later, qi.faulty = -5, -5
    later = sentinel.copy()
    lp = later.ctypes.data_as(C.c_void_p)
    assert L.gmsx_order_quality(g._h, good.ctypes.data_as(C.c_void_p), 1, -1, lp, None, None) == gpu.ERR_INVALID
    twice = good.copy()
    twice[3] = twice[4]                                  # not a permutation
    out_of_range = good.copy()
    out_of_range[5] = n                                  # an id that is no vertex
    negative = good.copy()
    negative[0] = -1
    for bad in (twice, out_of_range, negative):
        for fmt in (1, 0):
            assert L.gmsx_order_quality(g._h, bad.ctypes.data_as(C.c_void_p), fmt, -1, lp, C.byref(qi), None) == gpu.ERR_INVALID
            with pytest.raises(gpu.GmsxError) as ei:
                g.order_quality(bad, rank_format=bool(fmt))
            assert ei.value.status == gpu.ERR_INVALID
    assert np.all(later == -77) and qi.max_later == -5 and qi.faulty == -5
    assert L.gmsx_order_quality(g._h, good.ctypes.data_as(C.c_void_p), 1, -1, lp, C.byref(qi), None) == gpu.OK and qi.max_later >= 1 and later.min() >= 0
    g.free()
