"""GPU: gmsx_link_prediction / gmsx_link_prediction_precision (linkpred.hip) against
  1. the goldens of the compiled reference (tests/golden/link_prediction.json): exact for the count-based metrics, the tolerance rule of
     test_link_prediction_golden_cpu.py for Adamic-Adar and Resource;
  2. the device's own scores: every non-edge pushed through vertex_similarity_batch, the rule applied with numpy.lexsort on the host,
     byte-identical u, v, scores for all seven metrics (what the shared score function guarantees) — on the golden graphs and on edge shapes;
  3. its own variants: the slab path, the smallest chunk budget, a trusted upload, a small hub limit, a repeat call, shards + merge;
  4. the contract of include/gmsx.h, and the precision step against the golden and a numpy set intersection."""
import ctypes as C

import numpy as np
import pytest

from conftest import edges_to_csr, host_graph
from test_link_prediction_golden_cpu import (GRAPH_KEYS, LP, METRICS, RECORDS, check_against_record, digest, golden_csr, rule_from_pairs, split_np)

pytestmark = pytest.mark.gpu
COMMON = (0, 1, 2, 3, 4)  # the five common-neighbour metrics; 5, 6 rank every non-edge


def host_nonedges(off, adj, part=0, nparts=1):
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), np.diff(off)), adj] = True
    u, v = np.triu_indices(n, 1)
    keep = ~A[u, v] & (u % nparts == part)
    return u[keep].astype(np.int32), v[keep].astype(np.int32)


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a[:3], b[:3]))


def check_exact(gpu, g, off, adj, metrics=range(7)):
    """all seven metrics against the rule applied on the host to the device's own batch scores; q around the class boundaries"""
    n = off.size - 1
    u, v = host_nonedges(off, adj)
    out = {}
    for m in metrics:
        s = g.vertex_similarity_batch(m, u, v) if u.size else np.zeros(0)
        cands = int(np.count_nonzero(~np.isnan(s)))
        info1 = g.link_prediction(m, 1)[3]
        if m in COMMON:
            P = info1["positive"]
            qs = {1, P, P + 1, P + 50, cands + 10}
        else:
            assert info1["positive"] == -1
            qs = {1, 7, 100, cands + 10}
        for q in sorted(x for x in qs if x >= 1):
            got = g.link_prediction(m, q)
            want = rule_from_pairs(u, v, s, q)
            assert got[3]["found"] == min(q, cands) == want[0].size, (m, q)
            assert same_bytes(got, want), (METRICS[m], q)
            out[(m, q)] = got
        if m in COMMON:  # POS = the pairs with a common neighbour
            c = g.intersect_count_batch(u, v) if u.size else np.zeros(0)
            assert info1["positive"] == int(np.count_nonzero(c > 0)), METRICS[m]
    return out


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", GRAPH_KEYS)
def test_against_goldens(gpu, key):
    csr = golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    for rec in (r for r in RECORDS if r["graph"] == key):
        u, v, s, info = g.link_prediction(rec["metric"], rec["q"])
        assert info["found"] == rec["found"] == (rec["q"] - rec["padding"] if rec["found"] else 0), (rec["metric"], rec["q"])
        check_against_record(rec, (u, v, s))
    g.free()


# ---- 2. the device's own scores, exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", GRAPH_KEYS)
def test_exact_against_own_scores(gpu, key):
    csr = golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    check_exact(gpu, g, csr.offsets(), csr.neighbors())
    g.free()


def gnp(n, p, seed):
    r = np.random.RandomState(seed)
    return [(a, b) for a in range(n) for b in range(a + 1, n) if r.rand() < p]


def clique(a, b):
    return [(i, j) for i in range(a, b) for j in range(a, i)]


SHAPES = {
    "n1": ([], 1),
    "n2 edge": ([(0, 1)], 2),
    "n2 no edge": ([], 2),
    "K5": (clique(0, 5), 5),
    "five isolated": ([], 5),
    "star with 9 leaves": ([(0, i) for i in range(1, 10)], 10),
    "path of 10": ([(i, i + 1) for i in range(9)], 10),
    "two triangles and two isolated": (clique(0, 3) + clique(3, 6), 8),
    "last two vertices are the non-edge": (clique(0, 6) + [(i, 6) for i in range(6)] + [(i, 7) for i in range(6)], 8),
    "a source without a candidate above it": ([(2, 3), (2, 4), (3, 4), (0, 1)], 5),  # 2 is adjacent to every v > 2
}
for _n in (31, 32, 33, 63, 64, 65):
    SHAPES["gnp %d" % _n] = (gnp(_n, 0.2, _n), _n)


@pytest.mark.parametrize("name", ["n0"] + sorted(SHAPES))
def test_shapes(gpu, name):
    if name == "n0":  # (an edge list without edges builds one isolated vertex: the graph without vertices comes from its arrays)
        csr = gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    else:
        csr = edges_to_csr(gpu, SHAPES[name][0], n=SHAPES[name][1])
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    if name in ("n0", "n1", "n2 edge", "K5"):
        for m in range(7):
            u, v, s, info = g.link_prediction(m, 3)
            assert u.size == v.size == s.size == 0 and info["found"] == 0 and info["classes"] == 0
    if name not in ("n0",):
        out = check_exact(gpu, g, off, adj)
    if name == "five isolated":
        u, v, s, info = g.link_prediction("jaccard", 100)
        assert list(zip(u.tolist(), v.tolist())) == [(a, b) for a in range(5) for b in range(a + 1, 5)][::-1] and np.all(s == 1.0)
        assert info["classes"] == gpu.LP_CLASS_ONE and info["positive"] == 0
        assert g.link_prediction("overlap", 100)[3]["found"] == 0
        ci = g.link_prediction("common", 100)[3]
        assert (ci["found"], ci["scored"], ci["positive"], ci["classes"]) == (10, 0, 0, gpu.LP_CLASS_ZERO)
    if name == "star with 9 leaves":
        for m in COMMON:
            u, v, s, info = g.link_prediction(m, 36)
            assert list(zip(u.tolist(), v.tolist())) == [(a, b) for a in range(1, 10) for b in range(a + 1, 10)][::-1], METRICS[m]
            assert np.unique(s).size == 1 and info["classes"] == gpu.LP_CLASS_POS and info["positive"] == 36
    if name == "two triangles and two isolated":
        u, v, s, info = g.link_prediction("jaccard", 1000)
        assert info["classes"] == gpu.LP_CLASS_ONE | gpu.LP_CLASS_ZERO and (u[-1], v[-1], s[-1]) == (6, 7, 1.0)
        edges = clique(0, 3) + clique(3, 6) + [(4, 6), (0, 6)]  # … and vertex 6 as the common neighbour of 0 and 4: a POS pair
        h = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=9))
        u, v, s, info = h.link_prediction("jaccard", 1000)
        assert info["classes"] == gpu.LP_CLASS_ONE | gpu.LP_CLASS_POS | gpu.LP_CLASS_ZERO and (u[-1], v[-1], s[-1]) == (7, 8, 1.0)
        h.free()
    g.free()


# ---- 3. paths and hooks -----------------------------------------------------------------------------------------------------------------
def test_paths_and_hooks(gpu):
    csr = host_graph(gpu, "kronecker", 10, 8, False)
    g = gpu.DeviceGraph.from_csr(csr)
    for m in (0, 2):
        base = g.link_prediction(m, 500)
        assert base[3]["found"] == 500
        assert same_bytes(g.link_prediction(m, 500), base), "repeat call"
        with gpu.options(LP_LDS_MAXN=0):
            got = g.link_prediction(m, 500)
        assert same_bytes(got, base) and got[3] == base[3], "every bitmap in the global slab"
        with gpu.options(LP_SLAB_MB=1):
            got = g.link_prediction(m, 500)
        assert same_bytes(got, base), "smallest chunk budget"
        if m == 0:
            # the graph has 214 isolated vertices: Jaccard's best 500 are all ONE pairs (1.0), no POS chunk is filled under any budget, so the
            # chunk count asked for at q = 500 cannot exceed 1 here; it is asserted on a q above the ONE pairs of the graph instead (below)
            assert got[3]["classes"] == gpu.LP_CLASS_ONE and got[3]["chunks"] == base[3]["chunks"] == 0
        else:
            assert got[3]["chunks"] > 1 and got[3]["chunks"] > base[3]["chunks"]
        with gpu.options(LP_SLAB_MB=1, LP_LDS_MAXN=0):
            assert same_bytes(g.link_prediction(m, 500), base)
        for name, flags in (("trusted", gpu.UPLOAD_TRUSTED), ("hub limit 64", 64 << 8)):
            h = gpu.DeviceGraph.from_csr(csr, flags=flags)
            assert same_bytes(h.link_prediction(m, 500), base), name
            h.free()
    # a ZERO fill and the ALL class under the smallest budget
    # Jaccard above its ONE pairs (214 * 213 / 2 = 22791): the POS class runs
    for m, q in ((0, 25000), (4, 30000), (6, 3000)):
        base = g.link_prediction(m, q)
        with gpu.options(LP_SLAB_MB=1, LP_LDS_MAXN=0):
            got = g.link_prediction(m, q)
        assert same_bytes(got, base) and got[3]["chunks"] > 1 and got[3]["chunks"] > base[3]["chunks"]
        if m == 0:
            assert base[3]["classes"] & gpu.LP_CLASS_POS and base[3]["classes"] & gpu.LP_CLASS_ONE
    g.free()


@pytest.mark.parametrize("nparts", [3, 4])
def test_shards_merge_to_the_whole(gpu, nparts):
    csr = host_graph(gpu, "kronecker", 10, 8, False)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    for m, q in ((0, 500), (0, 5000), (2, 500), (1, 20000), (5, 700)):
        whole = g.link_prediction(m, q)
        parts = [g.link_prediction(m, q, part=p, nparts=nparts) for p in range(nparts)]
        for p, (u, v, s, info) in enumerate(parts):
            assert np.all(u % nparts == p)
        assert same_bytes(gpu.merge_link_predictions(parts, q), whole), (METRICS[m], q)
        if m in COMMON:
            assert sum(p[3]["positive"] for p in parts) == whole[3]["positive"]
    # one shard against the host rule on its own sources
    u, v = host_nonedges(off, adj, 1, nparts)
    s = g.vertex_similarity_batch(3, u, v)
    assert same_bytes(g.link_prediction(3, 900, part=1, nparts=nparts), rule_from_pairs(u, v, s, 900))
    g.free()


# ---- 4. contract ------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = host_graph(gpu, "kronecker", 8, 4, False)
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    cap = 16
    u, v, s = np.full(cap, -77, np.int32), np.full(cap, -77, np.int32), np.full(cap, -7.5)
    info = gpu.LinkPredictionInfo()
    info.found = -5
    pu, pv, ps = (x.ctypes.data_as(C.c_void_p) for x in (u, v, s))

    def call(h=g._h, metric=0, q=8, part=0, nparts=1, a=pu, b=pv, c=ps, capacity=cap, inf=C.byref(info)):
        return L.gmsx_link_prediction(h, metric, q, part, nparts, a, b, c, capacity, inf, None)
    bad = [dict(q=0), dict(q=-3), dict(metric=7), dict(metric=-1), dict(h=None), dict(inf=None), dict(a=None), dict(b=None), dict(c=None),
           dict(q=17), dict(q=1 << 40), dict(q=(1 << 63) - 1), dict(part=1), dict(part=-1, nparts=2), dict(part=2, nparts=2), dict(nparts=0)]
    for kw in bad:
        assert call(**kw) == gpu.ERR_INVALID, kw
    assert call(q=(1 << 27) + 1, capacity=(1 << 27) + 1) == gpu.ERR_UNSUPPORTED  # refused before an array is touched
    assert np.all(u == -77) and np.all(v == -77) and np.all(s == -7.5) and info.found == -5
    with pytest.raises(gpu.GmsxError) as ei:
        g.link_prediction(0, (1 << 27) + 1)
    assert ei.value.status == gpu.ERR_UNSUPPORTED
    with pytest.raises(gpu.GmsxError) as ei:
        g.link_prediction(0, 0)
    assert ei.value.status == gpu.ERR_INVALID
    assert call(q=16) == gpu.OK and info.found == 16 and np.all(u >= 0) and np.all(u < v)
    # capacity above q: only `found` entries are written
    u[:], v[:], s[:] = -77, -77, -7.5
    assert call(q=3) == gpu.OK and info.found == 3 and np.all(u[3:] == -77) and np.all(s[3:] == -7.5) and np.all(u[:3] >= 0)
    g.free()
    # the ALL class is refused above n = 131072; the common-neighbour metrics are not
    big = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [(i, i + 1) for i in range(131072)], n=131073))
    u[:] = -77
    for m in (5, 6):
        assert L.gmsx_link_prediction(big._h, m, 4, 0, 1, pu, pv, ps, cap, C.byref(info), None) == gpu.ERR_UNSUPPORTED
    assert np.all(u == -77)
    bu, bv, bs, binfo = big.link_prediction("common", 5)
    assert list(zip(bu.tolist(), bv.tolist())) == [(4, 6), (3, 5), (2, 4), (1, 3), (0, 2)] and np.all(bs == 1.0) and binfo["positive"] == 131071
    big.free()


# ---- 5. precision -----------------------------------------------------------------------------------------------------------------------
def test_precision(gpu):
    for p in LP["precision"]:
        csr = host_graph(gpu, p["generator"], p["scale"], p["degree"], p["relabel"])
        train, tu, tv = split_np(gpu, csr, p["seed"], p["test_fraction"])
        g_train = gpu.DeviceGraph.from_csr(train)
        g_test = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, np.stack([tu, tv], axis=1), n=csr.num_nodes))
        u, v, s, info = g_train.link_prediction(p["metric"], tu.size)
        assert info["found"] == p["q"] and digest(u, v, s) == p["prediction_sha256"]
        tp = len(set(zip(u.tolist(), v.tolist())) & set(zip(tu.tolist(), tv.tolist())))
        want = {"true_positives": p["true_positives"], "true_count": p["true_count"], "precision": float.fromhex(p["precision"]),
                "recall": float.fromhex(p["recall"])}
        assert tp == p["true_positives"]
        assert g_test.link_prediction_precision(u, v) == want
        assert g_test.link_prediction_precision(v[::-1], u[::-1]) == want, "reversed, endpoints swapped"
        # one entry twice: it counts once as an edge; n_pred is the length of the list
        hit = np.flatnonzero([(a, b) in set(zip(tu.tolist(), tv.tolist())) for a, b in zip(u.tolist(), v.tolist())])
        i = int(hit[0]) if hit.size else 0
        du, dv = np.concatenate([u, v[i:i + 1]]), np.concatenate([v, u[i:i + 1]])
        got = g_test.link_prediction_precision(du, dv)
        assert got["true_positives"] == tp and got["precision"] == tp / float(u.size + 1) and got["recall"] == want["recall"]
        empty = g_test.link_prediction_precision(np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert empty == {"true_positives": 0, "true_count": p["true_count"], "precision": 0.0, "recall": 0.0}
        for bu, bv in (([3], [3]), ([0], [csr.num_nodes]), ([-1], [2])):
            with pytest.raises(gpu.GmsxError) as ei:
                g_test.link_prediction_precision(np.array(bu, np.int32), np.array(bv, np.int32))
            assert ei.value.status == gpu.ERR_INVALID
        g_train.free()
        g_test.free()
    # an edgeless test graph: both denominators' zero cases give 0.0
    e = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=4))
    assert e.link_prediction_precision([0], [1]) == {"true_positives": 0, "true_count": 0, "precision": 0.0, "recall": 0.0}
    e.free()
