"""GPU: gmsx_min_spanning_forest through the C-ABI against the goldens (tests/golden/msf.{json,npz}) and the restatements of
tests/test_msf_golden_cpu.py (kruskal_np, boruvka_np, info_np, labels_np, mask_np).  All results are integers: every comparison is exact.

  goldens      every record: edge arrays, mask, labels and info; want_edges=False gives the same info
  ties         all weights 1 on a 64 x 64 grid, on K_64 and on a 4096-cycle: only (lo, hi) keeps the picks acyclic
  chain        a path of 4096 vertices with weights 1, 2, …: every vertex picks its left edge, one round hooks a chain of depth n; the same
               path with random weights: rounds is boruvka_np's
  mutual pick  n = 2 with one edge; a perfect matching of 512 pairs
  row classes  stars with 1 500 and 40 000 leaves at both ends of MSF_WAVE_ROW / MSF_WG_ROW and under MSF_PRUNE 0 / 1; kronecker 14 against
               its golden, and the same graph under a seeded renumbering with seeded weights against kruskal_np
  maximum      the MAXIMUM forest on w is the minimum forest on wmax + 1 - w, edge for edge
  extremes     weights 2^31 - 1 (total above 2^32), two components plus isolated vertices, n = 1, an edgeless graph
  consistency  arc_keep fed to gmsx_connected_components; unit weights on the testGraphs: edges == n - components
  same bytes   three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, a second handle, re-attached weights, every
               option combination: one tobytes() value for each output
  contract     no weights, unknown flag bits, two of the three edge arrays, NULL info: ERR_INVALID, arrays untouched; device bytes"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_components_golden_cpu import CC
from test_msf_golden_cpu import ARR, ARRAY_MAX_N, INFO_KEYS, J, boruvka_np, forest, golden_csr, info_np, kruskal_np, labels_np, mask_np, rec_id, record, sha_of
from test_traversal_golden_cpu import grid_edges

pytestmark = pytest.mark.gpu

HUGE = 2 ** 31 - 1
BINS = ((1, 1), (1, HUGE), (HUGE, HUGE))   # MSF_WAVE_ROW, MSF_WG_ROW: every row a workgroup's / a wave's / a lane's or a group's


def arrays(csr):
    return np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32), np.array(csr.weights(), dtype=np.int32)


def weighted_graph(gpu, csr, flags=0, shard=None, w=None):
    g = gpu.DeviceGraph.from_csr(csr, flags, shard=shard)
    g.set_weights(csr.weights() if w is None else w)
    return g


def edge_graph(gpu, src, dst, w, n):
    csr = gpu.HostCSR.from_weighted_edges(np.asarray(src), np.asarray(dst), np.asarray(w), num_nodes=n)
    return (weighted_graph(gpu, csr),) + arrays(csr)


class Expected:
    """what the restatement says of one (graph, weights, flag): computed once, shared by every call that is held to it"""

    def __init__(self, off, adj, w, maximum=False, edges=None):
        self.u, self.v, self.w = kruskal_np(off, adj, w, maximum) if edges is None else edges
        self.mask = mask_np(off, adj, self.u, self.v)
        self.label = labels_np(off.size - 1, self.u, self.v)
        self.info = info_np(off, self.u, self.v, self.w, 0)


def check(g, off, adj, w, maximum=False, want=None):
    """every output of one call against the restatement; returns (u, v, w, mask, label, info, stats)"""
    r = g.min_spanning_forest(maximum=maximum, want_edges=True, want_mask=True, want_labels=True, stats=True)
    u, v, ww, mask, label, info, st = r
    want = want or Expected(off, adj, w, maximum)
    assert np.array_equal(u, want.u) and np.array_equal(v, want.v) and np.array_equal(ww, want.w), maximum
    assert np.array_equal(mask, want.mask) and int(mask.sum()) == 2 * info["edges"]
    assert np.array_equal(label, want.label)
    assert info == dict(want.info, rounds=info["rounds"]) and info["edges"] == off.size - 1 - info["trees"]
    assert info["rounds"] <= int(np.floor(np.log2(max(info["largest_tree"], 1)))) and (info["rounds"] > 0) == (info["edges"] > 0)
    assert st["units"] == info["edges"] and st["probes"] == info["rounds"] and st["launches"] >= 5
    return r


_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        csr = golden_csr(gpu, key)
        _GRAPHS[key] = (weighted_graph(gpu, csr),) + arrays(csr)
    return _GRAPHS[key]


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_msf_equals_the_golden(gpu, rec):
    g, off, adj, w = device_graph(gpu, rec["graph"])
    u, v, ww, mask, label, info, st = check(g, off, adj, w, rec["maximum"], want=Expected(off, adj, w, edges=forest(gpu, rec["graph"], rec["maximum"])))
    assert info == {k: rec[k] for k in INFO_KEYS} and sha_of(u, v, ww) == rec["sha256"]
    if off.size - 1 <= ARRAY_MAX_N:
        for name, a in zip("uvw", (u, v, ww)):
            assert np.array_equal(a, ARR["%s_%s" % (name, rec_id(rec))])
    none = g.min_spanning_forest(maximum=rec["maximum"], want_edges=False)
    assert none[:5] == (None, None, None, None, None) and none[5] == info


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------------
def test_unit_weights_tie_break(gpu):
    k64 = np.array([(a, b) for a in range(64) for b in range(a + 1, 64)])
    cycle = np.stack([np.arange(4096), (np.arange(4096) + 1) % 4096], axis=1)
    for edges, n in ((grid_edges(64, 64), 4096), (k64, 64), (cycle, 4096)):
        g, off, adj, w = edge_graph(gpu, edges[:, 0], edges[:, 1], np.ones(len(edges), dtype=np.int64), n)
        for maximum in (False, True):
            info = check(g, off, adj, w, maximum)[5]
            assert info["edges"] == n - 1 and info["trees"] == 1 and info["total_weight"] == n - 1
        g.free()


# ---- 3. chain -------------------------------------------------------------------------------------------------------------------------
def test_chain(gpu):
    n = 4096
    g, off, adj, w = edge_graph(gpu, np.arange(n - 1), np.arange(1, n), np.arange(1, n), n)
    u, v, ww, mask, label, info, st = check(g, off, adj, w)
    assert info["rounds"] == 1 and info["edges"] == n - 1 and np.array_equal(u, np.arange(n - 1)) and np.all(label == 0)
    g.free()
    g, off, adj, w = edge_graph(gpu, np.arange(n - 1), np.arange(1, n), np.random.RandomState(1).randint(1, 256, size=n - 1), n)
    for maximum in (False, True):
        info = check(g, off, adj, w, maximum)[5]
        assert info["rounds"] == boruvka_np(off, adj, w, maximum)[1] and info["edges"] == n - 1
    g.free()


# ---- 4. mutual pick -------------------------------------------------------------------------------------------------------------------
def test_mutual_pick(gpu):
    g, off, adj, w = edge_graph(gpu, [0], [1], [7], 2)
    u, v, ww, mask, label, info, st = check(g, off, adj, w)
    assert (u.tolist(), v.tolist(), ww.tolist(), mask.tolist(), label.tolist()) == ([0], [1], [7], [1, 1], [0, 0]) and info["rounds"] == 1
    g.free()
    pairs = np.arange(512)
    g, off, adj, w = edge_graph(gpu, 2 * pairs, 2 * pairs + 1, np.random.RandomState(3).randint(1, 9, size=512), 1024)
    for maximum in (False, True):
        info = check(g, off, adj, w, maximum)[5]
        assert (info["edges"], info["trees"], info["largest_tree"], info["rounds"]) == (512, 512, 2, 1)
    g.free()


# ---- 5. row classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1500, 40000])
def test_star(gpu, leaves):
    wt = np.random.RandomState(leaves).randint(1, 256, size=leaves)
    g, off, adj, w = edge_graph(gpu, np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), wt, leaves + 1)
    want = Expected(off, adj, w)
    assert want.u.size == leaves   # the forest is every edge
    base = check(g, off, adj, w, want=want)
    for maximum in (False, True):
        examined = {}
        for prune in (0, 1):
            for wave_row, wg_row in BINS + ((256, 4096),):
                with gpu.options(MSF_WAVE_ROW=wave_row, MSF_WG_ROW=wg_row, MSF_PRUNE=prune):
                    r = check(g, off, adj, w, maximum, want=want)
                assert r[5] == base[5] and r[5]["rounds"] == 1 and r[5]["total_weight"] == int(wt.sum())
                examined.setdefault(prune, r[6]["alg_elements"])
                assert r[6]["alg_elements"] == examined[prune]
        assert examined[1] <= examined[0] and examined[1] >= 2 * leaves
    g.free()


def test_kronecker_14(gpu):
    g, off, adj, w = device_graph(gpu, "kronecker_14_16")
    for maximum in (False, True):
        rec = record("kronecker_14_16", maximum)
        got = {}
        for prune in (0, 1):
            with gpu.options(MSF_PRUNE=prune):
                u, v, ww, mask, label, info, st = g.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True, stats=True)
            assert info == {k: rec[k] for k in INFO_KEYS} and sha_of(u, v, ww) == rec["sha256"]
            got[prune] = st["alg_elements"]
        assert got[1] <= got[0]
    # the same graph under a seeded renumbering of its vertices, with seeded weights
    n = off.size - 1
    rng = np.random.RandomState(2)
    perm = rng.permutation(n)
    row = np.repeat(np.arange(n), np.diff(off))
    up = row < adj
    h, off2, adj2, w2 = edge_graph(gpu, perm[row[up]], perm[adj[up]], rng.randint(1, 256, size=int(up.sum())), n)
    assert adj2.size == adj.size
    for maximum in (False, True):
        check(h, off2, adj2, w2, maximum)
    with gpu.options(MSF_WAVE_ROW=1, MSF_WG_ROW=64):
        check(h, off2, adj2, w2)
    h.free()


# ---- 6. maximum -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["kronecker_10_16", "file_two_parts_a"])
def test_maximum_is_the_minimum_of_the_mirrored_weights(gpu, key):
    g, off, adj, w = device_graph(gpu, key)
    mirrored = (int(w.max()) + 1 - w).astype(np.int32)
    h = weighted_graph(gpu, golden_csr(gpu, key), w=mirrored)
    mx = g.min_spanning_forest(maximum=True, want_mask=True, want_labels=True)
    mn = h.min_spanning_forest(maximum=False, want_mask=True, want_labels=True)
    assert np.array_equal(mx[0], mn[0]) and np.array_equal(mx[1], mn[1]) and np.array_equal(mx[2], int(w.max()) + 1 - mn[2])
    assert np.array_equal(mx[3], mn[3]) and np.array_equal(mx[4], mn[4]) and mx[5]["rounds"] == mn[5]["rounds"]
    assert mx[5]["total_weight"] >= g.min_spanning_forest(want_edges=False)[5]["total_weight"]
    h.free()


# ---- 7. extremes ----------------------------------------------------------------------------------------------------------------------
def test_extremes(gpu):
    big = 2 ** 31 - 1
    g, off, adj, w = edge_graph(gpu, np.arange(7), np.arange(1, 8), np.full(7, big), 8)
    for maximum in (False, True):
        info = check(g, off, adj, w, maximum)[5]
        assert info["total_weight"] == 7 * big > 2 ** 32 and info["min_weight"] == info["max_weight"] == big
    g.free()
    g, off, adj, w = edge_graph(gpu, [0, 1, 4, 5, 4], [1, 2, 5, 6, 6], [3, 4, 5, 6, 2], 9)   # two components, 3, 7 and 8 isolated
    u, v, ww, mask, label, info, st = check(g, off, adj, w)
    assert list(zip(u.tolist(), v.tolist(), ww.tolist())) == [(0, 1, 3), (1, 2, 4), (4, 5, 5), (4, 6, 2)]
    assert label.tolist() == [0, 0, 0, 3, 4, 4, 4, 7, 8] and (info["trees"], info["isolated"], info["largest_tree"]) == (5, 3, 3)
    u, v, ww = check(g, off, adj, w, maximum=True)[:3]
    assert list(zip(u.tolist(), v.tolist(), ww.tolist())) == [(0, 1, 3), (1, 2, 4), (4, 5, 5), (5, 6, 6)]
    g.free()
    for key in ("file_two_parts_a", "file_two_parts_b"):
        info = check(*device_graph(gpu, key))[5]
        assert info["trees"] == 2 and info["isolated"] == 0
    one = gpu.HostCSR.from_arrays_weighted(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))   # n = 1
    g = weighted_graph(gpu, one)
    u, v, ww, mask, label, info = g.min_spanning_forest(want_mask=True, want_labels=True)
    assert u.size == v.size == ww.size == mask.size == 0 and label.tolist() == [0]
    assert info == {"edges": 0, "total_weight": 0, "trees": 1, "isolated": 1, "largest_tree": 1, "min_weight": 0, "max_weight": 0, "rounds": 0}
    g.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # edgeless, n = 5
    g.set_weights(np.zeros(0, dtype=np.int32))
    u, v, ww, mask, label, info = g.min_spanning_forest(maximum=True, want_mask=True, want_labels=True)
    assert u.size == 0 and mask.size == 0 and label.tolist() == [0, 1, 2, 3, 4]
    assert info == {"edges": 0, "total_weight": 0, "trees": 5, "isolated": 5, "largest_tree": 1, "min_weight": 0, "max_weight": 0, "rounds": 0}
    g.free()


# ---- 8. consistency -------------------------------------------------------------------------------------------------------------------
def test_mask_feeds_connected_components(gpu):
    for key in ("kronecker_12_16", "file_two_parts_b"):
        g, off, adj, w = device_graph(gpu, key)
        for maximum in (False, True):
            u, v, ww, mask, label, info = g.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True)
            whole, winfo = g.connected_components()
            kept, kinfo = g.connected_components(arc_keep=mask)
            assert whole.tobytes() == kept.tobytes() == label.tobytes()
            assert kinfo["kept_edges"] == info["edges"] and kinfo["components"] == winfo["components"] == info["trees"]
            assert kinfo["largest"] == info["largest_tree"] and kinfo["singletons"] == info["isolated"]
            row = np.repeat(np.arange(off.size - 1), np.diff(off))
            marked = set(zip(row[mask == 1].tolist(), adj[mask == 1].tolist()))
            assert len(marked) == 2 * info["edges"] and all((b, a) in marked for a, b in marked) and set(np.unique(mask).tolist()) <= {0, 1}


def test_unit_weights_on_the_test_graphs(gpu):
    keys = [k for k, r in CC.items() if r["source"]["kind"] == "file"]
    assert len(keys) == 6
    for key in keys:
        csr = gpu.HostCSR.load(os.path.join(GOLDEN, "testGraphs", CC[key]["source"]["name"]))
        g = gpu.DeviceGraph.from_csr(csr)
        g.set_weights(np.ones(csr.nnz, dtype=np.int32))
        u, v, ww, mask, label, info = g.min_spanning_forest(want_labels=True)
        assert info["edges"] == CC[key]["n"] - CC[key]["components"] and info["trees"] == CC[key]["components"]
        assert label.tobytes() == g.connected_components()[0].tobytes() and info["total_weight"] == info["edges"]
        g.free()


# ---- 9. same bytes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maximum", [False, True])
def test_same_bytes(gpu, maximum):
    csr = golden_csr(gpu, "kronecker_12_16")
    off, adj, w = arrays(csr)
    base = weighted_graph(gpu, csr)
    first = base.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True)
    assert sha_of(*first[:3]) == record("kronecker_12_16", maximum)["sha256"]

    def same(r):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r[:5], first[:5])) and r[5] == first[5]

    for _ in range(2):
        same(base.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True))
    for prune in (0, 1):
        for wave_row, wg_row in BINS:
            with gpu.options(MSF_WAVE_ROW=wave_row, MSF_WG_ROW=wg_row, MSF_PRUNE=prune):
                same(base.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True))
    base.set_weights(w)   # re-attached
    same(base.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True))
    base.set_weights(None)
    base.set_weights(w)   # detached and attached again
    same(base.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True))
    for flags, shard in ((gpu.UPLOAD_TRUSTED, None), (64 << 8, None), (0, (1, 2)), (0, None)):
        g = weighted_graph(gpu, csr, flags, shard)
        same(g.min_spanning_forest(maximum=maximum, want_mask=True, want_labels=True))
        g.free()
    base.free()


# ---- 10. contract ---------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = golden_csr(gpu, "file_two_parts_b")
    off, adj, w = arrays(csr)
    n, nnz = csr.num_nodes, csr.nnz
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    info = gpu.MsfInfo()
    info.edges = 77
    eu, ev, ew, label = (np.full(n, 77, dtype=np.int32) for _ in range(4))
    mask = np.full(nnz, 77, dtype=np.uint8)
    pu, pv, pw, pm, pl = (a.ctypes.data_as(C.c_void_p) for a in (eu, ev, ew, mask, label))

    def untouched():
        return bool(all(np.all(a == 77) for a in (eu, ev, ew, mask, label)) and info.edges == 77)

    assert L.gmsx_min_spanning_forest(g._h, 0, pu, pv, pw, pm, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()   # no weights attached
    g.set_weights(w)
    before = g.device_bytes
    for flags in (2, 4, 1 << 31, 3):
        assert L.gmsx_min_spanning_forest(g._h, flags, pu, pv, pw, pm, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    for trio in ((pu, pv, None), (pu, None, pw), (None, pv, pw), (pu, None, None), (None, None, pw)):
        assert L.gmsx_min_spanning_forest(g._h, 0, trio[0], trio[1], trio[2], pm, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_min_spanning_forest(g._h, 0, pu, pv, pw, pm, pl, None, None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_min_spanning_forest(None, 0, pu, pv, pw, pm, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_min_spanning_forest(g._h, 1, pu, pv, pw, pm, pl, C.byref(info), None) == gpu.OK and not untouched()
    assert info.edges == record("file_two_parts_b", True)["edges"] and np.all(eu[info.edges:] == 77)
    assert g.device_bytes == before
    check(g, off, adj, w)
    assert g.device_bytes == before
    # the call changes no other entry point's answer
    assert g.sssp(9)[0].tobytes() == weighted_graph(gpu, csr).sssp(9)[0].tobytes()
    g.free()
