"""GPU: gmsx_graph_set_weights, gmsx_sssp and gmsx_sssp_verify through the C-ABI against the goldens (tests/golden/sssp.{json,npz}) and the
restatement of tests/test_sssp_golden_cpu.py (dijkstra_np, parent_np, verify_np, info_np):

  goldens      every record at delta 1, 16, 0 (the library's choice) and 2^31 - 1
  re-entry     a path 0 - 1 - … - 2047 of weight 1 plus arcs (0, i) of weight 3 i: every vertex is improved again and again; with one bucket that
               is 2000+ rounds inside the one-workgroup kernel (SSSP_WG_FRONTIER 512) or as many kernel boundaries (0)
  row classes  a star with 1 500 leaves (above kLongRow), one with 40 000 (above kWgRowMax: the tail hands the round back), kronecker 14;
               on the stars info.relaxations is exactly the number of leaves at both ends of SSSP_WG_FRONTIER
  wide         an 8-vertex path of weights 2^31 - 1: distances above 2^32 in 64-bit words; SSSP_WIDE = 1 gives the bytes of the narrow run
  unreachable  two components, isolated vertices, n = 1, an edgeless graph with a weight array of length 0
  unit weights dist and parent are gmsx_bfs's depth and parent
  same bytes   three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, a second handle, re-attached weights, every delta
  verify       a correct array; one entry raised, lowered, set to -1 — each against verify_np's exact counts
  contract     no weights, a weight 0 or -1, an asymmetric array (accepted under TRUSTED), a bad source, delta < 0, NULL info; arrays untouched
               on error; device bytes"""
import ctypes as C

import numpy as np
import pytest

from conftest import host_graph
from test_sssp_golden_cpu import ARR, DELTAS, J, dijkstra_np, golden_csr, info_np, parent_np, rec_id, verify_np
from test_traversal_golden_cpu import grid_edges

pytestmark = pytest.mark.gpu

FACTS = ("reached", "reached_arcs", "dist_sum", "max_dist", "far_vertex")
CLEAN = {"violated_arcs": 0, "untight": 0, "wrong_unreached": 0, "source_ok": 1}


def arrays(csr):
    return np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32), np.array(csr.weights(), dtype=np.int32)


def weighted_graph(gpu, csr, flags=0, shard=None):
    g = gpu.DeviceGraph.from_csr(csr, flags, shard=shard)
    assert not g.has_weights
    g.set_weights(csr.weights())
    assert g.has_weights
    return g


def check(g, off, adj, w, source, delta=0, want=None):
    """dist, parent and the info facts of one call against the restatement; returns (dist, parent, info)"""
    dist, parent, info, st = g.sssp(source, delta, stats=True)
    wd = dijkstra_np(off, adj, w, source) if want is None else want
    assert np.array_equal(dist, wd), (source, delta)
    assert np.array_equal(parent, parent_np(off, adj, w, source, wd)), (source, delta)
    wi = info_np(off, wd, info["delta"])
    assert {k: info[k] for k in FACTS + ("buckets",)} == wi, (source, delta, info, wi)
    assert info["delta"] == delta or (delta == 0 and info["delta"] >= 1)
    assert st["units"] == wi["reached_arcs"] and st["probes"] == wi["buckets"] and st["launches"] >= 3
    assert info["rounds"] >= info["buckets"] - 1 and info["relaxations"] >= info["reached"] - 1
    return dist, parent, info


_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        csr = golden_csr(gpu, key)
        _GRAPHS[key] = (weighted_graph(gpu, csr),) + arrays(csr)
    return _GRAPHS[key]


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_sssp_equals_the_golden(gpu, rec):
    g, off, adj, w = device_graph(gpu, rec["graph"])
    gold = ARR["dist_" + rec_id(rec)].astype(np.int64)
    for delta in DELTAS:
        dist, parent, info = check(g, off, adj, w, rec["source"], delta, want=gold)
        assert np.array_equal(parent, ARR["parent_" + rec_id(rec)])
        assert {k: info[k] for k in ("reached", "dist_sum", "max_dist", "far_vertex")} == {k: rec[k] for k in ("reached", "dist_sum", "max_dist", "far_vertex")}
        assert info["wide"] == 0
    assert g.sssp_verify(rec["source"], gold) == CLEAN
    none_d, none_p, only_info = g.sssp(rec["source"], 16, want_dist=False, want_parent=False)
    assert none_d is None and none_p is None and only_info["dist_sum"] == rec["dist_sum"]


# ---- 2. re-entry ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wg_frontier", [512, 0])
def test_re_entry_chain(gpu, wg_frontier):
    n = 2048
    i = np.arange(2, n)
    src = np.concatenate([np.arange(n - 1), np.zeros(i.size, dtype=np.int64)])
    dst = np.concatenate([np.arange(1, n), i])
    wt = np.concatenate([np.ones(n - 1, dtype=np.int64), 3 * i])
    csr = gpu.HostCSR.from_weighted_edges(src, dst, wt, num_nodes=n)
    off, adj, w = arrays(csr)
    g = weighted_graph(gpu, csr)
    want = np.arange(n, dtype=np.int64)
    with gpu.options(SSSP_WG_FRONTIER=wg_frontier):
        dist, parent, info = check(g, off, adj, w, 0, 2 ** 31 - 1, want=want)   # one bucket: every improvement is a re-entry
        assert info["buckets"] == 1 and info["rounds"] >= 2000 and info["relaxations"] > 2 * n
        assert parent.tolist() == [0] + list(range(n - 1))
        check(g, off, adj, w, 0, 1, want=want)
        check(g, off, adj, w, 0, 0, want=want)
        check(g, off, adj, w, n - 1, 64)
    g.free()


# ---- 3. row classes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1500, 40000])
def test_star(gpu, leaves):
    rng = np.random.RandomState(leaves)
    wt = rng.randint(1, 256, size=leaves)
    csr = gpu.HostCSR.from_weighted_edges(np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), wt, num_nodes=leaves + 1)
    off, adj, w = arrays(csr)
    g = weighted_graph(gpu, csr)
    for source in (0, 7):
        for delta in (0, 16, 2 ** 31 - 1):
            dist, parent, info = check(g, off, adj, w, source, delta)
            assert g.sssp_verify(source, dist) == CLEAN
    assert dist[0] == wt[6] and parent[0] == 7 and np.all(np.delete(parent, [0, 7]) == 0)
    g.free()


@pytest.mark.parametrize("leaves", [1500, 40000])
def test_star_counts_every_relaxation_once(gpu, leaves):
    """info.relaxations is exact here, wherever the walkers flush their counts: every leaf has one arc in and is improved once, from infinity, and
    no arc back to the hub improves distance 0.  1 500 leaves: the hub's row is walked by k_frontier_round_long (frontier bound 0) or by the
    tail's own long walk (512); 40 000: the tail hands the round back."""
    wt = np.random.RandomState(leaves).randint(1, 256, size=leaves)
    csr = gpu.HostCSR.from_weighted_edges(np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), wt, num_nodes=leaves + 1)
    g = weighted_graph(gpu, csr)
    runs = []
    for wg_frontier in (512, 0, 512, 0):
        with gpu.options(SSSP_WG_FRONTIER=wg_frontier):
            dist, parent, info = g.sssp(0, 2 ** 31 - 1)
        assert info["relaxations"] == leaves and info["buckets"] == 1, (wg_frontier, info)
        runs.append((dist.tobytes(), parent.tobytes()))
    assert all(r == runs[0] for r in runs)
    assert np.array_equal(dist[1:], wt) and dist[0] == 0
    g.free()


def test_kronecker_14(gpu):
    csr = gpu.HostCSR.generate_weighted("kronecker", 14, 16, gpu.RELABEL_NEVER)
    off, adj, w = arrays(csr)
    g = weighted_graph(gpu, csr)
    source = int(csr.pick_sources(1)[0])
    want = dijkstra_np(off, adj, w, source)
    for delta in (0, 1, 2 ** 31 - 1):
        dist, parent, info = check(g, off, adj, w, source, delta, want=want)
    assert g.sssp_verify(source, dist) == CLEAN == verify_np(off, adj, w, source, dist)
    with gpu.options(SSSP_WG_FRONTIER=0):
        check(g, off, adj, w, source, 16, want=want)
    g.free()


# ---- 4. wide distances ------------------------------------------------------------------------------------------------------------------
def test_wide_distances(gpu):
    big = 2 ** 31 - 1
    csr = gpu.HostCSR.from_weighted_edges(np.arange(7), np.arange(1, 8), np.full(7, big), num_nodes=8)
    off, adj, w = arrays(csr)
    g = weighted_graph(gpu, csr)
    for delta in (0, 1, 2 ** 31 - 1, 2 ** 40):
        dist, parent, info = check(g, off, adj, w, 0, delta)
        assert info["wide"] == 1 and dist[7] == 7 * big > 2 ** 32 and info["max_dist"] == 7 * big and info["far_vertex"] == 7
    assert g.sssp_verify(0, dist) == CLEAN
    g.free()
    g, off, adj, w = device_graph(gpu, "kronecker_10_16")
    narrow = g.sssp(204, 16)
    with gpu.options(SSSP_WIDE=1):
        wide = g.sssp(204, 16)
    assert wide[2]["wide"] == 1 and narrow[2]["wide"] == 0
    assert narrow[0].tobytes() == wide[0].tobytes() and narrow[1].tobytes() == wide[1].tobytes()
    assert {k: v for k, v in narrow[2].items() if k not in ("wide", "rounds", "relaxations")} == {k: v for k, v in wide[2].items() if k not in ("wide", "rounds", "relaxations")}


# ---- 5. unreachable vertices ------------------------------------------------------------------------------------------------------------
def test_unreachable(gpu):
    csr = gpu.HostCSR.from_weighted_edges([0, 1, 4, 5], [1, 2, 5, 6], [3, 4, 5, 6], num_nodes=9)   # two components, 3, 7 and 8 isolated
    off, adj, w = arrays(csr)
    g = weighted_graph(gpu, csr)
    dist, parent, info = check(g, off, adj, w, 0, 0)
    assert dist.tolist() == [0, 3, 7, -1, -1, -1, -1, -1, -1] and parent.tolist() == [0, 0, 1, -1, -1, -1, -1, -1, -1]
    dist, parent, info = check(g, off, adj, w, 3, 1)   # an isolated source
    assert info["reached"] == 1 and info["far_vertex"] == 3 and info["max_dist"] == 0 and info["buckets"] == 1
    assert g.sssp_verify(3, dist) == CLEAN
    check(g, off, adj, w, 6, 2)
    g.free()
    one = gpu.HostCSR.from_arrays_weighted(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))   # n = 1
    g = weighted_graph(gpu, one)
    dist, parent, info = g.sssp(0)
    assert dist.tolist() == [0] and parent.tolist() == [0] and info["reached"] == 1 and info["reached_arcs"] == 0 and info["buckets"] == 1
    g.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # edgeless, n = 5
    g.set_weights(np.zeros(0, dtype=np.int32))
    assert g.has_weights
    dist, parent, info = g.sssp(2)
    assert dist.tolist() == [-1, -1, 0, -1, -1] and parent.tolist() == [-1, -1, 2, -1, -1] and info["far_vertex"] == 2
    g.free()


# ---- 6. unit weights: breadth-first search ----------------------------------------------------------------------------------------------
def test_unit_weights_are_bfs(gpu):
    grid = gpu.HostCSR.from_edges(*grid_edges(40, 40).T, num_nodes=1600)
    for csr, sources in ((host_graph(gpu, "kronecker", 12), (0, 71)), (grid, (0, 820))):
        g = gpu.DeviceGraph.from_csr(csr)
        g.set_weights(np.ones(csr.nnz, dtype=np.int32))
        for s in sources:
            depth, bparent, binfo = g.bfs(s)
            for delta in (0, 1, 3, 2 ** 31 - 1):
                dist, parent, info = g.sssp(s, delta)
                assert np.array_equal(dist, depth.astype(np.int64)) and np.array_equal(parent, bparent)
                assert (info["reached"], info["reached_arcs"], info["dist_sum"], info["max_dist"]) == \
                       (binfo["reached"], binfo["reached_arcs"], binfo["depth_sum"], binfo["levels"] - 1)
        g.free()


# ---- 7. same bytes ----------------------------------------------------------------------------------------------------------------------
def test_same_bytes(gpu):
    csr = golden_csr(gpu, "kronecker_12_16")
    off, adj, w = arrays(csr)
    source = 3585
    base = weighted_graph(gpu, csr)
    first = base.sssp(source, 16)
    assert np.array_equal(first[0], ARR["dist_kronecker_12_16-s3585"])

    def same(r, delta_free=False):
        assert r[0].tobytes() == first[0].tobytes() and r[1].tobytes() == first[1].tobytes()
        skip = ("rounds", "relaxations") + (("delta", "buckets") if delta_free else ())
        assert {k: v for k, v in r[2].items() if k not in skip} == {k: v for k, v in first[2].items() if k not in skip}

    for _ in range(2):
        same(base.sssp(source, 16))
    for delta in DELTAS:
        same(base.sssp(source, delta), delta_free=True)
    with gpu.options(SSSP_WG_FRONTIER=0):
        same(base.sssp(source, 16))
    with gpu.options(SSSP_DELTA_AUTO=1):
        same(base.sssp(source, 0), delta_free=True)
    base.set_weights(w)   # re-attached
    same(base.sssp(source, 16))
    bytes_with = base.device_bytes
    base.set_weights(None)
    assert not base.has_weights and base.device_bytes == bytes_with - 4 * csr.nnz
    base.set_weights(w)
    assert base.device_bytes == bytes_with
    same(base.sssp(source, 16))
    for flags, shard in ((gpu.UPLOAD_TRUSTED, None), (64 << 8, None), (0, (1, 2)), (0, None)):
        g = weighted_graph(gpu, csr, flags, shard)
        same(g.sssp(source, 16))
        g.free()
    base.free()


# ---- 8. verify --------------------------------------------------------------------------------------------------------------------------
def test_verify_counts(gpu):
    g, off, adj, w = device_graph(gpu, "file_two_parts_a")
    source = 12
    dist = ARR["dist_file_two_parts_a-s12"].astype(np.int64)
    assert g.sssp_verify(source, dist) == CLEAN
    # vertices with a child in the tree: lowering a leaf's distance breaks no arc, only the leaf's own tightness
    inner = [int(v) for v in np.unique(ARR["parent_file_two_parts_a-s12"]) if v >= 0 and v != source]
    assert len(inner) >= 3
    for v in (inner[0], inner[-1], inner[len(inner) // 2]):
        up = dist.copy()
        up[v] += 1
        got = g.sssp_verify(source, up)
        assert got == verify_np(off, adj, w, source, up) and got["untight"] + got["violated_arcs"] >= 1
        down = dist.copy()
        down[v] -= 1
        got = g.sssp_verify(source, down)
        assert got == verify_np(off, adj, w, source, down) and got["violated_arcs"] >= 1
        gone = dist.copy()
        gone[v] = -1
        got = g.sssp_verify(source, gone)
        assert got == verify_np(off, adj, w, source, gone) and got["wrong_unreached"] >= 1
    off_source = dist.copy()
    off_source[source] = 1
    assert g.sssp_verify(source, off_source)["source_ok"] == 0
    g2, off2, adj2, w2 = device_graph(gpu, "kronecker_12_16")   # long enough rows for both widths of the pull pass to matter
    d2 = ARR["dist_kronecker_12_16-s71"].astype(np.int64)
    rng = np.random.RandomState(5)
    bad = d2.copy()
    pick = rng.choice(np.flatnonzero(d2 > 0), 40, replace=False)
    bad[pick[:20]] += rng.randint(1, 9, size=20)
    bad[pick[20:30]] -= 1
    bad[pick[30:]] = -1
    assert g2.sssp_verify(71, bad) == verify_np(off2, adj2, w2, 71, bad)


# ---- 9. contract ------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = golden_csr(gpu, "file_two_parts_b")
    off, adj, w = arrays(csr)
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    info, check_out = gpu.SsspInfo(), gpu.SsspCheck()
    dist = np.full(csr.num_nodes, 77, dtype=np.int64)
    parent = np.full(csr.num_nodes, 77, dtype=np.int32)
    dp, pp = dist.ctypes.data_as(C.c_void_p), parent.ctypes.data_as(C.c_void_p)

    def untouched():
        return bool(np.all(dist == 77) and np.all(parent == 77))

    assert L.gmsx_sssp(g._h, 0, 0, dp, pp, C.byref(info), None) == gpu.ERR_INVALID and untouched()   # no weights attached
    assert L.gmsx_sssp_verify(g._h, 0, dp, C.byref(check_out), None) == gpu.ERR_INVALID
    before = g.device_bytes
    for v in (0, -1):
        bad = w.copy()
        bad[5] = v
        with pytest.raises(gpu.GmsxError) as ei:
            g.set_weights(bad)
        assert ei.value.status == gpu.ERR_INVALID and not g.has_weights and g.device_bytes == before
    skew = w.copy()
    skew[0] += 1
    with pytest.raises(gpu.GmsxError) as ei:
        g.set_weights(skew)
    assert ei.value.status == gpu.ERR_NOT_CANONICAL and not g.has_weights
    trusted = gpu.DeviceGraph.from_csr(csr, gpu.UPLOAD_TRUSTED)
    trusted.set_weights(skew)   # the symmetry check is the caller's promise under TRUSTED …
    bad = w.copy()
    bad[5] = 0
    with pytest.raises(gpu.GmsxError) as ei:   # … the range check is never skipped, and a failed attach keeps the earlier weights
        trusted.set_weights(bad)
    assert ei.value.status == gpu.ERR_INVALID and trusted.has_weights
    trusted.free()
    g.set_weights(w)
    assert g.device_bytes == before + 4 * csr.nnz
    n = csr.num_nodes
    for source in (-1, n, 2 ** 31 - 1):
        assert L.gmsx_sssp(g._h, source, 0, dp, pp, C.byref(info), None) == gpu.ERR_INVALID and untouched()
        assert L.gmsx_sssp_verify(g._h, source, dp, C.byref(check_out), None) == gpu.ERR_INVALID
    assert L.gmsx_sssp(g._h, 0, -1, dp, pp, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_sssp(g._h, 0, 0, dp, pp, None, None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_sssp(None, 0, 0, dp, pp, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_sssp_verify(g._h, 0, None, C.byref(check_out), None) == gpu.ERR_INVALID
    assert L.gmsx_sssp_verify(g._h, 0, dp, None, None) == gpu.ERR_INVALID
    assert L.gmsx_graph_set_weights(None, None) == gpu.ERR_INVALID and L.gmsx_graph_has_weights(None) == gpu.ERR_INVALID
    # the weights change no other entry point
    plain = gpu.DeviceGraph.from_csr(csr)
    assert g.tc_total() == plain.tc_total() and g.bfs(9)[0].tobytes() == plain.bfs(9)[0].tobytes()
    check(g, off, adj, w, 9, 0)
    plain.free()
    g.free()
