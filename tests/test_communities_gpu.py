"""GPU: gmsx_label_propagation and gmsx_modularity through the C-ABI against the goldens (tests/golden/communities.{json,npz}) and the restatements
of tests/test_communities_golden_cpu.py (lp_np, lp_seq, mod_np).  All results are integers: every comparison is exact, except the double
`modularity`, which is held to 1 ulp of the restatement's (numpy's long double is the C one only where the platform gives it 80 bits).

  goldens      every record: label, info, the sha, label=None gives the same info; both modularity blocks
  ties         K_64 ends with every label 0; a 4096-cycle, a 64 x 64 grid, a path of 4096, a perfect matching of 512 pairs, n = 2; a vertex
               whose own label ties with a smaller one keeps its own
  row classes  stars with 1 500 and 40 000 leaves whose centre acts first (that many distinct labels: the table-overflow path) and with the leaves
               pre-merged by a second hub; rows at both sides of every bin edge; LP_LDS_SLOTS = 64 with rows of 63, 64, 65 distinct labels; every
               bin forced; kronecker 14 under a seeded renumbering
  weights      one arc of 7 against three of 2; 2^31 - 1 on five arcs of one label; unit weights = the unweighted call
  colourings   largest-first and smallest-last colourings of gmsx_coloring_jp as the caller's; an improper colouring, a colour 0
  sweep cap    max_sweeps = 1, 2 on kronecker 12
  scheduling   LP_WG_WORK in {0, default, huge} x LP_ACTIVE in {0, 1}: one tobytes() per output
  same bytes   three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, a second handle, re-attached weights
  modularity   one label, all distinct, two K_8 and an edge, S above 2^64, unstable on Jarvis–Patrick and component labels
  consistency  communities inside components, isolated vertices, the two calls agree
  contract     every ERR_INVALID case, n = 1, an edgeless graph, the handle's device bytes"""
import ctypes as C

import numpy as np
import pytest

from test_communities_golden_cpu import (ARR, ARRAY_MAX_N, INFO_KEYS, J, MOD_KEYS, cc_labels_np, csr_of, graph_arrays, lf_rank, lp_np, lp_seq, mod_np,
                                         rec_id, run, sha_of, sl_rank, ulps_apart)
from test_msf_golden_cpu import golden_csr as weighted_golden_csr
from test_traversal_golden_cpu import grid_edges

pytestmark = pytest.mark.gpu

HUGE = 2 ** 31 - 1
BIG = 2 ** 31 - 1
# LP_WAVE_ROW, LP_LDS_ROW: every row long / every row up to 4096 entries medium / the defaults / no medium rows
BINS = ((0, 0), (0, 4096), (64, 2048), (64, 0), (8, 32))


def upload(gpu, off, adj, w=None, flags=0, shard=None):
    if w is None:
        csr = gpu.HostCSR.from_arrays(off, adj)
    else:
        csr = gpu.HostCSR.from_arrays_weighted(off, adj, w)
    g = gpu.DeviceGraph.from_csr(csr, flags, shard=shard)
    if w is not None:
        g.set_weights(w)
    return g


def edge_graph(gpu, edges, n, weights=None):
    off, adj, w = csr_of(edges, n, weights)
    return upload(gpu, off, adj, w), off, adj, w


def same_mod(got, want):
    assert {k: got[k] for k in MOD_KEYS} == {k: want[k] for k in MOD_KEYS}
    assert ulps_apart(got["modularity"], want["modularity"]) <= 1, (got["modularity"], want["modularity"])


def check(g, off, adj, w=None, coloring=None, max_sweeps=0, want=None):
    """every output of one call against the restatement (under the colouring the device itself gives when none is passed); returns
    (label, info, stats, modularity)"""
    if want is None:
        want = lp_np(off, adj, w, g.coloring_jp()[0] if coloring is None else coloring, max_sweeps)
    label, info, st = g.label_propagation(weighted=w is not None, coloring=coloring, max_sweeps=max_sweeps, stats=True)
    assert np.array_equal(label, want[0]) and info == want[1], (info, want[1])
    assert st["probes"] == info["sweeps"] and st["units"] >= info["changes"] and st["launches"] >= 1
    none = g.label_propagation(weighted=w is not None, coloring=coloring, max_sweeps=max_sweeps, want_labels=False)
    assert none[0] is None and none[1] == info
    mod = g.modularity(label, weighted=w is not None)
    assert (mod["communities"], mod["largest"]) == (info["communities"], info["largest"])
    assert info["singletons"] == int((np.bincount(label, minlength=1) == 1).sum())
    if info["converged"]:
        assert mod["unstable"] == 0
    return label, info, st, mod


_GRAPHS = {}


def device_graph(gpu, kind, key):
    if (kind, key) not in _GRAPHS:
        off, adj, w = graph_arrays(gpu, kind, key)
        _GRAPHS[(kind, key)] = (upload(gpu, off, adj, w), off, adj, w)
    return _GRAPHS[(kind, key)]


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_label_propagation_equals_the_golden(gpu, rec):
    g, off, adj, w = device_graph(gpu, "w" if rec["weighted"] else "u", rec["graph"])
    _, _, _, color, want_label, want_info, _ = run(gpu, rec)
    if rec["coloring"] == "default":
        assert np.array_equal(g.coloring_jp()[0], color)
    label, info, st, mod = check(g, off, adj, w, None if rec["coloring"] == "default" else color, want=(want_label, want_info))
    assert info == {k: rec[k] for k in INFO_KEYS} and sha_of(label) == rec["sha256"]
    if off.size - 1 <= ARRAY_MAX_N:
        assert np.array_equal(label, ARR["label_" + rec_id(rec)])
    for got, key in ((mod, "mod"), (g.modularity(g.connected_components()[0], weighted=rec["weighted"]), "mod_cc")):
        same_mod(got, dict(rec[key], sumsq=int(rec[key]["sumsq"]), modularity=float.fromhex(rec[key]["modularity"])))
        assert got["sumsq_hi"] == got["sumsq"] >> 64 and got["sumsq_lo"] == got["sumsq"] & (2 ** 64 - 1)


# ---- 2. ties and the keep rule ----------------------------------------------------------------------------------------------------------
def test_ties(gpu):
    k64 = np.array([(a, b) for a in range(64) for b in range(a + 1, 64)])
    cycle = np.stack([np.arange(4096), (np.arange(4096) + 1) % 4096], axis=1)
    path = np.stack([np.arange(4095), np.arange(1, 4096)], axis=1)
    pairs = np.stack([2 * np.arange(512), 2 * np.arange(512) + 1], axis=1)
    for edges, n in ((k64, 64), (cycle, 4096), (grid_edges(64, 64), 4096), (path, 4096), (pairs, 1024), (np.array([[0, 1]]), 2)):
        g, off, adj, _ = edge_graph(gpu, edges, n)
        label, info, st, mod = check(g, off, adj)
        if n == 64:
            assert np.all(label == 0) and info["communities"] == 1 and info["colors"] == 64
        if n == 1024:
            assert info["communities"] == 512 and info["largest"] == 2
        g.free()


def test_own_label_is_kept_on_a_tie(gpu):
    g, off, adj, _ = edge_graph(gpu, [(0, 2), (2, 3)], 4)
    color = np.array([3, 1, 2, 1], dtype=np.int32)   # 3 takes 2; then 2 sees its own label and the smaller 0 once each
    label, info, st, mod = check(g, off, adj, coloring=color)
    assert label.tolist() == [2, 1, 2, 2] and lp_seq(off, adj, None, color)[0].tolist() == [2, 1, 2, 2] and info["singletons"] == 1
    g.free()


# ---- 3. row classes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1500, 40000])
def test_star(gpu, leaves):
    # the centre has the highest id: it is coloured and acts first, and sees `leaves` distinct labels once each
    centre = leaves
    g, off, adj, _ = edge_graph(gpu, np.stack([np.full(leaves, centre), np.arange(leaves)], axis=1), leaves + 1)
    color = g.coloring_jp()[0]
    assert color[centre] == 1 and np.all(color[:leaves] == 2)
    want = lp_np(off, adj, None, color)
    assert np.all(want[0] == 0) and want[1]["first_sweep_changes"] == leaves   # the centre takes 0, then every other leaf does
    base = check(g, off, adj, want=want)
    for wave_row, lds_row in BINS:
        with gpu.options(LP_WAVE_ROW=wave_row, LP_LDS_ROW=lds_row):
            assert check(g, off, adj, want=want)[1] == base[1]
    g.free()
    # the leaves pre-merged by a second hub that acts before them: the centre sees ONE label on every arc
    hub = leaves + 1
    edges = np.concatenate([np.stack([np.full(leaves, centre), np.arange(leaves)], axis=1), np.stack([np.full(leaves, hub), np.arange(leaves)], axis=1)])
    g, off, adj, _ = edge_graph(gpu, edges, leaves + 2)
    color = np.full(leaves + 2, 2, dtype=np.int32)
    color[hub], color[centre] = 1, 3
    want = lp_np(off, adj, None, color)
    assert np.all(want[0] == 0)
    for wave_row, lds_row in BINS[:3]:
        with gpu.options(LP_WAVE_ROW=wave_row, LP_LDS_ROW=lds_row):
            check(g, off, adj, coloring=color, want=want)
    g.free()


def bin_edge_graph(degrees, pool, seed):
    """centres of the given degrees (the highest ids: they act first) over a shared pool of leaves, seeded weights 1 … 5"""
    rng = np.random.RandomState(seed)
    edges = np.concatenate([np.stack([np.full(d, pool + i), rng.choice(pool, size=d, replace=False)], axis=1) for i, d in enumerate(degrees)])
    return edges, pool + len(degrees), rng.randint(1, 6, size=len(edges))


def test_rows_at_the_bin_edges(gpu):
    edges, n, wt = bin_edge_graph([1, 15, 16, 17, 63, 64, 65, 100, 2047, 2048, 2049, 4095, 4096, 4097], 6000, 5)
    g, off, adj, w = edge_graph(gpu, edges, n, wt)
    want_w, want_u = lp_np(off, adj, w, g.coloring_jp()[0]), lp_np(off, adj, None, g.coloring_jp()[0])
    for wave_row, lds_row in BINS + ((16, 64), (17, 65), (63, 2047)):
        with gpu.options(LP_WAVE_ROW=wave_row, LP_LDS_ROW=lds_row):
            check(g, off, adj, w, want=want_w)
            label, info = g.label_propagation()
            assert np.array_equal(label, want_u[0]) and info == want_u[1]
    g.free()


def test_small_lds_table(gpu):
    edges, n, wt = bin_edge_graph([62, 63, 64, 65, 66, 128], 400, 9)
    g, off, adj, w = edge_graph(gpu, edges, n, wt)
    want = lp_np(off, adj, w, g.coloring_jp()[0])
    assert want[1]["first_sweep_changes"] >= 6   # every centre saw its whole row as distinct labels
    for wave_row, lds_row in ((0, 64), (0, 63), (8, 64), (0, 4096)):
        with gpu.options(LP_LDS_SLOTS=64, LP_WAVE_ROW=wave_row, LP_LDS_ROW=lds_row):
            check(g, off, adj, w, want=want)
    g.free()


def test_kronecker_14_renumbered(gpu):
    off, adj, _ = graph_arrays(gpu, "u", "kronecker_14_16")
    n = off.size - 1
    perm = np.random.RandomState(2).permutation(n)
    row = np.repeat(np.arange(n), np.diff(off))
    up = row < adj
    g, off2, adj2, _ = edge_graph(gpu, np.stack([perm[row[up]], perm[adj[up]]], axis=1), n)
    assert adj2.size == adj.size
    want = lp_np(off2, adj2, None, g.coloring_jp()[0])
    check(g, off2, adj2, want=want)
    for wave_row, lds_row in BINS[:2]:
        with gpu.options(LP_WAVE_ROW=wave_row, LP_LDS_ROW=lds_row):
            check(g, off2, adj2, want=want)
    g.free()


# ---- 4. weights -------------------------------------------------------------------------------------------------------------------------
def test_weights(gpu):
    g, off, adj, w = edge_graph(gpu, [(0, 1), (0, 2), (0, 3), (0, 4), (2, 3), (3, 4)], 5, [7, 2, 2, 2, 9, 9])
    color = np.array([4, 2, 1, 2, 3], dtype=np.int32)
    label, info, st, mod = check(g, off, adj, w, coloring=color)
    assert label.tolist() == [0, 0, 3, 3, 3]   # vertex 0: 7 for its own label against 3 x 2 for label 3
    assert g.label_propagation(coloring=color)[0].tolist() == lp_seq(off, adj, None, color)[0].tolist() != label.tolist()
    g.free()
    # five arcs of 2^31 - 1 to one label against six arcs of 2^30 to another: the sums pass 2^32
    edges = [(11, i) for i in range(11)] + [(12, i) for i in range(5)] + [(13, i) for i in range(5, 11)]
    wts = [BIG] * 5 + [2 ** 30] * 6 + [BIG] * 5 + [2 ** 30] * 6   # (in 32-bit sums 5 (2^31 - 1) would lose against 6 x 2^30)
    g, off, adj, w = edge_graph(gpu, edges, 14, wts)
    color = np.array([2] * 11 + [3, 1, 1], dtype=np.int32)   # 12 and 13 merge their leaves first, then 11 chooses between the two labels
    label, info, st, mod = check(g, off, adj, w, coloring=color)
    assert label[11] == label[0] == 0 and label[5] == 5 and mod["intra_weight"] > 2 ** 33
    for wave_row, lds_row in BINS[:2]:
        with gpu.options(LP_WAVE_ROW=wave_row, LP_LDS_ROW=lds_row):
            assert check(g, off, adj, w, coloring=color)[1] == info
    g.free()


def test_unit_weights_equal_the_unweighted_call(gpu):
    g, off, adj, _ = device_graph(gpu, "u", "kronecker_12_16")
    h = upload(gpu, off, adj, np.ones(adj.size, dtype=np.int32))
    a, b = g.label_propagation(), h.label_propagation(weighted=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert g.modularity(a[0]) == h.modularity(a[0], weighted=True) == h.modularity(a[0])
    h.free()


# ---- 5. colourings ----------------------------------------------------------------------------------------------------------------------
def test_callers_colourings(gpu):
    g, off, adj, w = device_graph(gpu, "w", "kronecker_10_16")
    for rank in (lf_rank(off), sl_rank(off, adj)):
        color = g.coloring_jp(rank)[0]
        check(g, off, adj, w, coloring=color)
        check(g, off, adj, None, coloring=color)
    L = gpu.lib()
    n = off.size - 1
    good = g.coloring_jp()[0]
    label = np.full(n, 77, dtype=np.int32)
    info = gpu.LpInfo()
    info.communities = 77
    improper = good.copy()
    v = int(np.argmax(np.diff(off)))
    improper[int(adj[off[v]])] = good[v]   # an edge with equal colours at its ends
    zero = good.copy()
    zero[3] = 0
    above = good.copy()
    above[3] = n + 1
    for bad in (improper, zero, above):
        rc = L.gmsx_label_propagation(g._h, 0, bad.ctypes.data_as(C.c_void_p), 0, label.ctypes.data_as(C.c_void_p), C.byref(info), None)
        assert rc == gpu.ERR_INVALID and np.all(label == 77) and info.communities == 77


# ---- 6. sweep cap -----------------------------------------------------------------------------------------------------------------------
def test_sweep_cap(gpu):
    g, off, adj, w = device_graph(gpu, "w", "kronecker_12_16")
    color = g.coloring_jp()[0]
    for cap in (1, 2):
        for ww in (None, w):
            label, info, st, mod = check(g, off, adj, ww, max_sweeps=cap, want=lp_np(off, adj, ww, color, cap))
            assert info["sweeps"] == cap and info["converged"] == 0 and mod["unstable"] > 0


# ---- 7. scheduling ----------------------------------------------------------------------------------------------------------------------
def test_scheduling_leaves_the_bytes_alone(gpu):
    for kind, key in (("w", "kronecker_12_16"), ("u", "kronecker_10_16_plain"), ("w", "file_two_parts_a")):
        g, off, adj, w = device_graph(gpu, kind, key)
        first = g.label_propagation(weighted=w is not None, stats=True)
        launches = {}
        for wg_work in (0, None, HUGE):
            for active in (0, 1):
                opts = {"LP_ACTIVE": active}
                if wg_work is not None:
                    opts["LP_WG_WORK"] = wg_work
                with gpu.options(**opts):
                    label, info, st = g.label_propagation(weighted=w is not None, stats=True)
                assert label.tobytes() == first[0].tobytes() and info == first[1]
                launches[(wg_work, active)] = st["launches"]
                if active == 0:
                    assert st["units"] == info["sweeps"] * int((np.diff(off) > 0).sum())   # every row in every sweep
                else:
                    assert st["units"] <= info["sweeps"] * int((np.diff(off) > 0).sum())
        assert launches[(HUGE, 0)] <= launches[(None, 0)] <= launches[(0, 0)] and launches[(0, 1)] <= launches[(0, 0)]


# ---- 8. same bytes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_same_bytes(gpu, weighted):
    csr = weighted_golden_csr(gpu, "kronecker_12_16")
    off, adj, w = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32), np.array(csr.weights(), dtype=np.int32)
    rec = next(r for r in J["records"] if r["weighted"] and r["graph"] == "kronecker_12_16" and r["coloring"] == "default")
    base = upload(gpu, off, adj, w)
    first = base.label_propagation(weighted=weighted)
    fmod = base.modularity(first[0], weighted=weighted)
    if weighted:
        assert sha_of(first[0]) == rec["sha256"]

    def same(g):
        r = g.label_propagation(weighted=weighted)
        assert r[0].tobytes() == first[0].tobytes() and r[1] == first[1]
        assert g.modularity(r[0], weighted=weighted) == fmod

    for _ in range(2):
        same(base)
    base.set_weights(w)   # re-attached
    same(base)
    base.set_weights(None)
    base.set_weights(w)   # detached and attached again
    same(base)
    for flags, shard in ((gpu.UPLOAD_TRUSTED, None), (64 << 8, None), (0, (1, 2)), (0, None)):
        g = gpu.DeviceGraph.from_csr(csr, flags, shard=shard)
        g.set_weights(w)
        same(g)
        g.free()
    base.free()


# ---- 9. modularity ----------------------------------------------------------------------------------------------------------------------
def test_modularity_closed_forms(gpu):
    g, off, adj, w = device_graph(gpu, "w", "kronecker_10_16")
    n = off.size - 1
    for ww in (None, w):
        total = int(adj.size if ww is None else ww.astype(np.int64).sum())
        one = g.modularity(np.zeros(n, dtype=np.int32), weighted=ww is not None)
        assert (one["total_weight"], one["intra_weight"], one["sumsq"], one["communities"], one["largest"]) == (total, total, total * total, 1, n)
        assert one["modularity"] == 0.0 and one["unstable"] == 0
        each = g.modularity(np.arange(n, dtype=np.int32), weighted=ww is not None)
        assert (each["total_weight"], each["intra_weight"], each["communities"], each["largest"]) == (total, 0, n, 1)
        same_mod(each, mod_np(off, adj, ww, np.arange(n)))
        assert each["unstable"] == int((np.diff(off) > 0).sum())
    k8 = [(i, j) for i in range(8) for j in range(i)]
    h, off, adj, _ = edge_graph(gpu, k8 + [(8 + i, 8 + j) for i, j in k8] + [(0, 8)], 16)
    m = h.modularity(np.repeat([0, 8], 8).astype(np.int32))
    assert (m["total_weight"], m["intra_weight"], m["sumsq"], m["unstable"], m["communities"], m["largest"]) == (114, 112, 2 * 57 * 57, 0, 2, 8)
    assert abs(m["modularity"] - (112 / 114 - 0.5)) < 1e-15
    h.free()
    h, off, adj, w = edge_graph(gpu, [(8, i) for i in range(8)], 9, [BIG] * 8)   # a weighted star: S passes 2^64
    m = h.modularity(np.zeros(9, dtype=np.int32), weighted=True)
    assert m["total_weight"] == 16 * BIG and m["sumsq"] == (16 * BIG) ** 2 > 2 ** 64 and m["sumsq_hi"] > 0 and m["modularity"] == 0.0
    same_mod(h.modularity(np.array([0, 0, 0, 0, 1, 1, 1, 1, 0], dtype=np.int32), weighted=True),
             mod_np(off, adj, w, np.array([0, 0, 0, 0, 1, 1, 1, 1, 0])))
    h.free()


def test_unstable_counts_on_other_clusterings(gpu):
    for kind, key in (("w", "kronecker_12_16"), ("u", "kronecker_10_16")):
        g, off, adj, w = device_graph(gpu, kind, key)
        jp = g.jarvis_patrick("jaccard", 0.05)[0]
        cc = g.connected_components()[0]
        assert np.array_equal(cc, cc_labels_np(off, adj))
        for label in (jp, cc):
            for ww in (None, w) if w is not None else (None,):
                got, want = g.modularity(label, weighted=ww is not None), mod_np(off, adj, ww, label)
                same_mod(got, want)
        assert g.modularity(cc)["unstable"] == 0 and g.modularity(jp)["unstable"] > 0


# ---- 10. consistency --------------------------------------------------------------------------------------------------------------------
def test_communities_lie_inside_components(gpu):
    for kind, key in (("u", "kronecker_12_16"), ("w", "file_two_parts_a"), ("u", "file_triangles_3")):
        g, off, adj, w = device_graph(gpu, kind, key)
        label, info = g.label_propagation(weighted=w is not None)
        cc, cinfo = g.connected_components()
        assert np.array_equal(cc[label], cc) and info["communities"] >= cinfo["components"]
        isolated = np.flatnonzero(np.diff(off) == 0)
        assert np.array_equal(label[isolated], isolated) and info["singletons"] >= isolated.size
        m = g.modularity(label, weighted=w is not None)
        assert (m["communities"], m["largest"], m["unstable"]) == (info["communities"], info["largest"], 0)


# ---- 11. contract -----------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    off, adj, w = graph_arrays(gpu, "w", "file_two_parts_b")
    n = off.size - 1
    g = upload(gpu, off, adj)   # no weights attached
    L = gpu.lib()
    info, minfo = gpu.LpInfo(), gpu.ModularityInfo()
    info.communities = minfo.communities = 77
    label = np.full(n, 77, dtype=np.int32)
    pl = label.ctypes.data_as(C.c_void_p)
    ok = np.zeros(n, dtype=np.int32)
    po = ok.ctypes.data_as(C.c_void_p)

    def untouched():
        return bool(np.all(label == 77) and info.communities == 77 and minfo.communities == 77)

    assert L.gmsx_label_propagation(g._h, 1, None, 0, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()   # WEIGHTED without weights
    assert L.gmsx_modularity(g._h, 1, po, C.byref(minfo), None) == gpu.ERR_INVALID and untouched()
    g.set_weights(w)
    before = g.device_bytes
    for flags in (2, 4, 1 << 31, 3):
        assert L.gmsx_label_propagation(g._h, flags, None, 0, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()
        assert L.gmsx_modularity(g._h, flags, po, C.byref(minfo), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_label_propagation(g._h, 0, None, -1, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_label_propagation(g._h, 0, None, 0, pl, None, None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_label_propagation(None, 0, None, 0, pl, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_modularity(g._h, 0, po, None, None) == gpu.ERR_INVALID and L.gmsx_modularity(None, 0, po, C.byref(minfo), None) == gpu.ERR_INVALID
    assert L.gmsx_modularity(g._h, 0, None, C.byref(minfo), None) == gpu.ERR_INVALID and untouched()
    for bad in (-1, n, 2 ** 31 - 1):
        out = ok.copy()
        out[n // 2] = bad
        assert L.gmsx_modularity(g._h, 0, out.ctypes.data_as(C.c_void_p), C.byref(minfo), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_label_propagation(g._h, 1, None, 0, pl, C.byref(info), None) == gpu.OK and not untouched()
    assert g.device_bytes == before
    check(g, off, adj, w)
    check(g, off, adj, None)
    assert g.device_bytes == before
    # the call changes no other entry point's answer
    h = upload(gpu, off, adj, w)
    assert g.sssp(9)[0].tobytes() == h.sssp(9)[0].tobytes() and g.coloring_jp()[0].tobytes() == h.coloring_jp()[0].tobytes()
    h.free()
    g.free()


def test_tiny_and_edgeless(gpu):
    one = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # n = 1
    label, info = one.label_propagation()
    assert label.tolist() == [0] and info == {"communities": 1, "largest": 1, "singletons": 1, "changes": 0, "first_sweep_changes": 0, "sweeps": 1,
                                              "colors": 1, "converged": 1, "largest_label": 0}
    m = one.modularity(label)
    assert (m["total_weight"], m["intra_weight"], m["sumsq"], m["communities"], m["largest"], m["unstable"], m["modularity"]) == (0, 0, 0, 1, 1, 0, 0.0)
    one.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # edgeless, n = 5
    g.set_weights(np.zeros(0, dtype=np.int32))
    for weighted in (False, True):
        label, info = g.label_propagation(weighted=weighted)
        assert label.tolist() == [0, 1, 2, 3, 4] and (info["communities"], info["singletons"], info["sweeps"], info["converged"]) == (5, 5, 1, 1)
        m = g.modularity(label, weighted=weighted)
        assert m["modularity"] == 0.0 and m["communities"] == 5 and m["total_weight"] == 0
    label, info = g.label_propagation(coloring=np.array([1, 2, 3, 1, 1], dtype=np.int32))
    assert label.tolist() == [0, 1, 2, 3, 4] and info["colors"] == 3
    g.free()
