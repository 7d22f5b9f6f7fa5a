"""GPU: gmsx_connected_components and gmsx_jarvis_patrick through the C-ABI, bit for bit against the goldens (tests/golden/components.{json,npz}:
the reference's ShiloachVishkin labels; the Jarvis–Patrick records of the restatement) and against components_np / jarvis_patrick_np of
tests/test_components_golden_cpu.py:

  goldens     every component record (literal labels or sha256, info), every Jarvis–Patrick record
  degenerate  no vertex, five isolated vertices, one edge, one vertex
  depth       a path on 4096 vertices numbered along it, in reverse and at random: one component, label 0, no cap tripped
  width       a star with 70 000 leaves; rows of degree 1, 15, 16, 17, 63, 64, 65 and CC_WAVE_ROW, CC_WG_ROW -1 / +0 / +1 at the default bins and at 4 / 8
  many        a perfect matching on 2^16 vertices plus 1000 isolated ones: exact labels
  the skip    kronecker 12 and one large component plus 500 triangles at CC_SAMPLE 0, 1, 2, 64: the same bytes
  masks       symmetric, u < v only, u > v only: the same labels and kept_edges; zeros: n singletons; ones: the NULL call; truss >= k isolates the
              planted clique of the truss tests
  clustering  two K8 and a bridge under common neighbours at 0, 1, 7; the mask fed back; the kept set equals the thresholded
              gmsx_vertex_similarity_batch scores for all seven metrics; a NaN threshold is refused
  same bytes  three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload
  contract    NULL arguments, unknown metric; untouched arrays on error; the options are enumerated"""
import ctypes as C

import numpy as np
import pytest

from conftest import edges_to_csr, host_graph
from test_components_golden_cpu import (ARR, BIN_DEGREES, CC, CC_WAVE_ROW, CC_WG_ROW, INFO_KEYS, JP, METRIC_IDS, bins_graph, components_np,
                                        giant_plus_triangles, golden_csr, jarvis_patrick_np, jp_id, matching_edges, path_edges, sha, sources,
                                        star_edges, two_k8_and_a_bridge)
from test_truss_golden_cpu import planted

pytestmark = pytest.mark.gpu


def facts(info):
    """info without the diagnostic"""
    return {k: info[k] for k in INFO_KEYS}


def check(g, off, adj, arc_keep=None):
    """labels and info of one call against components_np; returns (label, info)"""
    label, info, st = g.connected_components(arc_keep, stats=True)
    want, want_info = components_np(off, adj, arc_keep)
    assert np.array_equal(label, want) and facts(info) == want_info
    assert info["passes"] >= 1 and st["launches"] >= 3
    return label, info


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(CC))
def test_components_equal_the_reference(gpu, key):
    rec, csr = CC[key], golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    label, info, st = g.connected_components(stats=True)
    assert sha(label) == rec["label_sha256"]
    if rec["literal"]:
        assert np.array_equal(label, ARR["label_" + key])
    assert facts(info) == dict({k: rec[k] for k in INFO_KEYS if k != "kept_edges"}, kept_edges=rec["nnz"] // 2)
    assert 0 < st["units"] <= rec["nnz"] or rec["nnz"] == 0
    only_info = g.connected_components()[1]
    assert facts(only_info) == facts(info)
    g.free()


_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        _GRAPHS[key] = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    return _GRAPHS[key]


@pytest.mark.parametrize("rec", JP, ids=jp_id)
def test_jarvis_patrick_equals_the_golden(gpu, rec):
    g = device_graph(gpu, rec["graph"])
    label, info, mask, st = g.jarvis_patrick(rec["metric"], float.fromhex(rec["threshold"]), want_mask=True, stats=True)
    assert facts(info) == {k: rec[k] for k in INFO_KEYS} and sha(label) == rec["label_sha256"]
    if rec["literal"]:
        assert np.array_equal(label, ARR[rec["array"]])
    assert int(mask.sum()) == 2 * rec["kept_edges"] and set(np.unique(mask).tolist()) <= {0, 1}
    assert st["units"] == CC[rec["graph"]]["nnz"] // 2 and st["alg_elements"] == golden_csr(gpu, rec["graph"]).merge_elements()


# ---- 2. degenerate graphs ---------------------------------------------------------------------------------------------------------------
def test_degenerate_graphs(gpu):
    zero = dict.fromkeys(INFO_KEYS, 0)
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    label, info = g.connected_components()
    assert label.size == 0 and facts(info) == zero and info["passes"] == 0
    label, info = g.jarvis_patrick("common_neighbors", 1)
    assert label.size == 0 and facts(info) == zero
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=5))
    for label, info in (g.connected_components(), g.jarvis_patrick("jaccard", 0.1)[:2], g.connected_components(np.zeros(0, dtype=np.uint8))):
        assert label.tolist() == [0, 1, 2, 3, 4] and facts(info) == {"components": 5, "singletons": 5, "largest": 1, "largest_label": 0, "kept_edges": 0}
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [(0, 1)], n=2))
    label, info = g.connected_components()
    assert label.tolist() == [0, 0] and facts(info) == {"components": 1, "singletons": 0, "largest": 2, "largest_label": 0, "kept_edges": 1}
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=1))
    label, info = g.connected_components()
    assert label.tolist() == [0] and facts(info) == {"components": 1, "singletons": 1, "largest": 1, "largest_label": 0, "kept_edges": 0}


# ---- 3. depth ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["along", "reverse", "random"])
@pytest.mark.parametrize("sample", [0, 2])
def test_path(gpu, numbering, sample):
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, path_edges(4096, numbering), n=4096))
    with gpu.options(CC_SAMPLE=sample):
        label, info = g.connected_components()   # (a tripped cap raises GmsxError(GMSX_ERR_KERNEL))
    assert not label.any() and facts(info) == {"components": 1, "singletons": 0, "largest": 4096, "largest_label": 0, "kept_edges": 4095}
    label, info, mask = g.jarvis_patrick("common_neighbors", 0, want_mask=True)   # the same chain through the clustering kernel
    assert not label.any() and info["components"] == 1 and mask.all()
    g.free()


# ---- 4. width ---------------------------------------------------------------------------------------------------------------------------
def test_star_of_70000_leaves(gpu):
    csr = edges_to_csr(gpu, star_edges(70000), n=70001)
    g = gpu.DeviceGraph.from_csr(csr)
    for sample in (0, 2):
        with gpu.options(CC_SAMPLE=sample):
            label, info = check(g, csr.offsets(), csr.neighbors())
        assert not label.any() and info["largest"] == 70001
    mask = np.ones(140000, dtype=np.uint8)
    mask[:70000] = 0   # the hub's row off: every edge is visible from its leaf only
    label, info = check(g, csr.offsets(), csr.neighbors(), mask)
    assert not label.any() and info["kept_edges"] == 70000
    g.free()


@pytest.mark.parametrize("bins", [None, (4, 8)])
def test_every_row_bin(gpu, bins):
    e, n = bins_graph(BIN_DEGREES)
    csr = edges_to_csr(gpu, e, n=n)
    off, adj = csr.offsets(), csr.neighbors()
    assert np.diff(off)[:len(BIN_DEGREES)].tolist() == BIN_DEGREES
    g = gpu.DeviceGraph.from_csr(csr)
    opts = {} if bins is None else {"CC_WAVE_ROW": bins[0], "CC_WG_ROW": bins[1]}
    for sample in (0, 2, 20):
        with gpu.options(CC_SAMPLE=sample, **opts):
            label, info = check(g, off, adj)
            src = sources(off)
            check(g, off, adj, (src < adj).astype(np.uint8))   # the hubs' rows only: the masked source in every bin
        assert info["components"] == len(BIN_DEGREES) and info["largest"] == CC_WG_ROW + 2 and info["largest_label"] == len(BIN_DEGREES) - 1
    g.free()


# ---- 5. many components -------------------------------------------------------------------------------------------------------------------
def test_perfect_matching_and_isolated_vertices(gpu):
    e = matching_edges(1 << 15)
    csr = edges_to_csr(gpu, e, n=(1 << 16) + 1000)
    g = gpu.DeviceGraph.from_csr(csr)
    label, info = check(g, csr.offsets(), csr.neighbors())
    assert facts(info) == {"components": 32768 + 1000, "singletons": 1000, "largest": 2, "largest_label": 0, "kept_edges": 32768}
    assert np.array_equal(label[e[:, 0]], e.min(axis=1)) and np.array_equal(label[e[:, 1]], e.min(axis=1))
    assert np.array_equal(label[1 << 16:], np.arange(1 << 16, (1 << 16) + 1000))
    assert len(gpu.clusters(label)) == info["components"]
    g.free()


# ---- 6. the skip --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["kronecker 12", "giant plus 500 triangles"])
def test_sampling_changes_no_byte(gpu, which):
    if which == "kronecker 12":
        csr = host_graph(gpu, "kronecker", 12)
    else:
        e, n = giant_plus_triangles()
        csr = edges_to_csr(gpu, e, n=n)
    off, adj = csr.offsets(), csr.neighbors()
    want, want_info = components_np(off, adj)
    if which != "kronecker 12":
        assert want_info["components"] == 501 and want_info["largest"] == 3000
    g = gpu.DeviceGraph.from_csr(csr)
    units = {}
    for sample in (0, 1, 2, 64):
        with gpu.options(CC_SAMPLE=sample):
            label, info, st = g.connected_components(stats=True)
        assert np.array_equal(label, want) and facts(info) == want_info, sample   # a wrong skip loses exactly the small components' edges
        units[sample] = st["units"]
    assert units[0] == adj.size and units[2] < units[0]   # the skip did skip
    g.free()


# ---- 7. masks -----------------------------------------------------------------------------------------------------------------------------
def test_masks(gpu):
    csr = host_graph(gpu, "kronecker", 10)
    off, adj = csr.offsets(), csr.neighbors()
    src = sources(off)
    g = gpu.DeviceGraph.from_csr(csr)
    lo, hi = np.minimum(src, adj), np.maximum(src, adj)
    sym = ((((lo * 2654435761 + hi * 40503) >> 7) % 10) < 4).astype(np.uint8)   # a function of the edge: symmetric
    label, info = check(g, off, adj, sym)
    assert 0 < info["kept_edges"] < adj.size // 2 and info["components"] > components_np(off, adj)[1]["components"]
    for side in (src < adj, src > adj):
        l2, i2 = check(g, off, adj, sym * side)
        assert np.array_equal(l2, label) and facts(i2) == facts(info)
    l3, i3 = check(g, off, adj, sym * 255)   # any non-zero byte keeps
    assert np.array_equal(l3, label) and facts(i3) == facts(info)
    label, info = g.connected_components(np.zeros(adj.size, dtype=np.uint8))
    n = off.size - 1
    assert np.array_equal(label, np.arange(n)) and facts(info) == {"components": n, "singletons": n, "largest": 1, "largest_label": 0, "kept_edges": 0}
    ones, null = g.connected_components(np.ones(adj.size, dtype=np.uint8)), g.connected_components()
    assert np.array_equal(ones[0], null[0]) and facts(ones[1]) == facts(null[1])
    with pytest.raises(gpu.GmsxError) as ei:
        g.connected_components(np.ones(adj.size - 1, dtype=np.uint8))
    assert ei.value.status == gpu.ERR_INVALID
    g.free()


def test_truss_mask_isolates_the_planted_clique(gpu):
    csr = edges_to_csr(gpu, planted(), n=300)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    truss, tinfo = g.truss_decomposition()
    assert tinfo["max_truss"] == 14 and tinfo["top_edges"] == 91
    label, info = check(g, off, adj, (truss >= 14).astype(np.uint8))
    assert facts(info) == dict(components=300 - 14 + 1, singletons=300 - 14, largest=14, kept_edges=91, largest_label=info["largest_label"])
    members = np.flatnonzero(label == info["largest_label"])
    src = sources(off)
    assert members.size == 14 and set(members.tolist()) == set(src[truss >= 14].tolist()) and members[0] == info["largest_label"]
    g.free()


# ---- 8. Jarvis–Patrick --------------------------------------------------------------------------------------------------------------------
def test_two_k8_and_a_bridge(gpu):
    e, n = two_k8_and_a_bridge()
    csr = edges_to_csr(gpu, e, n=n)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    label, info, mask = g.jarvis_patrick("common_neighbors", 1, want_mask=True)
    assert label.tolist() == [0] * 8 + [8] * 8 and facts(info) == {"components": 2, "singletons": 0, "largest": 8, "largest_label": 0, "kept_edges": 56}
    src = sources(off)
    assert mask.sum() == 112 and not mask[(np.minimum(src, adj) == 7) & (np.maximum(src, adj) == 8)].any()
    l2, i2 = g.connected_components(mask)   # the mask fed back
    assert np.array_equal(l2, label) and facts(i2) == facts(info)
    assert facts(g.jarvis_patrick("common_neighbors", 0)[1]) == {"components": 1, "singletons": 0, "largest": 16, "largest_label": 0, "kept_edges": 57}
    label, info, mask = g.jarvis_patrick("common_neighbors", 7, want_mask=True)
    assert facts(info) == {"components": 16, "singletons": 16, "largest": 1, "largest_label": 0, "kept_edges": 0} and not mask.any()
    assert label.tolist() == list(range(16))
    with pytest.raises(gpu.GmsxError) as ei:
        g.jarvis_patrick("common_neighbors", float("nan"))
    assert ei.value.status == gpu.ERR_INVALID
    g.free()


@pytest.mark.parametrize("metric", sorted(METRIC_IDS))
def test_kept_set_is_the_thresholded_device_score(gpu, metric):
    csr = host_graph(gpu, "kronecker", 10)
    off, adj = csr.offsets(), csr.neighbors()
    src = sources(off)
    up = src < adj
    eu, ev = src[up].astype(np.int32), adj[up].astype(np.int32)
    g = device_graph(gpu, "kronecker_10_16")
    score = g.vertex_similarity_batch(metric, eu, ev)
    assert not np.isnan(score).any()
    for q in (0.3, 0.7):   # thresholds that ARE scores: ">=" is tested on equality, bit for bit
        thr = float(np.sort(score)[int(q * score.size)])
        keep = score >= thr
        assert 0 < keep.sum()
        label, info, mask = g.jarvis_patrick(metric, thr, want_mask=True)
        want_label, want_info, want_mask = jarvis_patrick_np(off, adj, metric, thr, (eu.astype(np.int64), ev.astype(np.int64), score))
        assert np.array_equal(mask, want_mask), (metric, q)
        assert np.array_equal(label, want_label) and facts(info) == want_info
        l2, i2 = g.connected_components(mask)
        assert np.array_equal(l2, label) and facts(i2) == facts(info)
        assert np.array_equal(g.jarvis_patrick(METRIC_IDS[metric], thr)[0], label)   # the metric by number, no mask asked for


# ---- 9. same bytes ------------------------------------------------------------------------------------------------------------------------
def test_same_bytes_in_every_variant(gpu):
    csr = host_graph(gpu, "kronecker", 12)
    rec = CC["kronecker_12_16"]
    g = gpu.DeviceGraph.from_csr(csr)
    variants = [("run 1", g), ("run 2", g), ("run 3", g), ("trusted", gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_TRUSTED)),
                ("hub limit 64", gpu.DeviceGraph.from_csr(csr, flags=64 << 8)), ("shard 1 of 4", gpu.DeviceGraph.from_csr(csr, shard=(1, 4)))]
    first = None
    for name, h in variants:
        label, info = h.connected_components()
        jl, ji, jm = h.jarvis_patrick("common_neighbors", 5, want_mask=True)
        got = (label.tobytes(), facts(info), jl.tobytes(), facts(ji), jm.tobytes())
        first = first or got
        assert got == first, name
        assert sha(label) == rec["label_sha256"]
        if h is not g:
            h.free()
    g.free()


# ---- 10. contract -------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    L = gpu.lib()
    csr = host_graph(gpu, "kronecker", 10)
    g = gpu.DeviceGraph.from_csr(csr)
    n, nnz = csr.num_nodes, csr.nnz
    label, mask = np.full(n, -77, dtype=np.int32), np.full(nnz, 0x5a, dtype=np.uint8)
    info = gpu.ComponentsInfo()
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    before = bytes(info)
    lp, mp = label.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)
    assert L.gmsx_connected_components(None, None, lp, C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_connected_components(g._h, None, lp, None, None) == gpu.ERR_INVALID
    assert L.gmsx_jarvis_patrick(None, 4, 1.0, lp, mp, C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_jarvis_patrick(g._h, 4, 1.0, lp, mp, None, None) == gpu.ERR_INVALID
    for bad in (-1, 7, 100):
        assert L.gmsx_jarvis_patrick(g._h, bad, 1.0, lp, mp, C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_jarvis_patrick(g._h, 4, float("nan"), lp, mp, C.byref(info), None) == gpu.ERR_INVALID
    assert np.all(label == -77) and np.all(mask == 0x5a) and bytes(info) == before
    # NULL label and NULL stats are allowed: info alone
    assert L.gmsx_connected_components(g._h, None, None, C.byref(info), None) == 0 and info.components == CC["kronecker_10_16"]["components"]
    assert L.gmsx_jarvis_patrick(g._h, 4, 2.0, None, None, C.byref(info), None) == 0 and info.kept_edges > 0
    names = gpu.option_names()
    assert {"CC_SAMPLE", "CC_WAVE_ROW", "CC_WG_ROW"} <= set(names)
    assert L.gmsx_version() == 320
    g.free()
