"""GPU: gmsx_bfs and gmsx_betweenness through the C-ABI against the goldens (tests/golden/traversal.{json,npz}) and against bfs_np /
betweenness_np / betweenness_exact of tests/test_traversal_golden_cpu.py:

  goldens     every BFS record (sha256, literal arrays, info, bottom_up_levels at the defaults) and every BC record within the derived bound
  degenerate  n = 0 refuses every source; one vertex; an isolated source; one edge
  depth       a path on 4096 vertices numbered along it, in reverse and at random, from an end and from the middle, at BFS_WG_FRONTIER 512 and 0
  width       a star with 70 000 leaves from the hub and from a leaf; rows of degree 1 … 1025 with the frontier neighbour first, last and just past
              the probe window, at BFS_BU_PROBE 15 / 16 / 17 and 3 / 4 / 5, in every direction
  direction   kronecker 12 and 16 from vertex 0 and from a picked source: BFS_DIRECTION 0 / 1 / 2 and alpha = beta = 1 / 1 000 000 give the same
              bytes, and bottom_up_levels is the replay's
  components  the reached set is the source's component of gmsx_connected_components
  counts      a 40 x 40 grid from a corner: path counts beyond 2^64, every score finite and within the bound of inexact counts
  long rows   betweenness of the star with 70 000 leaves (a parked row of 18 chunks: the slot map and the slot-order sum) from the hub, from a leaf
              and from both, against its closed form, exactly, in every direction and run; kronecker 16 (rows of three chunks) is among the goldens
  many levels betweenness of the path on 4096 vertices from an end and from the middle (more levels than the scan's workgroup has threads): n - 1 - i
  flags       the source's own term, NORMALIZE_MAX, an edgeless graph, a source listed twice, no source
  same bytes  three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, every BFS_DIRECTION
  contract    NULL arguments, ids out of range, unknown flag bits; untouched arrays on error; the options are enumerated and documented"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT, edges_to_csr, host_graph
from test_traversal_golden_cpu import (ARR, BC, BFS, GRAPHS, INFO_KEYS, PROBE_DEGREES, bc_bound, bc_bound_inexact, bc_id, bc_sources, betweenness_exact,
                                       betweenness_np, bfs_id, bfs_np, golden_csr, grid_edges, path_edges, probe_graph, sha, star_edges)

pytestmark = pytest.mark.gpu

ALL_KEYS = INFO_KEYS + ("bottom_up_levels",)


def facts(info):
    """info without bottom_up_levels, which the options may change"""
    return {k: info[k] for k in INFO_KEYS}


def check(g, off, adj, source, **replay):
    """depth, parent and info of one call against bfs_np (the replay under the options in force); returns them"""
    depth, parent, info, st = g.bfs(source, stats=True)
    wd, wp, wi = bfs_np(off, adj, source, **replay)
    assert np.array_equal(depth, wd) and np.array_equal(parent, wp) and info == wi, (source, replay, info, wi)
    assert st["units"] == wi["reached_arcs"] and st["probes"] == wi["levels"] and st["launches"] >= 3
    return depth, parent, info


_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        _GRAPHS[key] = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    return _GRAPHS[key]


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", BFS, ids=bfs_id)
def test_bfs_equals_the_golden(gpu, rec):
    g = device_graph(gpu, rec["graph"])
    depth, parent, info, st = g.bfs(rec["source"], stats=True)
    assert info == {k: rec[k] for k in ALL_KEYS}
    assert sha(depth) == rec["depth_sha256"] and sha(parent) == rec["parent_sha256"]
    if rec["literal"]:
        assert np.array_equal(depth, ARR["depth_%s_%d" % (rec["graph"], rec["source"])])
    if rec["literal_parent"]:
        assert np.array_equal(parent, ARR["parent_%s_%d" % (rec["graph"], rec["source"])])
    assert st["units"] == rec["reached_arcs"] and st["probes"] == rec["levels"]
    none_d, none_p, only_info = g.bfs(rec["source"], want_depth=False, want_parent=False)
    assert none_d is None and none_p is None and only_info == info


@pytest.mark.parametrize("rec", BC, ids=bc_id)
def test_betweenness_equals_the_golden(gpu, rec):
    g = device_graph(gpu, rec["graph"])
    srcs = bc_sources(rec)
    got, info, st = g.betweenness(srcs, exclude_source=rec["exclude_source"], normalize=rec["normalize"], stats=True)
    want = ARR[rec["array"]]
    bound = bc_bound(want, rec["max_levels"], GRAPHS[rec["graph"]]["max_degree"], len(srcs))
    worst = float(np.max(np.abs(got - want) - bound))
    print(f"{bc_id(rec)}: largest |got - want| - bound = {worst:.3e}, largest relative error {float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))):.3e}")
    assert np.all(np.abs(got - want) <= bound)
    assert info["sources"] == len(srcs) and info["max_levels"] == rec["max_levels"] and info["max_sigma"] == float(int(rec["max_sigma"]))
    assert st["probes"] >= rec["max_levels"]


# ---- 2. degenerate graphs ---------------------------------------------------------------------------------------------------------------
def test_degenerate_graphs(gpu):
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    for s in (0, -1, 1):
        with pytest.raises(gpu.GmsxError) as ei:
            g.bfs(s)
        assert ei.value.status == gpu.ERR_INVALID
    scores, info = g.betweenness([])
    assert scores.size == 0 and info["sources"] == 0
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=1))
    depth, parent, info = g.bfs(0)
    assert depth.tolist() == [0] and parent.tolist() == [0]
    assert info == {"reached": 1, "reached_arcs": 0, "depth_sum": 0, "widest": 1, "levels": 1, "widest_level": 0, "bottom_up_levels": 0}
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [(1, 2)], n=5))   # an isolated source
    depth, parent, info = g.bfs(3)
    assert depth.tolist() == [-1, -1, -1, 0, -1] and parent.tolist() == [-1, -1, -1, 3, -1] and info["reached"] == 1 and info["levels"] == 1
    scores, bi = g.betweenness([3])
    assert not scores.any() and bi["reached_total"] == 1 and bi["max_levels"] == 1
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [(0, 1)], n=2))
    depth, parent, info = g.bfs(1)
    assert depth.tolist() == [1, 0] and parent.tolist() == [1, 1]
    assert facts(info) == {"reached": 2, "reached_arcs": 2, "depth_sum": 1, "widest": 1, "levels": 2, "widest_level": 0}
    assert g.betweenness([0, 1])[0].tolist() == [1.0, 1.0] and not g.betweenness([0, 1], exclude_source=True)[0].any()


# ---- 3. depth ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["along", "reverse", "random"])
@pytest.mark.parametrize("wg_frontier", [512, 0])
def test_path(gpu, numbering, wg_frontier):
    e = path_edges(4096, numbering)
    csr = edges_to_csr(gpu, e, n=4096)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    with gpu.options(BFS_WG_FRONTIER=wg_frontier):
        for source, levels in ((int(e[0, 0]), 4096), (int(e[2046, 1]), 2049)):   # an end, the middle
            info = check(g, off, adj, source)[2]
            assert info["levels"] == levels and info["widest"] == (1 if levels == 4096 else 2)
    g.free()


# ---- 4. width ---------------------------------------------------------------------------------------------------------------------------
def test_star_of_70000_leaves(gpu):
    csr = edges_to_csr(gpu, star_edges(70000), n=70001)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    for direction in (0, 1, 2):   # (1: the hub's row is above kWgRowMax — the tail hands the round back to the grid-wide kernels)
        with gpu.options(BFS_DIRECTION=direction):
            depth, parent, info = check(g, off, adj, 0, direction=direction)
            assert info["levels"] == 2 and info["widest"] == 70000
            depth, parent, info = check(g, off, adj, 5, direction=direction)
            assert info["levels"] == 3 and depth[0] == 1 and parent[0] == 5 and np.all(parent[1:5] == 0)
    g.free()


@pytest.mark.parametrize("where", ["first", "last", "past"])
@pytest.mark.parametrize("base", [16, 4])
def test_every_row_bin_of_the_bottom_up_step(gpu, where, base):
    e, n, hubs = probe_graph(where, base)
    csr = edges_to_csr(gpu, e, n=n)
    off, adj = csr.offsets(), csr.neighbors()
    assert np.diff(off)[hubs].tolist() == PROBE_DEGREES
    g = gpu.DeviceGraph.from_csr(csr)
    anchor = int(adj[off[0]])
    for probe in (base - 1, base, base + 1):
        for direction in (2, 0, 1):
            with gpu.options(BFS_BU_PROBE=probe, BFS_DIRECTION=direction):
                depth, parent, info = check(g, off, adj, 0, direction=direction)
            assert np.all(depth[hubs] == 2) and np.all(parent[hubs] == anchor) and info["levels"] == 4
            if direction == 2:
                assert info["bottom_up_levels"] == 3
    g.free()


# ---- 5. direction -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [12, 16])
def test_every_direction_gives_the_same_bytes(gpu, scale):
    key = "kronecker_%d_16" % scale
    csr = golden_csr(gpu, key)
    off, adj = csr.offsets(), csr.neighbors()
    g = device_graph(gpu, key)
    for source in (0, GRAPHS[key]["picks"][0]):
        want = bfs_np(off, adj, source)
        first = None
        for opts, replay in (({}, {}), ({"BFS_DIRECTION": 1}, {"direction": 1}), ({"BFS_DIRECTION": 2}, {"direction": 2}),
                             ({"BFS_ALPHA": 1, "BFS_BETA": 1}, {"alpha": 1, "beta": 1}),
                             ({"BFS_ALPHA": 1000000, "BFS_BETA": 1000000}, {"alpha": 1000000, "beta": 1000000}),
                             ({"BFS_WG_FRONTIER": 0}, {})):
            with gpu.options(**opts):
                depth, parent, info = g.bfs(source)
                scores = g.betweenness([source, 0])[0]
            got = (depth.tobytes(), parent.tobytes(), facts(info), scores.tobytes())
            first = first or got
            assert got == first, (source, opts)
            assert info["bottom_up_levels"] == bfs_np(off, adj, source, **replay)[2]["bottom_up_levels"], (source, opts, info)
        assert np.array_equal(np.frombuffer(first[0], dtype=np.int32), want[0]) and np.array_equal(np.frombuffer(first[1], dtype=np.int32), want[1])
    if scale == 16:   # the bottom-up step is on the default path
        assert g.bfs(0)[2]["bottom_up_levels"] >= 1


# ---- 6. components ----------------------------------------------------------------------------------------------------------------------
def test_reached_set_is_the_component(gpu):
    g = device_graph(gpu, "kronecker_12_16")
    label, _ = g.connected_components()
    roots, sizes = np.unique(label, return_counts=True)
    picked = [int(roots[np.argmax(sizes)]), int(roots[sizes == 1][0]), int(roots[(sizes > 1) & (sizes < sizes.max())][0])]
    for source in picked:
        depth, _, info = g.bfs(source)
        assert np.array_equal(depth >= 0, label == label[source]) and info["reached"] == int((label == label[source]).sum())


# ---- 7. large counts --------------------------------------------------------------------------------------------------------------------
def test_path_counts_beyond_64_bits(gpu):
    csr = edges_to_csr(gpu, grid_edges(40, 40), n=1600)
    off, adj = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    got, info = g.betweenness([0])
    want, max_sigma, levels = betweenness_exact(off, adj, [0])
    assert max_sigma == math.comb(78, 39) and info["max_sigma"] > 2.0 ** 64 and info["max_levels"] == levels == 79
    assert abs(info["max_sigma"] - float(max_sigma)) <= 2.0 ** -53 * 79 * 4 * float(max_sigma)
    bound = bc_bound_inexact(want, levels, 4)
    print(f"grid: largest relative error {float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))):.3e}, bound {float(bound.max() / want.max()):.3e}")
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound)
    g.free()


# ---- 7b. long rows and many levels in the betweenness sweeps ----------------------------------------------------------------------------
def test_betweenness_of_a_star_of_70000_leaves(gpu):
    """Every path count is 1 and every term an integer, so the closed form holds EXACTLY whatever the order of a sum.  From the hub: delta(hub) = L.
    From leaf a: delta(hub) = L - 1 (one term per other leaf: the hub's row is parked and cut into 18 chunks), delta(a) = L."""
    L = 70000
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, star_edges(L), n=L + 1))
    want_hub, want_leaf = np.zeros(L + 1), np.zeros(L + 1)
    want_hub[0] = L
    want_leaf[0], want_leaf[5] = L - 1, L
    textbook = np.zeros(L + 1)
    textbook[0] = L - 1
    first = None
    for direction in (0, 1, 2, 0):
        with gpu.options(BFS_DIRECTION=direction):
            hub, hinfo = g.betweenness([0])
            leaf, linfo = g.betweenness([5])
            both, binfo = g.betweenness([0, 5, 5])
            excl, _ = g.betweenness([5, 0], exclude_source=True)
            norm, _ = g.betweenness([0, 5, 5], normalize=True)
        assert np.array_equal(hub, want_hub) and np.array_equal(leaf, want_leaf) and np.array_equal(both, want_hub + 2 * want_leaf)
        assert np.array_equal(excl, textbook) and np.array_equal(norm, both / (3 * L - 2)) and norm.max() == 1.0
        assert (hinfo["max_levels"], linfo["max_levels"], binfo["max_levels"]) == (2, 3, 3) and binfo["max_sigma"] == 1.0
        assert binfo["reached_total"] == 3 * (L + 1) and binfo["max_score"] == 3 * L - 2
        got = (hub.tobytes(), leaf.tobytes(), both.tobytes(), excl.tobytes(), norm.tobytes())
        first = first or got
        assert got == first, direction
    g.free()


@pytest.mark.parametrize("wg_frontier", [512, 0])
def test_betweenness_of_a_path_of_4096_vertices(gpu, wg_frontier):
    n = 4096
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, path_edges(n, "along"), n=n))
    i = np.arange(n, dtype=np.float64)
    with gpu.options(BFS_WG_FRONTIER=wg_frontier):
        end, einfo = g.betweenness([0])                            # delta(i) = n - 1 - i, the source's own term included
        mid, minfo = g.betweenness([2047], exclude_source=True)    # both arms: the vertices beyond i on its side
    assert np.array_equal(end, n - 1 - i) and einfo["max_levels"] == n and einfo["max_sigma"] == 1.0 and einfo["reached_total"] == n
    want = np.where(i < 2047, i, n - 1 - i)
    want[2047] = 0.0
    assert np.array_equal(mid, want) and minfo["max_levels"] == 2049
    g.free()


# ---- 8. flags ---------------------------------------------------------------------------------------------------------------------------
def test_flags(gpu):
    key = "kronecker_10_16"
    g = device_graph(gpu, key)
    rec = GRAPHS[key]
    srcs = rec["picks"][:4]
    default, info = g.betweenness(srcs)
    textbook, _ = g.betweenness(srcs, exclude_source=True)
    own = default - textbook
    reached = {s: g.bfs(s)[2]["reached"] for s in srcs}
    want = np.zeros(rec["n"])
    for s in srcs:
        want[s] += reached[s] - 1
    levels = info["max_levels"]
    assert np.all(np.abs(own - want) <= bc_bound(np.maximum(default, want), levels, rec["max_degree"], len(srcs)))
    assert not own[np.setdiff1d(np.arange(rec["n"]), srcs)].any()   # elsewhere the very same bits
    assert info["reached_total"] == sum(reached.values())
    norm, ninfo = g.betweenness(srcs, normalize=True)
    assert norm.max() == 1.0 and ninfo["max_score"] == default.max() and np.array_equal(norm, default / default.max())
    once, twice = g.betweenness(srcs[:1])[0], g.betweenness([srcs[0], srcs[0]])[0]
    assert np.array_equal(twice, 2.0 * once)
    zeros, zinfo = g.betweenness([])
    assert zeros.size == rec["n"] and not zeros.any() and zinfo["sources"] == 0
    e = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=7))
    for normalize in (False, True):
        scores, einfo = e.betweenness([0, 3, 6], normalize=normalize)
        assert scores.tolist() == [0.0] * 7 and einfo["max_score"] == 0.0 and einfo["reached_total"] == 3
    e.free()


# ---- 9. same bytes ------------------------------------------------------------------------------------------------------------------------
def test_same_bytes_in_every_variant(gpu):
    csr = host_graph(gpu, "kronecker", 12)
    rec = [r for r in BFS if r["graph"] == "kronecker_12_16" and r["kind"] == "pick"][0]
    srcs = GRAPHS["kronecker_12_16"]["picks"][:4]
    g = gpu.DeviceGraph.from_csr(csr)
    variants = [("run 1", g, {}), ("run 2", g, {}), ("run 3", g, {}), ("top-down", g, {"BFS_DIRECTION": 1}), ("bottom-up", g, {"BFS_DIRECTION": 2}),
                ("trusted", gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_TRUSTED), {}), ("hub limit 64", gpu.DeviceGraph.from_csr(csr, flags=64 << 8), {}),
                ("shard 1 of 4", gpu.DeviceGraph.from_csr(csr, shard=(1, 4)), {})]
    first = None
    for name, h, opts in variants:
        with gpu.options(**opts):
            depth, parent, info = h.bfs(rec["source"])
            scores, bi = h.betweenness(srcs)
        got = (depth.tobytes(), parent.tobytes(), facts(info), scores.tobytes(), bi)
        first = first or got
        assert got == first, name
        assert sha(depth) == rec["depth_sha256"] and sha(parent) == rec["parent_sha256"]
        if h is not g:
            h.free()
    g.free()


# ---- 10. contract -------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    L = gpu.lib()
    csr = host_graph(gpu, "kronecker", 10)
    g = gpu.DeviceGraph.from_csr(csr)
    n = csr.num_nodes
    depth, parent, scores = np.full(n, -77, dtype=np.int32), np.full(n, -78, dtype=np.int32), np.full(n, -79.0)
    info, bc = gpu.BfsInfo(), gpu.BcInfo()
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    C.memset(C.byref(bc), 0x5a, C.sizeof(bc))
    before = bytes(info), bytes(bc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    src, bad_src = np.array([1, 2], dtype=np.int32), np.array([1, n], dtype=np.int32)
    assert L.gmsx_bfs(None, 0, p(depth), p(parent), C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_bfs(g._h, 0, p(depth), p(parent), None, None) == gpu.ERR_INVALID
    for bad in (-1, n, n + 5, -(2 ** 31)):
        assert L.gmsx_bfs(g._h, bad, p(depth), p(parent), C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(None, 2, p(src), 0, p(scores), C.byref(bc), None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(g._h, 2, p(src), 0, p(scores), None, None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(g._h, 2, p(src), 0, None, C.byref(bc), None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(g._h, 2, None, 0, p(scores), C.byref(bc), None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(g._h, 2, p(bad_src), 0, p(scores), C.byref(bc), None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(g._h, 2, p(np.array([-1, 0], dtype=np.int32)), 0, p(scores), C.byref(bc), None) == gpu.ERR_INVALID
    for flags in (4, 8, 0x80000000):
        assert L.gmsx_betweenness(g._h, 2, p(src), flags, p(scores), C.byref(bc), None) == gpu.ERR_INVALID
    assert L.gmsx_betweenness(g._h, -1, p(src), 0, p(scores), C.byref(bc), None) == gpu.ERR_INVALID
    assert np.all(depth == -77) and np.all(parent == -78) and np.all(scores == -79.0) and (bytes(info), bytes(bc)) == before
    # NULL arrays and NULL stats are allowed: info alone
    assert L.gmsx_bfs(g._h, 0, None, None, C.byref(info), None) == 0 and info.reached == 896 and info.reserved == 0
    names = gpu.option_names()
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("BFS_DIRECTION", "BFS_ALPHA", "BFS_BETA", "BFS_BU_PROBE", "BFS_WG_FRONTIER"):
        assert name in names and name in hdr
    assert L.gmsx_version() == 320
    g.free()
