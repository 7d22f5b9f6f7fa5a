"""GPU: gmsx_bfs_multi through the C-ABI against the goldens (tests/golden/msbfs.{json,npz}), against gmsx_bfs on the same handle and against
closed forms:

  goldens      every record: the integers and closeness byte-equal, harmonic within the derived bound, the per-vertex arrays, info and stats
  single       kronecker 16 (64 picks, a row of degree 9 869) and kronecker 12 (130 picks): row i of depth and per_source[i] equal gmsx_bfs
  words        1, 63, 64, 65, 128, 129 sources at MSBFS_WORDS 1 and 2: passes, and the per-vertex arrays as sums of single-source depths
  duplicates   one source listed 3 times among 66
  depth        a path on 4096 vertices from both ends, the middle and 127 random vertices, every MSBFS_DIRECTION
  width        a star with 70 000 leaves from the hub, from 64 leaves, from 64 leaves and the hub, every MSBFS_DIRECTION
  early exit   K_130 from every vertex
  components   two cliques and isolated vertices, an edgeless graph, n = 1, n = 0
  rule         push_levels / pull_levels equal the numpy replay at MSBFS_ALPHA 1, 15 and 1 000 000
  same bytes   three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, every MSBFS_DIRECTION and MSBFS_WORDS
  contract     NULL arguments, ids out of range, untouched arrays on error, info alone, the options enumerated and documented"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, edges_to_csr, host_graph
from test_msbfs_golden_cpu import ARR, GRAPHS, INT_KEYS, golden_per_source, harmonic_bound, replay_rule, sha_of, sources_of
from test_traversal_golden_cpu import golden_csr, path_edges, star_edges

pytestmark = pytest.mark.gpu

WORDS = (1, 2)
OPTION_FACTS = ("passes", "push_levels", "pull_levels")  # the info fields the options may change


def default_words(count):
    """MSBFS_WORDS 0, the default: one word up to 64 sources, two beyond (gmsx.h, OPTIONS)"""
    return 1 if count <= 64 else 2


def facts(info):
    return {k: v for k, v in info.items() if k not in OPTION_FACTS}


def as_bytes(r):
    """every output that is a function of (graph, sources) alone"""
    per, depth, vertex, info = r[:4]
    return (per.tobytes(), None if depth is None else depth.tobytes(), tuple(a.tobytes() for a in vertex), tuple(sorted(facts(info).items())))


_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        _GRAPHS[key] = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    return _GRAPHS[key]


_SINGLE = {}


def single(gpu, key, source):
    """(depth, info) of gmsx_bfs from `source` on the shared handle of golden graph `key`: computed once"""
    if (key, source) not in _SINGLE:
        depth, _, info = device_graph(gpu, key).bfs(int(source), want_parent=False)
        _SINGLE[(key, source)] = (depth, info)
    return _SINGLE[(key, source)]


def check_levels(info, per, words):
    """passes, and push_levels + pull_levels = Σ over the passes of the largest levels - 1"""
    chunk = 64 * words
    assert info["passes"] == (len(per) + chunk - 1) // chunk
    want = sum(int(per["levels"][b:b + chunk].max()) - 1 for b in range(0, len(per), chunk))
    assert info["push_levels"] + info["pull_levels"] == want, (info, want)


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_equals_the_golden(gpu, key):
    rec, want = GRAPHS[key], golden_per_source(key)
    srcs = sources_of(key)
    g = device_graph(gpu, key)
    per, depth, (dist_sum, reach, far), info, st = g.bfs_multi(srcs, stats=True)
    assert depth is None
    for k in INT_KEYS:
        assert np.array_equal(per[k], want[k]), k
    assert not per["reserved"].any()
    assert per["closeness"].tobytes() == want["closeness"].tobytes()  # one division of exact integers
    nz = want["harmonic"] > 0
    assert np.all(per["harmonic"][~nz] == 0.0)
    rel = np.abs(per["harmonic"][nz] - want["harmonic"][nz]) / want["harmonic"][nz]
    bound = np.array([harmonic_bound(int(lv)) for lv in want["levels"][nz]])
    print(f"{key}: largest relative error of harmonic {float(rel.max()) if rel.size else 0.0:.3e}, "
          f"largest error / bound {float((rel / bound).max()) if rel.size else 0.0:.3f}")
    assert np.all(rel <= bound)
    assert facts(info) == rec["info"]
    words = default_words(len(srcs))
    check_levels(info, per, words)
    for name, got, dtype in (("dist_sum", dist_sum, "<i8"), ("reach", reach, "<i4"), ("far", far, "<i4")):
        assert sha_of(got, dtype) == rec["vertex_sha256"][name], name
        if rec["literal"]:
            assert np.array_equal(got, ARR[name + "_" + key]), name
    assert st["units"] == int(want["reached_arcs"].sum())
    assert st["probes"] == sum(int(want["levels"][b:b + 64 * words].max()) for b in range(0, len(srcs), 64 * words)) and st["launches"] >= 3
    if rec["sources"] == "all":
        assert np.array_equal(per["depth_sum"], dist_sum)  # farness
        assert np.array_equal(far, per["levels"] - 1)      # eccentricity inside the component


# ---- 2. against the single-source path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["kronecker_16_16", "kronecker_12_16"])
def test_equals_the_single_source_path(gpu, key):
    srcs = sources_of(key)
    g = device_graph(gpu, key)
    per, depth, _, info = g.bfs_multi(srcs, want_depth=True, want_vertex=False)
    assert depth.shape == (len(srcs), GRAPHS[key]["n"])
    for i, s in enumerate(srcs):
        want_depth, want = single(gpu, key, s)
        assert np.array_equal(depth[i], want_depth), (i, s)
        assert {k: int(per[k][i]) for k in INT_KEYS} == {k: want[k] for k in INT_KEYS}, (i, s)
    assert info["reached_total"] == int(per["reached"].sum())


# ---- 3. word boundaries -----------------------------------------------------------------------------------------------------------------
def boundary_sources(n):
    """129 vertices of kronecker_10_16, fixed: the relabelled graph keeps its isolated vertices at the largest ids, so both kinds are among them"""
    return np.random.default_rng(7).choice(n, size=129, replace=False).astype(np.int32)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 129])
def test_word_boundaries(gpu, count, words):
    key = "kronecker_10_16"
    n = GRAPHS[key]["n"]
    srcs = boundary_sources(n)[:count]
    rows = np.stack([single(gpu, key, s)[0] for s in srcs]).astype(np.int64)
    got = rows >= 0
    g = device_graph(gpu, key)
    with gpu.options(MSBFS_WORDS=words):
        per, depth, (dist_sum, reach, far), info = g.bfs_multi(srcs, want_depth=True)
    assert np.array_equal(depth, rows)
    assert np.array_equal(dist_sum, np.where(got, rows, 0).sum(axis=0)) and np.array_equal(reach, got.sum(axis=0))
    assert np.array_equal(far, rows.max(axis=0))
    assert np.array_equal(per["reached"], got.sum(axis=1)) and np.array_equal(per["depth_sum"], np.where(got, rows, 0).sum(axis=1))
    check_levels(info, per, words)
    assert info["sources"] == count and info["max_far"] == int(rows.max())


# ---- 4. duplicates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
def test_a_source_listed_three_times(gpu, words):
    key = "kronecker_10_16"
    base = boundary_sources(GRAPHS[key]["n"])[:64].tolist()
    dup = base[5]
    srcs = base[:20] + [dup] + base[20:] + [dup]  # 66 entries: positions 5, 20 and 65 — the last one in the second word or pass
    assert len(srcs) == 66 and srcs.count(dup) == 3
    g = device_graph(gpu, key)
    with gpu.options(MSBFS_WORDS=words):
        per, depth, (dist_sum, reach, far), info = g.bfs_multi(srcs, want_depth=True)
        once = g.bfs_multi(base, want_depth=True)
    at = [i for i, s in enumerate(srcs) if s == dup]
    assert at == [5, 20, 65]
    for i in at[1:]:
        assert np.array_equal(depth[i], depth[at[0]]) and per[i].tobytes() == per[at[0]].tobytes()
    row = depth[at[0]].astype(np.int64)
    assert np.array_equal(reach, once[2][1] + 2 * (row >= 0)) and np.array_equal(dist_sum, once[2][0] + 2 * np.where(row >= 0, row, 0))
    assert np.array_equal(far, once[2][2]) and info["reached_total"] == once[3]["reached_total"] + 2 * int(per["reached"][5])


# ---- 5. depth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["along", "random"])
def test_path_of_4096_vertices(gpu, numbering):
    n = 4096
    e = path_edges(n, numbering)
    order = np.concatenate([e[:1, 0], e[:, 1]])  # order[p] = the vertex at position p of the path
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    where = np.concatenate([[0, n - 1, n // 2], np.random.default_rng(11).choice(n, size=127, replace=False)])
    srcs = order[where].astype(np.int32)
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, e, n=n))
    first = None
    for direction in (0, 1, 2):
        with gpu.options(MSBFS_DIRECTION=direction):
            r = g.bfs_multi(srcs)
        per, _, (dist_sum, reach, far), info = r
        first = first or as_bytes(r)
        assert as_bytes(r) == first, direction
        check_levels(info, per, default_words(len(srcs)))
        assert (info["push_levels"] == 0) if direction == 2 else (info["pull_levels"] == 0) if direction == 1 else True
    p = where.astype(np.int64)
    assert np.array_equal(per["depth_sum"], p * (p + 1) // 2 + (n - 1 - p) * (n - p) // 2)
    assert np.array_equal(per["levels"], np.maximum(p, n - 1 - p) + 1) and np.all(per["reached"] == n)
    assert np.array_equal(far, np.maximum(pos, n - 1 - pos)) and np.all(reach == len(srcs))  # (both ends are sources)
    assert np.array_equal(dist_sum, np.abs(pos[:, None] - p[None, :]).sum(axis=1))
    assert info["max_far"] == n - 1 and info["max_levels"] == n and info["passes"] == 2
    assert per["harmonic"][0] == sum(1.0 / d for d in range(1, n))  # the same terms in the same order
    g.free()


# ---- 6. width -------------------------------------------------------------------------------------------------------------------------------
def test_star_of_70000_leaves(gpu):
    L = 70000
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, star_edges(L), n=L + 1))
    leaves = np.random.default_rng(3).choice(np.arange(1, L + 1), size=64, replace=False).astype(np.int32)
    first = {}
    for direction, words in ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)):   # (push from the hub cuts a parked row across the waves; the pull
        # into the hub exits at its first chunk; of 65 sources the hub is the first bit of the second word, or at MSBFS_WORDS 1 of a second pass)
        for name, srcs in (("hub", [0]), ("leaves", leaves.tolist()), ("leaves and hub", leaves.tolist() + [0])):
            with gpu.options(MSBFS_DIRECTION=direction, MSBFS_WORDS=words):
                r = g.bfs_multi(srcs)
            per, _, (dist_sum, reach, far), info = r
            assert as_bytes(r) == first.setdefault(name, as_bytes(r)), (name, direction)
            hub = np.array([s == 0 for s in srcs])
            nl, nh = int((~hub).sum()), int(hub.sum())
            assert np.all(per["reached"] == L + 1) and np.all(per["reached_arcs"] == 2 * L)
            assert np.array_equal(per["depth_sum"], np.where(hub, L, 2 * L - 1)) and np.array_equal(per["levels"], np.where(hub, 2, 3))
            assert np.array_equal(per["closeness"], np.where(hub, 1.0, L / (2 * L - 1)))
            assert np.array_equal(per["harmonic"], np.where(hub, float(L), 1.0 + (L - 1) / 2.0))
            want_dist = np.full(L + 1, 2 * nl + nh, dtype=np.int64)   # a leaf: 2 from every other leaf, 1 from the hub
            want_dist[0] = nl
            want_dist[leaves] -= 2 if nl else 0                        # … and 0 from itself
            want_far = np.full(L + 1, 2 if nl else 1, dtype=np.int32)
            want_far[0] = 1 if nl else 0
            assert np.array_equal(dist_sum, want_dist) and np.all(reach == len(srcs)) and np.array_equal(far, want_far)
            check_levels(info, per, words or default_words(len(srcs)))
    g.free()


# ---- 7. early exit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
def test_complete_graph_of_130_vertices(gpu, words):
    n = 130
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [(i, j) for i in range(n) for j in range(i)], n=n))
    for direction in (0, 1, 2):   # every vertex needs all the other bits at level 1 and has them after its first entries
        with gpu.options(MSBFS_DIRECTION=direction, MSBFS_WORDS=words):
            per, depth, (dist_sum, reach, far), info = g.bfs_multi(np.arange(n), want_depth=True)
        assert np.all(per["depth_sum"] == n - 1) and np.all(per["levels"] == 2) and np.all(per["reached"] == n) and np.all(per["closeness"] == 1.0)
        assert np.all(per["harmonic"] == float(n - 1)) and np.array_equal(depth, 1 - np.eye(n, dtype=np.int32))
        assert np.all(dist_sum == n - 1) and np.all(reach == n) and np.all(far == 1)
        assert info["passes"] == (3 if words == 1 else 2) and info["push_levels"] + info["pull_levels"] == info["passes"]
    g.free()


# ---- 8. components and isolated vertices ------------------------------------------------------------------------------------------------
def test_components_and_isolated_vertices(gpu):
    a, b = 70, 9   # vertices 0 .. 69 and 70 .. 78 are cliques, 79 .. 83 isolated
    edges = [(i, j) for i in range(a) for j in range(i)] + [(a + i, a + j) for i in range(b) for j in range(i)]
    n = a + b + 5
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=n))
    srcs = [0, a, n - 1, a - 1, n - 2]
    per, depth, (dist_sum, reach, far), info = g.bfs_multi(srcs, want_depth=True)
    assert per["reached"].tolist() == [a, b, 1, a, 1] and per["depth_sum"].tolist() == [a - 1, b - 1, 0, a - 1, 0]
    assert per["levels"].tolist() == [2, 2, 1, 2, 1] and per["reached_arcs"].tolist() == [a * (a - 1), b * (b - 1), 0, a * (a - 1), 0]
    assert per["closeness"].tolist() == [1.0, 1.0, 0.0, 1.0, 0.0] and per["harmonic"].tolist() == [a - 1.0, b - 1.0, 0.0, a - 1.0, 0.0]
    assert reach.tolist() == [2] * a + [1] * b + [0, 0, 0, 1, 1] and far.tolist() == [1] * (a - 1) + [1] + [0] + [1] * (b - 1) + [-1] * 3 + [0, 0]
    assert dist_sum.tolist() == [1] + [2] * (a - 2) + [1] + [0] + [1] * (b - 1) + [0] * 5
    assert np.array_equal(depth[2], np.where(np.arange(n) == n - 1, 0, -1)) and info["max_far"] == 1 and info["reached_total"] == 2 * a + b + 2
    g.free()
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=7))   # edgeless
    per, depth, (dist_sum, reach, far), info = g.bfs_multi([0, 3, 3, 6], want_depth=True)
    assert np.all(per["reached"] == 1) and np.all(per["levels"] == 1) and not per["closeness"].any() and not per["harmonic"].any()
    assert reach.tolist() == [1, 0, 0, 2, 0, 0, 1] and far.tolist() == [0, -1, -1, 0, -1, -1, 0] and not dist_sum.any()
    assert info == {"sources": 4, "passes": 1, "reached_total": 4, "max_levels": 1, "max_far": 0, "push_levels": 0, "pull_levels": 0}
    none = g.bfs_multi([])
    assert none[0].size == 0 and not none[2][0].any() and not none[2][1].any() and np.all(none[2][2] == -1) and not any(none[3].values())
    g.free()
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=1))
    per, depth, (dist_sum, reach, far), info = g.bfs_multi([0], want_depth=True)
    assert depth.tolist() == [[0]] and per["reached"].tolist() == [1] and (dist_sum.tolist(), reach.tolist(), far.tolist()) == ([0], [1], [0])
    g.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # n = 0
    per, _, (dist_sum, reach, far), info = g.bfs_multi([])
    assert per.size == 0 and dist_sum.size == 0 and not any(info.values())
    with pytest.raises(gpu.GmsxError) as ei:
        g.bfs_multi([0])
    assert ei.value.status == gpu.ERR_INVALID
    g.free()


# ---- 9. the direction rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
def test_direction_rule_equals_its_replay(gpu, words):
    key = "kronecker_12_16"
    srcs = sources_of(key)
    csr = golden_csr(gpu, key)
    deg, nnz = np.diff(np.asarray(csr.offsets(), dtype=np.int64)), int(csr.nnz)
    g = device_graph(gpu, key)
    rows = np.stack([single(gpu, key, s)[0] for s in srcs])
    seen = set()
    for alpha in (1, 15, 1000000):
        with gpu.options(MSBFS_ALPHA=alpha, MSBFS_WORDS=words):
            info = g.bfs_multi(srcs, want_vertex=False)[3]
        want = replay_rule(rows, deg, nnz, alpha=alpha, words=words)
        assert (info["passes"], info["push_levels"], info["pull_levels"]) == want, (alpha, info, want)
        seen.add(want)
    assert len(seen) >= 2  # the three settings do not all take the same levels the same way


# ---- 10. same bytes -------------------------------------------------------------------------------------------------------------------------
def test_same_bytes_in_every_variant(gpu):
    csr = host_graph(gpu, "kronecker", 12)
    srcs = sources_of("kronecker_12_16")
    g = gpu.DeviceGraph.from_csr(csr)
    variants = [("run 1", g, {}), ("run 2", g, {}), ("run 3", g, {}), ("push", g, {"MSBFS_DIRECTION": 1}), ("pull", g, {"MSBFS_DIRECTION": 2}),
                ("two words", g, {"MSBFS_WORDS": 2}), ("two words, push", g, {"MSBFS_WORDS": 2, "MSBFS_DIRECTION": 1}),
                ("two words, pull", g, {"MSBFS_WORDS": 2, "MSBFS_DIRECTION": 2}),
                ("trusted", gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_TRUSTED), {}), ("hub limit 64", gpu.DeviceGraph.from_csr(csr, flags=64 << 8), {}),
                ("shard 1 of 4", gpu.DeviceGraph.from_csr(csr, shard=(1, 4)), {})]
    first = None
    for name, h, opts in variants:
        with gpu.options(**opts):
            r = h.bfs_multi(srcs, want_depth=True)
        first = first or as_bytes(r)
        assert as_bytes(r) == first, name
        if h is not g:
            h.free()
    g.free()
    want = golden_per_source("kronecker_12_16")
    assert np.array_equal(r[0]["depth_sum"], want["depth_sum"])


# ---- 11. contract ---------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    L = gpu.lib()
    csr = host_graph(gpu, "kronecker", 10)
    g = gpu.DeviceGraph.from_csr(csr)
    n = csr.num_nodes
    per = np.zeros(2, dtype=gpu.BFS_SOURCE_DTYPE)
    per["reached"] = -70
    depth, dist = np.full(2 * n, -71, dtype=np.int32), np.full(n, -72, dtype=np.int64)
    reach, far = np.full(n, -73, dtype=np.int32), np.full(n, -74, dtype=np.int32)
    info = gpu.BfsMultiInfo()
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    before = bytes(info), per.tobytes()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    src = np.array([1, 2], dtype=np.int32)
    call = lambda h, k, s, i: L.gmsx_bfs_multi(h, k, s, p(per), p(depth), p(dist), p(reach), p(far), i, None)  # noqa: E731
    assert call(None, 2, p(src), C.byref(info)) == gpu.ERR_INVALID
    assert call(g._h, 2, p(src), None) == gpu.ERR_INVALID
    assert call(g._h, -1, p(src), C.byref(info)) == gpu.ERR_INVALID
    assert call(g._h, 2, None, C.byref(info)) == gpu.ERR_INVALID
    for bad in (-1, n, n + 5, -(2 ** 31)):
        assert call(g._h, 2, p(np.array([1, bad], dtype=np.int32)), C.byref(info)) == gpu.ERR_INVALID
    assert np.all(depth == -71) and np.all(dist == -72) and np.all(reach == -73) and np.all(far == -74) and (bytes(info), per.tobytes()) == before
    # every output pointer NULL: info alone
    assert L.gmsx_bfs_multi(g._h, 2, p(src), None, None, None, None, None, C.byref(info), None) == 0
    want = g.bfs(1)[2]["reached"] + g.bfs(2)[2]["reached"]
    assert (info.sources, info.passes, info.reached_total) == (2, 1, want) and info.max_levels >= 1 and info.max_far == info.max_levels - 1
    # n_sources = 0 with a NULL list
    assert call(g._h, 0, None, C.byref(info)) == 0
    assert not dist.any() and not reach.any() and np.all(far == -1) and np.all(depth == -71) and bytes(info) == bytes(C.sizeof(info))
    names = gpu.option_names()
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("MSBFS_DIRECTION", "MSBFS_ALPHA", "MSBFS_WORDS"):
        assert name in names and name in hdr
    assert L.gmsx_version() == 320
    g.free()
