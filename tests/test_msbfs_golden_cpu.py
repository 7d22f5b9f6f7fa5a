"""CPU: the goldens of batched multi-source BFS (tests/golden/msbfs.{json,npz}, written by tools/make_golden_msbfs.py) agree with the definitions
of include/gmsx.h restated here:

  * depths_np / msbfs_np: one plain BFS per source; the gmsx_bfs_source integers from the depths, the per-level counts, the per-vertex arrays
    dist_sum / reach / far as sums over the rows; harmonic as the exact rational Σ count_d / d rounded ONCE, closeness as one division;
  * the all-sources identity per_source.depth_sum == dist_sum[source];
  * the tie to tests/golden/traversal.json, whose BFS records come from the compiled reference: every (graph, source) recorded there gives the
    same reached, reached_arcs, depth_sum, levels and depth sha256 here;
  * harmonic_bound — the tolerance the GPU test allows — is at least the error of a left-to-right double sum, on every record;
  * replay_rule: push_levels / pull_levels / passes of the direction rule, a fact about (graph, sources, options).

msbfs_np, replay_rule, harmonic_bound and the record readers are what tests/test_msbfs_gpu.py checks the device against."""
import ctypes
import hashlib
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden
from test_traversal_golden_cpu import BFS as TRAV_BFS
from test_traversal_golden_cpu import _rows, golden_csr, sha

MS = load_golden("msbfs.json")
ARR = np.load(os.path.join(GOLDEN, "msbfs.npz"))
GRAPHS = MS["graphs"]
INT_KEYS = ("reached", "reached_arcs", "depth_sum", "levels")
EPS = 2.0 ** -53
ALPHA = 15  # the default of msbfs.hip (gmsx.h, OPTIONS)


def sha_of(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def depths_np(off, adj, source):
    """depth[v] = distance from source, -1 = unreachable (int32[n])"""
    n = off.size - 1
    depth = np.full(n, -1, dtype=np.int32)
    depth[source] = 0
    front, d = np.array([source], dtype=np.int64), 0
    while front.size:
        pos, _ = _rows(off, front)
        w = adj[pos]
        mark = np.zeros(n, dtype=bool)
        mark[w[depth[w] == -1]] = True
        front = np.flatnonzero(mark)
        d += 1
        depth[front] = d
    return depth


def harmonic_exact(counts):
    """Σ_{d >= 1} counts[d] / d as the exact rational, rounded once"""
    return float(sum((Fraction(int(c), d) for d, c in enumerate(counts) if d >= 1), Fraction(0)))


def harmonic_left_to_right(counts):
    """… as the library adds it: ascending in d, in double"""
    s = 0.0
    for d, c in enumerate(counts):
        if d >= 1:
            s += float(c) / float(d)
    return s


def harmonic_bound(levels):
    """relative error of a sum of at most levels - 1 positive terms, each one correctly rounded division, added by at most levels - 2 additions:
    (1 + eps)^levels - 1 <= levels eps / (1 - levels eps)"""
    return levels * EPS / (1.0 - levels * EPS)


def msbfs_np(off, adj, sources, want_depth=True):
    """the outputs of gmsx_bfs_multi: {per-source integer arrays, closeness, harmonic, counts (per-level, per source), depth (S x n) or None,
    dist_sum, reach, far, info}"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n, deg = off.size - 1, np.diff(off)
    S = len(sources)
    out = {k: np.zeros(S, dtype=np.int64) for k in INT_KEYS}
    out["closeness"], out["harmonic"], out["counts"] = np.zeros(S), np.zeros(S), []
    dist_sum, reach, far = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    rows = np.zeros((S, n), dtype=np.int32) if want_depth else None
    cache = {}
    for i, s in enumerate(sources):
        s = int(s)
        if s not in cache:
            cache[s] = depths_np(off, adj, s)
        depth = cache[s]
        got = depth >= 0
        counts = np.bincount(depth[got]).tolist()
        out["reached"][i], out["reached_arcs"][i] = int(got.sum()), int(deg[got].sum())
        out["depth_sum"][i], out["levels"][i] = int(depth[got].sum(dtype=np.int64)), len(counts)
        out["closeness"][i] = (out["reached"][i] - 1) / out["depth_sum"][i] if out["depth_sum"][i] else 0.0
        out["harmonic"][i] = harmonic_exact(counts)
        out["counts"].append(counts)
        dist_sum[got] += depth[got]
        reach[got] += 1
        far[got] = np.maximum(far[got], depth[got])
        if want_depth:
            rows[i] = depth
        if len(cache) > 256:
            cache.clear()
    out.update(depth=rows, dist_sum=dist_sum, reach=reach, far=far)
    out["info"] = {"sources": S, "reached_total": int(out["reached"].sum()), "max_levels": int(out["levels"].max()) if S else 0,
                   "max_far": int(far.max()) if S and n else 0}
    return out


def replay_rule(depth_rows, deg, nnz, alpha=ALPHA, direction=0, words=1):
    """(passes, push_levels, pull_levels): per pass of 64 * words rows, level L = 1 .. the largest depth is pushed when the degrees of the
    vertices that some row of the pass holds at depth L - 1 add up to at most nnz // alpha"""
    S = depth_rows.shape[0]
    per = 64 * words
    passes = push = pull = 0
    for base in range(0, S, per):
        rows = depth_rows[base:base + per]
        passes += 1
        for level in range(1, int(rows.max()) + 1):
            active = np.any(rows == level - 1, axis=0)
            is_push = direction == 1 or (direction == 0 and int(deg[active].sum()) <= nnz // alpha)
            push, pull = push + is_push, pull + (not is_push)
    return passes, push, pull


def sources_of(key):
    g = GRAPHS[key]
    return list(range(g["n"])) if g["sources"] == "all" else list(g["sources"])


def golden_per_source(key):
    """the recorded per-source fields as arrays (the doubles from their hex form)"""
    p = GRAPHS[key]["per_source"]
    r = {k: np.array(p[k], dtype=np.int64) for k in INT_KEYS}
    for k in ("closeness", "harmonic"):
        r[k] = np.array([float.fromhex(x) for x in p[k]], dtype=np.float64)
    return r


_NP = {}


def restated(capi, key):
    if key not in _NP:
        csr = golden_csr(capi, key)
        _NP[key] = msbfs_np(csr.offsets(), csr.neighbors(), sources_of(key), want_depth=False)
    return _NP[key]


def test_goldens_are_complete():
    all_sources = {"file_eppsteinExample", "file_micro", "file_smallRandom1", "file_tomitaExample", "file_triangles_1", "file_triangles_3",
                   "kronecker_10_16", "kronecker_10_16_raw", "uniform_10_16"}
    assert set(GRAPHS) == all_sources | {"kronecker_12_16", "kronecker_16_16", "uniform_16_16"}
    for key, g in GRAPHS.items():
        want = "all" if key in all_sources else None
        assert (g["sources"] == "all") == (want == "all")
        assert len(sources_of(key)) == (g["n"] if want else 130 if key == "kronecker_12_16" else 64)
        assert g["literal"] == (key not in ("kronecker_16_16", "uniform_16_16"))  # those two: per-vertex arrays as sha256 only
        for name in ("dist_sum", "reach", "far"):
            assert (name + "_" + key in ARR.files) == g["literal"] and len(g["vertex_sha256"][name]) == 64
        assert all(len(g["per_source"][k]) == len(sources_of(key)) for k in INT_KEYS + ("closeness", "harmonic"))
    size = sum(os.path.getsize(os.path.join(GOLDEN, "msbfs." + e)) for e in ("json", "npz"))
    assert size <= 959201  # no larger than tests/golden/traversal.npz was when these goldens were added


@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_restatement_reproduces_the_golden(capi, key):
    g = GRAPHS[key]
    csr = golden_csr(capi, key)
    assert (csr.num_nodes, csr.nnz) == (g["n"], g["nnz"])
    if g["sources"] != "all":
        assert csr.pick_sources(len(g["sources"])).tolist() == g["sources"]
    got, want = restated(capi, key), golden_per_source(key)
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert got["closeness"].tobytes() == want["closeness"].tobytes() and got["harmonic"].tobytes() == want["harmonic"].tobytes()
    assert got["info"] == g["info"]
    for name, dtype in (("dist_sum", "<i8"), ("reach", "<i4"), ("far", "<i4")):
        assert sha_of(got[name], dtype) == g["vertex_sha256"][name]
        if g["literal"]:
            assert np.array_equal(got[name], ARR[name + "_" + key])


@pytest.mark.parametrize("key", sorted(k for k in GRAPHS if GRAPHS[k]["sources"] == "all"))
def test_all_sources_identity(capi, key):
    got = restated(capi, key)
    assert np.array_equal(got["depth_sum"], got["dist_sum"])  # sources in id order: per_source[i].depth_sum == dist_sum[i]
    assert np.all(got["reach"] == got["reached"])             # … and a vertex is reached by exactly its component
    assert np.all(got["far"] == got["levels"] - 1)            # … its eccentricity there


def test_tie_to_the_traversal_goldens(capi):
    """every BFS record of traversal.json — the compiled reference's depths — against the restatement used here"""
    seen = 0
    for rec in TRAV_BFS:
        csr = golden_csr(capi, rec["graph"])
        off, adj = np.asarray(csr.offsets(), dtype=np.int64), np.asarray(csr.neighbors(), dtype=np.int64)
        r = msbfs_np(off, adj, [rec["source"]])
        assert {k: int(r[k][0]) for k in INT_KEYS} == {k: rec[k] for k in INT_KEYS}, (rec["graph"], rec["source"])
        assert sha(r["depth"][0]) == rec["depth_sha256"]
        srcs = sources_of(rec["graph"])
        if rec["source"] in srcs:  # … and the golden record of the same source
            i, p = srcs.index(rec["source"]), GRAPHS[rec["graph"]]["per_source"]
            assert {k: p[k][i] for k in INT_KEYS} == {k: rec[k] for k in INT_KEYS}
            seen += 1
    assert seen >= 2 * len(GRAPHS)


@pytest.mark.parametrize("key", sorted(GRAPHS))
def test_harmonic_bound_covers_a_left_to_right_sum(capi, key):
    got, want = restated(capi, key), golden_per_source(key)
    worst = 0.0
    for i, counts in enumerate(got["counts"]):
        h = harmonic_left_to_right(counts)
        if want["harmonic"][i] == 0.0:
            assert h == 0.0
            continue
        rel = abs(h - want["harmonic"][i]) / want["harmonic"][i]
        worst = max(worst, rel / harmonic_bound(len(counts)))
        assert rel <= harmonic_bound(len(counts))
    print(f"{key}: largest error of a left-to-right sum = {worst:.3f} of the bound")


def test_restatement_on_the_shapes_of_the_gpu_tests():
    from test_components_golden_cpu import csr_of, path_edges, star_edges
    n = 9
    off, adj = csr_of(path_edges(n, "along"), n)
    r = msbfs_np(off, adj, list(range(n)))
    i = np.arange(n)
    assert np.array_equal(r["dist_sum"], i * (i + 1) // 2 + (n - 1 - i) * (n - i) // 2) and np.array_equal(r["far"], np.maximum(i, n - 1 - i))
    assert r["info"]["max_far"] == n - 1 and r["harmonic"][0] == harmonic_exact([1] * n)
    assert replay_rule(r["depth"], np.diff(off), int(adj.size), alpha=1) == (1, n - 1, 0)
    assert replay_rule(r["depth"], np.diff(off), int(adj.size), direction=2) == (1, 0, n - 1)
    off, adj = csr_of(star_edges(5), 6)
    r = msbfs_np(off, adj, [0, 3, 3])
    assert r["reach"].tolist() == [3] * 6 and r["dist_sum"].tolist() == [2, 5, 5, 1, 5, 5] and r["levels"].tolist() == [2, 3, 3]
    assert r["closeness"].tolist() == [1.0, 5 / 9, 5 / 9] and r["harmonic"].tolist() == [5.0, 3.0, 3.0]


def test_new_symbol_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    assert "gmsx_bfs_multi" in capi.SYMBOLS and hasattr(L, "gmsx_bfs_multi") and "gmsx_bfs_multi(" in hdr
    for name in ("MSBFS_DIRECTION", "MSBFS_ALPHA", "MSBFS_WORDS"):
        assert name in capi.option_names() and name in hdr
    assert ctypes.sizeof(capi.BfsSource) == 48 == capi.BFS_SOURCE_DTYPE.itemsize and ctypes.sizeof(capi.BfsMultiInfo) == 40
    assert capi.lib().gmsx_version() == 320


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_entry_point_fails_loudly_without_gpu(capi):
    L = capi.lib()
    out = np.full(4, -77, dtype=np.int32)
    src = np.zeros(1, dtype=np.int32)
    info = capi.BfsMultiInfo()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(1 << 16)))  # never read: the call checks the device before the handle
    assert L.gmsx_bfs_multi(fake, 1, p(src), None, None, None, p(out), None, ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_bfs_multi(None, 1, p(src), None, None, None, p(out), None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_bfs_multi(fake, 1, p(src), None, None, None, p(out), None, None, None) == capi.ERR_INVALID
    assert L.gmsx_bfs_multi(fake, 1, None, None, None, None, p(out), None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_bfs_multi(fake, -1, p(src), None, None, None, p(out), None, ctypes.byref(info), None) == capi.ERR_INVALID
    assert np.all(out == -77)
