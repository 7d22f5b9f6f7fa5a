"""CPU: the goldens of PageRank (tests/golden/pagerank.{json,npz}, written by tools/make_golden_pagerank.py) agree with the definitions of
include/gmsx.h restated here:

  * pagerank_np: the sweeps in numpy float64 — contrib = scores / deg (0 for an isolated vertex, never divided), a row's sum taken in ascending
    position (np.bincount adds its weights in input order, and the CSR is in row order), new = (1 - d) t + d sum (+ (d D) t with `dangling`),
    error = Σ |new - old|, the dangling mass D by tree_sum — the fixed tree pagerank.hip states for it —; with float32=True scores and
    contrib are rounded to float after every sweep, the sums stay in double;
  * residual_np: one sweep over given scores, PRVerifier's number;
  * pr_bound(k, damping, dmax, eps): what two implementations of k sweeps may differ by in L1.  One computed sweep differs from the exact map
    by at most gamma = (dmax + 3) eps in L1 — a row sum of at most dmax terms in any order carries (dmax - 1) eps, the division, the product with
    the damping and the final sum one eps each, all relative, and the mass is <= 1 —; the exact map contracts L1 by `damping`, so k sweeps
    accumulate at most min(k, 1 / (1 - damping)) gamma, and two implementations twice that; 1.01 covers the second-order terms.  float32 storage
    adds 2 * 2^-24 to gamma (the stored score and the stored contribution), the dangling mass (isolated + 2) eps (its sum and two products);
  * closed forms: cycle, complete graph, star.

pagerank_np, residual_np, pr_bound, the shapes and the record readers are what tests/test_pagerank_gpu.py checks the device against."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph, load_golden

PR = load_golden("pagerank.json")
ARR = np.load(os.path.join(GOLDEN, "pagerank.npz"))
GRAPHS = PR["graphs"]
RECORDS = PR["records"]
EPS = 2.0 ** -53
EPS32 = 2.0 ** -24
PR_DANGLING, PR_FLOAT32 = 1, 2
K_LANE_ROW, K_GROUP_ROW, K_CHUNK = 16, 1024, 4096   # pagerank.hip: the constants of its summation rule
TELEPORTS = ("uniform", "degree", "first")


def teleport_of(kind, off):
    """the teleport vectors of the records, unnormalised: None (uniform), deg + 1, or everything on vertex 0"""
    n = off.size - 1
    if kind == "uniform":
        return None
    if kind == "degree":
        return (np.diff(off) + 1).astype(np.float64)
    assert kind == "first"
    t = np.zeros(n)
    t[0] = 3.0
    return t


def normalised(teleport, n):
    """t as the library forms it: the sum ascending in double, then one division per entry"""
    if teleport is None:
        return np.full(n, 1.0 / n)
    s = 0.0
    for x in np.asarray(teleport, dtype=np.float64).tolist():
        s += x
    return np.asarray(teleport, dtype=np.float64) / s


def _wave_tree(w):
    """rows of 64 values -> their sums by the shuffle tree 32, 16, … 1 (lane i takes lane i + o)"""
    w = w.copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[:, :o] = w[:, :o] + w[:, o:2 * o]
    return w[:, 0]


def tree_sum(values):
    """Σ values by the fixed tree pagerank.hip states for its reductions (THE REDUCTIONS): blocks of 256 consecutive values — per wave of 64 the
    shuffle tree, the four waves in order —, then one workgroup over the blocks' cells: thread t the cells t, t + 1024, … ascending, its 16 waves
    by the same tree, the 16 sums in order.  The dangling mass enters every score, so its rounding is part of the definition."""
    v = np.asarray(values, dtype=np.float64)
    if v.size == 0:
        return 0.0
    cells = (v.size + 255) // 256
    w = _wave_tree(np.concatenate([v, np.zeros(cells * 256 - v.size)]).reshape(-1, 64)).reshape(cells, 4)
    cell = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    per_thread = np.zeros(1024)
    for b in range(0, cells, 1024):   # ascending: thread t adds cell b + t
        chunk = cell[b:b + 1024]
        per_thread[:chunk.size] = per_thread[:chunk.size] + chunk
    waves = _wave_tree(per_thread.reshape(16, 64))
    total = waves[0]
    for x in waves[1:]:
        total = total + x
    return float(total)


def _sweep(off, adj, rows, deg, t, scores, damping, dangling, float32):
    safe = np.where(deg > 0, deg, 1).astype(np.float64)
    contrib = np.where(deg > 0, scores / safe, 0.0)
    if float32:
        contrib = contrib.astype(np.float32).astype(np.float64)
    sums = np.bincount(rows, weights=contrib[adj], minlength=off.size - 1) if adj.size else np.zeros(off.size - 1)
    new = (1.0 - damping) * t + damping * sums
    if dangling:
        new = new + (damping * tree_sum(scores[deg == 0])) * t   # (the isolated vertices ascending in their id)
    if float32:
        new = new.astype(np.float32).astype(np.float64)
    return new


def pagerank_np(off, adj, damping=0.85, max_iters=20, tolerance=1e-4, teleport=None, dangling=False, float32=False):
    """(scores, info, errors): info as gmsx_pagerank_info, errors = the error of every sweep"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    deg = np.diff(off)
    rows = np.repeat(np.arange(n), deg)
    t = normalised(teleport, n)
    scores = t.astype(np.float32).astype(np.float64) if float32 else t.copy()
    errors, converged = [], False
    for _ in range(max_iters):
        new = _sweep(off, adj, rows, deg, t, scores, damping, dangling, float32)
        errors.append(float(np.abs(new - scores).sum()))
        scores = new
        if errors[-1] < tolerance:
            converged = True
            break
    order = np.lexsort((np.arange(n), -scores))
    info = {"iterations": len(errors), "converged": int(converged), "argmax": int(order[0]) if n else -1, "error": errors[-1] if errors else 0.0,
            "sum": float(scores.sum()), "max_score": float(scores.max()) if n else 0.0, "isolated": int((deg == 0).sum())}
    return scores, info, errors


def residual_np(off, adj, scores, damping=0.85, teleport=None, dangling=False, float32=False):
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    deg = np.diff(off)
    s = np.asarray(scores, dtype=np.float64)
    if float32:
        s = s.astype(np.float32).astype(np.float64)
    new = _sweep(off, adj, np.repeat(np.arange(n), deg), deg, normalised(teleport, n), s, damping, dangling, float32)
    return float(np.abs(new - s).sum())


def top_five(scores):
    return np.lexsort((np.arange(scores.size), -scores))[:5].tolist()   # ties: the smaller id


def pr_bound(k, damping, dmax, eps, float32=False, isolated=None):
    """L1 distance two implementations of k sweeps may have (the module's docstring derives it); isolated: with GMSX_PR_DANGLING, their number"""
    gamma = (dmax + 3) * eps
    if float32:
        gamma = 2 * EPS32 + (dmax + 3) * EPS
    if isolated is not None:
        gamma += (isolated + 2) * eps
    horizon = min(float(k), 1.0 / (1.0 - damping)) if damping < 1.0 else float(k)
    return 2.0 * horizon * gamma * 1.01


def record_bound(rec, k=None):
    g = GRAPHS[rec["graph"]]
    return pr_bound(rec["iterations"] if k is None else k, rec["damping"], g["max_degree"], EPS, float32=bool(rec["flags"] & PR_FLOAT32),
                    isolated=g["isolated"] if rec["flags"] & PR_DANGLING else None)


def scalar_bound(bound, n, value):
    """… and a sum of n non-negative terms (error, sum) taken in two orders over two such arrays: the arrays' distance (twice for the error,
    which reads new and old) plus (n - 1) eps relative for either order"""
    return 2.0 * bound + 2.0 * n * EPS * abs(value)


def golden_csr(capi, key):
    src = GRAPHS[key]["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def rec_id(r):
    return "%s-d%g-i%d-t%g-%s-f%d" % (r["graph"], r["damping"], r["max_iters"], r["tolerance"], r["teleport"], r["flags"])


# ---- shapes the GPU tests run -------------------------------------------------------------------------------------------------------------------
CLASS_DEGREES = [1, K_LANE_ROW - 1, K_LANE_ROW, K_LANE_ROW + 1, K_GROUP_ROW - 1, K_GROUP_ROW, K_GROUP_ROW + 1, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1,
                 2 * K_CHUNK + 1]


def class_probe_graph():
    """(edges, n, hubs): hub i has degree CLASS_DEGREES[i] — one row on either side of every class threshold and of the chunk size.  The hubs
    share one pool of leaves (hub i takes the first d_i of them, so the leaves' degrees run from 1 to the number of hubs), the hubs are chained
    to each other through two of their entries, and two isolated vertices end the id range."""
    h = len(CLASS_DEGREES)
    hubs = list(range(h))
    edges, pool = [], 0
    for i, d in enumerate(CLASS_DEGREES):
        chain = [j for j in (i - 1, i + 1) if 0 <= j < h and d > 2 and CLASS_DEGREES[j] > 2]
        edges += [(i, j) for j in chain if j > i]
        edges += [(i, h + x) for x in range(d - len(chain))]
        pool = max(pool, d - len(chain))
    return np.array(edges, dtype=np.int64), h + pool + 2, hubs


def star_edges(leaves):
    return np.stack([np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1)], axis=1)


def csr_of(edges, n):
    """symmetric CSR with ascending rows from an edge list (numpy only)"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    both = np.concatenate([e, e[:, ::-1]])
    both = np.unique(both[both[:, 0] != both[:, 1]], axis=0)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(both[:, 0], minlength=n), out=off[1:])
    return off, both[:, 1].copy()


# ---- the goldens --------------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_complete():
    want = {"file_eppsteinExample", "file_micro", "file_smallRandom1", "file_tomitaExample", "file_triangles_1", "file_triangles_3",
            "kronecker_10_16", "kronecker_12_16", "uniform_10_16", "kronecker_10_16_raw"}
    assert set(GRAPHS) == want
    assert all(g["n"] <= 4096 for g in GRAPHS.values())
    assert os.path.getsize(os.path.join(GOLDEN, "pagerank.npz")) < 512 * 1024
    for key in want:
        recs = [r for r in RECORDS if r["graph"] == key]
        assert {r["flags"] for r in recs} >= {0, PR_DANGLING, PR_FLOAT32} and {r["teleport"] for r in recs} == set(TELEPORTS)
        assert any(r["reference"] for r in recs)   # the compiled reference was compared on every graph
        for r in recs:
            assert r["array"] in ARR.files and len(r["top"]) == min(5, GRAPHS[key]["n"])
            assert r["reference"] <= (r["damping"] == 0.85 and r["teleport"] == "uniform" and not r["flags"] & PR_DANGLING)
    assert any(r["converged"] for r in RECORDS) and any(not r["converged"] for r in RECORDS)
    assert any(GRAPHS[r["graph"]]["isolated"] > 0 and r["flags"] & PR_DANGLING for r in RECORDS)


@pytest.mark.parametrize("rec", RECORDS, ids=rec_id)
def test_restatement_reproduces_the_golden(capi, rec):
    csr = golden_csr(capi, rec["graph"])
    off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int64)
    g = GRAPHS[rec["graph"]]
    assert (off.size - 1, adj.size, int(np.diff(off).max()), int((np.diff(off) == 0).sum())) == (g["n"], g["nnz"], g["max_degree"], g["isolated"])
    # the record holds the float64 restatement, whatever its flags' storage type: the device's float32 runs are held to it by the float bound
    scores, info, errors = pagerank_np(off, adj, rec["damping"], rec["max_iters"], rec["tolerance"], teleport_of(rec["teleport"], off),
                                       dangling=bool(rec["flags"] & PR_DANGLING))
    assert scores.tobytes() == ARR[rec["array"]].tobytes()
    for k in ("iterations", "converged", "argmax"):
        assert info[k] == rec[k], k
    assert top_five(scores) == rec["top"] and info["error"] == rec["error"] and info["sum"] == rec["sum"]
    # (c) of tools/make_golden_pagerank.py: no sweep's error is near the tolerance, so the iteration count is a fact (tolerance 0 stops no run)
    bound = record_bound(rec, k=rec["max_iters"])
    assert rec["tolerance"] == 0 or all(abs(e - rec["tolerance"]) > 4.0 * scalar_bound(bound, g["n"], e) for e in errors)
    if rec["flags"] & PR_FLOAT32:   # … and the float32 restatement stops at the same sweep and lies within the bound
        s32, i32, _ = pagerank_np(off, adj, rec["damping"], rec["max_iters"], rec["tolerance"], teleport_of(rec["teleport"], off),
                                  dangling=bool(rec["flags"] & PR_DANGLING), float32=True)
        assert i32["iterations"] == rec["iterations"] and np.abs(s32 - scores).sum() <= record_bound(rec)
        assert np.array_equal(s32, s32.astype(np.float32).astype(np.float64))


# ---- closed forms of the restatement ----------------------------------------------------------------------------------------------------------
def test_closed_forms():
    n = 64
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    for edges, nn in ((ring, n), ([(i, j) for i in range(12) for j in range(i)], 12)):
        off, adj = csr_of(edges, nn)
        for k in (1, 20):
            s, info, _ = pagerank_np(off, adj, max_iters=k, tolerance=0)
            assert np.abs(s - 1.0 / nn).sum() <= pr_bound(k, 0.85, int(np.diff(off).max()), EPS) and info["iterations"] == k
    leaves, d = 500, 0.85
    off, adj = csr_of(star_edges(leaves), leaves + 1)
    s, info, _ = pagerank_np(off, adj, max_iters=10000, tolerance=1e-12)
    b = (1 - d) / (leaves + 1)
    hub = b * (1 + d * leaves) / (1 - d * d)
    assert info["converged"] and abs(s[0] - hub) < 1e-11 and np.all(np.abs(s[1:] - (b + d * hub / leaves)) < 1e-11)
    assert residual_np(off, adj, s) < 1e-11
    # isolated vertices: the default drops their mass, `dangling` hands it back
    off, adj = csr_of([(0, 1), (1, 2), (0, 2)], 5)
    s, info, _ = pagerank_np(off, adj, max_iters=30, tolerance=0)
    assert np.all(s[3:] == (1 - d) * 0.2) and info["sum"] < 1 and info["isolated"] == 2
    s, info, _ = pagerank_np(off, adj, max_iters=30, tolerance=0, dangling=True)
    assert abs(info["sum"] - 1) <= pr_bound(30, d, 2, EPS, isolated=2)
    # a personalised walk reaches distance k after k sweeps
    off, adj = csr_of([(i, i + 1) for i in range(9)], 10)
    t = np.zeros(10)
    t[0] = 2.5
    s, _, _ = pagerank_np(off, adj, max_iters=4, tolerance=0, teleport=t)
    assert np.all(s[:5] > 0) and np.all(s[5:] == 0)
    assert pagerank_np(off, adj, max_iters=0)[0].tobytes() == np.full(10, 0.1).tobytes()
    assert pr_bound(5, 1.0, 3, EPS) == 2 * 5 * 6 * EPS * 1.01 and pr_bound(0, 0.85, 3, EPS) == 0.0


def test_class_probe_graph_has_every_class_boundary():
    edges, n, hubs = class_probe_graph()
    off, _ = csr_of(edges, n)
    deg = np.diff(off)
    assert deg[hubs].tolist() == CLASS_DEGREES and int((deg == 0).sum()) == 2
    assert int(deg.max()) == 2 * K_CHUNK + 1 and len(edges) == len(np.unique(np.sort(edges, axis=1), axis=0))


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_exported(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_pagerank", "gmsx_pagerank_residual"):
        assert name in capi.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    for name in ("GMSX_PR_DEFAULT = 0", "GMSX_PR_DANGLING = 1", "GMSX_PR_FLOAT32 = 2", "gmsx_pagerank_info"):
        assert name in hdr
    assert ctypes.sizeof(capi.PagerankInfo) == 48 and (capi.PR_DANGLING, capi.PR_FLOAT32) == (PR_DANGLING, PR_FLOAT32)
    assert capi.lib().gmsx_version() == 320
    src = open(os.path.join(ROOT, "gms_amd", "csrc", "hip", "pagerank.hip")).read()
    for text in ("kPrLaneRow = %d" % K_LANE_ROW, "kPrGroupRow = %d" % K_GROUP_ROW, "kPrChunk = %d" % K_CHUNK, "THE RULE"):
        assert text in src


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a GPU-less host")
def test_entry_points_fail_loudly_without_gpu(capi):
    L = capi.lib()
    scores = np.full(4, -77.0)
    info, res = capi.PagerankInfo(), ctypes.c_double(-5.0)
    ctypes.memset(ctypes.byref(info), 0x5a, ctypes.sizeof(info))
    before = bytes(info)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(1 << 16)))  # never read: the calls check the device before the handle
    assert L.gmsx_pagerank(fake, 0.85, 20, 1e-4, None, 0, p(scores), ctypes.byref(info), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_pagerank_residual(fake, p(scores), 0.85, None, 0, ctypes.byref(res), None) == capi.ERR_NO_DEVICE
    assert L.gmsx_pagerank(None, 0.85, 20, 1e-4, None, 0, p(scores), ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_pagerank(fake, 0.85, 20, 1e-4, None, 0, p(scores), None, None) == capi.ERR_INVALID
    for damping, iters, tol, flags in ((1.5, 20, 1e-4, 0), (-0.1, 20, 1e-4, 0), (float("nan"), 20, 1e-4, 0), (0.85, -1, 1e-4, 0), (0.85, 20, -1e-4, 0),
                                       (0.85, 20, float("nan"), 0), (0.85, 20, 1e-4, 4)):
        assert L.gmsx_pagerank(fake, damping, iters, tol, None, flags, p(scores), ctypes.byref(info), None) == capi.ERR_INVALID
    assert L.gmsx_pagerank_residual(fake, p(scores), 0.85, None, 0, None, None) == capi.ERR_INVALID
    assert L.gmsx_pagerank_residual(fake, p(scores), 2.0, None, 0, ctypes.byref(res), None) == capi.ERR_INVALID
    assert L.gmsx_pagerank_residual(fake, p(scores), 0.85, None, 8, ctypes.byref(res), None) == capi.ERR_INVALID
    assert np.all(scores == -77.0) and bytes(info) == before and res.value == -5.0
