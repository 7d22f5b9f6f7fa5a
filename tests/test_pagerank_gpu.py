"""GPU: gmsx_pagerank and gmsx_pagerank_residual through the C-ABI against the goldens (tests/golden/pagerank.{json,npz}), against the numpy
restatement of tests/test_pagerank_golden_cpu.py and against closed forms.  Distances are L1 and held to pr_bound (derived in that module);
every test prints its largest distance / bound.

  goldens        every record: iterations, converged, argmax and the top five equal; scores, error and sum within the bound
  larger         kronecker 16 (a row of degree 9 869: three chunks) against the restatement, in both storage types
  classes        one graph with a row on either side of every class threshold and of the chunk size: against the restatement, and
                 gmsx_pagerank_residual of the result of 200 sweeps at tolerance 1e-13
  closed forms   a cycle on 4096 vertices and K_130 after 1 and 20 sweeps; a star with 70 000 leaves iterated to 1e-12
  personalised   teleport on one end of a 64-path: +0.0 beyond distance k; an unnormalised teleport gives the bytes of its normalised form
  isolated       two cliques and isolated vertices, an edgeless graph, n = 1, n = 0, with and without GMSX_PR_DANGLING
  stopping       max_iters = 0, tolerance = 0, damping = 0 and damping = 1
  same bytes     three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, a second handle
  contract       every GMSX_ERR_INVALID case, untouched arrays, info alone, stats"""
import ctypes as C

import numpy as np
import pytest

from conftest import edges_to_csr, host_graph
from test_pagerank_golden_cpu import (ARR, EPS, GRAPHS, PR_DANGLING, PR_FLOAT32, RECORDS, class_probe_graph, csr_of, golden_csr, pagerank_np, pr_bound,
                                      rec_id, record_bound, residual_np, scalar_bound, star_edges, teleport_of, top_five)

pytestmark = pytest.mark.gpu

_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        _GRAPHS[key] = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    return _GRAPHS[key]


def within(name, got, want, bound):
    """the L1 distance of two score arrays against its bound, printed before it is asserted"""
    dist = float(np.abs(np.asarray(got) - np.asarray(want)).sum())
    print(f"{name}: L1 distance {dist:.3e}, bound {bound:.3e}, distance / bound {dist / bound if bound > 0 else 0.0:.3f}")
    assert dist <= bound, (name, dist, bound)


def is_float(a):
    return np.array_equal(a, a.astype(np.float32).astype(np.float64))


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", RECORDS, ids=rec_id)
def test_equals_the_golden(gpu, rec):
    g, meta = device_graph(gpu, rec["graph"]), GRAPHS[rec["graph"]]
    csr = golden_csr(gpu, rec["graph"])
    teleport = teleport_of(rec["teleport"], np.asarray(csr.offsets(), dtype=np.int64))
    scores, info, st = g.pagerank(rec["damping"], rec["max_iters"], rec["tolerance"], teleport, dangling=bool(rec["flags"] & PR_DANGLING),
                                  float32=bool(rec["flags"] & PR_FLOAT32), stats=True)
    want = ARR[rec["array"]]
    assert (info["iterations"], info["converged"], info["argmax"]) == (rec["iterations"], rec["converged"], rec["argmax"])
    assert top_five(scores) == rec["top"]
    bound = record_bound(rec)
    within(rec_id(rec), scores, want, bound)
    n = meta["n"]
    assert abs(info["error"] - rec["error"]) <= scalar_bound(bound, n, rec["error"])
    assert abs(info["sum"] - rec["sum"]) <= scalar_bound(bound, n, rec["sum"])
    assert info["max_score"] == scores[info["argmax"]] == scores.max() and info["isolated"] == meta["isolated"]
    assert st["units"] == rec["iterations"] * meta["nnz"] and st["probes"] == rec["iterations"] and st["launches"] >= 2 * rec["iterations"]
    if rec["flags"] & PR_FLOAT32:
        assert is_float(scores)


# ---- 2. a larger graph ------------------------------------------------------------------------------------------------------------------
_BIG = {}


def big(gpu):
    """kronecker 16: (handle, off, adj, the float64 restatement at the reference's arguments), computed once"""
    if not _BIG:
        csr = host_graph(gpu, "kronecker", 16)
        off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int64)
        _BIG["v"] = (gpu.DeviceGraph.from_csr(csr), off, adj, pagerank_np(off, adj))
    return _BIG["v"]


@pytest.mark.parametrize("float32", [False, True])
def test_kronecker_16(gpu, float32):
    g, off, adj, (want, winfo, errors) = big(gpu)
    deg = np.diff(off)
    n, dmax = deg.size, int(deg.max())
    assert dmax == 9869
    bound = pr_bound(winfo["iterations"], 0.85, dmax, EPS, float32=float32)
    # the iteration count is a fact: no sweep's error of the restatement is near the tolerance
    assert all(abs(e - 1e-4) > 4.0 * scalar_bound(pr_bound(20, 0.85, dmax, EPS, float32=float32), n, e) for e in errors)
    scores, info = g.pagerank(float32=float32)
    assert (info["iterations"], info["converged"], info["argmax"]) == (winfo["iterations"], 1, winfo["argmax"]) and top_five(scores) == top_five(want)
    within("kronecker_16_16 float32=%s" % float32, scores, want, bound)
    assert abs(info["error"] - winfo["error"]) <= scalar_bound(bound, n, winfo["error"]) and abs(info["sum"] - winfo["sum"]) <= scalar_bound(bound, n, 1.0)
    assert info["isolated"] == int((deg == 0).sum()) and (is_float(scores) or not float32)
    res = g.pagerank_residual(scores, float32=float32)
    want_res = residual_np(off, adj, scores, float32=float32)
    assert abs(res - want_res) <= scalar_bound(pr_bound(1, 0.85, dmax, EPS, float32=float32), n, want_res) and res < 1e-4   # PRVerifier's rule


# ---- 3. the classes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dangling,float32", [(False, False), (True, False), (False, True), (True, True)])
def test_every_class_boundary(gpu, dangling, float32):
    edges, n, hubs = class_probe_graph()
    off, adj = csr_of(edges, n)
    deg = np.diff(off)
    dmax, iso = int(deg.max()), int((deg == 0).sum())
    key = ("probe",)
    if key not in _GRAPHS:
        _GRAPHS[key] = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=n))
    g = _GRAPHS[key]
    teleport = (deg + 1).astype(np.float64)   # (the hubs' scores differ from each other and from the leaves')
    for k in (1, 20):
        want, winfo, _ = pagerank_np(off, adj, max_iters=k, tolerance=0, teleport=teleport, dangling=dangling)
        scores, info = g.pagerank(max_iters=k, tolerance=0, teleport=teleport, dangling=dangling, float32=float32)
        bound = pr_bound(k, 0.85, dmax, EPS, float32=float32, isolated=iso if dangling else None)
        within("classes k=%d dangling=%s float32=%s" % (k, dangling, float32), scores, want, bound)
        assert info["iterations"] == k and info["argmax"] == winfo["argmax"] and info["isolated"] == iso
        assert abs(info["error"] - winfo["error"]) <= scalar_bound(bound, n, winfo["error"])
    # a fixed point of the device's own sweep: 200 sweeps reach 1e-13 (0.85^200 = 8e-15), and one more sweep moves the result by less
    tol = 1e-13 if not float32 else 1e-6
    scores, info = g.pagerank(max_iters=200, tolerance=tol, teleport=teleport, dangling=dangling, float32=float32)
    assert info["converged"] == 1
    res = g.pagerank_residual(scores, teleport=teleport, dangling=dangling, float32=float32)
    one = pr_bound(1, 0.85, dmax, EPS, float32=float32, isolated=iso if dangling else None)
    want_res = residual_np(off, adj, scores, teleport=teleport, dangling=dangling, float32=float32)
    print(f"classes: residual {res:.3e}, restated {want_res:.3e}, last error {info['error']:.3e}")
    assert abs(res - want_res) <= scalar_bound(one, n, want_res)
    assert res <= info["error"] + scalar_bound(one, n, info["error"])   # (the map contracts: the next sweep moves less than the last)


# ---- 4. closed forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cycle", "complete"])
def test_regular_graphs_keep_the_uniform_vector(gpu, shape):
    if shape == "cycle":
        n = 4096
        ids = np.random.RandomState(5).permutation(n)
        edges = np.stack([ids, np.roll(ids, 1)], axis=1)
    else:
        n = 130
        edges = [(i, j) for i in range(n) for j in range(i)]
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=n))
    dmax = 2 if shape == "cycle" else n - 1
    for float32 in (False, True):
        for k in (1, 20):
            scores, info = g.pagerank(max_iters=k, tolerance=0, float32=float32)
            within("%s k=%d float32=%s" % (shape, k, float32), scores, np.full(n, 1.0 / n), pr_bound(k, 0.85, dmax, EPS, float32=float32))
            assert info["iterations"] == k and info["argmax"] == 0 and info["isolated"] == 0   # (every score is the same: the smallest id)
    g.free()


def test_star_of_70000_leaves(gpu):
    L, d = 70000, 0.85
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, star_edges(L), n=L + 1))
    tol = 1e-12
    scores, info = g.pagerank(damping=d, max_iters=1000, tolerance=tol)
    assert info["converged"] == 1 and info["argmax"] == 0 and 100 < info["iterations"] < 1000
    b = (1 - d) / (L + 1)
    hub = b * (1 + d * L) / (1 - d * d)
    want = np.full(L + 1, b + d * hub / L)
    want[0] = hub
    # the computed sweeps stay within pr_bound of the exact ones, and the exact iterate whose step is below tol lies within tol d / (1 - d) of the fixed point
    within("star", scores, want, pr_bound(info["iterations"], d, L, EPS) + tol * d / (1 - d))
    assert np.all(scores[1:] == scores[1])   # (every leaf is computed by the same operations)
    g.free()


# ---- 5. personalised --------------------------------------------------------------------------------------------------------------------------
def test_personalised_path(gpu):
    n = 64
    ids = np.random.RandomState(9).permutation(n)   # ids[p] = the vertex at position p of the path
    edges = np.stack([ids[:-1], ids[1:]], axis=1)
    off, adj = csr_of(edges, n)
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=n))
    teleport = np.zeros(n)
    teleport[ids[0]] = 5.0
    for float32 in (False, True):
        for k in (0, 1, 7, 63):
            scores, info = g.pagerank(max_iters=k, tolerance=0, teleport=teleport, float32=float32)
            far = scores[ids[k + 1:]]
            assert np.all(far == 0.0) and not np.signbit(far).any() and np.all(scores[ids[:k + 1]] > 0)
            want = pagerank_np(off, adj, max_iters=k, tolerance=0, teleport=teleport)[0]
            if k > 0:
                within("path k=%d float32=%s" % (k, float32), scores, want, pr_bound(k, 0.85, 2, EPS, float32=float32))
            else:
                assert scores.tobytes() == want.tobytes()
    # an unnormalised vector and its normalised form (exact: the weights are dyadic and add up to 8)
    w = np.zeros(n)
    w[[3, 17, 40]] = (4.0, 3.0, 1.0)
    a, b = g.pagerank(teleport=w), g.pagerank(teleport=w / 8.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    ones = g.pagerank(teleport=np.full(n, 7.0))
    uniform = g.pagerank()
    assert ones[0].tobytes() == uniform[0].tobytes() and ones[1] == uniform[1]
    g.free()


# ---- 6. isolated vertices ---------------------------------------------------------------------------------------------------------------------
def test_isolated_vertices(gpu):
    a, b, d = 70, 9, 0.85   # vertices 0 .. 69 and 70 .. 78 are cliques, 79 .. 83 isolated
    edges = [(i, j) for i in range(a) for j in range(i)] + [(a + i, a + j) for i in range(b) for j in range(i)]
    n = a + b + 5
    off, adj = csr_of(edges, n)
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=n))
    teleport = np.arange(1, n + 1, dtype=np.float64)
    t = teleport / teleport.sum()
    for tp, tn in ((None, np.full(n, 1.0 / n)), (teleport, t)):
        scores, info = g.pagerank(damping=d, max_iters=20, tolerance=0, teleport=tp)
        assert scores[a + b:].tobytes() == ((1.0 - d) * tn[a + b:]).tobytes() and info["isolated"] == 5 and info["sum"] < 1.0
        within("isolated, default", scores, pagerank_np(off, adj, d, 20, 0, tp)[0], pr_bound(20, d, a - 1, EPS))
        for float32 in (False, True):
            scores, info = g.pagerank(damping=d, max_iters=20, tolerance=0, teleport=tp, dangling=True, float32=float32)
            bound = pr_bound(20, d, a - 1, EPS, float32=float32, isolated=5)
            print(f"dangling float32={float32}: |sum - 1| = {abs(info['sum'] - 1.0):.3e}, bound {bound:.3e}")
            assert abs(info["sum"] - 1.0) <= scalar_bound(bound, n, 1.0) / 2
            within("isolated, dangling", scores, pagerank_np(off, adj, d, 20, 0, tp, dangling=True)[0], bound)
    g.free()
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=7))   # edgeless
    scores, info = g.pagerank()
    assert scores.tobytes() == np.full(7, (1.0 - 0.85) * (1.0 / 7)).tobytes() and (info["iterations"], info["converged"], info["argmax"]) == (2, 1, 0)
    assert info["error"] == 0.0 and info["isolated"] == 7
    scores, info = g.pagerank(dangling=True)
    within("edgeless, dangling", scores, np.full(7, 1.0 / 7), pr_bound(info["iterations"], 0.85, 0, EPS, isolated=7))
    assert g.pagerank_residual(np.full(7, (1.0 - 0.85) * (1.0 / 7))) == 0.0
    g.free()
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=1))
    scores, info = g.pagerank(max_iters=3, tolerance=0)
    assert scores.tolist() == [1.0 - 0.85] and (info["iterations"], info["argmax"], info["isolated"]) == (3, 0, 1)
    assert g.pagerank(max_iters=0)[0].tolist() == [1.0]
    g.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # n = 0
    scores, info = g.pagerank()
    assert scores.size == 0 and info == {"iterations": 0, "converged": 0, "argmax": -1, "error": 0.0, "sum": 0.0, "max_score": 0.0, "isolated": 0}
    assert g.pagerank_residual(np.zeros(0)) == 0.0
    g.free()


# ---- 7. stopping --------------------------------------------------------------------------------------------------------------------------------
def test_stopping_rules(gpu):
    key = "kronecker_10_16"
    g, meta = device_graph(gpu, key), GRAPHS[key]
    csr = golden_csr(gpu, key)
    off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int64)
    n = meta["n"]
    teleport = (np.diff(off) + 1).astype(np.float64)
    s = 0.0
    for x in teleport.tolist():
        s += x
    for tp, t in ((None, np.full(n, 1.0 / n)), (teleport, teleport / s)):
        scores, info = g.pagerank(max_iters=0, teleport=tp)
        assert scores.tobytes() == t.tobytes() and (info["iterations"], info["converged"], info["error"]) == (0, 0, 0.0)
        assert info["argmax"] == int(np.lexsort((np.arange(n), -t))[0]) and info["max_score"] == t.max()
        s32 = g.pagerank(max_iters=0, teleport=tp, float32=True)[0]
        assert s32.tobytes() == t.astype(np.float32).astype(np.float64).tobytes()
    for k in (1, 7, 33):
        scores, info = g.pagerank(max_iters=k, tolerance=0.0)
        assert (info["iterations"], info["converged"]) == (k, 0)
    # damping 0: one sweep gives t and moves nothing
    scores, info = g.pagerank(damping=0.0, teleport=teleport)
    assert scores.tobytes() == (teleport / s).tobytes() and (info["iterations"], info["converged"], info["error"]) == (1, 1, 0.0)
    # damping 1: no teleport at all; with GMSX_PR_DANGLING the mass stays 1
    want, winfo, _ = pagerank_np(off, adj, damping=1.0, max_iters=12, tolerance=0, dangling=True)
    scores, info = g.pagerank(damping=1.0, max_iters=12, tolerance=0, dangling=True)
    bound = pr_bound(12, 1.0, meta["max_degree"], EPS, isolated=meta["isolated"])
    within("damping 1", scores, want, bound)
    assert info["iterations"] == 12 and abs(info["sum"] - 1.0) <= scalar_bound(bound, n, 1.0) / 2


# ---- 8. same bytes ------------------------------------------------------------------------------------------------------------------------------
def test_same_bytes_in_every_variant(gpu):
    csr = host_graph(gpu, "kronecker", 12)
    g = gpu.DeviceGraph.from_csr(csr)
    variants = [("run 1", g), ("run 2", g), ("run 3", g), ("trusted", gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_TRUSTED)),
                ("hub limit 64", gpu.DeviceGraph.from_csr(csr, flags=64 << 8)), ("shard 1 of 4", gpu.DeviceGraph.from_csr(csr, shard=(1, 4))),
                ("second handle", gpu.DeviceGraph.from_csr(csr))]
    first = {}
    for name, h in variants:
        for dangling, float32 in ((False, False), (True, False), (False, True)):
            scores, info = h.pagerank(dangling=dangling, float32=float32)
            res = h.pagerank_residual(scores, dangling=dangling, float32=float32)
            got = (scores.tobytes(), tuple(sorted(info.items())), res)
            assert got == first.setdefault((dangling, float32), got), (name, dangling, float32)
        if h is not g:
            h.free()
    g.free()
    rec = next(r for r in RECORDS if r["graph"] == "kronecker_12_16" and r["flags"] == 0 and r["tolerance"] == 1e-4)
    assert dict(first[(False, False)][1])["iterations"] == rec["iterations"]


# ---- 9. contract --------------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    L = gpu.lib()
    csr = host_graph(gpu, "kronecker", 10)
    g = gpu.DeviceGraph.from_csr(csr)
    n = csr.num_nodes
    scores = np.full(n, -71.0)
    info, res = gpu.PagerankInfo(), C.c_double(-5.0)
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    before = bytes(info)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok_t = np.ones(n)
    run = lambda h=g._h, d=0.85, k=20, tol=1e-4, t=None, f=0, i=C.byref(info): L.gmsx_pagerank(h, d, k, tol, t, f, p(scores), i, None)  # noqa: E731
    assert run(h=None) == gpu.ERR_INVALID and run(i=None) == gpu.ERR_INVALID
    for d in (-0.01, 1.01, float("nan"), float("inf")):
        assert run(d=d) == gpu.ERR_INVALID
    assert run(k=-1) == gpu.ERR_INVALID and run(tol=-1e-9) == gpu.ERR_INVALID and run(tol=float("nan")) == gpu.ERR_INVALID
    for f in (4, 8, 1 << 31, 7):
        assert run(f=f) == gpu.ERR_INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        t = ok_t.copy()
        t[n // 2] = bad
        assert run(t=p(t)) == gpu.ERR_INVALID
    assert run(t=p(np.zeros(n))) == gpu.ERR_INVALID
    call = lambda h=g._h, s=p(scores), d=0.85, t=None, f=0, r=C.byref(res): L.gmsx_pagerank_residual(h, s, d, t, f, r, None)  # noqa: E731
    assert call(h=None) == gpu.ERR_INVALID and call(r=None) == gpu.ERR_INVALID and call(s=None) == gpu.ERR_INVALID
    assert call(d=1.5) == gpu.ERR_INVALID and call(d=float("nan")) == gpu.ERR_INVALID and call(f=4) == gpu.ERR_INVALID
    assert call(t=p(np.zeros(n))) == gpu.ERR_INVALID and call(t=p(-ok_t)) == gpu.ERR_INVALID
    assert np.all(scores == -71.0) and bytes(info) == before and res.value == -5.0
    # info alone
    assert L.gmsx_pagerank(g._h, 0.85, 20, 1e-4, None, 0, None, C.byref(info), None) == 0
    want, winfo = g.pagerank()
    assert info.as_dict() == winfo and info.reserved == 0 and np.all(scores == -71.0)
    # the edges of the ranges are valid
    assert run(d=0.0) == 0 and run(d=1.0) == 0 and run(k=0) == 0 and run(tol=0.0, k=1) == 0
    _, _, st = g.pagerank(stats=True)
    assert st["units"] == winfo["iterations"] * csr.nnz and st["probes"] == winfo["iterations"] and st["kernel_ms"] > 0 and st["setup_ms"] > 0
    assert st["launches"] >= 3 * winfo["iterations"] and st["alg_elements"] == 0 and st["stream_bytes"] == 0
    r, st = g.pagerank_residual(want, stats=True)
    assert 0 <= r < 1e-4 and st["units"] == csr.nnz and st["probes"] == 1
    with pytest.raises(ValueError):
        g.pagerank(teleport=np.ones(n + 1))
    assert L.gmsx_version() == 320
    g.free()
