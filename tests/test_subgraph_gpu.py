"""GPU tests of subgraph matching (gmsx_subgraph_match; the device counterpart of the reference's VF2): every list against the goldens of
tools/make_golden_subgraph.py (the reference's sequential VF2 mapping, a plain enumerator's counts and hashes) and a vectorised host checker
— every row injective, every pattern edge a target arc, in INDUCED mode every pattern non-edge a non-arc, rows strictly ascending in the
matching order (hence distinct), count and sha256 equal to the golden or to a closed form: together that is the whole list."""
import ctypes as C
import hashlib
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, edges_to_csr, host_graph, load_golden

pytestmark = pytest.mark.gpu

GOLD = load_golden("subgraph.json")
PATTERNS = {k: [tuple(e) for e in v] for k, v in GOLD["patterns"].items()}
RECORDS = {}
for _r in GOLD["records"]:
    RECORDS.setdefault(_r["graph"], []).append(_r)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def target_csr(gpu, key):
    src = GOLD["graphs"][key]
    if src["kind"] == "file":
        return gpu.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]), relabel=gpu.RELABEL_NEVER)
    if src["kind"] == "edges":
        return edges_to_csr(gpu, src["edges"], src["n"])
    return host_graph(gpu, src["generator"], src["scale"], src["degree"], src["relabel"])


def dense(csr):
    o, a = np.array(csr.offsets()), np.array(csr.neighbors())
    n = o.size - 1
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), np.diff(o)), a] = True
    return A


def pattern_matrix(edges):
    k = max(max(e) for e in edges) + 1 if edges else 1
    P = np.zeros((k, k), dtype=bool)
    for a, b in edges:
        P[a, b] = P[b, a] = True
    return P


def sha(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, dtype="<i4").tobytes()).hexdigest()


def check_list(A, edges, order, rows, induced):
    """the host checker: every property of the list but its length"""
    P = pattern_matrix(edges)
    k, n, E = P.shape[0], A.shape[0], rows.shape[0]
    assert rows.shape == (E, k) and rows.dtype == np.int32
    if E == 0:
        return
    assert np.all((rows >= 0) & (rows < n))
    if k > 1:
        s = np.sort(rows, axis=1)
        assert np.all(s[:, 1:] > s[:, :-1]), "a row is not injective"
    for a in range(k):
        for b in range(a + 1, k):
            hit = A[rows[:, a], rows[:, b]]
            if P[a, b]:
                assert np.all(hit), f"pattern edge {a}-{b} is not an arc of some row"
            elif induced:
                assert not np.any(hit), f"pattern non-edge {a}-{b} is an arc of some row"
    keys = rows[:, list(order)].astype(np.int64)
    ne = keys[1:] != keys[:-1]
    assert np.all(ne.any(axis=1)), "a row is listed twice"
    col = ne.argmax(axis=1)
    idx = np.arange(E - 1)
    assert np.all(keys[1:][idx, col] > keys[:-1][idx, col]), "rows are not ascending in the matching order"


def listed(g, A, edges, induced, want=None, **kw):
    rows, st = g.subgraph_match(edges, induced=induced, stats=True, **kw)
    order = st["info"]["order"]
    assert st["info"]["embeddings"] == rows.shape[0] and st["info"]["k"] == rows.shape[1]
    check_list(A, edges, order, rows, induced)
    if want is not None:
        assert rows.shape[0] == want, (rows.shape[0], want)
    return rows


def hub_graph(width, p, seed):
    """vertex 0 adjacent to 1 .. width, plus a seeded sparse G(width, p) among the rest"""
    r = np.random.RandomState(seed).random_sample((width + 1, width + 1))
    return [(0, v) for v in range(1, width + 1)] + [(a, b) for a in range(1, width + 1) for b in range(a + 1, width + 1) if r[a, b] < p]


def closed_forms(A):
    d = A.sum(axis=1).astype(np.int64)
    M = A.astype(np.int64)
    T = int(np.trace(M @ M @ M)) // 6
    return {"mono_claw": int((d * (d - 1) * (d - 2)).sum()), "mono_P3": int((d * (d - 1)).sum()), "ind_P3": int((d * (d - 1)).sum()) - 6 * T,
            "K3": 6 * T}


def cycle(n):
    return [(i, (i + 1) % n) for i in range(n)]


def path(vs):
    return [(vs[i], vs[i + 1]) for i in range(len(vs) - 1)]


def clique(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


# ---- 1. the goldens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(RECORDS))
def test_subgraph_goldens(gpu, key):
    csr = target_csr(gpu, key)
    assert (csr.num_nodes, csr.nnz) == (GOLD["graphs"][key]["n"], GOLD["graphs"][key]["nnz"])
    A = dense(csr)
    g = gpu.DeviceGraph.from_csr(csr)
    seen = 0
    for rec in RECORDS[key]:
        edges = PATTERNS[rec["pattern"]]
        assert gpu.subgraph_order(edges).tolist() == rec["order"]
        for mode, induced in (("induced", True), ("mono", False)):
            ent = rec[mode]
            if ent["count"] is None:  # the golden has no list of this size (make_golden_subgraph.py: LIST_LIMIT); FIRST is tested below
                continue
            info = g.subgraph_match_info(edges, induced=induced)
            assert (info["embeddings"], info["k"], info["order"]) == (ent["count"], len(rec["order"]), rec["order"]), (rec["pattern"], mode)
            rows = listed(g, A, edges, induced, want=ent["count"])
            assert sha(rows) == ent["sha256"], (rec["pattern"], mode)
            assert (rows[0].tolist() if rows.shape[0] else None) == ent["row0"]
            if induced:
                assert ent["row0"] == rec["ref"]  # the reference's sequential VF2, element for element
            seen += 1
    assert seen == sum(rec[mode]["count"] is not None for rec in RECORDS[key] for mode in ("induced", "mono")) >= 10
    g.free()


# ---- 2. chunk boundaries --------------------------------------------------------------------------------------------------------------
def test_subgraph_hub_rows(gpu):
    edges = hub_graph(199, 0.03, 7)
    csr = edges_to_csr(gpu, edges, 200)
    A = dense(csr)
    assert A[0].sum() == 199  # chunks of 64, 64, 64, 7
    cf = closed_forms(A)
    g = gpu.DeviceGraph.from_csr(csr)
    assert listed(g, A, PATTERNS["K3"], True).shape[0] == listed(g, A, PATTERNS["K3"], False).shape[0] == cf["K3"] > 0
    assert listed(g, A, PATTERNS["claw"], False).shape[0] == cf["mono_claw"]
    assert listed(g, A, PATTERNS["P3"], False).shape[0] == cf["mono_P3"]
    assert listed(g, A, PATTERNS["P3"], True).shape[0] == cf["ind_P3"]
    claw = listed(g, A, PATTERNS["claw"], True)
    assert 0 < claw.shape[0] < cf["mono_claw"]
    paw_i, paw_m = listed(g, A, PATTERNS["paw"], True), listed(g, A, PATTERNS["paw"], False)
    # MONO paw: a triangle (0, 1, 2) in order and a further neighbour of 2 outside it
    M = A.astype(np.int64)
    d = M.sum(axis=1)
    tri_at = (M @ M * M).sum(axis=1)  # ordered (a, b) pairs closing a triangle with the vertex
    assert paw_m.shape[0] == int((tri_at * (d - 2)).sum()) and 0 < paw_i.shape[0] < paw_m.shape[0]
    g.free()


@pytest.mark.parametrize("width", [63, 64, 65])
def test_subgraph_longest_row_at_a_chunk_boundary(gpu, width):
    csr = edges_to_csr(gpu, hub_graph(width, 0.1, width), width + 1)
    A = dense(csr)
    assert A.sum(axis=1).max() == width
    cf = closed_forms(A)
    g = gpu.DeviceGraph.from_csr(csr)
    assert listed(g, A, PATTERNS["K3"], True).shape[0] == cf["K3"] > 0
    assert listed(g, A, PATTERNS["P3"], False).shape[0] == cf["mono_P3"]
    assert listed(g, A, PATTERNS["P3"], True).shape[0] == cf["ind_P3"]
    assert listed(g, A, PATTERNS["claw"], False).shape[0] == cf["mono_claw"]
    listed(g, A, PATTERNS["paw"], True)
    listed(g, A, PATTERNS["diamond"], True)
    g.free()


# ---- 3. closed forms against the existing entry points --------------------------------------------------------------------------------
def test_subgraph_counts_against_other_entry_points(gpu):
    csr = host_graph(gpu, "kronecker", 10, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    for induced in (True, False):
        assert g.subgraph_match_info(PATTERNS["K3"], induced=induced)["embeddings"] == 6 * g.tc_total()
        assert g.subgraph_match_info(PATTERNS["K4"], induced=induced)["embeddings"] == g.kclique_count(4)[0]
    A = dense(csr).astype(np.float64)  # (exact: every entry of A² is below 2^53)
    c = (A @ A).astype(np.int64)
    np.fill_diagonal(c, 0)
    assert g.subgraph_match_info(PATTERNS["C4"], induced=False)["embeddings"] == int((c * (c - 1)).sum())
    g.free()
    csr = host_graph(gpu, "kronecker", 8, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    assert g.subgraph_match_info(PATTERNS["K5"])["embeddings"] == g.kclique_count(5)[0] > 0
    Ad = dense(csr)
    for k in (3, 4):
        rows = listed(g, Ad, clique(k), True)
        want = g.kclique_star_list(k, cliques_only=True)[0]
        assert rows.shape[0] == math.factorial(k) * want.shape[0]
        got = np.unique(np.sort(rows, axis=1), axis=0)
        assert np.array_equal(got, want[np.lexsort(want[:, ::-1].T)])
    g.free()


# ---- 4. depth -------------------------------------------------------------------------------------------------------------------------
def test_subgraph_depth(gpu):
    p32 = path(list(range(32)))
    mid = list(range(1, 17)) + [0] + list(range(17, 32))  # the same path, vertex 0 in the middle
    p32_mid = path(mid)
    assert gpu.subgraph_order(p32_mid).tolist() != list(range(32))
    c40, c32 = edges_to_csr(gpu, cycle(40), 40), edges_to_csr(gpu, cycle(32), 32)
    g40, g32 = gpu.DeviceGraph.from_csr(c40), gpu.DeviceGraph.from_csr(c32)
    A40, A32 = dense(c40), dense(c32)
    for pat in (p32, p32_mid):
        for induced in (True, False):
            listed(g40, A40, pat, induced, want=80)
        listed(g32, A32, pat, False, want=64)
        listed(g32, A32, pat, True, want=0)
    g40.free()
    g32.free()
    k9 = edges_to_csr(gpu, clique(9), 9)
    g = gpu.DeviceGraph.from_csr(k9)
    listed(g, dense(k9), clique(8), True, want=362880)
    with pytest.raises(gpu.GmsxError) as ei:
        g.subgraph_match_info(path(list(range(33))))
    assert ei.value.status == gpu.ERR_UNSUPPORTED
    g.free()


# ---- 5. automorphisms -----------------------------------------------------------------------------------------------------------------
def test_subgraph_automorphisms(gpu):
    cube = [(a, a ^ (1 << b)) for a in range(8) for b in range(3) if a < a ^ (1 << b)]
    petersen = [tuple(e) for e in GOLD["graphs"]["petersen"]["edges"]]
    for edges, aut in ((petersen, 120), (PATTERNS["C5"], 10), (PATTERNS["K4"], 24), (PATTERNS["claw"], 6), (PATTERNS["P4"], 2), (cube, 48)):
        csr = edges_to_csr(gpu, edges)
        g = gpu.DeviceGraph.from_csr(csr)
        listed(g, dense(csr), edges, True, want=aut)
        g.free()


# ---- 6. relabelling -------------------------------------------------------------------------------------------------------------------
def test_subgraph_relabelled_patterns(gpu):
    r = np.random.RandomState(11).random_sample((30, 30))
    csr = edges_to_csr(gpu, [(a, b) for a in range(30) for b in range(a + 1, 30) if r[a, b] < 0.4], 30)
    A = dense(csr)
    g = gpu.DeviceGraph.from_csr(csr)
    for name in ("P4", "claw", "C4", "paw", "diamond", "K4"):
        for induced in (True, False):
            base = listed(g, A, PATTERNS[name], induced)
            base = base[np.lexsort(base[:, ::-1].T)]
            assert base.shape[0] > 0
            for perm in itertools.permutations(range(4)):
                q = [(perm[a], perm[b]) for a, b in PATTERNS[name]]
                rows = listed(g, A, q, induced, want=base.shape[0])  # sorted in its own matching order (check_list)
                back = rows[:, list(perm)]  # f(a) = g(perm[a])
                assert np.array_equal(back[np.lexsort(back[:, ::-1].T)], base), (name, perm)
    g.free()


# ---- 7. FIRST -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch_tasks", [None, 64])
def test_subgraph_first(gpu, launch_tasks):
    opts = {} if launch_tasks is None else {"SGM_LAUNCH_TASKS": launch_tasks}
    none_seen = 0
    for key in sorted(RECORDS):
        g = gpu.DeviceGraph.from_csr(target_csr(gpu, key))
        with gpu.options(**opts):
            for rec in RECORDS[key]:
                edges = PATTERNS[rec["pattern"]]
                for mode, induced in (("induced", True), ("mono", False)):
                    row0 = rec[mode]["row0"]
                    rows = g.subgraph_match(edges, induced=induced, first=True)
                    assert rows.tolist() == ([row0] if row0 is not None else []), (key, rec["pattern"], mode)
                    info = g.subgraph_match_info(edges, induced=induced, first=True)  # maps = NULL: existence only
                    assert info["embeddings"] == (0 if row0 is None else 1) and info["order"] == rec["order"]
                    none_seen += row0 is None
                assert rec["induced"]["row0"] == rec["ref"]
        g.free()
    assert none_seen > 0
    k5_uniform = next(r for r in RECORDS["uniform_8_8"] if r["pattern"] == "K5")
    assert k5_uniform["ref"] is None and k5_uniform["mono"]["row0"] is None


def test_subgraph_first_none_and_launches(gpu):
    bip = edges_to_csr(gpu, [(a, 6 + b) for a in range(6) for b in range(6)], 12)  # K_6,6: no triangle
    g = gpu.DeviceGraph.from_csr(bip)
    for induced in (True, False):
        assert g.subgraph_match(PATTERNS["K3"], induced=induced, first=True).shape == (0, 3)
        assert g.subgraph_match(clique(13), induced=induced, first=True).shape == (0, 13)  # k > n
        assert g.subgraph_match_info(clique(13), induced=induced)["embeddings"] == 0
    g.free()
    # the first embedding starts at vertex 0: one search launch and the single-task fill, where the listing's count pass needs many
    csr = target_csr(gpu, "gnp_48_50")
    g = gpu.DeviceGraph.from_csr(csr)
    rec = next(r for r in RECORDS["gnp_48_50"] if r["pattern"] == "house")
    assert rec["ref"][0] == 0
    with gpu.options(SGM_LAUNCH_TASKS=64):
        rows, st = g.subgraph_match(PATTERNS["house"], first=True, stats=True)
        assert rows.tolist() == [rec["ref"]] and st["fill"]["launches"] == 2
        _, st0 = g.subgraph_match_info(PATTERNS["house"], first=True, stats=True)
        assert st0["launches"] == 1
        info, st1 = g.subgraph_match_info(PATTERNS["house"], stats=True)
        assert st1["launches"] == -(-info["tasks"] // 64) > 2 and st1["units"] == info["tasks"]
    g.free()


# ---- 8. launch splits -----------------------------------------------------------------------------------------------------------------
def test_subgraph_launch_splits(gpu):
    g = gpu.DeviceGraph.from_csr(target_csr(gpu, "gnp_48_50"))
    for name in ("house", "C5"):
        want = g.subgraph_match(PATTERNS[name])
        assert want.shape[0] > 0
        for per in (1, 7, 64):
            with gpu.options(SGM_LAUNCH_TASKS=per):
                got, st = g.subgraph_match(PATTERNS[name], stats=True)
            assert got.tobytes() == want.tobytes(), (name, per)
            assert st["sizing"]["launches"] == -(-st["info"]["tasks"] // per)
    g.free()


# ---- 9. shards ------------------------------------------------------------------------------------------------------------------------
def test_subgraph_shards(gpu):
    csr = target_csr(gpu, "kronecker_8_8")
    g = gpu.DeviceGraph.from_csr(csr)
    g_shard = gpu.DeviceGraph.from_csr(csr, shard=(1, 2))
    for name in ("paw", "C5"):
        whole, st = g.subgraph_match(PATTERNS[name], stats=True)
        order = st["info"]["order"]
        assert whole.shape[0] > 0
        assert g_shard.subgraph_match(PATTERNS[name]).tobytes() == whole.tobytes()  # a sharded upload: the same bytes
        for nparts in (2, 3, 8):
            parts = [g.subgraph_match(PATTERNS[name], part=p, nparts=nparts) for p in range(nparts)]
            assert sum(p.shape[0] for p in parts) == whole.shape[0]
            firsts = [set(np.unique(p[:, order[0]]).tolist()) for p in parts]
            assert all(firsts[i].isdisjoint(firsts[j]) for i in range(nparts) for j in range(i + 1, nparts))
            assert gpu.merge_subgraph_matches(parts, order).tobytes() == whole.tobytes()
            assert [g.subgraph_match_info(PATTERNS[name], part=p, nparts=nparts)["embeddings"] for p in range(nparts)] == [p.shape[0] for p in parts]
    g.free()
    g_shard.free()


# ---- 10. protocol ---------------------------------------------------------------------------------------------------------------------
def test_subgraph_protocol(gpu):
    lib = gpu.lib()
    csr = target_csr(gpu, "gnp_48_15")
    A = dense(csr)
    g = gpu.DeviceGraph.from_csr(csr)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    paw = gpu.pattern_arrays(PATTERNS["paw"])
    dia = gpu.pattern_arrays(PATTERNS["diamond"])  # the same k, other arrays
    k = 4
    want = g.subgraph_match(PATTERNS["paw"])
    ne = want.shape[0]
    assert ne > 1 and g.subgraph_match(PATTERNS["paw"]).tobytes() == want.tobytes()  # two runs are byte-identical
    info, st = gpu.SubgraphInfo(), gpu.Stats()

    def call(p, flags, part, nparts, buf, cap, infop=info, stp=None):
        return lib.gmsx_subgraph_match(g._h, p[0].size - 1, vp(p[0]), vp(p[1]), flags, part, nparts, None if buf is None else vp(buf), cap,
                                       None if infop is None else C.byref(infop), None if stp is None else C.byref(stp))

    # a too small capacity: ERR_INVALID, info holds the need, the buffer untouched
    for cap in (ne - 1, 0):
        buf = np.full(ne * k, -7, dtype=np.int32)
        info.embeddings = -1
        assert call(paw, 0, 0, 1, buf, cap) == gpu.ERR_INVALID
        assert (info.embeddings, info.k) == (ne, k) and np.all(buf == -7)
    # sizing, then the fill re-uses pass 1: fewer launches than a sizing and a fill apart
    with gpu.options(SGM_LAUNCH_TASKS=16):
        assert call(paw, 0, 0, 1, None, 0, stp=st) == 0
        sizing_launches = st.launches
        buf = np.full(ne * k, -7, dtype=np.int32)
        assert call(paw, 0, 0, 1, buf, ne, stp=st) == 0
        assert st.launches == sizing_launches > 1 and buf.tobytes() == want.tobytes()
        # a sizing call for one pattern, then a fill for another pattern of the same k and flags: searched again, and correct
        want_dia = g.subgraph_match(PATTERNS["diamond"])
        assert call(paw, 0, 0, 1, None, 0) == 0
        buf = np.full(max(ne, want_dia.shape[0]) * k, -7, dtype=np.int32)
        assert call(dia, 0, 0, 1, buf, buf.size // k, stp=st) == 0
        assert info.embeddings == want_dia.shape[0] and st.launches == 2 * -(-info.tasks // 16)
        assert buf[:want_dia.size].tobytes() == want_dia.tobytes() and np.all(buf[want_dia.size:] == -7)
        check_list(A, PATTERNS["diamond"], info.order[:k], buf[:want_dia.size].reshape(-1, k), True)
    # every error of the contract
    assert call(paw, 0, 0, 1, None, 0, infop=None) == gpu.ERR_INVALID
    assert lib.gmsx_subgraph_match(None, k, vp(paw[0]), vp(paw[1]), 0, 0, 1, None, 0, C.byref(info), None) == gpu.ERR_INVALID
    assert lib.gmsx_subgraph_match(g._h, k, None, vp(paw[1]), 0, 0, 1, None, 0, C.byref(info), None) == gpu.ERR_INVALID
    assert lib.gmsx_subgraph_match(g._h, k, vp(paw[0]), None, 0, 0, 1, None, 0, C.byref(info), None) == gpu.ERR_INVALID
    assert lib.gmsx_subgraph_match(g._h, 0, vp(paw[0]), vp(paw[1]), 0, 0, 1, None, 0, C.byref(info), None) == gpu.ERR_INVALID
    assert call(paw, 4, 0, 1, None, 0) == gpu.ERR_INVALID and call(paw, 8, 0, 1, None, 0) == gpu.ERR_INVALID  # unknown flag bits
    assert call(paw, 0, 0, 1, None, -1) == gpu.ERR_INVALID
    for part, nparts in ((0, 0), (-1, 2), (2, 2), (5, 3)):
        assert call(paw, 0, part, nparts, None, 0) == gpu.ERR_INVALID
    buf = np.full(k, -7, dtype=np.int32)
    assert call(paw, gpu.SGM_FIRST, 0, 1, buf, 0) == gpu.ERR_INVALID and np.all(buf == -7)  # FIRST with maps needs capacity >= 1
    assert call(paw, gpu.SGM_FIRST | gpu.SGM_MONO, 0, 1, buf, 1) == 0 and info.embeddings == 1
    assert buf.tolist() == g.subgraph_match(PATTERNS["paw"], induced=False)[0].tolist()
    unsorted = (np.array([0, 1, 3, 4], np.int64), np.array([1, 2, 0, 1], np.int32))
    assert call(unsorted, 0, 0, 1, None, 0) == gpu.ERR_NOT_CANONICAL
    two = (np.array([0, 1, 2, 3, 4], np.int64), np.array([1, 0, 3, 2], np.int32))
    assert call(two, 0, 0, 1, None, 0) == gpu.ERR_UNSUPPORTED  # disconnected
    p33 = gpu.pattern_arrays(path(list(range(33))))
    assert call(p33, 0, 0, 1, None, 0) == gpu.ERR_UNSUPPORTED
    # k = 1 and k = 2; an empty graph
    for induced in (True, False):
        assert g.subgraph_match((np.array([0, 0]), np.zeros(0, np.int32)), induced=induced).tolist() == [[v] for v in range(48)]
    assert g.subgraph_match((np.array([0, 0]), np.zeros(0, np.int32)), first=True).tolist() == [[0]]
    assert listed(g, A, PATTERNS["K2"], True).shape[0] == csr.nnz
    _, st2 = g.subgraph_match(PATTERNS["paw"], stats=True)
    assert st2["sizing"]["units"] == st2["info"]["tasks"] > 0 and st2["sizing"]["kernel_ms"] > 0 and st2["fill"]["kernel_ms"] > 0
    assert st2["sizing"]["setup_ms"] > 0
    g.free()
    empty = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, np.zeros((0, 2), np.int32), n=0))
    assert empty.subgraph_match(PATTERNS["K3"]).shape == (0, 3) and empty.subgraph_match(PATTERNS["K3"], first=True).shape == (0, 3)
    empty.free()


# ---- 11. driver -----------------------------------------------------------------------------------------------------------------------
def test_subgraph_driver(gpu, tmp_path):
    drv = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")
    pat = tmp_path / "house.el"
    pat.write_text("".join(f"{a} {b}\n" for a, b in PATTERNS["house_r1"]))
    for name in ("eppsteinExample", "smallRandom1"):
        rec = next(r for r in RECORDS["file_" + name] if r["pattern"] == "house_r1")
        out = tmp_path / (name + ".txt")
        r = subprocess.run([drv, "sgi", "-f", os.path.join(GOLDEN, "testGraphs", name + ".el"), "-p", "pattern-file=" + str(pat), "-v", "--list", str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "PASS" in r.stdout and "@@@" in r.stdout
        if rec["ref"] is None:
            assert "No isomorphisms were found" in r.stdout
        else:  # the mapping as the reference keeps it: target vertex -> pattern vertex, by ascending target vertex
            want = " ".join(f"{t}:{p}" for t, p in sorted((t, p) for p, t in enumerate(rec["ref"])))
            assert "isomorphism: " + want in r.stdout, r.stdout
        rows = np.array([[int(x) for x in ln.split()] for ln in out.read_text().splitlines() if ln.strip()], dtype=np.int32).reshape(-1, 5)
        assert rows.shape[0] == rec["induced"]["count"] and sha(rows) == rec["induced"]["sha256"]
    r = subprocess.run([drv, "sgi", "-f", os.path.join(GOLDEN, "testGraphs", "eppsteinExample.el"), "-p", "pattern-file=" + str(pat), "--mono", "--list",
                        str(tmp_path / "mono.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rec = next(r_ for r_ in RECORDS["file_eppsteinExample"] if r_["pattern"] == "house_r1")
    rows = np.array([[int(x) for x in ln.split()] for ln in (tmp_path / "mono.txt").read_text().splitlines() if ln.strip()], dtype=np.int32).reshape(-1, 5)
    assert rows.shape[0] == rec["mono"]["count"] and sha(rows) == rec["mono"]["sha256"]
