"""GPU tests of the HIP k-clique-star LISTING (gmsx_kclique_star_list = KCliqueStar::Par::CliqueStarList, and with CLIQUES_ONLY the k-clique
listing): the lists against the goldens of the compiled reference, a host checker (rows ascending and distinct, every pair of members an
edge, every star the intersection of the members' rows, the counts pinned by gmsx_kclique_star_count and the oracle: together that is the
whole list), the kernel paths, the shards, the API contract, kronecker-14 in four shards, the C++ adaptor and the driver."""
import hashlib
import math
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, edges_to_csr, host_graph, load_golden

pytestmark = pytest.mark.gpu


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def canonical(cl, soff, mem):
    """The pairs sorted by clique row, lexicographically: (clique matrix, star sizes, stars concatenated in that order)."""
    cl = np.asarray(cl, dtype=np.int32)
    order = np.lexsort(cl[:, ::-1].T) if cl.shape[0] else np.zeros(0, dtype=np.int64)
    if soff is None:
        return cl[order], None, None
    sizes = np.diff(soff)
    ssz = sizes[order]
    new_starts = np.concatenate([[0], np.cumsum(ssz)])[:-1]
    gather = np.repeat(soff[:-1][order] - new_starts, ssz) + np.arange(int(ssz.sum()), dtype=np.int64)
    return cl[order], ssz, np.asarray(mem, dtype=np.int32)[gather]


def canonical_sha256(cl, soff, mem):
    c, s, m = canonical(cl, soff, mem)
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(c, dtype="<i4").tobytes())
    h.update(np.ascontiguousarray(s, dtype="<i8").tobytes())
    h.update(np.ascontiguousarray(m, dtype="<i4").tobytes())
    return h.hexdigest()


def info_of(cl, soff, mem, k):
    if soff is None:
        return {"cliques": int(cl.shape[0]), "star_members": 0, "k": k, "max_star": 0}
    sizes = np.diff(soff)
    return {"cliques": int(cl.shape[0]), "star_members": int(mem.size), "k": k, "max_star": int(sizes.max()) if sizes.size else 0}


def is_edge(o, a, u, v):
    """Vectorised: is (u[i], v[i]) an arc of the CSR (rows ascending, so the keys u * n + v are ascending as a whole)?"""
    n = o.size - 1
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(o)) * n + a.astype(np.int64)
    q = np.asarray(u, dtype=np.int64) * n + np.asarray(v, dtype=np.int64)
    pos = np.searchsorted(keys, q)
    return (pos < keys.size) & (keys[np.minimum(pos, max(keys.size - 1, 0))] == q) if keys.size else np.zeros(q.shape, dtype=bool)


def check_pairs(o, a, k, cl, soff, mem, sample=None, seed=0):
    """cliques_only lists pass soff = mem = None.  Everything but the per-pair intersect1d is checked on EVERY pair."""
    n = o.size - 1
    C = cl.shape[0]
    assert cl.shape == (C, k) and cl.dtype == np.int32
    assert np.all((cl >= 0) & (cl < max(n, 1)))
    assert np.all(cl[:, 1:] > cl[:, :-1]), "a clique row is not strictly ascending"
    for i in range(k):
        for j in range(i + 1, k):
            assert np.all(is_edge(o, a, cl[:, i], cl[:, j])), f"members {i}, {j} of some clique are not adjacent"
    assert np.unique(cl, axis=0).shape[0] == C, "a clique is listed twice"
    if soff is None:
        return
    assert soff.dtype == np.int64 and soff.size == C + 1 and soff[0] == 0 and soff[-1] == mem.size
    sizes = np.diff(soff)
    assert np.all(sizes >= 0)
    assert np.all((mem >= 0) & (mem < max(n, 1)))
    if mem.size > 1:  # ascending inside each star
        same = np.ones(mem.size - 1, dtype=bool)
        inner = soff[1:-1]
        same[inner[(inner > 0) & (inner < mem.size)] - 1] = False
        assert np.all(mem[1:][same] > mem[:-1][same]), "a star is not strictly ascending"
    owner = np.repeat(np.arange(C), sizes)
    for j in range(k):  # every star member is adjacent to every member of its clique (hence outside it)
        assert np.all(is_edge(o, a, cl[owner, j], mem)), f"a star member misses member {j} of its clique"
    idx = np.arange(C) if sample is None or sample >= C else np.random.default_rng(seed).choice(C, sample, replace=False)
    for i in idx:
        common = None
        for u in cl[i]:
            row = a[o[u]:o[u + 1]]
            common = row if common is None else np.intersect1d(common, row, assume_unique=True)
        assert np.array_equal(common, mem[soff[i]:soff[i + 1]]), f"star of clique {cl[i].tolist()}"


def host_check(gpu, oracle, csr, ks, sample=60000, use_oracle=True, **kw):
    """Both modes of every k on one upload; returns {k: (cliques, star_offsets, star_members)}."""
    g = gpu.DeviceGraph.from_csr(csr, **kw)
    o, a = csr.offsets(), csr.neighbors()
    out = {}
    for k in ks:
        cl, soff, mem = g.kclique_star_list(k)
        assert g.kclique_star_list_info(k) == info_of(cl, soff, mem, k)
        check_pairs(o, a, k, cl, soff, mem, sample=sample)
        assert (cl.shape[0], mem.size) == g.kclique_star_count(k), k  # with the sound stars above: every star is complete
        if use_oracle and cl.shape[0] <= 100000:
            assert (cl.shape[0], mem.size) == oracle.kclique_star_count(o, a, k), k
        c2, s2, m2 = g.kclique_star_list(k, cliques_only=True)
        assert s2 is None and m2 is None
        assert g.kclique_star_list_info(k, cliques_only=True) == info_of(c2, None, None, k)
        check_pairs(o, a, k, c2, None, None)
        assert np.array_equal(canonical(c2, None, None)[0], canonical(cl, None, None)[0])
        out[k] = (cl, soff, mem)
    g.free()
    return out


def gnp_edges(n, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    return np.stack([iu[keep], ju[keep]], axis=1).astype(np.int32)


# ---- 1. goldens of the compiled reference ---------------------------------------------------------------------------------------------
LISTS = load_golden("kcstar_lists.json")
GRAPHS = load_golden("graphs.json")


def golden_csr(gpu, rec):
    src = rec["source"]
    if src["kind"] == "file":
        return gpu.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    if src["kind"] == "edges":
        return edges_to_csr(gpu, src["edges"], n=src.get("n", -1))
    return host_graph(gpu, src["generator"], src["scale"], src["degree"], src["relabel"])


def as_pairs(cl, soff, mem):
    return sorted((tuple(int(x) for x in cl[i]), tuple(int(x) for x in mem[soff[i]:soff[i + 1]])) for i in range(cl.shape[0]))


@pytest.mark.parametrize("key", sorted(LISTS))
def test_kcstar_list_equals_reference_golden(gpu, key):
    rec = LISTS[key]
    k = rec["k"]
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, rec))
    cl, soff, mem = g.kclique_star_list(k)
    info = g.kclique_star_list_info(k)
    c2, s2, m2 = g.kclique_star_list(k, cliques_only=True)
    info2 = g.kclique_star_list_info(k, cliques_only=True)
    g.free()
    assert info == {"cliques": rec["cliques"], "star_members": rec["star_members"], "k": k, "max_star": rec["max_star"]}
    assert cl.shape == (rec["cliques"], k) and soff.size == rec["cliques"] + 1 and mem.size == rec["star_members"]
    assert canonical_sha256(cl, soff, mem) == rec["sha256"]
    if "list" in rec:
        assert as_pairs(cl, soff, mem) == sorted((tuple(c), tuple(s)) for c, s in rec["list"])
    assert info2 == {"cliques": rec["cliques"], "star_members": 0, "k": k, "max_star": 0}
    assert s2 is None and m2 is None
    assert np.array_equal(canonical(c2, None, None)[0], canonical(cl, None, None)[0])


# ---- 2. host checker ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,seed", [(40, 0.3, 1), (120, 0.1, 2), (200, 0.5, 3), (64, 0.9, 4)])
def test_kcstar_list_gnp(gpu, oracle, n, p, seed):
    ks = (1, 2, 3, 4) if n == 200 else (1, 2, 3, 4, 5) if n != 64 else (1, 2, 3)  # bounded by the size of the lists, not by the kernel
    host_check(gpu, oracle, edges_to_csr(gpu, gnp_edges(n, p, seed), n=n), ks)


def test_kcstar_list_planted_cliques(gpu, oracle):
    rng = np.random.default_rng(7)
    n = 300
    e = [gnp_edges(n, 0.03, 8)]
    for size in (12, 20, 33, 70):  # one clique wider than a wave
        c = rng.choice(n, size, replace=False)
        iu, ju = np.triu_indices(size, 1)
        e.append(np.stack([c[iu], c[ju]], axis=1))
    out = host_check(gpu, oracle, edges_to_csr(gpu, np.concatenate(e).astype(np.int32), n=n), (1, 2, 3))
    cl, soff, mem = out[2]
    assert np.diff(soff).max() >= 68  # an edge of the 70-clique: a star wider than a wave


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65])
def test_kcstar_list_complete_graph(gpu, oracle, n):
    iu, ju = np.triu_indices(n, 1)
    csr = edges_to_csr(gpu, np.stack([iu, ju], axis=1).astype(np.int32), n=n)
    ks = [k for k in range(1, 7) if math.comb(n, k) <= 50000]  # K_64 / K_65: up to k = 3 (k = 4 is 0.6 M pairs of 60 star ids)
    if n == 65:
        ks.append(63)
    out = host_check(gpu, oracle, csr, ks, use_oracle=n <= 5)
    for k in ks:
        cl, soff, mem = out[k]
        assert cl.shape[0] == math.comb(n, k)
        if cl.shape[0]:
            assert np.all(np.diff(soff) == n - k)


def test_kcstar_list_empty_isolated_star(gpu, oracle):
    # no vertex at all
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, np.zeros((0, 2), np.int32), n=0))
    for k in (1, 2, 3):
        cl, soff, mem = g.kclique_star_list(k)
        assert cl.shape == (0, k) and soff.tolist() == [0] and mem.size == 0
        assert g.kclique_star_list(k, cliques_only=True)[0].shape == (0, k)
        assert g.kclique_star_list_info(k)["cliques"] == 0
    g.free()
    # isolated vertices: k = 1 lists them with empty stars, k = 2 lists nothing
    out = host_check(gpu, oracle, edges_to_csr(gpu, np.zeros((0, 2), np.int32), n=7), (1, 2))
    assert sorted(out[1][0][:, 0].tolist()) == list(range(7)) and out[1][2].size == 0
    assert out[2][0].shape == (0, 2)
    out = host_check(gpu, oracle, edges_to_csr(gpu, [[0, 1], [5, 6]], n=9), (1, 2, 3))
    assert sorted(out[1][0][:, 0].tolist()) == list(range(9)) and out[1][2].size == 4
    assert sorted(map(tuple, out[2][0].tolist())) == [(0, 1), (5, 6)] and out[2][2].size == 0
    assert out[3][0].shape == (0, 3)
    # a star with 200 leaves: k = 1 gives the centre a star of 200, k = 2 lists 200 edges with empty stars, k = 3 nothing
    out = host_check(gpu, oracle, edges_to_csr(gpu, [[0, i] for i in range(1, 201)]), (1, 2, 3))
    assert out[1][0].shape[0] == 201 and np.diff(out[1][1]).max() == 200
    assert out[2][0].shape[0] == 200 and out[2][2].size == 0
    assert out[3][0].shape[0] == 0


@pytest.mark.parametrize("scale", [9, 10, 11])
def test_kcstar_list_kronecker_not_relabelled(gpu, oracle, scale):
    host_check(gpu, oracle, host_graph(gpu, "kronecker", scale, 16, False), (3,))


# ---- 3. paths -------------------------------------------------------------------------------------------------------------------------
def test_kcstar_list_paths_same_list(gpu):
    csr = host_graph(gpu, "kronecker", 10, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    want = {}
    for k in (3, 4):
        cl, soff, mem = g.kclique_star_list(k)
        c0 = g.kclique_star_list(k, cliques_only=True)[0]
        want[k] = canonical_sha256(cl, soff, mem)
        with gpu.options(KCSTAR_SLAB_MB=1):  # a tiny slab budget: many launches
            c2, s2, m2, st = g.kclique_star_list(k, stats=True)
            assert st["sizing"]["launches"] > 1 and st["fill"]["launches"] > 1
            assert c2.tobytes() == cl.tobytes() and s2.tobytes() == soff.tobytes() and m2.tobytes() == mem.tobytes()
            c3, _, _, st = g.kclique_star_list(k, cliques_only=True, stats=True)
            assert st["sizing"]["launches"] > 1
            assert c3.tobytes() == c0.tobytes()
    g.free()
    g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_HUB_LIMIT(16) if hasattr(gpu, "UPLOAD_HUB_LIMIT") else (16 << 8))  # tail containers
    for k in (3, 4):
        assert canonical_sha256(*g.kclique_star_list(k)) == want[k]
    g.free()


# ---- 4. shards ------------------------------------------------------------------------------------------------------------------------
def test_kcstar_list_shards(gpu):
    csr = host_graph(gpu, "kronecker", 11, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    k = 3
    cl, soff, mem = g.kclique_star_list(k)
    whole = g.kclique_star_list_info(k)
    want = canonical_sha256(cl, soff, mem)
    for nparts in (2, 3, 8):
        cls, offs, mems, infos, seen = [], [np.zeros(1, dtype=np.int64)], [], [], set()
        base = 0
        for part in range(nparts):
            c, s, m = g.kclique_star_list(k, part=part, nparts=nparts)
            infos.append(g.kclique_star_list_info(k, part=part, nparts=nparts))
            assert infos[-1] == info_of(c, s, m, k)
            keys = set(map(tuple, c.tolist()))
            assert len(keys) == c.shape[0] and not (keys & seen), (nparts, part)
            seen |= keys
            only = g.kclique_star_list(k, cliques_only=True, part=part, nparts=nparts)[0]
            assert np.array_equal(canonical(only, None, None)[0], canonical(c, None, None)[0])
            cls.append(c)
            offs.append(s[1:] + base)
            base += m.size
            mems.append(m)
        assert canonical_sha256(np.concatenate(cls), np.concatenate(offs), np.concatenate(mems)) == want
        assert sum(i["cliques"] for i in infos) == whole["cliques"]
        assert sum(i["star_members"] for i in infos) == whole["star_members"]
        assert max(i["max_star"] for i in infos) == whole["max_star"]
    g.free()


# ---- 5. API contract ------------------------------------------------------------------------------------------------------------------
def test_kcstar_list_api_contract(gpu):
    import ctypes as C
    lib = gpu.lib()
    csr = host_graph(gpu, "kronecker", 8, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    k = 3
    cl, soff, mem = g.kclique_star_list(k)
    assert cl.shape[0] > 0 and mem.size > 0
    # deterministic: byte-identical arrays
    c2, s2, m2 = g.kclique_star_list(k)
    assert cl.tobytes() == c2.tobytes() and soff.tobytes() == s2.tobytes() and mem.tobytes() == m2.tobytes()
    info = gpu.KcliqueStarListInfo()
    nc, nm = cl.shape[0], mem.size
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    # too small capacities: ERR_INVALID, info holds the sizes, buffers untouched
    for ccap, scap in ((nc - 1, nm), (nc, nm - 1), (0, 0)):
        cb = np.full(nc * k, -7, dtype=np.int32)
        ob = np.full(nc + 1, -7, dtype=np.int64)
        mb = np.full(nm, -7, dtype=np.int32)
        info.cliques = info.star_members = -1
        rc = lib.gmsx_kclique_star_list(g._h, k, 0, 0, 1, vp(cb), vp(ob), vp(mb), ccap, scap, C.byref(info), None)
        assert rc == gpu.ERR_INVALID
        assert (info.cliques, info.star_members, info.k) == (nc, nm, k)
        assert np.all(cb == -7) and np.all(ob == -7) and np.all(mb == -7)
    # exact capacities fill, and echo k
    cb, ob, mb = np.full(nc * k, -7, dtype=np.int32), np.full(nc + 1, -7, dtype=np.int64), np.full(nm, -7, dtype=np.int32)
    assert lib.gmsx_kclique_star_list(g._h, k, 0, 0, 1, vp(cb), vp(ob), vp(mb), nc, nm, C.byref(info), None) == 0
    assert cb.tobytes() == cl.tobytes() and ob.tobytes() == soff.tobytes() and mb.tobytes() == mem.tobytes()
    for kk in (1, 2, 5):
        assert lib.gmsx_kclique_star_list(g._h, kk, 0, 0, 1, None, None, None, 0, 0, C.byref(info), None) == 0
        assert info.k == kk
    # NULL info, bad shards, k out of range
    assert lib.gmsx_kclique_star_list(g._h, k, 0, 0, 1, None, None, None, 0, 0, None, None) == gpu.ERR_INVALID
    for part, nparts in ((0, 0), (-1, 2), (2, 2), (5, 3)):
        assert lib.gmsx_kclique_star_list(g._h, k, 0, part, nparts, None, None, None, 0, 0, C.byref(info), None) == gpu.ERR_INVALID
    for kk in (0, -1):
        assert lib.gmsx_kclique_star_list(g._h, kk, 0, 0, 1, None, None, None, 0, 0, C.byref(info), None) == gpu.ERR_INVALID
    assert lib.gmsx_kclique_star_list(g._h, 64, 0, 0, 1, None, None, None, 0, 0, C.byref(info), None) == gpu.ERR_UNSUPPORTED
    assert lib.gmsx_kclique_star_list(g._h, 64, 1, 0, 1, None, None, None, 0, 0, C.byref(info), None) == gpu.ERR_UNSUPPORTED
    # star pointers with CLIQUES_ONLY
    cb = np.full(nc * k, -7, dtype=np.int32)
    assert lib.gmsx_kclique_star_list(g._h, k, 1, 0, 1, vp(cb), vp(ob), None, nc, 0, C.byref(info), None) == gpu.ERR_INVALID
    assert lib.gmsx_kclique_star_list(g._h, k, 1, 0, 1, vp(cb), None, vp(mb), nc, nm, C.byref(info), None) == gpu.ERR_INVALID
    assert np.all(cb == -7)
    assert lib.gmsx_kclique_star_list(g._h, k, 1, 0, 1, vp(cb), None, None, nc, 0, C.byref(info), None) == 0
    assert (info.cliques, info.star_members, info.k, info.max_star) == (nc, 0, k, 0)
    assert np.array_equal(canonical(cb.reshape(nc, k), None, None)[0], canonical(cl, None, None)[0])
    # stats: tasks, launches, times
    _, _, _, st = g.kclique_star_list(k, stats=True)
    assert st["sizing"]["units"] > 0 and st["sizing"]["launches"] >= 1 and st["fill"]["launches"] >= 1
    assert st["sizing"]["kernel_ms"] > 0 and st["fill"]["kernel_ms"] > 0 and st["sizing"]["setup_ms"] > 0
    g.free()


# ---- 6. size --------------------------------------------------------------------------------------------------------------------------
def test_kcstar_list_kronecker14_four_shards(gpu):
    rec = GRAPHS["kronecker-14-16-relabel"]
    csr = host_graph(gpu, "kronecker", 14, 16, True)
    o, a = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    cliques = members = 0
    for part in range(4):
        t0 = time.perf_counter()
        info = g.kclique_star_list_info(3, part=part, nparts=4)
        t1 = time.perf_counter()
        cl, soff, mem = g.kclique_star_list(3, part=part, nparts=4)
        t2 = time.perf_counter()
        print(f"kronecker-14 k=3 shard {part}/4: {info['cliques']} pairs, {info['star_members']} star ids, max star {info['max_star']}; "
              f"sizing {1e3 * (t1 - t0):.0f} ms, sizing + fill {1e3 * (t2 - t1):.0f} ms")
        assert info == info_of(cl, soff, mem, 3)
        pick = np.sort(np.random.default_rng(part).choice(cl.shape[0], 20000, replace=False))
        sizes = np.diff(soff)[pick]
        sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        gather = np.repeat(soff[:-1][pick] - sub_off[:-1], sizes) + np.arange(int(sizes.sum()), dtype=np.int64)
        check_pairs(o, a, 3, cl[pick], sub_off, mem[gather])
        assert np.all(cl[:, 1:] > cl[:, :-1])
        cliques += info["cliques"]
        members += info["star_members"]
        del cl, soff, mem
    g.free()
    assert cliques == rec["triangles"] == 2862425
    assert members == 4 * (rec["kc4"] // 24) == 146330716


# ---- 7. adaptor -----------------------------------------------------------------------------------------------------------------------
def parse_pairs(text):
    out = []
    for line in text.splitlines():
        if not line.strip():
            continue
        left, right = line.split("|")
        out.append((tuple(int(x) for x in left.split()), tuple(int(x) for x in right.split())))
    return sorted(out)


def test_kcstar_list_adaptor(gpu, tmp_path):
    exe = tmp_path / "kcstar_list_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_kcstar_list_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    keys = [key for key, v in LISTS.items() if v["source"]["kind"] == "file" and "list" in v]
    assert keys
    for key in keys:
        rec = LISTS[key]
        path = os.path.join(GOLDEN, "testGraphs", rec["source"]["name"])
        out = subprocess.run([str(exe), path, str(rec["k"])], check=True, capture_output=True, text=True, timeout=120).stdout
        assert parse_pairs(out) == sorted((tuple(c), tuple(s)) for c, s in rec["list"]), key


# ---- 8. driver ------------------------------------------------------------------------------------------------------------------------
def test_kcstar_list_driver(gpu, tmp_path):
    rec = LISTS["eppsteinExample.el|k=3"]
    out = tmp_path / "pairs.txt"
    drv = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")
    r = subprocess.run([drv, "kcstar", "-f", os.path.join(GOLDEN, "testGraphs", "eppsteinExample.el"), "-p", "clique-size=3", "-v", "--list", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"total 3-cliques: {rec['cliques']}" in r.stdout
    assert "PASS" in r.stdout
    got = parse_pairs(out.read_text())
    for c, s in got:
        assert list(c) == sorted(c) and list(s) == sorted(s)
    assert got == sorted((tuple(c), tuple(s)) for c, s in rec["list"])
