"""GPU tests of the HIP Bron–Kerbosch maximal-clique LISTING (gmsx_bk_list = the `sol` of BkEppsteinPar::mceBench in a listing build):
the lists against the goldens of the compiled reference, a host checker (every listed set sorted, distinct, a clique and maximal, the
number pinned by the oracle: together that is the whole list), the kernel paths, the shards, the API contract, BASELINE configs[3], the
C++ adaptor and the driver."""
import hashlib
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, edges_to_csr, host_graph, load_golden

pytestmark = pytest.mark.gpu


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def cliques_of(off, mem):
    return [mem[off[i]:off[i + 1]] for i in range(off.size - 1)]


def canonical_sha256(off, mem):
    """sha256 of the canonical form: members ascending, cliques sorted lexicographically (a proper prefix first), each serialised as a
    little-endian uint32 size followed by its int32 members."""
    cl = sorted(tuple(int(x) for x in np.sort(c)) for c in cliques_of(off, mem))
    h = hashlib.sha256()
    for c in cl:
        h.update(np.uint32(len(c)).astype("<u4").tobytes())
        h.update(np.asarray(c, dtype="<i4").tobytes())
    return h.hexdigest()


def info_of(off, mem):
    sizes = np.diff(off)
    hist = np.zeros(65, dtype=np.int64)
    np.add.at(hist, np.minimum(sizes, 64), 1)
    hist[0] = 0
    return {"cliques": int(sizes.size), "members": int(mem.size), "max_size": int(sizes.max()) if sizes.size else 0, "size_hist": hist.tolist()}


def check_cliques(csr_off, csr_adj, off, mem, sample=None, seed=0):
    """Every (sampled) listed set is strictly ascending, a clique and maximal; all listed sets are distinct."""
    n = csr_off.size - 1
    sizes = np.diff(off)
    assert off[0] == 0 and np.all(sizes >= 1) and off[-1] == mem.size
    assert np.all((mem >= 0) & (mem < max(n, 1)))
    # ascending inside each clique (vectorised): consecutive members of one clique increase
    if mem.size > 1:
        same = np.ones(mem.size - 1, dtype=bool)
        same[off[1:-1] - 1] = False
        assert np.all(mem[1:][same] > mem[:-1][same])
    idx = np.arange(sizes.size) if sample is None or sample >= sizes.size else np.random.default_rng(seed).choice(sizes.size, sample, replace=False)
    for i in idx:
        c = mem[off[i]:off[i + 1]]
        common = None
        for u in c:
            row = csr_adj[csr_off[u]:csr_off[u + 1]]
            others = c[c != u]
            assert np.all(np.isin(others, row, assume_unique=True)), f"clique {i} {c.tolist()} misses an edge at {u}"
            common = row if common is None else np.intersect1d(common, row, assume_unique=True)
        # maximal: no vertex outside C is adjacent to every member (members are never in their own rows)
        assert common.size == 0, f"clique {i} {c.tolist()} extends by {common[:4].tolist()}"


def distinct(off, mem):
    keys = {bytes(np.asarray(c, dtype="<i4").tobytes()) for c in cliques_of(off, mem)}
    return len(keys) == off.size - 1


def host_check_graph(gpu, oracle, csr, **kw):
    g = gpu.DeviceGraph.from_csr(csr, **kw)
    off, mem = g.bk_list()
    info = g.bk_list_info()
    g.free()
    o, a = csr.offsets(), csr.neighbors()
    check_cliques(o, a, off, mem)
    assert distinct(off, mem)
    assert off.size - 1 == oracle.bk_count(o, a)
    assert info == info_of(off, mem)
    return off, mem


def gnp_edges(n, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.random(iu.size) < p
    return np.stack([iu[keep], ju[keep]], axis=1).astype(np.int32)


# ---- 1. goldens of the compiled reference ---------------------------------------------------------------------------------------------
BK_LISTS = load_golden("bk_lists.json")
GRAPHS = load_golden("graphs.json")


def golden_csr(gpu, key):
    src = BK_LISTS[key]["source"]
    if src["kind"] == "file":
        return gpu.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    if src["kind"] == "edges":
        return edges_to_csr(gpu, src["edges"], n=src.get("n", -1))
    return host_graph(gpu, src["generator"], src["scale"], src["degree"], src["relabel"])


@pytest.mark.parametrize("key", sorted(BK_LISTS))
def test_bk_list_equals_reference_golden(gpu, key):
    rec = BK_LISTS[key]
    csr = golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    off, mem = g.bk_list()
    info = g.bk_list_info()
    g.free()
    assert info["cliques"] == rec["cliques"] == off.size - 1
    assert info["members"] == rec["members"] == mem.size
    assert info["max_size"] == rec["max_size"]
    assert info["size_hist"] == rec["size_hist"]
    assert canonical_sha256(off, mem) == rec["sha256"]
    if "list" in rec:
        assert sorted(tuple(int(x) for x in c) for c in cliques_of(off, mem)) == sorted(tuple(c) for c in rec["list"])


# ---- 2. host checker ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,seed", [(40, 0.3, 1), (120, 0.1, 2), (200, 0.5, 3), (64, 0.9, 4)])
def test_bk_list_gnp(gpu, oracle, n, p, seed):
    host_check_graph(gpu, oracle, edges_to_csr(gpu, gnp_edges(n, p, seed), n=n))


def test_bk_list_planted_cliques(gpu, oracle):
    rng = np.random.default_rng(7)
    n = 300
    e = [gnp_edges(n, 0.03, 8)]
    for size in (12, 20, 33, 70):  # one clique wider than a wave
        c = rng.choice(n, size, replace=False)
        iu, ju = np.triu_indices(size, 1)
        e.append(np.stack([c[iu], c[ju]], axis=1))
    off, mem = host_check_graph(gpu, oracle, edges_to_csr(gpu, np.concatenate(e).astype(np.int32), n=n))
    assert np.diff(off).max() >= 70


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 100])
def test_bk_list_complete_graph(gpu, oracle, n):
    iu, ju = np.triu_indices(n, 1)
    csr = edges_to_csr(gpu, np.stack([iu, ju], axis=1).astype(np.int32), n=n)
    off, mem = host_check_graph(gpu, oracle, csr)
    assert off.tolist() == [0, n] and mem.tolist() == list(range(n))


def test_bk_list_empty_isolated_stars_disjoint(gpu, oracle):
    # no vertex at all
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, np.zeros((0, 2), np.int32), n=0))
    off, mem = g.bk_list()
    assert off.tolist() == [0] and mem.size == 0
    assert g.bk_list_info()["cliques"] == 0
    g.free()
    # isolated vertices only, and isolated vertices beside edges: each is the clique {v}
    off, mem = host_check_graph(gpu, oracle, edges_to_csr(gpu, np.zeros((0, 2), np.int32), n=7))
    assert sorted(mem.tolist()) == list(range(7))
    off, mem = host_check_graph(gpu, oracle, edges_to_csr(gpu, [[0, 1], [5, 6]], n=9))
    assert sorted(tuple(c.tolist()) for c in cliques_of(off, mem)) == [(0, 1), (2,), (3,), (4,), (5, 6), (7,), (8,)]
    # stars: every edge is a maximal clique
    for leaves in (1, 3, 200):
        off, mem = host_check_graph(gpu, oracle, edges_to_csr(gpu, [[0, i] for i in range(1, leaves + 1)]))
        assert off.size - 1 == leaves
    # disjoint cliques
    e, base = [], 0
    for size in (3, 4, 7, 31, 33):
        iu, ju = np.triu_indices(size, 1)
        e.append(np.stack([iu + base, ju + base], axis=1))
        base += size
    off, mem = host_check_graph(gpu, oracle, edges_to_csr(gpu, np.concatenate(e).astype(np.int32)))
    assert sorted(np.diff(off).tolist()) == [3, 4, 7, 31, 33]


@pytest.mark.parametrize("scale", [9, 10, 11])
def test_bk_list_kronecker_not_relabelled(gpu, oracle, scale):
    host_check_graph(gpu, oracle, host_graph(gpu, "kronecker", scale, 16, False))


# ---- 3. paths -------------------------------------------------------------------------------------------------------------------------
def test_bk_list_paths_same_set(gpu, oracle):
    csr = host_graph(gpu, "kronecker", 11, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    off, mem = g.bk_list()
    want = canonical_sha256(off, mem)
    assert off.size - 1 == oracle.bk_count(csr.offsets(), csr.neighbors())
    with gpu.options(BK_LIST_ARENA_MB=1):  # a tiny arena: many launches, a start vertex alone in its own
        o2, m2, st = g.bk_list(stats=True)
        assert st["sizing"]["launches"] > 1
        assert np.array_equal(o2, off) and np.array_equal(m2, mem)
    g.free()
    g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_HUB_LIMIT(16) if hasattr(gpu, "UPLOAD_HUB_LIMIT") else (16 << 8))  # tail containers
    o3, m3 = g.bk_list()
    assert canonical_sha256(o3, m3) == want
    g.free()


# ---- 4. shards ------------------------------------------------------------------------------------------------------------------------
def test_bk_list_shards(gpu, oracle):
    csr = host_graph(gpu, "kronecker", 11, 16, True)
    g = gpu.DeviceGraph.from_csr(csr)
    off, mem = g.bk_list()
    whole = g.bk_list_info()
    want = canonical_sha256(off, mem)
    for nparts in (2, 3, 8):
        offs, mems, seen, infos = [0], [], set(), []
        for part in range(nparts):
            o, m = g.bk_list(part=part, nparts=nparts)
            infos.append(g.bk_list_info(part=part, nparts=nparts))
            assert infos[-1] == info_of(o, m)
            keys = {tuple(c.tolist()) for c in cliques_of(o, m)}
            assert not (keys & seen), (nparts, part)
            seen |= keys
            offs.extend((o[1:] + offs[-1]).tolist())
            mems.append(m)
        u_off, u_mem = np.asarray(offs, dtype=np.int64), np.concatenate(mems)
        assert canonical_sha256(u_off, u_mem) == want
        assert sum(i["cliques"] for i in infos) == whole["cliques"]
        assert sum(i["members"] for i in infos) == whole["members"]
        assert max(i["max_size"] for i in infos) == whole["max_size"]
        assert np.array_equal(np.sum([i["size_hist"] for i in infos], axis=0), whole["size_hist"])
    g.free()


# ---- 5. API contract ------------------------------------------------------------------------------------------------------------------
def test_bk_list_api_contract(gpu):
    import ctypes as C
    lib = gpu.lib()
    ka = load_golden("known_answers.json")
    c = ka["bk_random"][0]
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, c["edges"], n=c["n"]))
    off, mem = g.bk_list()
    assert off.size - 1 == c["bk"]
    # deterministic: byte-identical arrays
    o2, m2 = g.bk_list()
    assert off.tobytes() == o2.tobytes() and mem.tobytes() == m2.tobytes()
    # a rank is validated and does not change the set
    perm = np.random.default_rng(3).permutation(c["n"]).astype(np.int32)
    o3, m3 = g.bk_list(rank=perm)
    assert canonical_sha256(o3, m3) == canonical_sha256(off, mem)
    for bad in (np.zeros(c["n"], dtype=np.int32), np.arange(1, c["n"] + 1, dtype=np.int32)):
        with pytest.raises(gpu.GmsxError) as ei:
            g.bk_list(rank=bad)
        assert ei.value.status == gpu.ERR_INVALID
    # too small capacities: ERR_INVALID, info holds the sizes, buffers untouched
    info = gpu.BkListInfo()
    nc, nm = off.size - 1, mem.size
    for ocap, mcap in ((nc, nm), (nc + 1, nm - 1), (0, 0)):
        ob = np.full(nc + 1, -7, dtype=np.int64)
        mb = np.full(max(nm, 1), -7, dtype=np.int32)
        rc = lib.gmsx_bk_list(g._h, None, 0, 1, ob.ctypes.data_as(C.c_void_p), mb.ctypes.data_as(C.c_void_p), ocap, mcap, C.byref(info), None)
        assert rc == gpu.ERR_INVALID
        assert info.cliques == nc and info.members == nm
        assert np.all(ob == -7) and np.all(mb == -7)
    # NULL info, bad shards
    assert lib.gmsx_bk_list(g._h, None, 0, 1, None, None, 0, 0, None, None) == gpu.ERR_INVALID
    for part, nparts in ((0, 0), (-1, 2), (2, 2), (5, 3)):
        assert lib.gmsx_bk_list(g._h, None, part, nparts, None, None, 0, 0, C.byref(info), None) == gpu.ERR_INVALID
    g.free()


# ---- 6. BASELINE configs[3] -----------------------------------------------------------------------------------------------------------
def test_bk_list_baseline_config3(gpu):
    rec = GRAPHS["rmat-21-56-a45-b22-c22"]
    csr = host_graph(gpu, "rmat", rec["scale"], rec["degree"], rec["relabel"])
    o, a = csr.offsets(), csr.neighbors()
    g = gpu.DeviceGraph.from_csr(csr)
    total = 0
    for part in range(8):
        t0 = time.perf_counter()
        info = g.bk_list_info(part=part, nparts=8)
        t1 = time.perf_counter()
        off, mem = g.bk_list(part=part, nparts=8)
        t2 = time.perf_counter()
        print(f"configs[3] shard {part}/8: {info['cliques']} cliques, {info['members']} members, max {info['max_size']}; "
              f"sizing {1e3 * (t1 - t0):.0f} ms, sizing + fill {1e3 * (t2 - t1):.0f} ms")
        assert off.size - 1 == info["cliques"] and mem.size == info["members"]
        hist = np.asarray(info["size_hist"], dtype=np.int64)
        assert hist.sum() == info["cliques"]
        if hist[64] == 0:
            assert int((np.arange(65) * hist).sum()) == info["members"]
        check_cliques(o, a, off, mem, sample=20000, seed=part)
        total += info["cliques"]
        del off, mem
    g.free()
    assert total == rec["bk"] == 276888703


# ---- 7. adaptor -----------------------------------------------------------------------------------------------------------------------
def test_bk_list_adaptor(gpu, tmp_path):
    exe = tmp_path / "bk_list_adaptor"
    lib_dir = os.path.join(ROOT, "gms_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_bk_list_adaptor.cpp"),
                    "-L" + lib_dir, "-lgmsx", "-Wl,-rpath," + lib_dir, "-o", str(exe)], check=True)
    names = [k for k, v in BK_LISTS.items() if v["source"]["kind"] == "file" and "list" in v]
    assert names
    for key in names:
        path = os.path.join(GOLDEN, "testGraphs", BK_LISTS[key]["source"]["name"])
        out = subprocess.run([str(exe), path], check=True, capture_output=True, text=True, timeout=120).stdout
        got = sorted(tuple(int(x) for x in line.split()) for line in out.splitlines() if line.strip())
        assert got == sorted(tuple(c) for c in BK_LISTS[key]["list"]), key


# ---- 8. driver ------------------------------------------------------------------------------------------------------------------------
def test_bk_list_driver(gpu, tmp_path):
    key = "eppsteinExample.el"
    out = tmp_path / "cliques.txt"
    drv = os.path.join(ROOT, "gms_amd", "lib", "gmsx_driver")
    r = subprocess.run([drv, "bk", "-f", os.path.join(GOLDEN, "testGraphs", key), "--list", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = sorted(tuple(int(x) for x in line.split()) for line in out.read_text().splitlines() if line.strip())
    for c in got:
        assert list(c) == sorted(c)
    assert got == sorted(tuple(c) for c in BK_LISTS[key]["list"])
