"""GPU: gmsx_greedy_matching and gmsx_matching_verify through the C-ABI against the goldens (tests/golden/matching.{json,npz}) and the restatements
of tests/test_matching_golden_cpu.py (greedy_np, rounds_np, check_np, info_np, pairs_np).  All results are integers: every comparison is exact.

  goldens      every record: mate, the pair arrays and info; rounds is rounds_np's; want_edges=False gives the same info; the verifier certifies it
  ties         unit weights on a 64 x 64 grid, K_64, a 4096-cycle and a 4096-path; unweighted and weighted with all-ones weights: the same bytes
  hash tie     n = 62 097 with the edges {0, 50549} and {50549, 62096} of equal weight, whose h collide: (lo, hi) decides, in every binning
  chain        a path of 256 vertices with weights 1, 2, …: one round per pair; the same path with random weights: rounds is rounds_np's
  re-search    a - b - c - d with weights 1, 2, 3: b's first candidate is taken in round 1, b pairs with a in round 2; MATCH_KEEP 0 and 1
  mutual pick  n = 2; a perfect matching of 512 pairs in one round
  row classes  stars with 1 500 and 40 000 leaves, distinct weights and unit weights, at both ends of MATCH_WAVE_ROW / MATCH_WG_ROW; kronecker 14
               under a seeded renumbering with seeded weights
  keep         MATCH_KEEP = 1 never examines more arcs than 0, same bytes
  extremes     weights 2^31 - 1 (total above 2^32), two components plus isolated vertices, n = 1, an edgeless graph, K_3
  verifier     perturbed mate arrays: all six integers are check_np's
  same bytes   three runs, GMSX_UPLOAD_TRUSTED, GMSX_UPLOAD_HUB_LIMIT(64), a sharded upload, a second handle, re-attached weights, every
               option combination: one tobytes() value for each output
  contract     every GMSX_ERR_INVALID case leaves the caller's arrays untouched; device bytes"""
import ctypes as C

import numpy as np
import pytest

from test_matching_golden_cpu import (ARR, ARRAY_MAX_N, INFO_KEYS, J, check_np, complete_edges, golden_csr, greedy_np, grid_edges, info_np, matching,
                                      mix_np, pairs_np, path_edges, rec_id, record, rounds_np, sha_of)

pytestmark = pytest.mark.gpu

HUGE = 2 ** 31 - 1
BINS = ((1, 1), (1, HUGE), (HUGE, HUGE), (256, 4096))   # MATCH_WAVE_ROW, MATCH_WG_ROW: every row a workgroup's / a wave's / a lane's or a group's / the defaults


def arrays(csr, weighted=True):
    return (np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32),
            np.array(csr.weights(), dtype=np.int32) if weighted else None)


def edge_graph(gpu, src, dst, w, n):
    """(handle with the weights attached, off, adj, w)"""
    csr = gpu.HostCSR.from_weighted_edges(np.asarray(src), np.asarray(dst), np.asarray(w), num_nodes=n)
    g = gpu.DeviceGraph.from_csr(csr)
    g.set_weights(csr.weights())
    return (g,) + arrays(csr)


def check(g, off, adj, w, weighted, mate=None, rounds=None):
    """every output of one call against the restatement (mate / rounds: what greedy_np / rounds_np gave, if the caller has them), and the
    verifier on the result; returns (mate, u, v, w, info, stats)"""
    ww = w if weighted else None
    r = g.greedy_matching(weighted=weighted, want_mate=True, want_edges=True, stats=True)
    got, u, v, pw, info, st = r
    want = greedy_np(off, adj, ww) if mate is None else mate
    assert np.array_equal(got, want), weighted
    eu, ev, ew = pairs_np(off, adj, ww, want)
    assert np.array_equal(u, eu) and np.array_equal(v, ev) and np.array_equal(pw, ew)
    assert np.all(u < v) and np.all(np.diff(u) > 0) and 2 * info["pairs"] + info["free_vertices"] == off.size - 1
    assert info == info_np(off, adj, ww, want, info["rounds"] if rounds is None else rounds)
    assert (info["rounds"] > 0) == (info["pairs"] > 0) and info["rounds"] <= info["pairs"]
    assert st["units"] == info["pairs"] and st["probes"] == info["rounds"]
    c = g.matching_verify(got, weighted=weighted)
    assert c == {"invalid": 0, "pairs": info["pairs"], "total_weight": info["total_weight"], "free_vertices": info["free_vertices"],
                 "augmentable": 0, "undominated": 0}
    return r


_GRAPHS = {}


def device_graph(gpu, key):
    if key not in _GRAPHS:
        csr = golden_csr(gpu, key)
        g = gpu.DeviceGraph.from_csr(csr)
        has = J["graphs"][key]["source"]["kind"] != "el"   # the .el files carry no weights
        if has:
            g.set_weights(csr.weights())
        _GRAPHS[key] = (g,) + arrays(csr, has)
    return _GRAPHS[key]


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_matching_equals_the_golden(gpu, rec):
    g, off, adj, w = device_graph(gpu, rec["graph"])
    want, rounds = matching(gpu, rec["graph"], rec["weighted"])
    mate, u, v, pw, info, st = check(g, off, adj, w, rec["weighted"], mate=want, rounds=rounds)
    assert info == {k: rec[k] for k in INFO_KEYS} and sha_of(mate) == rec["sha256"]
    if off.size - 1 <= ARRAY_MAX_N:
        assert np.array_equal(mate, ARR["mate_" + rec_id(rec)])
    none = g.greedy_matching(weighted=rec["weighted"], want_mate=False, want_edges=False)
    assert none[:4] == (None, None, None, None) and none[4] == info


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------------
def test_unit_weights_tie_break(gpu):
    cycle = (np.arange(4096), (np.arange(4096) + 1) % 4096)
    for (src, dst), n in ((grid_edges(64, 64), 4096), (complete_edges(64), 64), (cycle, 4096), (path_edges(4096), 4096)):
        g, off, adj, w = edge_graph(gpu, src, dst, np.ones(len(src), dtype=np.int64), n)
        want, rounds = rounds_np(off, adj)
        a = check(g, off, adj, w, False, mate=want, rounds=rounds)
        b = check(g, off, adj, w, True, mate=want, rounds=rounds)   # all-ones weights: the same order
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4] and a[4]["rounds"] <= 16
        g.free()


# ---- 3. hash tie ----------------------------------------------------------------------------------------------------------------------
def test_hash_tie_is_broken_by_the_ids(gpu):
    assert int(mix_np(0, 50549)) == int(mix_np(50549, 62096))
    g, off, adj, w = edge_graph(gpu, [0, 50549], [50549, 62096], [5, 5], 62097)
    for weighted in (False, True):
        want, rounds = rounds_np(off, adj, w if weighted else None)
        for wave_row, wg_row in BINS:
            for keep in (0, 1):
                with gpu.options(MATCH_WAVE_ROW=wave_row, MATCH_WG_ROW=wg_row, MATCH_KEEP=keep):
                    mate, u, v, pw, info, st = check(g, off, adj, w, weighted, mate=want, rounds=rounds)
                assert (u.tolist(), v.tolist(), mate[62096], info["pairs"], info["exposed"], info["rounds"]) == ([0], [50549], -1, 1, 1, 1)
    g.free()


# ---- 4. chain -------------------------------------------------------------------------------------------------------------------------
def test_chain(gpu):
    n = 256
    g, off, adj, w = edge_graph(gpu, *path_edges(n), np.arange(1, n), n)
    mate, u, v, pw, info, st = check(g, off, adj, w, True)
    assert info["rounds"] == 128 and np.array_equal(mate, np.arange(n) ^ 1) and np.array_equal(pw, np.arange(1, n, 2))
    g.free()
    g, off, adj, w = edge_graph(gpu, *path_edges(n), np.random.RandomState(1).randint(1, 256, size=n - 1), n)
    want, rounds = rounds_np(off, adj, w)
    check(g, off, adj, w, True, mate=want, rounds=rounds)
    g.free()


# ---- 5. re-search ---------------------------------------------------------------------------------------------------------------------
def test_a_vertex_whose_candidate_was_taken_searches_again(gpu):
    g, off, adj, w = edge_graph(gpu, [0, 1, 2], [1, 2, 3], [1, 2, 3], 4)   # a - b - c - d: c and d pair first, then b falls back to a
    for keep in (0, 1):
        with gpu.options(MATCH_KEEP=keep):
            mate, u, v, pw, info, st = check(g, off, adj, w, True)
        assert mate.tolist() == [1, 0, 3, 2] and pw.tolist() == [1, 3] and info["rounds"] == 2 and info["total_weight"] == 4
    g.free()


# ---- 6. mutual pick -------------------------------------------------------------------------------------------------------------------
def test_mutual_pick(gpu):
    g, off, adj, w = edge_graph(gpu, [0], [1], [7], 2)
    for weighted in (False, True):
        mate, u, v, pw, info, st = check(g, off, adj, w, weighted)
        assert (mate.tolist(), u.tolist(), v.tolist(), pw.tolist(), info["rounds"]) == ([1, 0], [0], [1], [7 if weighted else 1], 1)
    g.free()
    pairs = np.arange(512)
    g, off, adj, w = edge_graph(gpu, 2 * pairs, 2 * pairs + 1, np.random.RandomState(3).randint(1, 9, size=512), 1024)
    for weighted in (False, True):
        info = check(g, off, adj, w, weighted)[4]
        assert (info["pairs"], info["free_vertices"], info["rounds"]) == (512, 0, 1)
    g.free()


# ---- 7. row classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [1500, 40000])
def test_star(gpu, leaves):
    wt = np.random.RandomState(leaves).permutation(leaves) + 1   # distinct
    g, off, adj, w = edge_graph(gpu, np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1), wt, leaves + 1)
    heaviest = int(np.argmax(wt)) + 1
    lightest_h = int(np.argmin(mix_np(np.zeros(leaves), np.arange(1, leaves + 1)))) + 1
    for weighted, leaf in ((True, heaviest), (False, lightest_h)):
        want, rounds = rounds_np(off, adj, w if weighted else None)
        assert (want[0], rounds) == (leaf, 1)
        for wave_row, wg_row in BINS:
            for keep in (0, 1):
                with gpu.options(MATCH_WAVE_ROW=wave_row, MATCH_WG_ROW=wg_row, MATCH_KEEP=keep):
                    mate, u, v, pw, info, st = check(g, off, adj, w, weighted, mate=want, rounds=rounds)
                assert (u.tolist(), v.tolist(), info["pairs"], info["exposed"]) == ([0], [leaf], 1, leaves - 1)
                assert info["total_weight"] == (leaves if weighted else 1) and st["alg_elements"] >= 2 * leaves
    g.free()


def test_kronecker_14_renumbered(gpu):
    g, off, adj, w = device_graph(gpu, "kronecker_14_16")
    n = off.size - 1
    rng = np.random.RandomState(2)
    perm = rng.permutation(n)
    row = np.repeat(np.arange(n), np.diff(off))
    up = row < adj
    h, off2, adj2, w2 = edge_graph(gpu, perm[row[up]], perm[adj[up]], rng.randint(1, 256, size=int(up.sum())), n)
    assert adj2.size == adj.size
    for weighted in (False, True):
        want, rounds = rounds_np(off2, adj2, w2 if weighted else None)
        assert np.array_equal(want, greedy_np(off2, adj2, w2 if weighted else None))
        check(h, off2, adj2, w2, weighted, mate=want, rounds=rounds)
        with gpu.options(MATCH_WAVE_ROW=1, MATCH_WG_ROW=64):
            check(h, off2, adj2, w2, weighted, mate=want, rounds=rounds)
    h.free()


# ---- 8. MATCH_KEEP --------------------------------------------------------------------------------------------------------------------
def test_keep_never_examines_more_arcs(gpu):
    g, off, adj, w = device_graph(gpu, "kronecker_14_16")
    for weighted in (False, True):
        rec = record("kronecker_14_16", weighted)
        got = {}
        for keep in (0, 1):
            with gpu.options(MATCH_KEEP=keep):
                mate, u, v, pw, info, st = g.greedy_matching(weighted=weighted, want_edges=True, stats=True)
            assert info == {k: rec[k] for k in INFO_KEYS} and sha_of(mate) == rec["sha256"]
            got[keep] = (st["alg_elements"], mate.tobytes(), u.tobytes(), v.tobytes(), pw.tobytes())
        assert got[1][0] <= got[0][0] and got[1][1:] == got[0][1:] and got[1][0] >= adj.size   # the first round walks every row


# ---- 9. extremes ----------------------------------------------------------------------------------------------------------------------
def test_extremes(gpu):
    big = 2 ** 31 - 1
    g, off, adj, w = edge_graph(gpu, np.arange(7), np.arange(1, 8), np.full(7, big), 8)
    info = check(g, off, adj, w, True)[4]
    assert info["total_weight"] == info["pairs"] * big > 2 ** 32 and info["min_weight"] == info["max_weight"] == big and info["pairs"] >= 3
    g.free()
    g, off, adj, w = edge_graph(gpu, [0, 1, 4, 5, 4], [1, 2, 5, 6, 6], [3, 4, 5, 6, 2], 9)   # two components, 3, 7 and 8 isolated
    mate, u, v, pw, info, st = check(g, off, adj, w, True)
    assert list(zip(u.tolist(), v.tolist(), pw.tolist())) == [(1, 2, 4), (5, 6, 6)] and mate.tolist() == [-1, 2, 1, -1, -1, 6, 5, -1, -1]
    assert (info["free_vertices"], info["exposed"]) == (5, 2)
    check(g, off, adj, w, False)
    g.free()
    g, off, adj, w = edge_graph(gpu, [0, 0, 1], [1, 2, 2], [1, 1, 1], 3)   # K_3
    for weighted in (False, True):
        info = check(g, off, adj, w, weighted)[4]
        assert (info["pairs"], info["free_vertices"], info["exposed"], info["rounds"]) == (1, 1, 1, 1)
    g.free()
    empty = {"pairs": 0, "total_weight": 0, "free_vertices": 1, "exposed": 0, "min_weight": 0, "max_weight": 0, "rounds": 0}
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # n = 1
    mate, u, v, pw, info = g.greedy_matching(want_edges=True)
    assert mate.tolist() == [-1] and u.size == v.size == pw.size == 0 and info == empty
    assert g.matching_verify(mate) == {"invalid": 0, "pairs": 0, "total_weight": 0, "free_vertices": 1, "augmentable": 0, "undominated": 0}
    g.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32)))   # edgeless, n = 5
    g.set_weights(np.zeros(0, dtype=np.int32))
    for weighted in (False, True):
        mate, u, v, pw, info = g.greedy_matching(weighted=weighted, want_edges=True)
        assert mate.tolist() == [-1] * 5 and u.size == 0 and info == dict(empty, free_vertices=5)
    assert g.matching_verify(np.array([-1, 3, -1, 1, 9]))["invalid"] == 3
    g.free()


# ---- 10. the verifier on bad input ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["wel_two_parts_a", "kronecker_10_16"])
def test_verifier_on_perturbed_matchings(gpu, key):
    g, off, adj, w = device_graph(gpu, key)
    n, m = off.size - 1, adj.size // 2
    for weighted in (False, True):
        ww = w if weighted else None
        mate = matching(gpu, key, weighted)[0]

        def verify(bad, ww=ww, weighted=weighted):
            got, want = g.matching_verify(bad, weighted=weighted), check_np(off, adj, ww, bad)
            assert got == want
            return got

        matched = np.flatnonzero(mate >= 0)
        a = int(matched[0])
        stranger = int(next(x for x in matched if x != a and x != mate[a] and x not in adj[off[a]:off[a + 1]]))
        bad = mate.copy()   # a mate that is not a neighbour (mutual, so that only the row decides)
        bad[[mate[a], mate[stranger]]] = -1
        bad[a], bad[stranger] = stranger, a
        assert verify(bad)["invalid"] == 2
        bad = mate.copy()   # a mate whose mate is someone else
        free_nb = int(next(x for x in range(n) if mate[x] < 0 and off[x + 1] > off[x]))
        bad[free_nb] = adj[off[free_nb]]
        assert verify(bad)["invalid"] == 1
        bad = mate.copy()   # mates out of range
        bad[mate[a]], bad[a] = -1, n
        bad[free_nb] = -2
        c = verify(bad)
        assert c["invalid"] == 2 and c["augmentable"] >= 1
        c = verify(-np.ones(n, dtype=np.int32))   # nothing matched
        assert (c["invalid"], c["pairs"], c["free_vertices"], c["augmentable"], c["undominated"]) == (0, 0, n, m, m)
        bad = mate.copy()   # one pair dropped
        bad[[a, mate[a]]] = -1
        c = verify(bad)
        assert c["invalid"] == 0 and c["augmentable"] >= 1 and c["undominated"] >= c["augmentable"] and c["pairs"] == record(key, weighted)["pairs"] - 1
        other = greedy_np(off, adj, None if weighted else w)   # THE matching of the other order is valid and maximal, and not certified
        c = verify(other)
        assert c["invalid"] == 0 and c["augmentable"] == 0 and (c["undominated"] > 0) == (not np.array_equal(other, mate))


# ---- 11. same bytes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_same_bytes(gpu, weighted):
    csr = golden_csr(gpu, "kronecker_10_16")
    off, adj, w = arrays(csr)

    def upload(flags=0, shard=None):
        g = gpu.DeviceGraph.from_csr(csr, flags, shard=shard)
        g.set_weights(w)
        return g

    def run(g):
        r = g.greedy_matching(weighted=weighted, want_edges=True)
        return tuple(a.tobytes() for a in r[:4]) + (tuple(sorted(r[4].items())),)

    base = upload()
    first = run(base)
    assert sha_of(np.frombuffer(first[0], dtype=np.int32)) == record("kronecker_10_16", weighted)["sha256"]
    for _ in range(2):
        assert run(base) == first
    for keep in (0, 1):
        for wave_row, wg_row in BINS:
            with gpu.options(MATCH_WAVE_ROW=wave_row, MATCH_WG_ROW=wg_row, MATCH_KEEP=keep):
                assert run(base) == first
    base.set_weights(w)   # re-attached
    assert run(base) == first
    base.set_weights(None)
    base.set_weights(w)   # detached and attached again
    assert run(base) == first
    for flags, shard in ((gpu.UPLOAD_TRUSTED, None), (64 << 8, None), (0, (1, 2)), (0, None)):
        g = upload(flags, shard)
        assert run(g) == first
        g.free()
    base.free()


# ---- 12. contract ---------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = golden_csr(gpu, "wel_two_parts_b")
    off, adj, w = arrays(csr)
    n = csr.num_nodes
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    info, out = gpu.MatchingInfo(), gpu.MatchingCheck()
    info.pairs = out.invalid = 77
    mate, eu, ev, ew = (np.full(n, 77, dtype=np.int32) for _ in range(4))
    pm, pu, pv, pw = (a.ctypes.data_as(C.c_void_p) for a in (mate, eu, ev, ew))

    def untouched():
        return bool(all(np.all(a == 77) for a in (mate, eu, ev, ew)) and info.pairs == 77 and out.invalid == 77)

    assert L.gmsx_greedy_matching(g._h, 1, pm, pu, pv, pw, C.byref(info), None) == gpu.ERR_INVALID and untouched()   # weighted, no weights attached
    assert L.gmsx_matching_verify(g._h, 1, pm, C.byref(out), None) == gpu.ERR_INVALID and untouched()
    g.set_weights(w)
    before = g.device_bytes
    for flags in (2, 4, 1 << 31, 3):
        assert L.gmsx_greedy_matching(g._h, flags, pm, pu, pv, pw, C.byref(info), None) == gpu.ERR_INVALID and untouched()
        assert L.gmsx_matching_verify(g._h, flags, pm, C.byref(out), None) == gpu.ERR_INVALID and untouched()
    for trio in ((pu, pv, None), (pu, None, pw), (None, pv, pw), (pu, None, None), (None, None, pw)):
        assert L.gmsx_greedy_matching(g._h, 0, pm, trio[0], trio[1], trio[2], C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_greedy_matching(g._h, 0, pm, pu, pv, pw, None, None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_greedy_matching(None, 0, pm, pu, pv, pw, C.byref(info), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_matching_verify(None, 0, pm, C.byref(out), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_matching_verify(g._h, 0, None, C.byref(out), None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_matching_verify(g._h, 0, pm, None, None) == gpu.ERR_INVALID and untouched()
    assert L.gmsx_greedy_matching(g._h, 1, pm, pu, pv, pw, C.byref(info), None) == gpu.OK and not untouched()
    rec = record("wel_two_parts_b", True)
    assert info.pairs == rec["pairs"] and np.all(eu[info.pairs:] == 77) and sha_of(mate) == rec["sha256"]
    assert L.gmsx_matching_verify(g._h, 1, pm, C.byref(out), None) == gpu.OK and (out.invalid, out.undominated, out.pairs) == (0, 0, rec["pairs"])
    assert g.device_bytes == before
    check(g, off, adj, w, True)
    check(g, off, adj, w, False)
    assert g.device_bytes == before
    # the call changes no other entry point's answer
    h = gpu.DeviceGraph.from_csr(csr)
    h.set_weights(w)
    assert g.sssp(9)[0].tobytes() == h.sssp(9)[0].tobytes()
    h.free()
    g.free()
