"""GPU: gmsx_coloring_jp and gmsx_coloring_verify through the C-ABI, against the goldens of the compiled reference's JonesV3
(tests/golden/coloring.{json,npz}) and the numpy restatement of the rounds kept in tests/test_coloring_golden_cpu.py:

  goldens      every (graph, order): coloring and info bit for bit, round_of = the depth in the priority DAG; under three uploads and at both
               ends of COLOR_WG_FRONTIER
  composition  color("sl") stays within degeneracy + 1 and verifies clean; color("lf") / color("ff") are the goldens of those orders
  shapes       cliques at the word boundaries of the bitmap, a clique of long rows, a star from both ends, a path of 4 096 rounds, a crown
               graph under two orders, an edgeless graph, the empty graph — closed-form answers
  hand-back    small frontiers too heavy for the one-workgroup kernel (more long rows than it parks, more entries than it may walk, one row above
               its bound) and a golden graph at a threshold of 3: the same bytes at every COLOR_WG_FRONTIER
  errors       a non-permutation and a NULL info are GMSX_ERR_INVALID and write nothing
  verify       clean on a device colouring; planted conflicts and a zeroed entry are counted exactly
  determinism  the same bytes on a second call and in a fresh process"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, edges_to_csr, host_graph
from test_coloring_golden_cpu import COL, COL_ARR, ORDERS, golden_rank, jp_golden, jp_np
from test_core_golden_cpu import CORE, golden_csr

pytestmark = pytest.mark.gpu
WG_NONE, WG_ALL = 0, 2 ** 31 - 1
HUB_LIMIT_64 = 64 << 8


def both_ends(gpu, g, rank, rank_format=True):
    """(coloring, round_of, info) at the default COLOR_WG_FRONTIER, after checking that 0 — every round a kernel boundary — gives the same bytes"""
    col, rnd, info, st = g.coloring_jp(rank, rank_format=rank_format, want_rounds=True, stats=True)
    with gpu.options(COLOR_WG_FRONTIER=WG_NONE):
        col0, rnd0, info0, st0 = g.coloring_jp(rank, rank_format=rank_format, want_rounds=True, stats=True)
    assert col0.tobytes() == col.tobytes() and rnd0.tobytes() == rnd.tobytes() and info0 == info
    n = g.num_nodes
    assert st["units"] == n == st0["units"] and st["probes"] == info["rounds"] == st0["probes"]
    if n:
        # setup 4; a grid-wide round 3; the one-workgroup kernel 1 for as many rounds as it takes (a round it hands back costs its launch too)
        assert st0["launches"] == 4 + 3 * info["rounds"] and 5 <= st["launches"] <= 4 + 4 * info["rounds"]
    return col, rnd, info


def check_against_restatement(gpu, g, off, adj, rank, rank_format=True):
    r = rank if rank is not None else np.arange(off.size - 1)
    if not rank_format:
        r = np.argsort(rank)
    want_col, want_rnd, want_info = jp_np(off, adj, r)
    col, rnd, info = both_ends(gpu, g, rank, rank_format)
    assert np.array_equal(col, want_col) and np.array_equal(rnd, want_rnd) and info == want_info
    return col, rnd, info


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(COL))
def test_golden_parity(gpu, key):
    csr = golden_csr(gpu, key)
    n = csr.num_nodes
    graphs = [gpu.DeviceGraph.from_csr(csr), gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_TRUSTED), gpu.DeviceGraph.from_csr(csr, flags=HUB_LIMIT_64)]
    for order in ORDERS:
        rec = COL[key]["orders"][order]
        want = COL_ARR["color_%s_%s" % (order, key)]
        _, want_rnd, _ = jp_golden(gpu, key, order)
        rank = None if order == "id" else golden_rank(key, order)
        for g in graphs:
            col, rnd, info = both_ends(gpu, g, rank)
            assert col.dtype == np.int32 and col.tobytes() == np.ascontiguousarray(want, dtype=np.int32).tobytes(), (key, order)
            assert info == {f: rec[f] for f in ("colors", "rounds", "max_pred", "first_round")}, (key, order)
            assert np.array_equal(rnd, want_rnd), (key, order)
        g = graphs[0]
        if order == "id":  # NULL is order[v] = v
            assert g.coloring_jp(golden_rank(key, "id"))[0].tobytes() == col.tobytes()
        as_order = np.argsort(golden_rank(key, order)).astype(np.int32)  # the same priority in order format
        col2, info2 = g.coloring_jp(as_order, rank_format=False)
        assert col2.tobytes() == col.tobytes() and info2 == info
        assert g.order_quality(golden_rank(key, order), core_number=0)["max_later"] == info["max_pred"]
    info = gpu.ColoringInfo()
    assert gpu.lib().gmsx_coloring_jp(graphs[0]._h, None, 1, None, None, C.byref(info), None) == gpu.OK  # both arrays may be NULL
    assert info.colors == COL[key]["orders"]["id"]["colors"] and n == COL[key]["n"]
    for g in graphs:
        g.free()


# ---- 2. composition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["kronecker_12_16", "kronecker_14_16"])
def test_heuristics_compose_from_the_rank_producers(gpu, key):
    csr = golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    degeneracy = CORE[key]["degeneracy"]
    assert degeneracy == {"kronecker_12_16": 65, "kronecker_14_16": 123}[key]
    col, info = g.color("sl")
    assert info["colors"] <= degeneracy + 1 and info["max_pred"] == degeneracy
    chk = g.coloring_verify(col)
    assert chk["conflicts"] == 0 and chk["invalid"] == 0 and chk["max_color"] == chk["distinct"] == info["colors"]
    assert chk["max_degree"] == int(np.diff(csr.offsets()).max())
    lf, lf_info = g.color("lf")
    assert lf.tobytes() == COL_ARR["color_degree_" + key].tobytes() and lf_info["colors"] == COL[key]["orders"]["degree"]["colors"]
    ff, ff_info = g.color("ff")
    assert ff.tobytes() == COL_ARR["color_ff_" + key].tobytes() and ff_info["colors"] == COL[key]["orders"]["ff"]["colors"]
    assert g.color("id")[0].tobytes() == COL_ARR["color_id_" + key].tobytes()
    adg, adg_info = g.color("adg")
    chk = g.coloring_verify(adg)
    assert chk["conflicts"] == 0 and chk["invalid"] == 0 and chk["distinct"] == adg_info["colors"] <= adg_info["max_pred"] + 1
    with pytest.raises(gpu.GmsxError):
        g.color("matula")
    g.free()


# ---- 3. known-answer shapes -----------------------------------------------------------------------------------------------------------
def clique_edges(lo, hi):
    i, j = np.triu_indices(hi - lo, 1)
    return np.stack([i + lo, j + lo], axis=1)


def test_cliques_at_the_word_boundaries(gpu):
    sizes, edges, lo = (31, 32, 33, 63, 64, 65, 66), [], 0
    for s in sizes:
        edges.append(clique_edges(lo, lo + s))
        lo += s
    csr = edges_to_csr(gpu, np.concatenate(edges), n=lo)
    g = gpu.DeviceGraph.from_csr(csr)
    col, rnd, info = check_against_restatement(gpu, g, csr.offsets(), csr.neighbors(), None)
    lo = 0
    for s in sizes:  # the id order colours the highest id first: vertex lo + i of a component takes colour s - i
        assert col[lo:lo + s].tolist() == list(range(s, 0, -1)) and rnd[lo:lo + s].tolist() == list(range(s - 1, -1, -1))
        lo += s
    assert info == {"colors": 66, "rounds": 66, "max_pred": 65, "first_round": 7}
    g.free()


def test_clique_of_long_rows(gpu):
    n = 1100  # rows of 1 099 entries: above the long-row threshold, every predecessor colour distinct
    csr = edges_to_csr(gpu, clique_edges(0, n), n=n)
    g = gpu.DeviceGraph.from_csr(csr)
    col, rnd, info = both_ends(gpu, g, None)
    assert col.tolist() == list(range(n, 0, -1)) and rnd.tolist() == list(range(n - 1, -1, -1))
    assert info == {"colors": n, "rounds": n, "max_pred": n - 1, "first_round": 1}
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    col, rnd, info = both_ends(gpu, g, perm)
    assert np.array_equal(col, n - perm) and info["colors"] == n
    g.free()


def test_star_from_both_ends(gpu):
    leaves = 5000
    csr = edges_to_csr(gpu, [(0, i) for i in range(1, leaves + 1)], n=leaves + 1)
    g = gpu.DeviceGraph.from_csr(csr)
    hub_first = np.arange(leaves, -1, -1, dtype=np.int32)
    col, rnd, info = both_ends(gpu, g, hub_first)
    assert col[0] == 1 and np.all(col[1:] == 2) and rnd[0] == 0 and np.all(rnd[1:] == 1)
    assert info == {"colors": 2, "rounds": 2, "max_pred": 1, "first_round": 1}
    col, rnd, info = both_ends(gpu, g, None)  # the hub last: 5 000 predecessors of colour 1
    assert col[0] == 2 and np.all(col[1:] == 1) and rnd[0] == 1 and np.all(rnd[1:] == 0)
    assert info == {"colors": 2, "rounds": 2, "max_pred": leaves, "first_round": leaves}
    # verify: the hub overwritten with the leaves' colour
    chk = g.coloring_verify(col)
    assert chk == {"conflicts": 0, "invalid": 0, "max_color": 2, "distinct": 2, "max_degree": leaves}
    col[0] = 1
    chk = g.coloring_verify(col)
    assert chk == {"conflicts": leaves, "invalid": 0, "max_color": 1, "distinct": 1, "max_degree": leaves}
    g.free()


def test_path_of_4096_rounds(gpu):
    n = 4096
    csr = edges_to_csr(gpu, [(i, i + 1) for i in range(n - 1)], n=n)
    g = gpu.DeviceGraph.from_csr(csr)
    col, rnd, info = both_ends(gpu, g, None)  # one vertex per round: the one-workgroup tail; at 0 every round is a launch
    assert info == {"colors": 2, "rounds": n, "max_pred": 1, "first_round": 1}
    assert rnd.tolist() == list(range(n - 1, -1, -1)) and np.array_equal(col, 1 + (np.arange(n - 1, -1, -1) & 1))
    g.free()


def test_crown_graph_under_two_orders(gpu):
    k = 64  # u_i = i, v_j = k + j, u_i ~ v_j iff i != j
    csr = edges_to_csr(gpu, [(i, k + j) for i in range(k) for j in range(k) if i != j], n=2 * k)
    g = gpu.DeviceGraph.from_csr(csr)
    off, adj = csr.offsets(), csr.neighbors()
    interleaved = np.empty(2 * k, dtype=np.int32)  # coloured in the sequence u_0, v_0, u_1, v_1, …: the first of it has the highest position
    interleaved[np.arange(k)] = 2 * k - 1 - 2 * np.arange(k)
    interleaved[k + np.arange(k)] = 2 * k - 2 - 2 * np.arange(k)
    col, rnd, info = check_against_restatement(gpu, g, off, adj, interleaved)
    assert info["colors"] == k and col[:k].tolist() == list(range(1, k + 1)) and col[k:].tolist() == list(range(1, k + 1))
    sides = np.arange(2 * k - 1, -1, -1, dtype=np.int32)  # all u's, then all v's
    col, rnd, info = check_against_restatement(gpu, g, off, adj, sides)
    assert info["colors"] == 2 and info["rounds"] == 2 and np.all(col[:k] == 1) and np.all(col[k:] == 2)
    sequence = np.argsort(sides).astype(np.int32)  # the same priority in order format (position i = i-th vertex)
    col2, info2 = g.coloring_jp(sequence, rank_format=False)
    assert col2.tobytes() == col.tobytes() and info2 == info
    g.free()


def test_edgeless_and_empty(gpu):
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=1000))
    col, rnd, info = both_ends(gpu, g, None)
    assert np.all(col == 1) and np.all(rnd == 0) and info == {"colors": 1, "rounds": 1, "max_pred": 0, "first_round": 1000}
    assert g.coloring_verify(col) == {"conflicts": 0, "invalid": 0, "max_color": 1, "distinct": 1, "max_degree": 0}
    g.free()
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    assert g.num_nodes == 0
    col, rnd, info = both_ends(gpu, g, None)
    assert col.size == 0 and rnd.size == 0 and info == {"colors": 0, "rounds": 0, "max_pred": 0, "first_round": 0}
    assert g.coloring_jp(np.zeros(0, np.int32))[1] == info
    assert g.coloring_verify(np.zeros(0, np.int32)) == {"conflicts": 0, "invalid": 0, "max_color": 0, "distinct": 0, "max_degree": 0}
    g.free()


# ---- 3a. the hand-back between the one-workgroup kernel and the grid-wide ones -----------------------------------------------------------
def every_threshold(gpu, g, rank):
    """both_ends, plus a tiny COLOR_WG_FRONTIER and one that leaves every round it may take to the one-workgroup kernel: the same bytes"""
    col, rnd, info = both_ends(gpu, g, rank)
    for wg in (3, WG_ALL):
        with gpu.options(COLOR_WG_FRONTIER=wg):
            col2, rnd2, info2 = g.coloring_jp(rank, want_rounds=True)
        assert col2.tobytes() == col.tobytes() and rnd2.tobytes() == rnd.tobytes() and info2 == info, wg
    return col, rnd, info


@pytest.mark.parametrize("hubs,leaves", [(300, 1100),   # one frontier of 300 long rows: more than the one-workgroup kernel parks
                                         (450, 600)])   # short rows, 270 000 entries in one frontier: above its work bound
def test_independent_hubs_go_back_to_the_grid(gpu, hubs, leaves):
    n = hubs + hubs * leaves  # hub h = vertex h; its private leaves follow the hubs
    leaf = np.arange(hubs, n, dtype=np.int64)
    csr = edges_to_csr(gpu, np.stack([(leaf - hubs) // leaves, leaf], axis=1), n=n)
    g = gpu.DeviceGraph.from_csr(csr)
    col, rnd, info = every_threshold(gpu, g, None)  # the id order colours the highest ids, the leaves, first
    assert np.all(col[hubs:] == 1) and np.all(rnd[hubs:] == 0) and np.all(col[:hubs] == 2) and np.all(rnd[:hubs] == 1)
    assert info == {"colors": 2, "rounds": 2, "max_pred": leaves, "first_round": hubs * leaves}
    col, rnd, info = every_threshold(gpu, g, np.arange(n - 1, -1, -1, dtype=np.int32))  # reversed: the hubs first
    assert np.all(col[:hubs] == 1) and np.all(rnd[:hubs] == 0) and np.all(col[hubs:] == 2) and np.all(rnd[hubs:] == 1)
    assert info == {"colors": 2, "rounds": 2, "max_pred": 1, "first_round": hubs}
    g.free()


def test_star_of_40000_from_both_ends(gpu):
    leaves = 40000  # one row above the one-workgroup kernel's row bound, alone in its frontier
    csr = edges_to_csr(gpu, np.stack([np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1)], axis=1), n=leaves + 1)
    g = gpu.DeviceGraph.from_csr(csr)
    col, rnd, info = every_threshold(gpu, g, np.arange(leaves, -1, -1, dtype=np.int32))  # the hub first
    assert col[0] == 1 and np.all(col[1:] == 2) and rnd[0] == 0 and np.all(rnd[1:] == 1)
    assert info == {"colors": 2, "rounds": 2, "max_pred": 1, "first_round": 1}
    col, rnd, info = every_threshold(gpu, g, None)  # the hub last: 40 000 predecessors of colour 1
    assert col[0] == 2 and np.all(col[1:] == 1) and rnd[0] == 1 and np.all(rnd[1:] == 0)
    assert info == {"colors": 2, "rounds": 2, "max_pred": leaves, "first_round": leaves}
    g.free()


def test_golden_graph_at_every_threshold(gpu):
    key = "kronecker_12_16"  # at 3 the run switches between the one-workgroup kernel and the grid-wide ones many times
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    col, rnd, info = every_threshold(gpu, g, golden_rank(key, "degree"))
    rec = COL[key]["orders"]["degree"]
    assert col.tobytes() == COL_ARR["color_degree_" + key].tobytes() and info == {f: rec[f] for f in ("colors", "rounds", "max_pred", "first_round")}
    assert np.array_equal(rnd, jp_golden(gpu, key, "degree")[1])
    g.free()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    csr = host_graph(gpu, "kronecker", 8, 16, True)
    n = csr.num_nodes
    g = gpu.DeviceGraph.from_csr(csr)
    L = gpu.lib()
    col, rnd = np.full(n, -77, dtype=np.int32), np.full(n, -77, dtype=np.int32)
    cp, rp = col.ctypes.data_as(C.c_void_p), rnd.ctypes.data_as(C.c_void_p)
    good = g.degree_rank()
    info = gpu.ColoringInfo()
    info.colors, info.first_round = -5, -5
    assert L.gmsx_coloring_jp(g._h, good.ctypes.data_as(C.c_void_p), 1, cp, rp, None, None) == gpu.ERR_INVALID
    assert L.gmsx_coloring_jp(None, good.ctypes.data_as(C.c_void_p), 1, cp, rp, C.byref(info), None) == gpu.ERR_INVALID
    twice = good.copy()
    twice[3] = twice[4]                                  # a duplicate
    out_of_range = good.copy()
    out_of_range[5] = n                                  # an id = n
    negative = good.copy()
    negative[0] = -1
    for bad in (twice, out_of_range, negative):
        for fmt in (1, 0):
            assert L.gmsx_coloring_jp(g._h, bad.ctypes.data_as(C.c_void_p), fmt, cp, rp, C.byref(info), None) == gpu.ERR_INVALID
            with pytest.raises(gpu.GmsxError) as ei:
                g.coloring_jp(bad, rank_format=bool(fmt))
            assert ei.value.status == gpu.ERR_INVALID
    assert np.all(col == -77) and np.all(rnd == -77) and info.colors == -5 and info.first_round == -5
    chk = gpu.ColoringCheck()
    assert L.gmsx_coloring_verify(g._h, cp, None, None) == gpu.ERR_INVALID
    assert L.gmsx_coloring_verify(None, cp, C.byref(chk), None) == gpu.ERR_INVALID
    assert L.gmsx_coloring_verify(g._h, None, C.byref(chk), None) == gpu.ERR_INVALID
    assert L.gmsx_coloring_jp(g._h, good.ctypes.data_as(C.c_void_p), 1, cp, rp, C.byref(info), None) == gpu.OK
    assert col.min() >= 1 and col.max() == info.colors and rnd.min() == 0 and rnd.max() == info.rounds - 1
    g.free()


# ---- 5. verify ------------------------------------------------------------------------------------------------------------------------
def conflicts_np(off, adj, col):
    src = np.repeat(np.arange(off.size - 1), np.diff(off))
    return int(((col[src] == col[adj]) & (src < adj)).sum())


def test_verify_counts_planted_faults(gpu):
    csr = host_graph(gpu, "kronecker", 12, 16, True)
    off, adj = csr.offsets().astype(np.int64), csr.neighbors().astype(np.int64)
    n = off.size - 1
    g = gpu.DeviceGraph.from_csr(csr)
    col, info = g.color("lf")
    clean = {"conflicts": 0, "invalid": 0, "max_color": info["colors"], "distinct": info["colors"], "max_degree": int(np.diff(off).max())}
    assert g.coloring_verify(col) == clean
    rng = np.random.default_rng(11)
    planted = col.copy()
    for v in rng.choice(np.flatnonzero(np.diff(off) > 0), 50, replace=False):  # 50 vertices take a neighbour's colour
        planted[v] = planted[adj[off[v] + rng.integers(off[v + 1] - off[v])]]
    want = conflicts_np(off, adj, planted)
    assert want >= 1
    chk = g.coloring_verify(planted)
    assert chk["conflicts"] == want and chk["invalid"] == 0 and chk["distinct"] == np.unique(planted).size
    zeroed = col.copy()
    v = int(np.flatnonzero(np.diff(off) > 0)[7])
    zeroed[v] = 0
    chk = g.coloring_verify(zeroed)
    assert chk["invalid"] == 1 and chk["conflicts"] == 0 and chk["distinct"] == np.unique(zeroed).size == np.unique(col[np.arange(n) != v]).size + 1
    odd = col.copy()  # colours the presence bitmap does not cover are still counted
    odd[1], odd[2], odd[3] = -3, n + 9, n + 9
    chk = g.coloring_verify(odd)
    assert chk["invalid"] == 1 and chk["max_color"] == n + 9 and chk["distinct"] == np.unique(odd).size and chk["conflicts"] == conflicts_np(off, adj, odd)
    g.free()


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------
CHILD = """import sys, hashlib
sys.path.insert(0, %r)
import numpy as np
from gms_amd import capi
capi.init(0)
csr = capi.HostCSR.generate('kronecker', 12, 16, capi.RELABEL_AUTO)
g = capi.DeviceGraph.from_csr(csr)
perm = np.load(%r)['perm_kronecker_12_16']
col, rnd, info = g.coloring_jp(perm, want_rounds=True)
print(hashlib.sha256(col.tobytes() + rnd.tobytes()).hexdigest(), info['colors'], info['rounds'], info['max_pred'], info['first_round'])
"""


def test_same_bytes_in_every_call_and_process(gpu):
    key = "kronecker_12_16"
    csr = golden_csr(gpu, key)
    g = gpu.DeviceGraph.from_csr(csr)
    perm = golden_rank(key, "random")
    col, rnd, info = g.coloring_jp(perm, want_rounds=True)
    col2, rnd2, info2 = g.coloring_jp(perm, want_rounds=True)
    assert col2.tobytes() == col.tobytes() and rnd2.tobytes() == rnd.tobytes() and info2 == info
    assert col.tobytes() == COL_ARR["color_random_" + key].tobytes()
    g.free()
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests", "golden", "coloring.npz"))], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    want = [hashlib.sha256(col.tobytes() + rnd.tobytes()).hexdigest()] + [str(info[f]) for f in ("colors", "rounds", "max_pred", "first_round")]
    assert out.stdout.split() == want
