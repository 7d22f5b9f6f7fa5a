"""CPU: the goldens of gmsx_label_propagation and gmsx_modularity (tests/golden/communities.{json,npz}; tools/make_golden_communities.py) against
restatements in plain Python / numpy, which are also what tests/test_communities_gpu.py holds the device to:
  * lp_seq — THE restatement of include/gmsx.h: the sequential asynchronous propagation that visits the vertices ascending by (colour, id); a
    vertex keeps its label if that is a heaviest one among its neighbours, else takes the smallest heaviest label.  It also returns the rise
    of the monochromatic weight at every change;
  * lp_np — the same sweeps colour class by colour class in numpy (a class is an independent set, so its vertices can act at once); it equals
    lp_seq wherever both are run, and is what the larger graphs use;
  * mod_np — W, I, S = Σ D_c² as Python integers, communities, largest, unstable, and Q by the library's fixed expression in numpy's long double.
The reference has no community detection.  Q: the integers are compared exactly; the double is held to 1 ulp, because numpy's long double is
the C one only where the platform gives it 80 bits."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph, load_golden
from test_coloring_golden_cpu import COL, COL_ARR, jp_np
from test_core_golden_cpu import golden_csr as core_golden_csr
from test_core_golden_cpu import rows_of
from test_msf_golden_cpu import golden_csr as weighted_golden_csr

J = load_golden("communities.json")
ARR = np.load(os.path.join(GOLDEN, "communities.npz"))
UNWEIGHTED = ["file_eppsteinExample", "file_micro", "file_smallRandom1", "file_tomitaExample", "file_triangles_1", "file_triangles_3",
              "kronecker_10_16", "kronecker_10_16_plain", "kronecker_12_16", "kronecker_14_16"]   # kronecker_10_16_plain: not relabelled
WEIGHTED = ["file_two_parts_a", "file_two_parts_b", "kronecker_10_16", "kronecker_10_16_relabelled", "kronecker_12_16", "kronecker_14_16"]
COLORINGS = ("default", "lf")
INFO_KEYS = ("communities", "largest", "singletons", "changes", "first_sweep_changes", "sweeps", "colors", "converged", "largest_label")
MOD_KEYS = ("total_weight", "intra_weight", "sumsq", "communities", "largest", "unstable")
ARRAY_MAX_N = 1 << 12
SWEEP_CAP = 1000
LP_OPTIONS = ("LP_WAVE_ROW", "LP_LDS_ROW", "LP_LDS_SLOTS", "LP_WG_WORK", "LP_ACTIVE")


def graph_ids():
    return [("u", k) for k in UNWEIGHTED] + [("w", k) for k in WEIGHTED]


_CSR = {}


def graph_arrays(capi, kind, key):
    """(off int64, adj int32, w int32 or None) of a golden graph; kind 'u': the unweighted graphs, 'w': the weighted ones"""
    if (kind, key) not in _CSR:
        if kind == "w":
            c = weighted_golden_csr(capi, key)
            w = np.array(c.weights(), dtype=np.int32)
        else:
            c = host_graph(capi, "kronecker", 10, 16, False) if key == "kronecker_10_16_plain" else core_golden_csr(capi, key)
            w = None
        _CSR[(kind, key)] = (np.array(c.offsets(), dtype=np.int64), np.array(c.neighbors(), dtype=np.int32), w)
    return _CSR[(kind, key)]


def lf_rank(off):
    """largest first: the vertex of the highest rank is coloured first — the largest degree, of equal degrees the smallest id"""
    deg = np.diff(np.asarray(off, dtype=np.int64))
    order = np.lexsort((-np.arange(deg.size), deg))
    rank = np.empty(deg.size, dtype=np.int32)
    rank[order] = np.arange(deg.size, dtype=np.int32)
    return rank


def sl_rank(off, adj):
    """smallest last: the vertices are removed by smallest remaining degree (ties: the smallest id); the one removed LAST is coloured first"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    deg = np.diff(off).copy()
    gone = np.zeros(n, dtype=bool)
    rank = np.empty(n, dtype=np.int32)
    for i in range(n):
        v = int(np.flatnonzero(~gone)[np.argmin(deg[~gone])])
        gone[v] = True
        rank[v] = i
        deg[adj[off[v]:off[v + 1]]] -= 1
    return rank


def coloring_of(off, adj, which):
    n = len(off) - 1
    rank = np.arange(n, dtype=np.int32) if which == "default" else lf_rank(off) if which == "lf" else sl_rank(off, adj)
    return jp_np(off, adj, rank)[0]


def lp_seq(off, adj, w, color, max_sweeps=0):
    """(label, info, rises): rises = by how much the total weight of the arcs whose ends share a label (both directions) rose at every change"""
    n = len(off) - 1
    offl, adjl = [int(x) for x in off], [int(x) for x in adj]
    wl = [1] * len(adjl) if w is None else [int(x) for x in w]
    order = sorted(range(n), key=lambda v: (int(color[v]), v))
    label = list(range(n))
    cap = SWEEP_CAP if max_sweeps == 0 else max_sweeps
    rises, sweeps, changes, first, converged = [], 0, 0, 0, 0
    while sweeps < cap:
        here = 0
        for v in order:
            tot = {}
            for j in range(offl[v], offl[v + 1]):
                tot[label[adjl[j]]] = tot.get(label[adjl[j]], 0) + wl[j]
            if not tot:
                continue
            m = max(tot.values())
            own = tot.get(label[v], 0)
            if own == m:
                continue
            label[v] = min(l for l, t in tot.items() if t == m)
            rises.append(2 * (m - own))
            here += 1
        sweeps += 1
        changes += here
        if sweeps == 1:
            first = here
        if here == 0:
            converged = 1
            break
    label = np.array(label, dtype=np.int32)
    return label, lp_info(label, color, sweeps, changes, first, converged), rises


def lp_info(label, color, sweeps, changes, first, converged):
    n = label.size
    sizes = np.bincount(label, minlength=max(n, 1))[:n] if n else np.zeros(0, dtype=np.int64)
    return {"communities": int((sizes > 0).sum()), "largest": int(sizes.max()) if n else 0, "singletons": int((sizes == 1).sum()),
            "changes": int(changes), "first_sweep_changes": int(first), "sweeps": int(sweeps), "colors": int(np.max(color)) if n else 0,
            "converged": int(converged), "largest_label": int(np.argmax(sizes)) if n else 0}


def evaluate_np(off, adj, w, label, vs):
    """for the vertices vs (all with an arc): (M, the smallest label at M, W_v(own)) as int64 arrays"""
    n = off.size - 1
    idx = rows_of(off, vs)
    lens = off[vs + 1] - off[vs]
    owner = np.repeat(np.arange(vs.size, dtype=np.int64), lens)
    lab = label[adj[idx]].astype(np.int64)
    ww = np.ones(idx.size, dtype=np.int64) if w is None else w[idx].astype(np.int64)
    key = owner * n + lab
    order = np.argsort(key, kind="stable")
    key, ww = key[order], ww[order]
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    sums = np.add.reduceat(ww, start)
    o, l = key[start] // n, key[start] % n
    first = np.flatnonzero(np.concatenate([[True], o[1:] != o[:-1]]))   # every owner has an entry, and they ascend
    m = np.maximum.reduceat(sums, first)
    best = np.minimum.reduceat(np.where(sums == m[o], l, n), first)
    own = np.zeros(vs.size, dtype=np.int64)
    mine = l == label[vs][o]
    own[o[mine]] = sums[mine]
    return m, best, own


def lp_np(off, adj, w, color, max_sweeps=0):
    """(label, info, rise): the sweeps class by class; rise = the total rise of the monochromatic weight, every change's share of it positive"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    color = np.asarray(color, dtype=np.int64)
    deg = np.diff(off)
    classes = [np.flatnonzero((color == c) & (deg > 0)) for c in range(1, int(color.max()) + 1)] if n else []
    label = np.arange(n, dtype=np.int64)
    cap = SWEEP_CAP if max_sweeps == 0 else max_sweeps
    rise, sweeps, changes, first, converged = 0, 0, 0, 0, 0
    while sweeps < cap:
        here = 0
        for vs in classes:
            if vs.size == 0:
                continue
            m, best, own = evaluate_np(off, adj, w, label, vs)
            move = own < m
            assert np.all(m[move] - own[move] > 0)
            rise += 2 * int((m[move] - own[move]).sum())
            label[vs[move]] = best[move]
            here += int(move.sum())
        sweeps += 1
        changes += here
        if sweeps == 1:
            first = here
        if here == 0:
            converged = 1
            break
    label = label.astype(np.int32)
    return label, lp_info(label, color, sweeps, changes, first, converged), rise


def q_of(total, intra, sumsq):
    """the library's fixed expression, in numpy's long double, rounded to double once"""
    if total == 0:
        return 0.0
    L = np.longdouble
    w = L(total)
    sq = L(sumsq >> 64) * L(18446744073709551616.0) + L(sumsq & 0xFFFFFFFFFFFFFFFF)
    return float(L(intra) / w - sq / (w * w))


def mod_np(off, adj, w, label):
    off, adj, label = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64), np.asarray(label, dtype=np.int64)
    n = off.size - 1
    ww = np.ones(adj.size, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    wdeg = np.zeros(n, dtype=np.int64)
    np.add.at(wdeg, src, ww)
    d = {}
    for l, x in zip(label.tolist(), wdeg.tolist()):
        d[l] = d.get(l, 0) + x
    total, intra = int(ww.sum()), int(ww[label[src] == label[adj]].sum())
    sumsq = sum(x * x for x in d.values())
    vs = np.flatnonzero(np.diff(off) > 0)
    unstable = 0
    if vs.size:
        m, _, own = evaluate_np(off, adj, None if w is None else ww, label, vs)
        unstable = int((own < m).sum())
    sizes = np.bincount(label, minlength=max(n, 1))
    return {"total_weight": total, "intra_weight": intra, "sumsq": sumsq, "communities": int((sizes > 0).sum()),
            "largest": int(sizes.max()) if n else 0, "unstable": unstable, "modularity": q_of(total, intra, sumsq)}


def cc_labels_np(off, adj):
    """the smallest vertex id of every vertex's connected component"""
    off, adj = np.asarray(off, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    n = off.size - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    label = np.arange(n, dtype=np.int64)
    while True:
        nxt = label.copy()
        np.minimum.at(nxt, src, label[adj])
        nxt = nxt[nxt]
        if np.array_equal(nxt, label):
            return label.astype(np.int32)
        label = nxt


def ulps_apart(a, b):
    x, y = np.array([a, b], dtype=np.float64).view(np.int64)
    return abs(int(x) - int(y)) if (a >= 0) == (b >= 0) else (0 if a == b else 2)


def sha_of(label):
    return hashlib.sha256(np.ascontiguousarray(label, dtype="<i4").tobytes()).hexdigest()


def fnv_of(label):
    """FNV-1a over the same bytes: what the C++ adaptor test prints"""
    x = 1469598103934665603
    for b in np.ascontiguousarray(label, dtype="<i4").tobytes():
        x = ((x ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return x


def rec_id(r):
    return "%s-%s-%s" % ("w" if r["weighted"] else "u", r["graph"], r["coloring"])


def mod_record(m):
    """a modularity dict as the JSON keeps it (sumsq as a decimal string, Q as a hex float)"""
    return dict({k: m[k] for k in MOD_KEYS if k != "sumsq"}, sumsq=str(m["sumsq"]), modularity=float(m["modularity"]).hex())


_RUN = {}


def run(capi, rec):
    """lp_np of one golden record, computed once per session (the GPU tests share it): (off, adj, w, color, label, info, rise)"""
    k = rec_id(rec)
    if k not in _RUN:
        off, adj, w = graph_arrays(capi, "w" if rec["weighted"] else "u", rec["graph"])
        color = coloring_of(off, adj, rec["coloring"])
        _RUN[k] = (off, adj, w, color) + lp_np(off, adj, w, color)
    return _RUN[k]


def test_goldens_are_complete():
    want = sorted("%s-%s-%s" % (kind, key, c) for kind, key in graph_ids() for c in COLORINGS)
    assert sorted(rec_id(r) for r in J["records"]) == want and len(want) == 32
    for r in J["records"]:
        assert set(INFO_KEYS) <= set(r) and len(r["sha256"]) == 64 and set(r["mod"]) == set(r["mod_cc"]) == set(MOD_KEYS) | {"modularity"}
        assert (("label_" + rec_id(r)) in ARR.files) == (r["n"] <= ARRAY_MAX_N), rec_id(r)
    for name in ("communities.json", "communities.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20


@pytest.mark.parametrize("rec", J["records"], ids=rec_id)
def test_restatement_reproduces_the_golden(capi, rec):
    off, adj, w, color, label, info, rise = run(capi, rec)
    n = off.size - 1
    assert (n, adj.size) == (rec["n"], rec["nnz"])
    if rec["coloring"] == "default" and not rec["weighted"] and rec["graph"] in COL:   # the default colouring is the golden of coloring.npz
        assert np.array_equal(color, COL_ARR["color_id_" + rec["graph"]])
    assert info == {k: rec[k] for k in INFO_KEYS}
    assert sha_of(label) == rec["sha256"] and str(fnv_of(label)) == rec["fnv"]
    if n <= ARRAY_MAX_N:
        assert np.array_equal(ARR["label_" + rec_id(rec)], label)
    # the monochromatic weight starts at 0 (all labels distinct), rises strictly with every change, and ends at I
    m = mod_np(off, adj, w, label)
    assert rise == m["intra_weight"] and rec["converged"] == 1 and m["unstable"] == 0
    for got, key in ((m, "mod"), (mod_np(off, adj, w, cc_labels_np(off, adj)), "mod_cc")):
        assert {k: got[k] for k in MOD_KEYS if k != "sumsq"} == {k: rec[key][k] for k in MOD_KEYS if k != "sumsq"}
        assert str(got["sumsq"]) == rec[key]["sumsq"]
        assert ulps_apart(got["modularity"], float.fromhex(rec[key]["modularity"])) <= 1
    assert rec["mod_cc"]["intra_weight"] == rec["mod_cc"]["total_weight"]   # no arc leaves a component
    assert info["communities"] == m["communities"] and info["largest"] == m["largest"]


@pytest.mark.parametrize("rec", [r for r in J["records"] if r["n"] <= 1 << 10], ids=rec_id)
def test_the_sequential_loop_is_the_class_wise_one(capi, rec):
    off, adj, w, color, label, info, rise = run(capi, rec)
    slabel, sinfo, rises = lp_seq(off, adj, w, color)
    assert np.array_equal(slabel, label) and sinfo == info
    assert all(r > 0 for r in rises) and sum(rises) == rise and len(rises) == info["changes"]
    for cap in (1, 2):
        a, b = lp_seq(off, adj, w, color, cap), lp_np(off, adj, w, color, cap)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1]["sweeps"] == min(cap, info["sweeps"])


def csr_of(edges, n, weights=None):
    """symmetric CSR (off, adj, w) of an edge list"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    ww = np.ones(len(e), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    e, ww = np.concatenate([e, e[:, ::-1]]), np.concatenate([ww, ww])
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, ww = e[order], ww[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]).astype(np.int64)
    return off, e[:, 1].astype(np.int32), (None if weights is None else ww.astype(np.int32))


def test_rules_on_small_shapes():
    # K_5 under the default colouring (vertex 4 first: colour 1 … vertex 0 last): every label ends at the smallest id that is reached first
    off, adj, _ = csr_of([(i, j) for i in range(5) for j in range(i)], 5)
    label, info, _ = lp_seq(off, adj, None, coloring_of(off, adj, "default"))
    assert label.tolist() == [0] * 5 and info["communities"] == 1 and info["converged"] == 1 and info["colors"] == 5
    # the keep rule: vertex 2 holds label 2 and sees labels {2, 0} once each (its neighbours 3 -> 2 and 0): it keeps 2 although 0 is smaller
    off, adj, _ = csr_of([(0, 2), (2, 3)], 4)
    color = np.array([3, 1, 2, 1], dtype=np.int32)   # 3 acts first and takes 2; then 2 (a tie between 0 and its own 2), then 0
    label, info, _ = lp_seq(off, adj, None, color)
    assert label.tolist() == [2, 1, 2, 2] and info["singletons"] == 1
    # weights: one arc of 7 beats three arcs of 2 to another label
    off, adj, w = csr_of([(0, 1), (0, 2), (0, 3), (0, 4), (2, 3), (3, 4)], 5, [7, 2, 2, 2, 9, 9])
    label, _, _ = lp_seq(off, adj, w, np.array([4, 2, 1, 2, 3], dtype=np.int32))   # 2, 3 and 4 end with label 3; 0 sees 7 for its own label against 3 x 2
    assert label[0] == label[1]
    # modularity of two K_8 joined by one edge: W = 2 * 57, I = 2 * 56, D = 57 each
    off, adj, _ = csr_of([(i, j) for i in range(8) for j in range(i)] + [(8 + i, 8 + j) for i in range(8) for j in range(i)] + [(0, 8)], 16)
    m = mod_np(off, adj, None, np.repeat([0, 8], 8))
    assert (m["total_weight"], m["intra_weight"], m["sumsq"], m["unstable"]) == (114, 112, 2 * 57 * 57, 0)
    assert m["modularity"] == q_of(114, 112, 6498) and abs(m["modularity"] - (112 / 114 - 0.5)) < 1e-15
    assert mod_np(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), None, np.arange(3))["modularity"] == 0.0


def test_new_symbols_declared_exported_and_documented(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmsx.h")).read()
    for name in ("gmsx_label_propagation", "gmsx_modularity"):
        assert hasattr(L, name) and name in capi.SYMBOLS and re.search(r"\bint %s\(" % name, hdr), name
    assert "} gmsx_lp_info;" in hdr and "} gmsx_modularity_info;" in hdr and "GMSX_LP_WEIGHTED = 1u" in hdr
    for opt in LP_OPTIONS:
        assert opt in capi.option_names() and re.search(r"\b%s\b" % opt, hdr), opt
    assert ctypes.sizeof(capi.LpInfo) == 56 and ctypes.sizeof(capi.ModularityInfo) == 64 and capi.LP_WEIGHTED == 1
    assert capi.lib().gmsx_version() == 320
