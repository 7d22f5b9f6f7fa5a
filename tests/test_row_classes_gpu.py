"""GPU: the row classes of gms_amd/csrc/hip/row_classes.hpp at their edges, once for each of their four users.  One graph (bins_graph: vertex i
is the hub of a star of BIN_DEGREES[i] leaves: 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097) goes through
gmsx_connected_components, gmsx_biconnected_components, gmsx_min_spanning_forest and gmsx_greedy_matching under three settings of the
algorithm's own …_WAVE_ROW / …_WG_ROW: the defaults, (4, 8) and (17, 65), so that a row sits just below, on and just above every bound in
use.  The weights are seeded per undirected edge, which puts a row's winning arc at an arbitrary lane.  Every array and info block equals
the restatement of the algorithm's *_golden_cpu.py module exactly, and for each algorithm the three settings give the same bytes.

The two-width pass of the same header (msf's count and fill, matching_verify's check, bicc's ranks, the pull pass of sssp and sssp_verify) has
one bound, 1024 entries; the second half of this file puts rows below, on and above it and checks the same way, launches included."""
import numpy as np
import pytest

from test_bicc_golden_cpu import bicc_np
from test_components_golden_cpu import BIN_DEGREES, INFO_KEYS, bins_graph, components_np
from test_matching_golden_cpu import greedy_np, pairs_np, rounds_np
from test_matching_golden_cpu import info_np as matching_info_np
from test_msf_golden_cpu import boruvka_np, kruskal_np, labels_np, mask_np
from test_msf_golden_cpu import info_np as msf_info_np
from test_sssp_golden_cpu import dijkstra_np, parent_np, verify_np
from test_sssp_golden_cpu import info_np as sssp_info_np

pytestmark = pytest.mark.gpu

SSSP_FACTS = ("reached", "reached_arcs", "dist_sum", "max_dist", "far_vertex")
BINS = (None, (4, 8), (17, 65))   # …_WAVE_ROW, …_WG_ROW; None: the defaults 256, 4096


def bin_options(prefix, bins):
    return {} if bins is None else {prefix + "_WAVE_ROW": bins[0], prefix + "_WG_ROW": bins[1]}


def same_bytes(runs):
    """every run's arrays are the first run's, byte for byte"""
    return all(len(r) == len(runs[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(r, runs[0])) for r in runs[1:])


@pytest.fixture(scope="module")
def stars(gpu):
    """(handle with the weights attached, off, adj, w) of the graph"""
    e, n = bins_graph(BIN_DEGREES)
    w = np.random.RandomState(1).randint(1, 256, size=len(e))
    csr = gpu.HostCSR.from_weighted_edges(e[:, 0], e[:, 1], w, num_nodes=n)
    off, adj, wgt = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32), np.array(csr.weights(), dtype=np.int32)
    assert np.diff(off)[:len(BIN_DEGREES)].tolist() == BIN_DEGREES and off.size - 1 == n
    g = gpu.DeviceGraph.from_csr(csr)
    g.set_weights(csr.weights())
    yield g, off, adj, wgt
    g.free()


def test_components(gpu, stars):
    g, off, adj, _ = stars
    want, want_info = components_np(off, adj)
    runs = []
    for bins in BINS:
        with gpu.options(**bin_options("CC", bins)):
            label, info = g.connected_components()
        assert np.array_equal(label, want) and {k: info[k] for k in INFO_KEYS} == want_info, bins
        runs.append((label,))
    assert same_bytes(runs) and want_info["components"] == len(BIN_DEGREES)


def test_bicc(gpu, stars):
    g, off, adj, _ = stars
    wb, wa, wk, wi = bicc_np(off, adj)
    runs = []
    for bins in BINS:
        with gpu.options(**bin_options("BCC", bins)):
            block, at, keep, info = g.biconnected_components(want_mask=True)
        assert info == wi, bins
        assert np.array_equal(block, wb) and np.array_equal(at, wa) and np.array_equal(keep, wk), bins
        runs.append((block, at, keep))
    assert same_bytes(runs) and wi["bridges"] == sum(BIN_DEGREES)


@pytest.mark.parametrize("maximum", [False, True])
def test_msf(gpu, stars, maximum):
    g, off, adj, w = stars
    u, v, ww = kruskal_np(off, adj, w, maximum)
    rounds = boruvka_np(off, adj, w, maximum)[1]
    want_mask, want_label, want_info = mask_np(off, adj, u, v), labels_np(off.size - 1, u, v), msf_info_np(off, u, v, ww, rounds)
    for prune in (0, 1):
        runs, examined = [], []
        for bins in BINS:
            with gpu.options(MSF_PRUNE=prune, **bin_options("MSF", bins)):
                r = g.min_spanning_forest(maximum=maximum, want_edges=True, want_mask=True, want_labels=True, stats=True)
            assert r[5] == want_info, (prune, bins)
            assert np.array_equal(r[0], u) and np.array_equal(r[1], v) and np.array_equal(r[2], ww), (prune, bins)
            assert np.array_equal(r[3], want_mask) and np.array_equal(r[4], want_label), (prune, bins)
            runs.append(r[:5])
            examined.append(r[6]["alg_elements"])
        assert same_bytes(runs)
        if prune == 0:   # the arcs examined do not depend on who walks a row
            assert len(set(examined)) == 1 and examined[0] > 0, examined


@pytest.mark.parametrize("weighted", [True, False])
def test_matching(gpu, stars, weighted):
    g, off, adj, w = stars
    ww = w if weighted else None
    want = greedy_np(off, adj, ww)
    by_rounds, rounds = rounds_np(off, adj, ww)
    assert np.array_equal(by_rounds, want)
    eu, ev, ew = pairs_np(off, adj, ww, want)
    want_info = matching_info_np(off, adj, ww, want, rounds)
    for keep in (0, 1):
        runs = []
        for bins in BINS:
            with gpu.options(MATCH_KEEP=keep, **bin_options("MATCH", bins)):
                mate, pu, pv, pw, info = g.greedy_matching(weighted=weighted, want_mate=True, want_edges=True)
                c = g.matching_verify(mate, weighted=weighted)
            assert info == want_info, (keep, bins)
            assert np.array_equal(mate, want) and np.array_equal(pu, eu) and np.array_equal(pv, ev) and np.array_equal(pw, ew), (keep, bins)
            assert c["invalid"] == 0 and c["undominated"] == 0 and c["pairs"] == info["pairs"], (keep, bins)
            runs.append((mate, pu, pv, pw))
        assert same_bytes(runs)


# ---- the two-width pass (launch_rows_two_width): a 16-lane group per row of at most LONG_ROW entries, a wave per longer row ------------------
# Its one bound is LONG_ROW, which BIN_DEGREES does not touch.  Two graphs: stars of 1, 15, 16, 17, 1023 and 1024 leaves and three isolated
# vertices ("narrow": no row is long, the wave launch is not made), and the same with stars of 1025 and 2049 leaves ("wide").  A hub's row
# holds its leaves in ascending order, so the leaf at position k of hub h's row is known.
LONG_ROW = 1024   # kLongRow of frontier_rounds.hpp
NARROW_DEGREES = [1, 15, 16, 17, LONG_ROW - 1, LONG_ROW]
WIDE_DEGREES = NARROW_DEGREES + [LONG_ROW + 1, 2 * LONG_ROW + 1]
ISOLATED = 3
GROUP_HUB, WAVE_HUB = 5, 6   # the hubs of the 1024 star (the longest group-walked row) and of the 1025 star (the shortest wave-walked one)

# gmsx_stats.launches of every call below, AS THE COMMIT BEFORE THE TWO-WIDTH PLAN REPORTED THEM on an MI355X for the same call on the same
# graph (its library run once through this file; the numbers were not taken from the library under test).
LAUNCHES = {
    "narrow": {
        "bicc": 47, "matching_unit": 11, "matching_verify_free_unit": 2, "matching_verify_free_weighted": 2, "matching_verify_greedy_unit": 2,
        "matching_verify_greedy_weighted": 2, "matching_weighted": 11, "msf_max": 18, "msf_min": 18, "sssp_group_hub": 8, "sssp_group_leaf_0": 8,
        "sssp_group_leaf_1023": 8, "sssp_group_leaf_63": 8, "sssp_group_leaf_64": 8, "sssp_isolated": 5, "sssp_verify_true": 1,
        "sssp_verify_wrong": 1,
    },
    "wide": {
        "bicc": 49, "matching_unit": 11, "matching_verify_free_unit": 3, "matching_verify_free_weighted": 3, "matching_verify_greedy_unit": 3,
        "matching_verify_greedy_weighted": 3, "matching_weighted": 11, "msf_max": 20, "msf_min": 20, "sssp_group_hub": 9, "sssp_group_leaf_0": 9,
        "sssp_group_leaf_1023": 9, "sssp_group_leaf_63": 9, "sssp_group_leaf_64": 9, "sssp_isolated": 6, "sssp_verify_true": 2,
        "sssp_verify_wrong": 2, "sssp_wave_hub": 9, "sssp_wave_leaf_0": 9, "sssp_wave_leaf_1024": 9, "sssp_wave_leaf_63": 9, "sssp_wave_leaf_64": 9,
    },
}
# the two-width passes of a call: where the graph has a long row each of them is one launch more, and nothing else changes
TWO_WIDTH_PASSES = {"msf": 2, "matching": 0, "matching_verify": 1, "bicc": 2, "sssp": 1, "sssp_verify": 1}


def launches_are(kind, call, st):
    """the launches of a call against the recorded ones (printed first: -s shows what a library reports)"""
    print(f"launches {kind} {call} {st['launches']}")
    assert st["launches"] == LAUNCHES[kind][call], (kind, call, st["launches"])


def two_width_edges(kind):
    degrees = WIDE_DEGREES if kind == "wide" else NARROW_DEGREES
    e, n = bins_graph(degrees)
    return degrees, e, n + ISOLATED, np.random.RandomState(2).randint(1, 256, size=len(e))


def leaf_at(off, adj, hub, k):
    """the leaf at position k of hub's row"""
    return int(adj[off[hub] + k])


def sssp_sources(kind, off, adj):
    """name -> source: hubs, the leaves that are the one tight entry at a stated position of their hub's row, an isolated vertex"""
    n = off.size - 1
    s = {"group_hub": GROUP_HUB, "isolated": n - 1}
    s.update({f"group_leaf_{k}": leaf_at(off, adj, GROUP_HUB, k) for k in (0, 63, 64, LONG_ROW - 1)})
    if kind == "wide":
        s["wave_hub"] = WAVE_HUB
        s.update({f"wave_leaf_{k}": leaf_at(off, adj, WAVE_HUB, k) for k in (0, 63, 64, LONG_ROW)})
    return s


@pytest.fixture(scope="module", params=["narrow", "wide"])
def long_rows(gpu, request):
    """(kind, handle with the weights attached, off, adj, w, undirected edges) of one of the two graphs"""
    kind = request.param
    degrees, e, n, w = two_width_edges(kind)
    csr = gpu.HostCSR.from_weighted_edges(e[:, 0], e[:, 1], w, num_nodes=n)
    off, adj, wgt = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32), np.array(csr.weights(), dtype=np.int32)
    deg = np.diff(off)
    assert deg[:len(degrees)].tolist() == degrees and off.size - 1 == n and np.all(deg[-ISOLATED:] == 0)
    assert (deg.max() > LONG_ROW) == (kind == "wide")
    for hub in (GROUP_HUB, WAVE_HUB)[:2 if kind == "wide" else 1]:   # a hub's row is its leaves, ascending and consecutive
        assert np.array_equal(adj[off[hub]:off[hub + 1]], adj[off[hub]] + np.arange(deg[hub]))
    g = gpu.DeviceGraph.from_csr(csr)
    g.set_weights(csr.weights())
    yield kind, g, off, adj, wgt, len(e)
    g.free()


def test_recorded_launches_differ_by_the_two_width_passes():
    """between the two graphs a call's launches differ by its two-width passes: only they are launched once more for the long rows"""
    narrow, wide = LAUNCHES["narrow"], LAUNCHES["wide"]
    assert set(narrow) <= set(wide) and all(call.startswith("sssp_wave_") for call in set(wide) - set(narrow))
    for call in narrow:
        algorithm = max((a for a in TWO_WIDTH_PASSES if call.startswith(a)), key=len)   # "matching_verify_…" is not "matching"
        assert wide[call] - narrow[call] == TWO_WIDTH_PASSES[algorithm], call


@pytest.mark.parametrize("maximum", [False, True])
def test_two_width_msf(long_rows, maximum):
    kind, g, off, adj, w, _ = long_rows
    u, v, ww = kruskal_np(off, adj, w, maximum)
    rounds = boruvka_np(off, adj, w, maximum)[1]
    r = g.min_spanning_forest(maximum=maximum, want_edges=True, want_mask=True, want_labels=True, stats=True)
    assert r[5] == msf_info_np(off, u, v, ww, rounds)
    assert np.array_equal(r[0], u) and np.array_equal(r[1], v) and np.array_equal(r[2], ww)
    assert np.array_equal(r[3], mask_np(off, adj, u, v)) and np.array_equal(r[4], labels_np(off.size - 1, u, v))
    launches_are(kind, "msf_max" if maximum else "msf_min", r[6])


@pytest.mark.parametrize("weighted", [True, False])
def test_two_width_matching(long_rows, weighted):
    kind, g, off, adj, w, edges = long_rows
    ww, name = (w, "weighted") if weighted else (None, "unit")
    want = greedy_np(off, adj, ww)
    eu, ev, ew = pairs_np(off, adj, ww, want)
    mate, pu, pv, pw, info, st = g.greedy_matching(weighted=weighted, want_mate=True, want_edges=True, stats=True)
    assert info == matching_info_np(off, adj, ww, want, rounds_np(off, adj, ww)[1])
    assert np.array_equal(mate, want) and np.array_equal(pu, eu) and np.array_equal(pv, ev) and np.array_equal(pw, ew)
    launches_are(kind, "matching_" + name, st)
    c, st = g.matching_verify(mate, weighted=weighted, stats=True)
    assert c["invalid"] == 0 and c["augmentable"] == 0 and c["undominated"] == 0 and c["pairs"] == info["pairs"]
    launches_are(kind, "matching_verify_greedy_" + name, st)
    # nobody matched: every edge is augmentable and undominated, the long rows' share included
    c, st = g.matching_verify(np.full(off.size - 1, -1, dtype=np.int32), weighted=weighted, stats=True)
    assert c["invalid"] == 0 and c["pairs"] == 0 and c["augmentable"] == edges and c["undominated"] == edges
    launches_are(kind, "matching_verify_free_" + name, st)


def test_two_width_bicc(long_rows):
    kind, g, off, adj, _, edges = long_rows
    wb, wa, wk, wi = bicc_np(off, adj)
    block, at, keep, info, st = g.biconnected_components(want_mask=True, stats=True)
    assert info == wi and wi["bridges"] == edges and wi["isolated"] == ISOLATED
    assert np.array_equal(block, wb) and np.array_equal(at, wa) and np.array_equal(keep, wk)
    launches_are(kind, "bicc", st)


def test_two_width_sssp(long_rows):
    kind, g, off, adj, w, _ = long_rows
    for name, source in sssp_sources(kind, off, adj).items():
        want = dijkstra_np(off, adj, w, source)
        dist, parent, info, st = g.sssp(source, stats=True)
        assert np.array_equal(dist, want) and np.array_equal(parent, parent_np(off, adj, w, source, want)), name
        assert {k: info[k] for k in SSSP_FACTS} == sssp_info_np(off, want), (name, info)
        launches_are(kind, "sssp_" + name, st)


def test_two_width_sssp_verify(long_rows):
    kind, g, off, adj, w, _ = long_rows
    hub = WAVE_HUB if kind == "wide" else GROUP_HUB   # the longest row the graph's plan walks with its widest class
    source = leaf_at(off, adj, hub, 0)
    dist = dijkstra_np(off, adj, w, source)
    c, st = g.sssp_verify(source, dist, stats=True)
    assert c == {"violated_arcs": 0, "untight": 0, "wrong_unreached": 0, "source_ok": 1} == verify_np(off, adj, w, source, dist)
    launches_are(kind, "sssp_verify_true", st)
    wrong = dist.copy()
    wrong[hub] += 1                            # the hub's row: its arc from the source is violated, and no entry is tight
    wrong[leaf_at(off, adj, hub, 64)] = -1     # an unreached leaf beside the reached hub
    want = verify_np(off, adj, w, source, wrong)
    assert want["violated_arcs"] > 0 and want["untight"] > 0 and want["wrong_unreached"] > 0
    c, st = g.sssp_verify(source, wrong, stats=True)
    assert c == want
    launches_are(kind, "sssp_verify_wrong", st)
