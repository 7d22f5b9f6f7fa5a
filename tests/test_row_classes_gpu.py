"""GPU: the row classes of gms_amd/csrc/hip/row_classes.hpp at their edges, once for each of their four users.  One graph (bins_graph: vertex i
is the hub of a star of BIN_DEGREES[i] leaves: 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097) goes through
gmsx_connected_components, gmsx_biconnected_components, gmsx_min_spanning_forest and gmsx_greedy_matching under three settings of the
algorithm's own …_WAVE_ROW / …_WG_ROW: the defaults, (4, 8) and (17, 65), so that a row sits just below, on and just above every bound in
use.  The weights are seeded per undirected edge, which puts a row's winning arc at an arbitrary lane.  Every array and info block equals
the restatement of the algorithm's *_golden_cpu.py module exactly, and for each algorithm the three settings give the same bytes."""
import numpy as np
import pytest

from test_bicc_golden_cpu import bicc_np
from test_components_golden_cpu import BIN_DEGREES, INFO_KEYS, bins_graph, components_np
from test_matching_golden_cpu import greedy_np, pairs_np, rounds_np
from test_matching_golden_cpu import info_np as matching_info_np
from test_msf_golden_cpu import boruvka_np, kruskal_np, labels_np, mask_np
from test_msf_golden_cpu import info_np as msf_info_np

pytestmark = pytest.mark.gpu

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
