"""gmsx_cycle4_count, gmsx_cycle4_partial and gmsx_motif_census4 on the device.
  closed forms   K_n, K_{a,b}, C_n, Q_4, the 8×8 grid, Petersen, a star, a wheel and a friendship graph — the smallest shapes that cross a lane,
                 wave or bin edge — each also with 7 isolated vertices appended and as two disjoint copies
  goldens        kronecker 8 / 10 / 12 and uniform 10 (tests/golden/motifs.json): the sixteen counts, at_vertex, wedges_walked, max_codegree;
                 kronecker 10 once more under GMSX_UPLOAD_HUB_LIMIT(64)
  options        C4_LDS_SPAN, C4_SLAB_MB, C4_SPLIT_WEDGES and their combination give the default run's bytes; two calls on one handle agree
  cross-checks   against gmsx_subgraph_match (induced and mono), gmsx_tc_total, gmsx_kclique_count and gmsx_edge_support
  shards         the partials of 2, 3 and 8 parts add up; (0, 1) is the whole; (3, 3) is refused
  overflow       the star K_{1,4 000 000} returns C(4·10⁶, 3) exactly, K_{1,4 900 000} returns GMSX_ERR_OVERFLOW and writes nothing
  edge cases     n = 0, no edge, NULL arguments, at_vertex NULL and non-NULL"""
import ctypes as C
from math import comb

import numpy as np
import pytest

from conftest import edges_to_csr
from test_motifs_golden_cpu import ARR, AUT, CLOSED, GENERATED, MOTIFS, PATTERNS, RECS, golden_csr, variant

pytestmark = pytest.mark.gpu

SETTINGS = [{"C4_LDS_SPAN": 0}, {"C4_LDS_SPAN": 64}, {"C4_SLAB_MB": 1}, {"C4_SPLIT_WEDGES": 1}, {"C4_SPLIT_WEDGES": 1 << 62},
            {"C4_LDS_SPAN": 0, "C4_SLAB_MB": 1, "C4_SPLIT_WEDGES": 1}]


def everything(g):
    """every output of the three calls on one handle, the times left out"""
    census = g.motif_census4()
    cycles, at = g.cycle4_count(at_vertex=True)
    plain, st = g.cycle4_count(stats=True)
    assert cycles == plain == census["subgraphs"]["cycle4"] and int(at.sum()) == 4 * cycles
    assert st["alg_elements"] == census["wedges_walked"]
    return census, at.tobytes()


def check_record(g, rec, at_want, factor=1):
    census, at = everything(g)
    assert census["subgraphs"] == {k: factor * v for k, v in rec["subgraphs"].items()}
    assert census["induced"] == {k: factor * v for k, v in rec["induced"].items()}
    assert (census["wedges_walked"], census["max_codegree"]) == (factor * rec["wedges_walked"], rec["max_codegree"])
    assert at == np.ascontiguousarray(at_want, dtype="<i8").tobytes()


# ---- 1. closed forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["plain", "isolated", "twice"])
@pytest.mark.parametrize("key", sorted(CLOSED))
def test_closed_forms(gpu, key, how):
    n, edges = variant(*CLOSED[key], how)
    base = ARR["at_" + key]
    at = {"plain": base, "isolated": np.r_[base, np.zeros(7, dtype=base.dtype)], "twice": np.r_[base, base]}[how]
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, edges, n=n))
    check_record(g, RECS[key], at, 2 if how == "twice" else 1)
    g.free()


# ---- 2. goldens ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(GENERATED))
def test_generated_graphs_equal_the_goldens(gpu, key):
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    check_record(g, RECS[key], ARR["at_" + key])
    g.free()


def test_hub_limit_changes_nothing(gpu):
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, "kronecker_10_16"), flags=64 << 8)
    check_record(g, RECS["kronecker_10_16"], ARR["at_kronecker_10_16"])
    g.free()


# ---- 3. options ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["kronecker_10_16", "K_65_130"])
def test_option_settings_give_the_same_bytes(gpu, key):
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, key))
    want = everything(g)
    assert want[0]["subgraphs"] == RECS[key]["subgraphs"]
    for setting in SETTINGS:
        with gpu.options(**setting):
            assert everything(g) == want, setting
            assert everything(g) == want, setting   # a clean-up walk that left a counter behind shows in the second call
    assert everything(g) == want
    g.free()


# ---- 4. the device's own independent code ---------------------------------------------------------------------------------------------------
def test_cross_checks_on_kronecker_8(gpu):
    csr = golden_csr(gpu, "kronecker_8_8")
    g = gpu.DeviceGraph.from_csr(csr)
    census = g.motif_census4()
    for name, aut in AUT.items():
        induced = g.subgraph_match_info(PATTERNS[name], induced=True)["embeddings"]
        mono = g.subgraph_match_info(PATTERNS[name], induced=False)["embeddings"]
        assert induced % aut == 0 and mono % aut == 0
        assert census["induced"][name] == induced // aut, name
        assert census["subgraphs"][name] == mono // aut, name
    assert census["subgraphs"]["triangle"] == census["induced"]["triangle"] == g.tc_total()
    assert census["subgraphs"]["clique4"] == g.kclique_count(4)[1]
    support = g.edge_support()[0].astype(np.int64)
    assert census["subgraphs"]["diamond"] == int((support * (support - 1) // 2).sum()) // 2   # (every edge on both of its arcs)
    g.free()


# ---- 5. shards ----------------------------------------------------------------------------------------------------------------------------
def test_shards_add_up(gpu):
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, "kronecker_10_16"))
    whole = g.cycle4_count()
    assert whole == RECS["kronecker_10_16"]["subgraphs"]["cycle4"] == g.cycle4_partial(0, 1)
    for nparts in (2, 3, 8):
        parts = [g.cycle4_partial(p, nparts) for p in range(nparts)]
        assert sum(parts) == whole and all(0 < p < whole for p in parts)
    for part, nparts in ((3, 3), (-1, 2), (0, 0)):
        with pytest.raises(gpu.GmsxError) as e:
            g.cycle4_partial(part, nparts)
        assert e.value.status == gpu.ERR_INVALID
    g.free()


# ---- 6. overflow --------------------------------------------------------------------------------------------------------------------------
def star_graph(gpu, leaves):
    return gpu.DeviceGraph.from_csr(gpu.HostCSR.from_edges(np.zeros(leaves, dtype=np.int32), np.arange(1, leaves + 1, dtype=np.int32), num_nodes=leaves + 1))


def test_star3_at_the_edge_of_64_bits(gpu):
    """C(4 000 000, 3) fits 64 bits, C(4 900 000, 3) does not; neither star has a triangle or a 4-cycle"""
    g = star_graph(gpu, 4_000_000)
    census = g.motif_census4()
    zero = {"triangle", "path4", "paw", "cycle4", "diamond", "clique4"}
    assert census["subgraphs"] == dict({k: 0 for k in zero}, wedge=comb(4_000_000, 2), star3=comb(4_000_000, 3))
    assert census["induced"] == census["subgraphs"] and census["wedges_walked"] == 0 and census["max_codegree"] == 0
    assert comb(4_000_000, 3) < 1 << 64 <= comb(4_900_000, 3)
    g.free()
    g = star_graph(gpu, 4_900_000)
    info = gpu.MotifInfo()
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    before = bytes(info)
    assert gpu.lib().gmsx_motif_census4(g._h, C.byref(info), None) == gpu.ERR_OVERFLOW
    assert bytes(info) == before
    assert g.cycle4_count() == 0   # (the 4-cycle count itself has nothing to overflow)
    g.free()


# ---- 7. edge cases ------------------------------------------------------------------------------------------------------------------------
def test_degenerate_graphs_and_null_arguments(gpu):
    zero = {"subgraphs": dict.fromkeys(MOTIFS, 0), "induced": dict.fromkeys(MOTIFS, 0), "wedges_walked": 0, "max_codegree": 0}
    g = gpu.DeviceGraph.from_csr(gpu.HostCSR.from_arrays(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    assert g.motif_census4() == zero and g.cycle4_count() == 0 and g.cycle4_partial(1, 2) == 0
    cycles, at = g.cycle4_count(at_vertex=True)
    assert cycles == 0 and at.size == 0
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [], n=5))
    cycles, at = g.cycle4_count(at_vertex=True)
    assert g.motif_census4() == zero and cycles == 0 and at.tolist() == [0] * 5
    g = gpu.DeviceGraph.from_csr(edges_to_csr(gpu, [(0, 1)], n=2))
    assert g.motif_census4() == zero and g.cycle4_count() == 0
    L, out, info = gpu.lib(), C.c_uint64(77), gpu.MotifInfo()
    assert L.gmsx_cycle4_count(None, C.byref(out), None, None) == gpu.ERR_INVALID
    assert L.gmsx_cycle4_count(g._h, None, None, None) == gpu.ERR_INVALID
    assert L.gmsx_cycle4_partial(None, 0, 1, C.byref(out), None) == gpu.ERR_INVALID
    assert L.gmsx_cycle4_partial(g._h, 0, 1, None, None) == gpu.ERR_INVALID
    assert L.gmsx_motif_census4(None, C.byref(info), None) == gpu.ERR_INVALID
    assert L.gmsx_motif_census4(g._h, None, None) == gpu.ERR_INVALID
    assert out.value == 77


def test_at_vertex_does_not_change_the_count(gpu):
    g = gpu.DeviceGraph.from_csr(golden_csr(gpu, "kronecker_8_8"))
    with_at, at = g.cycle4_count(at_vertex=True)
    assert g.cycle4_count() == with_at == RECS["kronecker_8_8"]["subgraphs"]["cycle4"]
    assert np.array_equal(at, ARR["at_kronecker_8_8"])
    g.free()
