"""CPU checks of tests/golden/kcstar_lists.json (the (clique, star) lists of the compiled reference, tools/make_golden_kcstar_lists.py): the
file parses and is self-consistent, and each record's numbers agree with the oracle's kclique_star_count on the regenerated graph — and,
where the compiled reference is available, with KCliqueStar::Par::CliqueStarList itself."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, edges_to_csr, host_graph, load_golden

LISTS = load_golden("kcstar_lists.json")
MAX_PAIRS = 200000  # keeps the oracle's recount in seconds


def golden_csr(capi, rec):
    src = rec["source"]
    if src["kind"] == "file":
        return capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", src["name"]))
    if src["kind"] == "edges":
        return edges_to_csr(capi, src["edges"], n=src.get("n", -1))
    return host_graph(capi, src["generator"], src["scale"], src["degree"], src["relabel"])


def test_golden_file_is_well_formed():
    assert len(LISTS) >= 100
    for key, rec in LISTS.items():
        assert key == f"{rec['graph']}|k={rec['k']}"
        assert 1 <= rec["k"] <= 5
        assert rec["cliques"] >= 0 and rec["star_members"] >= 0 and 0 <= rec["max_star"] <= rec["star_members"]
        assert len(rec["sha256"]) == 64
        assert ("list" in rec) == (rec["cliques"] <= 50)
        if "list" in rec:
            assert len(rec["list"]) == rec["cliques"]
            assert sum(len(s) for _, s in rec["list"]) == rec["star_members"]
            assert max([len(s) for _, s in rec["list"]], default=0) == rec["max_star"]
            for c, s in rec["list"]:
                assert len(c) == rec["k"] and c == sorted(set(c)) and s == sorted(set(s)) and not set(c) & set(s)
            assert rec["list"] == sorted(rec["list"], key=lambda p: p[0])
    # the sizes the device tests are planned with
    assert (LISTS["kronecker-8-16-relabel|k=4"]["cliques"], LISTS["kronecker-8-16-relabel|k=4"]["star_members"]) == (34440, 406205)
    assert (LISTS["kronecker-10-16-relabel|k=3"]["cliques"], LISTS["kronecker-10-16-relabel|k=3"]["star_members"]) == (74720, 1638660)
    assert LISTS["kronecker-12-16-relabel|k=3"]["cliques"] == 483489


def _graph_keys():
    return sorted({rec["graph"] for rec in LISTS.values()})


@pytest.mark.parametrize("graph", _graph_keys())
def test_golden_numbers_agree_with_the_oracle(oracle, capi, graph):
    recs = [rec for rec in LISTS.values() if rec["graph"] == graph and rec["cliques"] <= MAX_PAIRS]
    if not recs:
        return
    csr = golden_csr(capi, recs[0])
    off, ng = csr.offsets(), csr.neighbors()
    for rec in recs:
        assert oracle.kclique_star_count(off, ng, rec["k"]) == (rec["cliques"], rec["star_members"]), (graph, rec["k"])
        if "list" in rec:  # the literal pairs: cliques of the graph with exactly their common neighbours
            for c, s in rec["list"]:
                common = None
                for u in c:
                    row = ng[off[u]:off[u + 1]]
                    common = row if common is None else np.intersect1d(common, row, assume_unique=True)
                    assert all(v in row for v in c if v != u)
                assert common.tolist() == s


@pytest.mark.parametrize("graph", ["eppsteinExample.el", "kronecker-8-16-relabel", "uniform-10-16-relabel"])
def test_golden_numbers_agree_with_the_compiled_reference(reference, capi, graph):
    recs = [rec for rec in LISTS.values() if rec["graph"] == graph and rec["cliques"] <= MAX_PAIRS]
    assert recs
    src = recs[0]["source"]
    csr = golden_csr(capi, recs[0])
    if src["kind"] == "file":
        g = reference.load_file(os.path.join(GOLDEN, "testGraphs", src["name"]))
    else:
        g = reference.generate(src["generator"], src["scale"], src["degree"], relabel=src["relabel"])
    try:
        off, ng = reference.csr(g)
        assert np.array_equal(off, csr.offsets()) and np.array_equal(ng, csr.neighbors())
        for rec in recs:
            assert reference.kclique_star(g, rec["k"]) == (rec["cliques"], rec["star_members"]), (graph, rec["k"])
    finally:
        reference.free(g)
