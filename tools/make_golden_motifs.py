#!/usr/bin/env python3
"""Writes tests/golden/motifs.json and tests/golden/motifs.npz: the goldens of gmsx_cycle4_count / gmsx_motif_census4.

Nothing here runs on the device or shares code with it.  The records come from the numpy / scipy restatement kept in
tests/test_motifs_golden_cpu.py (census_np): 4-cycles from the sparse product A·A, ½ Σ_{u<w} C((A²)_uw, 2); wedges, 3-stars, 4-paths, tailed
triangles, diamonds and 4-cliques from their definitions; wedges_walked and max_codegree from the counting rule written in rank ids.  For every
graph of at most 40 vertices the literal enumerator over all 3- and 4-subsets (enumerate_literally) must agree before anything is written, and
the closed forms (K_n, K_{a,b}, Q_4, the 8×8 grid, Petersen, C_n) are asserted.  Graphs: the closed-form constructions of the test module and
the project's host generator.

Per graph the JSON holds n, nnz, the sixteen counts, wedges_walked, max_codegree and the sha256 of the <i8 at_vertex array; the arrays are in
the .npz."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gms_amd import capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    import test_motifs_golden_cpu as T  # the restatement and the graphs
    recs, arrays = {}, {}
    for key in list(T.CLOSED) + list(T.GENERATED):
        if key in T.CLOSED:
            n, edges = T.CLOSED[key]
            off, adj = T.arrays_of(n, edges)
            csr = T.golden_csr(capi, key)   # the loader builds the same CSR from the edge list
            assert np.array_equal(off, csr.offsets()) and np.array_equal(adj, csr.neighbors()), key
        else:
            csr = T.golden_csr(capi, key)
            off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32)
            n, edges = off.size - 1, None
        got = T.census_np(off, adj)
        rec = {"n": int(n), "nnz": int(adj.size), "subgraphs": got["subgraphs"], "induced": got["induced"], "wedges_walked": got["wedges_walked"],
               "max_codegree": got["max_codegree"], "at_vertex_sha256": T.sha(got["at_vertex"]), "enumerated": False}
        assert all(0 <= v < 1 << 64 for v in rec["subgraphs"].values()) and all(v >= 0 for v in rec["induced"].values()), key
        assert int(got["at_vertex"].astype(object).sum()) == 4 * rec["subgraphs"]["cycle4"], key
        if edges is not None and n <= 40:
            sub, ind = T.enumerate_literally(n, edges)
            assert sub == rec["subgraphs"] and ind == rec["induced"], key
            rec["enumerated"] = True
        if key in T.CLOSED_C4:
            assert rec["subgraphs"]["cycle4"] == T.CLOSED_C4[key], key
        recs[key] = rec
        arrays["at_" + key] = got["at_vertex"].astype("<i8")
        print(f"{key}: n {n}, nnz {adj.size}, cycle4 {rec['subgraphs']['cycle4']}, clique4 {rec['subgraphs']['clique4']}, wedges walked "
              f"{rec['wedges_walked']}, max codegree {rec['max_codegree']}", flush=True)
    with open(os.path.join(GOLDEN, "motifs.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(recs[k], sort_keys=True)}" for k in sorted(recs)) + "\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "motifs.npz"), **arrays)
    print("wrote", len(recs), "records and", len(arrays), "arrays")


if __name__ == "__main__":
    main()
