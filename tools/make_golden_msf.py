#!/usr/bin/env python3
"""Writes tests/golden/msf.json and tests/golden/msf.npz: the goldens of gmsx_min_spanning_forest.

The reference has no spanning forest, so the goldens come from the restatement of tests/test_msf_golden_cpu.py — kruskal_np(off, adj, w,
maximum) under the order of include/gmsx.h — over the six graphs of tests/golden/sssp.json (the same files and generator settings, read through
golden_csr) plus kronecker_14_16.  Asserted before anything is written, per (graph, minimum / maximum):
  (a) boruvka_np (full rounds under the same order) gives the same edges; its round count is the recorded `rounds`;
  (b) scipy.sparse.csgraph.minimum_spanning_tree agrees on the total weight and the edge count (the maximum on weights wmax + 1 - w), and
      connected_components over the forest's edges gives `trees`.
Stored per record: the integers of gmsx_msf_info, a sha256 and an FNV-1a of the (u, v, w) int32 arrays, and in the .npz the arrays themselves
for the graphs of at most 2^12 vertices."""
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
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
    if not os.path.exists(os.path.join(GOLDEN, "msf.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "msf.json"), "w").write('{"graphs": {}, "records": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "msf.npz"))
    import test_msf_golden_cpu as T  # the restatements
    from test_sssp_golden_cpu import J as SSSP
    graphs, records, arrays = {}, [], {}
    for key in T.graph_keys():
        off, adj, w = T.golden_arrays(capi, key)
        n, wmax = off.size - 1, int(w.max())
        if key in SSSP["graphs"]:
            source = SSSP["graphs"][key]["source"]
            assert (SSSP["graphs"][key]["n"], SSSP["graphs"][key]["nnz"]) == (n, adj.size), key
        else:
            kind, scale, deg = T.EXTRA[key]
            source = {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": False}
        graphs[key] = {"source": source, "n": int(n), "nnz": int(adj.size), "wmax": wmax}
        for maximum in (False, True):
            u, v, ww = T.kruskal_np(off, adj, w, maximum)
            (bu, bv, bw), rounds = T.boruvka_np(off, adj, w, maximum)
            assert np.array_equal(u, bu) and np.array_equal(v, bv) and np.array_equal(ww, bw), (key, maximum)  # (a)
            info = T.info_np(off, u, v, ww, rounds)
            vals = (wmax + 1 - w.astype(np.int64)) if maximum else w.astype(np.int64)
            t = minimum_spanning_tree(sp.csr_matrix((vals.astype(np.float64), adj, off), shape=(n, n)))
            total = int(round(t.sum()))
            assert t.nnz == info["edges"] and (info["edges"] * (wmax + 1) - total if maximum else total) == info["total_weight"], (key, maximum)  # (b)
            trees, _ = connected_components(sp.csr_matrix((np.ones(u.size), (u, v)), shape=(n, n)), directed=False)
            assert trees == info["trees"] == n - info["edges"], (key, maximum)
            rec = dict(info, graph=key, maximum=maximum, sha256=T.sha_of(u, v, ww), fnv=str(T.fnv_of(u, v, ww)))
            if n <= T.ARRAY_MAX_N:
                for name, a in zip("uvw", (u, v, ww)):
                    arrays["%s_%s" % (name, T.rec_id(rec))] = a
            records.append(rec)
            print(T.rec_id(rec), {k: rec[k] for k in T.INFO_KEYS}, flush=True)
    with open(os.path.join(GOLDEN, "msf.json"), "w") as fh:
        fh.write('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) + '\n },\n "records": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "msf.npz"), **arrays)
    print("wrote", len(graphs), "graphs,", len(records), "records,", os.path.getsize(os.path.join(GOLDEN, "msf.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
