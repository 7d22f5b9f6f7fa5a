#!/usr/bin/env python3
"""Writes tests/golden/communities.json and tests/golden/communities.npz: the goldens of gmsx_label_propagation and gmsx_modularity.

The reference has no community detection, so the goldens come from the restatements of tests/test_communities_golden_cpu.py and need no
reference binary: lp_np (the sweeps of include/gmsx.h colour class by colour class) over
  unweighted  the six tests/golden/testGraphs/*.el files, kronecker 10 (relabelled and not), 12 and 14 at degree 16;
  weighted    the two tests/golden/sssp/two_parts_*.wel files and the weighted generator at kronecker 10 (relabelled and not), 12 and 14,
each under the default colouring (Jones–Plassmann under the id order, the restatement of tests/test_coloring_golden_cpu.py) and under the
largest-first colouring.  Asserted before anything is written, per record:
  (a) the default colouring equals the golden of coloring.npz where that has the graph;
  (b) for n <= 1024 the sequential loop lp_seq gives the same labels and info, and every change raises the monochromatic weight;
  (c) the propagation converged and the final labelling has unstable == 0.
Stored per record: the integers of gmsx_lp_info, a sha256 and an FNV-1a of the int32 labels, the modularity integers (S as a decimal string, Q
as a hex float) of the final labelling and of label = connected components, and in the .npz the labels of the graphs of at most 2^12 vertices."""
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
    if not os.path.exists(os.path.join(GOLDEN, "communities.json")):  # the test module loads the goldens when it is imported
        open(os.path.join(GOLDEN, "communities.json"), "w").write('{"records": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "communities.npz"))
    import test_communities_golden_cpu as T  # the restatements
    records, arrays = [], {}
    for kind, key in T.graph_ids():
        off, adj, w = T.graph_arrays(capi, kind, key)
        n = off.size - 1
        cc = T.mod_record(T.mod_np(off, adj, w, T.cc_labels_np(off, adj)))
        for which in T.COLORINGS:
            color = T.coloring_of(off, adj, which)
            if which == "default" and kind == "u" and key in T.COL:
                assert np.array_equal(color, T.COL_ARR["color_id_" + key]), key  # (a)
            label, info, rise = T.lp_np(off, adj, w, color)
            if n <= 1 << 10:
                slabel, sinfo, rises = T.lp_seq(off, adj, w, color)
                assert np.array_equal(slabel, label) and sinfo == info and all(r > 0 for r in rises) and sum(rises) == rise, (key, which)  # (b)
            m = T.mod_np(off, adj, w, label)
            assert info["converged"] == 1 and m["unstable"] == 0 and m["intra_weight"] == rise, (key, which)  # (c)
            rec = dict(info, graph=key, weighted=kind == "w", coloring=which, n=int(n), nnz=int(adj.size), sha256=T.sha_of(label),
                       fnv=str(T.fnv_of(label)), mod=T.mod_record(m), mod_cc=cc)
            if n <= T.ARRAY_MAX_N:
                arrays["label_" + T.rec_id(rec)] = label
            records.append(rec)
            print(T.rec_id(rec), {k: rec[k] for k in T.INFO_KEYS}, float.fromhex(rec["mod"]["modularity"]), flush=True)
    with open(os.path.join(GOLDEN, "communities.json"), "w") as fh:
        fh.write('{\n "records": [\n' + ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "communities.npz"), **arrays)
    print("wrote", len(records), "records,", os.path.getsize(os.path.join(GOLDEN, "communities.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
