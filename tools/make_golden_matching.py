#!/usr/bin/env python3
"""Writes tests/golden/matching.json and tests/golden/matching.npz: the goldens of gmsx_greedy_matching.

The reference has no matching, so the goldens come from the restatements of tests/test_matching_golden_cpu.py — greedy_np(off, adj, w) under the
order of include/gmsx.h — over every file of tests/golden/testGraphs (unit weights), the two files of tests/golden/sssp and kronecker 10 / 14
(unweighted and with the loader's weights).  Asserted before anything is written, per (graph, unweighted / weighted):
  (a) rounds_np (the locally dominant rounds under the same order) gives the same mate; its round count is the recorded `rounds`;
  (b) check_np certifies it: invalid = augmentable = undominated = 0.
Stored per record: the integers of gmsx_matching_info, a sha256 and an FNV-1a of the mate int32 array, and in the .npz the array itself for the
graphs of at most 2^12 vertices.  build(capi) returns what main() writes; the CPU test compares it with the files."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden")


def build(capi):
    import test_matching_golden_cpu as T  # the restatements
    graphs, records, arrays = {}, [], {}
    for key, weighted in T.record_keys():
        off, adj, w = T.golden_arrays(capi, key)
        w = w if weighted else None
        n = off.size - 1
        graphs[key] = {"source": T.GRAPHS[key], "n": int(n), "nnz": int(adj.size)}
        mate, rounds = T.matching(capi, key, weighted)  # (a): greedy_np and rounds_np agree
        c = T.check_np(off, adj, w, mate)
        assert (c["invalid"], c["augmentable"], c["undominated"]) == (0, 0, 0), (key, weighted)  # (b)
        rec = dict(T.info_np(off, adj, w, mate, rounds), graph=key, weighted=weighted, sha256=T.sha_of(mate), fnv=str(T.fnv_of(mate)))
        assert (c["pairs"], c["total_weight"], c["free_vertices"]) == (rec["pairs"], rec["total_weight"], rec["free_vertices"])
        if n <= T.ARRAY_MAX_N:
            arrays["mate_" + T.rec_id(rec)] = mate
        records.append(rec)
    return graphs, records, arrays


def json_text(graphs, records):
    return ('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) +
            '\n },\n "records": [\n' + ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]\n}\n")


def main():
    from gms_amd import capi
    if not os.path.exists(os.path.join(GOLDEN, "matching.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "matching.json"), "w").write('{"graphs": {}, "records": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "matching.npz"))
    graphs, records, arrays = build(capi)
    for rec in records:
        print(rec["graph"], rec["weighted"], {k: v for k, v in rec.items() if k not in ("graph", "weighted", "sha256", "fnv")}, flush=True)
    with open(os.path.join(GOLDEN, "matching.json"), "w") as fh:
        fh.write(json_text(graphs, records))
    np.savez_compressed(os.path.join(GOLDEN, "matching.npz"), **arrays)
    print("wrote", len(graphs), "graphs,", len(records), "records,", os.path.getsize(os.path.join(GOLDEN, "matching.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
