#!/usr/bin/env python3
"""Writes tests/golden/bicc.json and tests/golden/bicc.npz: the goldens of gmsx_biconnected_components.

The reference has no biconnectivity, so the goldens come from the restatement of tests/test_bicc_golden_cpu.py — bicc_np(off, adj), an
iterative Hopcroft–Tarjan whose blocks are renumbered by their smallest `u < v` arc — over the six tests/golden/testGraphs/*.el, kronecker 10,
12, 14 and uniform 12 at degree 16, and kronecker 12 at degree 2 (many bridges and small blocks), none relabelled.  Asserted before anything
is written, per graph:
  (a) networkx (biconnected_component_edges, articulation_points, bridges) gives the same edge partition, the same cut vertices and the same
      bridges, and the ids ascend with each block's smallest edge;
  (b) the three identities of include/gmsx.h: Σ blocks_at = n - components + blocks; the components over arc_keep (components_np) =
      components + bridges; Σ over the blocks of their edges = nnz / 2.
Stored per record: the integers of gmsx_bicc_info and a sha256 of block and of blocks_at (int32), and in the .npz the two arrays themselves
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
    if not os.path.exists(os.path.join(GOLDEN, "bicc.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "bicc.json"), "w").write('{"graphs": {}, "records": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "bicc.npz"))
    import test_bicc_golden_cpu as T  # the restatement
    graphs, records, arrays = {}, [], {}
    for key in T.graph_keys():
        off, adj = T.golden_arrays(capi, key)
        n = off.size - 1
        block, blocks_at, arc_keep, info = T.bicc_np(off, adj)
        T.against_networkx(off, adj, block, blocks_at, arc_keep)  # (a)
        assert T.identities_hold(off, adj, block, blocks_at, arc_keep, info), key  # (b)
        if key in T.GENERATED:
            kind, scale, deg = T.GENERATED[key]
            source = {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": False}
        else:
            source = {"kind": "file", "name": key[len("file_"):] + ".el"}
        graphs[key] = {"source": source, "n": int(n), "nnz": int(adj.size)}
        rec = dict(info, graph=key, sha256_block=T.sha(block), sha256_blocks_at=T.sha(blocks_at))
        if n <= T.ARRAY_MAX_N:
            arrays["block_" + key] = block
            arrays["blocks_at_" + key] = blocks_at
        records.append(rec)
        print(key, {k: rec[k] for k in T.INFO_KEYS}, flush=True)
    with open(os.path.join(GOLDEN, "bicc.json"), "w") as fh:
        fh.write('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) + '\n },\n "records": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "bicc.npz"), **arrays)
    print("wrote", len(graphs), "graphs,", len(records), "records,", os.path.getsize(os.path.join(GOLDEN, "bicc.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
