#!/usr/bin/env python3
"""Writes tests/golden/msbfs.json and tests/golden/msbfs.npz: the goldens of gmsx_bfs_multi.

Source of truth: the numpy restatement of tests/test_msbfs_golden_cpu.py (msbfs_np: one plain BFS per source; harmonic as the exact rational
rounded once).  Before anything is written, every (graph, source) that has a BFS record in tests/golden/traversal.json — those records come from
the compiled reference — must agree with the restatement on reached, reached_arcs, depth_sum, levels and the depth sha256.

Graphs and sources:
  the six file_* graphs, kronecker_10_16, kronecker_10_16_raw, uniform_10_16   all n vertices, in id order
  kronecker_12_16                                                             the first 130 picks of gmsx_csr_pick_sources
  kronecker_16_16, uniform_16_16                                              the first 64 picks
Per graph: the per-source integers and closeness / harmonic as hex floats (json); dist_sum, reach and far as arrays (npz) and as sha256 — for
the two 65 536-vertex graphs as sha256 only."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gms_amd import capi  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ALL_SOURCES = ("kronecker_10_16", "kronecker_10_16_raw", "uniform_10_16")
PICKS = {"kronecker_12_16": 130, "kronecker_16_16": 64, "uniform_16_16": 64}
SHA_ONLY = ("kronecker_16_16", "uniform_16_16")


def main():
    if not os.path.exists(os.path.join(GOLDEN, "msbfs.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "msbfs.json"), "w").write('{"graphs": {}}\n')
        np.savez_compressed(os.path.join(GOLDEN, "msbfs.npz"))
    import test_msbfs_golden_cpu as M  # the restatement
    import test_traversal_golden_cpu as T
    keys = sorted(k for k in T.GRAPHS if k.startswith("file_")) + list(ALL_SOURCES) + list(PICKS)
    assert set(keys) == set(T.GRAPHS)
    # ---- the cross-check against the compiled reference's records
    for rec in T.BFS:
        csr = T.golden_csr(capi, rec["graph"])
        r = M.msbfs_np(csr.offsets(), csr.neighbors(), [rec["source"]])
        assert {k: int(r[k][0]) for k in M.INT_KEYS} == {k: rec[k] for k in M.INT_KEYS}, (rec["graph"], rec["source"])
        assert T.sha(r["depth"][0]) == rec["depth_sha256"], (rec["graph"], rec["source"])
    print("agrees with the", len(T.BFS), "BFS records of traversal.json", flush=True)
    graphs, arrays = {}, {}
    for key in keys:
        csr = T.golden_csr(capi, key)
        n = csr.num_nodes
        srcs = csr.pick_sources(PICKS[key]).tolist() if key in PICKS else list(range(n))
        if key in PICKS:
            assert srcs[:16] == T.GRAPHS[key]["picks"]  # (recorded there from the reference's SourcePicker)
        r = M.msbfs_np(csr.offsets(), csr.neighbors(), srcs, want_depth=False)
        per = {k: [int(x) for x in r[k]] for k in M.INT_KEYS}
        per["closeness"] = [float(x).hex() for x in r["closeness"]]
        per["harmonic"] = [float(x).hex() for x in r["harmonic"]]
        literal = key not in SHA_ONLY
        graphs[key] = {"source": T.GRAPHS[key]["source"], "n": int(n), "nnz": int(csr.nnz), "sources": srcs if key in PICKS else "all",
                       "literal": literal, "info": r["info"], "per_source": per,
                       "vertex_sha256": {"dist_sum": M.sha_of(r["dist_sum"], "<i8"), "reach": M.sha_of(r["reach"], "<i4"),
                                         "far": M.sha_of(r["far"], "<i4")}}
        if literal:
            for name in ("dist_sum", "reach", "far"):
                arrays[name + "_" + key] = r[name]
        print(f"{key}: {len(srcs)} sources, reached_total {r['info']['reached_total']}, max_levels {r['info']['max_levels']}", flush=True)
    with open(os.path.join(GOLDEN, "msbfs.json"), "w") as fh:
        fh.write('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) + "\n }\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "msbfs.npz"), **arrays)
    size = sum(os.path.getsize(os.path.join(GOLDEN, "msbfs." + e)) for e in ("json", "npz"))
    assert size <= os.path.getsize(os.path.join(GOLDEN, "traversal.npz")), size
    print("wrote", len(graphs), "graphs,", len(arrays), "arrays,", size, "bytes")


if __name__ == "__main__":
    main()
