"""GPU probe: gmsx_connected_components and gmsx_jarvis_patrick on one handle, in one process (run it under `timeout`).  Per graph one JSON
line, every time the MEDIAN of --reps warm calls (default 5) by the calls' own HIP events (kernel_ms + setup_ms) with the wall time beside it:

  cc            gmsx_connected_components at CC_SAMPLE = 0 and at each value of --samples (default "2": the library's default), in ms and in
                arcs / s, the arcs examined (stats.units), the flatten rounds, and the fraction of the ceiling reached: one read of the CSR
                (8 (n + 1) + 4 nnz bytes) at the rate gmsx_hbm_read_probe reports in this process
  jp            gmsx_jarvis_patrick (common neighbours, threshold 2) beside the route a caller had before it: gmsx_vertex_similarity_batch over
                the same u < v edge list plus a host threshold (the pair batch's kernel_ms leaves out its copies: its wall time is the honest
                comparison; the union-find that would still have to follow is not in it), and the clustering call once more with a threshold no
                score reaches (jp_nothing_kept: what the scores alone cost in that kernel).  --no-jp skips all three.

usage: components_probe.py [--reps N] [--samples a,b,..] [--no-jp] GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | path-SCALE (2^SCALE
vertices numbered along the path: the worst case for depth) | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
valued = ("--reps", "--samples")
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
samples = [int(x) for x in argv[argv.index("--samples") + 1].split(",")] if "--samples" in argv else [2]
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in valued)]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]))
    if len(parts) == 2 and parts[0] == "path":
        n = 1 << int(parts[1])
        ids = np.arange(n, dtype=np.int32)
        return capi.HostCSR.from_edges(ids[:-1], ids[1:], num_nodes=n)
    return capi.HostCSR.load(name)


def median_call(fn):
    """(result of the last call, median device ms, median wall ms, stats of the last call)"""
    dev, wall, r = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(r[-1]["kernel_ms"] + r[-1]["setup_ms"])
    return r, float(np.median(dev)), float(np.median(wall)), r[-1]


capi.init(0)
read_gbs = capi.hbm_read_probe()
for name in names:
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    csr_bytes = 8 * (n + 1) + 4 * nnz
    ceiling_ms = csr_bytes / (read_gbs * 1e6)
    out = {"graph": name, "n": n, "nnz": nnz, "read_gbs": round(read_gbs, 1), "csr_read_ms": round(ceiling_ms, 4), "reps": reps, "cc": {}}
    g.connected_components()  # warm-up: the first launches of the kernels
    first = None
    for s in [0] + [x for x in samples if x != 0]:
        with capi.options(CC_SAMPLE=s):
            (label, info, st), dev, wall, st = median_call(lambda: g.connected_components(stats=True))
        first = first if first is not None else label.tobytes()
        assert label.tobytes() == first
        out.update(components=info["components"], largest=info["largest"])
        out["cc"]["sample_%d" % s] = {"ms": round(dev, 4), "kernel_ms": round(st["kernel_ms"], 4), "wall_ms": round(wall, 3), "arcs_per_s": round(nnz / (dev * 1e-3), 0),
                                      "examined": st["units"], "launches": st["launches"], "passes": info["passes"],
                                      "fraction_of_csr_read": round(ceiling_ms / dev, 4)}
    if "--no-jp" not in argv:
        off, adj = csr.offsets(), csr.neighbors()
        src = np.repeat(np.arange(n, dtype=np.int32), np.diff(off))
        up = src < adj
        eu, ev = np.ascontiguousarray(src[up]), np.ascontiguousarray(adj[up], dtype=np.int32)
        del src, up
        g.jarvis_patrick("common_neighbors", 2.0)
        g.vertex_similarity_batch("common_neighbors", eu[:1024], ev[:1024])
        (jl, ji, jst), jdev, jwall, jst = median_call(lambda: g.jarvis_patrick("common_neighbors", 2.0, stats=True))

        (_, ni, nst), ndev, _, nst = median_call(lambda: g.jarvis_patrick("common_neighbors", float(n), stats=True))  # the scores alone: nothing reaches n
        assert ni["kept_edges"] == 0

        def batch():
            score, st = g.vertex_similarity_batch("common_neighbors", eu, ev, stats=True)
            keep = score >= 2.0
            return keep, st

        (keep, bst), bdev, bwall, bst = median_call(batch)
        assert int(keep.sum()) == ji["kept_edges"]
        out["jp"] = {"ms": round(jdev, 3), "kernel_ms": round(jst["kernel_ms"], 3), "wall_ms": round(jwall, 3), "kept_edges": ji["kept_edges"],
                     "components": ji["components"], "edges_per_s": round(eu.size / (jdev * 1e-3), 0)}
        out["jp_nothing_kept"] = {"ms": round(ndev, 3), "kernel_ms": round(nst["kernel_ms"], 3)}
        out["similarity_batch_plus_host_threshold"] = {"kernel_ms": round(bst["kernel_ms"], 3), "wall_ms": round(bwall, 3)}
        del eu, ev
    print(json.dumps(out), flush=True)
    g.free()
    del csr
