"""GPU probe: gmsx_bfs and gmsx_betweenness on one handle, in one process (run it under `timeout`).  Per graph one JSON line, every time the
MEDIAN of --reps warm calls (default 5) by the calls' own HIP events (kernel_ms + setup_ms), with the smallest and the largest of them (the
run-to-run spread) and the wall time beside it:

  bfs           gmsx_bfs from vertex 0 and from the first picked source at BFS_DIRECTION 0, 1 and 2: ms, arcs / s against reached_arcs,
                levels, bottom_up_levels, launches, and the time of ONE read of the CSR (8 (n + 1) + 4 nnz bytes) at the rate
                gmsx_hbm_read_probe reports in this process
  cc            gmsx_connected_components on the same handle: the only other whole-graph sweep of the library
  bc            gmsx_betweenness for the first 1 and 8 picked sources; `forward_ms` is the sum of the gmsx_bfs medians of the same sources at
                the default direction, `sort_sigma_delta_ms` the rest (the call has one pair of events: the split is by subtraction).
                --no-bc skips it.

--directions a,b,.. limits the BFS_DIRECTION values (a path of 2^20 vertices is 2^20 levels: three launches and a read-back per bottom-up level).

usage: traversal_probe.py [--reps N] [--directions a,b,..] [--no-bc] GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | path-SCALE (2^SCALE vertices
numbered along the path: one vertex per level) | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
directions = [int(x) for x in argv[argv.index("--directions") + 1].split(",")] if "--directions" in argv else [0, 1, 2]
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--reps", "--directions"))]


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
    """(result of the last call, [median, min, max] device ms, median wall ms)"""
    dev, wall, r = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(r[-1]["kernel_ms"] + r[-1]["setup_ms"])
    return r, [round(float(np.median(dev)), 4), round(min(dev), 4), round(max(dev), 4)], round(float(np.median(wall)), 3)


capi.init(0)
read_gbs = capi.hbm_read_probe()
for name in names:
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    picks = csr.pick_sources(8).tolist()
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    out = {"graph": name, "n": n, "nnz": nnz, "read_gbs": round(read_gbs, 1), "csr_read_ms": round((8 * (n + 1) + 4 * nnz) / (read_gbs * 1e6), 4),
           "reps": reps, "bfs": {}}
    g.bfs(0, want_depth=False, want_parent=False)  # warm-up: the first launches of the kernels
    forward = {}
    for source in dict.fromkeys([0, picks[0]]):
        first = None
        for direction in directions:
            with capi.options(BFS_DIRECTION=direction):
                (depth, parent, info, st), dev, wall = median_call(lambda: g.bfs(source, stats=True))
            first = first if first is not None else (depth.tobytes(), parent.tobytes())
            assert (depth.tobytes(), parent.tobytes()) == first
            out["bfs"]["source_%d_direction_%d" % (source, direction)] = {
                "ms_median_min_max": dev, "wall_ms": wall, "arcs_per_s": round(info["reached_arcs"] / (dev[0] * 1e-3), 0), "reached": info["reached"],
                "levels": info["levels"], "bottom_up_levels": info["bottom_up_levels"], "launches": st["launches"]}
            if direction == directions[0]:
                forward[source] = dev[0]
    g.connected_components()
    (_, ci, cst), dev, wall = median_call(lambda: g.connected_components(stats=True))
    out["cc"] = {"ms_median_min_max": dev, "wall_ms": wall, "components": ci["components"]}
    if "--no-bc" not in argv:
        out["bc"] = {}
        for k in (1, 8):
            g.betweenness(picks[:k])
            (scores, bi, st), dev, wall = median_call(lambda: g.betweenness(picks[:k], stats=True))
            fwd = sum(forward[s] if s in forward else median_call(lambda: g.bfs(s, want_depth=False, want_parent=False, stats=True))[1][0] for s in picks[:k])
            out["bc"]["sources_%d" % k] = {"ms_median_min_max": dev, "wall_ms": wall, "forward_ms": round(fwd, 4), "sort_sigma_delta_ms": round(dev[0] - fwd, 4),
                                           "levels_sum": st["probes"], "launches": st["launches"], "max_sigma": bi["max_sigma"]}
    print(json.dumps(out), flush=True)
    g.free()
    del csr
