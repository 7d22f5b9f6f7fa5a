"""GPU probe: gmsx_bfs_multi against the same sources one after the other through gmsx_bfs, on one handle, in one process (run it under
`timeout`, one process per graph).  Per graph one JSON line, every time the MEDIAN of --reps warm calls (default 5) by the calls' own HIP events
(kernel_ms + setup_ms), with the smallest and the largest of them (the run-to-run spread):

  multi         gmsx_bfs_multi without depth for the first --sources picked sources (default 64) at MSBFS_DIRECTION 0, 1 and 2 and MSBFS_WORDS 1
                and 2: ms, passes, push_levels / pull_levels, launches
  single        the SUM of gmsx_bfs over the same sources at its defaults (neither depth nor parent copied out): per repetition one sum
  ratio         single / multi per variant, from the medians; `beyond_spread` says whether the slowest multi call still beat the fastest sum
  twice         gmsx_bfs_multi for twice as many picked sources at the defaults, MSBFS_WORDS 1 (two passes of 8-byte words) against 2 (one pass of
                16-byte words): where W = 2 can pay
  read          the time of ONE read of the CSR (8 (n + 1) + 4 nnz bytes) at the rate gmsx_hbm_read_probe reports in this process
  levels        with --levels: one more call at the defaults under option TIMING, whose per-level lines (direction, active vertices, degree sum)
                go to stderr
  all_sources   with --all-sources: one call with every vertex as a source (exact closeness of every vertex), timed once

usage: msbfs_probe.py [--reps N] [--sources K] [--levels] [--all-sources] GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | a file
the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
count = int(argv[argv.index("--sources") + 1]) if "--sources" in argv else 64
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--reps", "--sources"))]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]))
    return capi.HostCSR.load(name)


def spread(ms):
    return [round(float(np.median(ms)), 4), round(min(ms), 4), round(max(ms), 4)]


capi.init(0)
read_gbs = capi.hbm_read_probe()
for name in names:
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    picks = csr.pick_sources(count).tolist()
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    out = {"graph": name, "n": n, "nnz": nnz, "sources": count, "reps": reps, "read_gbs": round(read_gbs, 1),
           "csr_read_ms": round((8 * (n + 1) + 4 * nnz) / (read_gbs * 1e6), 4), "multi": {}}
    # ---- (b) the sources one after the other
    g.bfs(picks[0], want_depth=False, want_parent=False)  # warm-up: the first launches of the kernels
    sums, reached = [], 0
    for _ in range(reps):
        total, reached = 0.0, 0
        for s in picks:
            _, _, info, st = g.bfs(s, want_depth=False, want_parent=False, stats=True)
            total += st["kernel_ms"] + st["setup_ms"]
            reached += info["reached"]
        sums.append(total)
    single = spread(sums)
    out["single"] = {"ms_median_min_max": single}
    # ---- (a) all of them per sweep
    first = None
    for words in (1, 2):
        for direction in (0, 1, 2):
            with capi.options(MSBFS_WORDS=words, MSBFS_DIRECTION=direction):
                g.bfs_multi(picks)
                ms = []
                for _ in range(reps):
                    per, _, vertex, info, st = g.bfs_multi(picks, stats=True)
                    ms.append(st["kernel_ms"] + st["setup_ms"])
            got = (per.tobytes(),) + tuple(a.tobytes() for a in vertex)
            first = first if first is not None else got
            assert got == first and info["reached_total"] == reached
            dev = spread(ms)
            out["multi"]["words_%d_direction_%d" % (words, direction)] = {
                "ms_median_min_max": dev, "passes": info["passes"], "push_levels": info["push_levels"], "pull_levels": info["pull_levels"],
                "launches": st["launches"], "single_over_multi": round(single[0] / dev[0], 2), "beyond_spread": bool(dev[2] < single[1])}
    # ---- W = 2 where it can pay: twice the sources, one pass of 16-byte words against two passes of 8-byte words
    twice = csr.pick_sources(2 * count).tolist()
    out["twice_the_sources"] = {}
    for words in (1, 2):
        with capi.options(MSBFS_WORDS=words):
            g.bfs_multi(twice, want_vertex=False)
            ms = []
            for _ in range(reps):
                _, _, _, info, st = g.bfs_multi(twice, want_vertex=False, stats=True)
                ms.append(st["kernel_ms"] + st["setup_ms"])
        out["twice_the_sources"]["words_%d" % words] = {"ms_median_min_max": spread(ms), "passes": info["passes"]}
    if "--levels" in argv:
        print("levels of %s at the defaults:" % name, file=sys.stderr, flush=True)
        with capi.options(TIMING=1):
            g.bfs_multi(picks, want_vertex=False)
    if "--all-sources" in argv:
        t0 = time.perf_counter()
        per, _, _, info, st = g.bfs_multi(np.arange(n, dtype=np.int32), want_vertex=False, stats=True)
        out["all_sources"] = {"ms": round(st["kernel_ms"] + st["setup_ms"], 3), "wall_ms": round(1e3 * (time.perf_counter() - t0), 3), "passes": info["passes"],
                              "push_levels": info["push_levels"], "pull_levels": info["pull_levels"], "max_far": info["max_far"],
                              "largest_closeness": float(per["closeness"].max())}
    print(json.dumps(out), flush=True)
    g.free()
    del csr
