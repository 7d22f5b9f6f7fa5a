"""GPU probe: gmsx_cycle4_count and gmsx_motif_census4 on one handle, in one process (run it under `timeout`).  Per graph one JSON line; every
time is the MEDIAN of --reps warm calls (default 5) by the calls' own HIP events (kernel_ms, and kernel_ms + setup_ms as "ms"), wall time beside:

  paths      which of the three counter paths the sources take at the default options, restated on the host from the CSR (rank ids, later
             neighbours, wedge bound): sources and wedge bound per path, as counts and shares
  cycle4     gmsx_cycle4_count at the default and at each option setting of SETTINGS — a setting that forces every source onto one path times
             that path alone —, wedges per second by kernel_ms, and the same call with at_vertex
  census     gmsx_motif_census4 at the default
  baseline   (--sgm, small graphs only) the INDUCED and MONO 4-cycle sizing calls of gmsx_subgraph_match, divided by |Aut(C4)| = 8: the only
             route to this number before gmsx_cycle4_count

usage: motif_probe.py [--reps N] [--sgm] GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--reps")]
LDS_SPAN, SPLIT_WEDGES = 8192, 1 << 18  # the defaults of motifs.hip (gmsx.h, OPTIONS)
SETTINGS = {"default": {}, "all_split": {"C4_SPLIT_WEDGES": 1}, "no_split": {"C4_SPLIT_WEDGES": 1 << 62}, "no_lds": {"C4_LDS_SPAN": 0},
            "all_slab": {"C4_LDS_SPAN": 0, "C4_SPLIT_WEDGES": 1 << 62}, "slab_64mb": {"C4_SLAB_MB": 64}, "slab_8192mb": {"C4_SLAB_MB": 8192}}
C4 = [(0, 1), (1, 2), (2, 3), (3, 0)]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]))
    return capi.HostCSR.load(name)


def median_call(fn):
    """(result of the last call, stats of the last call, median kernel ms, median kernel + setup ms, median wall ms)"""
    ker, dev, wall, r = [], [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        ker.append(r[-1]["kernel_ms"])
        dev.append(r[-1]["kernel_ms"] + r[-1]["setup_ms"])
    return r, r[-1], float(np.median(ker)), float(np.median(dev)), float(np.median(wall))


def path_shares(off, adj):
    """sources and wedge bound per path at the default options"""
    n = off.size - 1
    deg = np.diff(off)
    order = np.lexsort((-np.arange(n), -deg))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    src = np.repeat(np.arange(n), deg)
    later = rank[adj] > rank[src]
    l = np.bincount(src[later], minlength=n)
    b = np.bincount(src[later], weights=deg[adj[later]].astype(np.float64), minlength=n).astype(np.int64)
    walked = l >= 2
    split = walked & (b > SPLIT_WEDGES)
    lds = walked & ~split & (n - rank - 1 <= LDS_SPAN)
    slab = walked & ~split & ~lds
    tot_s, tot_b = max(int(walked.sum()), 1), max(int(b[walked].sum()), 1)
    return {k: {"sources": int(m.sum()), "source_share": round(int(m.sum()) / tot_s, 4), "wedge_bound": int(b[m].sum()),
                "wedge_share": round(int(b[m].sum()) / tot_b, 4)} for k, m in (("lds", lds), ("slab", slab), ("split", split))}


capi.init(0)
for name in names:
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    out = {"graph": name, "n": n, "nnz": nnz, "reps": reps, "paths": path_shares(np.asarray(csr.offsets()), np.asarray(csr.neighbors())), "cycle4": {}}
    g.cycle4_count()  # warm-up: the first launches of the kernels
    want = None
    for key, setting in SETTINGS.items():
        with capi.options(**setting):
            g.cycle4_count()
            (cycles, st), st, ker, dev, wall = median_call(lambda: g.cycle4_count(stats=True))
        want = cycles if want is None else want
        assert cycles == want
        out["cycle4"][key] = {"kernel_ms": round(ker, 4), "ms": round(dev, 4), "wall_ms": round(wall, 3), "launches": st["launches"], "sources": st["units"],
                              "wedges_per_s": round(st["alg_elements"] / (ker * 1e-3), 0) if ker > 0 else None}
    out.update(cycles=want, wedges_walked=st["alg_elements"])
    (_, _, st), st, ker, dev, wall = median_call(lambda: g.cycle4_count(at_vertex=True, stats=True))
    out["cycle4_at_vertex"] = {"kernel_ms": round(ker, 4), "ms": round(dev, 4), "wall_ms": round(wall, 3), "launches": st["launches"]}
    g.motif_census4()
    (census, st), st, ker, dev, wall = median_call(lambda: g.motif_census4(stats=True))
    assert census["subgraphs"]["cycle4"] == want
    out["census"] = {"kernel_ms": round(ker, 4), "ms": round(dev, 4), "wall_ms": round(wall, 3), "launches": st["launches"], "subgraphs": census["subgraphs"],
                     "max_codegree": census["max_codegree"]}
    if "--sgm" in argv:
        for mode, induced, expect in (("induced", True, census["induced"]["cycle4"]), ("mono", False, want)):
            g.subgraph_match_info(C4, induced=induced)
            (info, st), st, ker, dev, wall = median_call(lambda: g.subgraph_match_info(C4, induced=induced, stats=True))
            assert info["embeddings"] == 8 * expect
            out["subgraph_match_" + mode] = {"kernel_ms": round(ker, 4), "ms": round(dev, 4), "wall_ms": round(wall, 3), "embeddings": info["embeddings"]}
        out["ratio_mono_over_cycle4"] = round(out["subgraph_match_mono"]["ms"] / out["cycle4"]["default"]["ms"], 1)
    print(json.dumps(out), flush=True)
    g.free()
    del csr
