"""GPU probe: k-clique-star LISTING next to gmsx_kclique_star_count of the same k, in one process.  Per shard: the sizing call, the fill call
(re-using the sizing pass) and the share of the fill that is not kernel time (the device-to-host copy), wall and HIP-event times.
usage: kcstar_list_probe.py [generator scale degree] [--k K] [--nparts N] [--cliques-only]   (default kronecker 14 16, k = 3, 1 shard)"""
import ctypes as C
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi
argv = sys.argv[1:]
opt = lambda name, dflt: int(argv[argv.index(name) + 1]) if name in argv else dflt  # noqa: E731
k, nparts, only = opt("--k", 3), opt("--nparts", 1), "--cliques-only" in argv
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--k", "--nparts"))]
gen, scale, deg = (pos[0], int(pos[1]), int(pos[2])) if len(pos) > 2 else ("kronecker", 14, 16)
capi.init(0)
csr = capi.HostCSR.generate(gen, scale, deg)
g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
counts = []
for _ in range(3):
    stars, members, st = g.kclique_star_count(k, members=not only, stats=True)
    counts.append(round(st["kernel_ms"], 2))
print(json.dumps({"graph": [gen, scale, deg], "k": k, "cliques_only": only, "kclique_star_count": [stars, members], "count_kernel_ms": counts}), flush=True)
L = capi.lib()
flags = capi.KCSTAR_CLIQUES_ONLY if only else capi.KCSTAR_DEFAULT
tot = {"cliques": 0, "star_members": 0, "sizing_ms": 0.0, "sizing_kernel_ms": 0.0, "fill_ms": 0.0, "fill_kernel_ms": 0.0, "bytes": 0}
vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
for part in range(nparts):
    info, st = capi.KcliqueStarListInfo(), capi.Stats()
    t0 = time.perf_counter()
    assert L.gmsx_kclique_star_list(g._h, k, flags, part, nparts, None, None, None, 0, 0, C.byref(info), C.byref(st)) == 0
    t1 = time.perf_counter()
    sizing_kernel, setup, tasks = st.kernel_ms, st.setup_ms, st.units
    cl = np.empty(max(info.cliques * k, 1), dtype=np.int32)
    off = None if only else np.empty(info.cliques + 1, dtype=np.int64)
    mem = None if only else np.empty(max(info.star_members, 1), dtype=np.int32)
    for x in (cl, off, mem):  # first touch outside the timed call
        if x is not None:
            x[:] = 0
    t2 = time.perf_counter()
    assert L.gmsx_kclique_star_list(g._h, k, flags, part, nparts, vp(cl), vp(off), vp(mem), info.cliques, info.star_members, C.byref(info),
                                    C.byref(st)) == 0
    t3 = time.perf_counter()
    nbytes = 4 * info.cliques * k + (0 if only else 8 * (info.cliques + 1) + 4 * info.star_members)
    rec = {"part": part, "cliques": info.cliques, "star_members": info.star_members, "max_star": info.max_star, "tasks": tasks,
           "sizing_ms": round(1e3 * (t1 - t0), 2), "sizing_kernel_ms": round(sizing_kernel, 2), "task_list_ms": round(setup, 2),
           "fill_ms": round(1e3 * (t3 - t2), 2), "fill_kernel_ms": round(st.kernel_ms, 2),
           "copy_and_host_ms": round(1e3 * (t3 - t2) - st.kernel_ms, 2), "launches": st.launches, "output_mb": round(nbytes / 1e6, 1)}
    print(json.dumps(rec), flush=True)
    tot["cliques"] += info.cliques
    tot["star_members"] += info.star_members
    tot["sizing_ms"] += 1e3 * (t1 - t0)
    tot["sizing_kernel_ms"] += sizing_kernel
    tot["fill_ms"] += 1e3 * (t3 - t2)
    tot["fill_kernel_ms"] += st.kernel_ms
    tot["bytes"] += nbytes
    del cl, off, mem
tot = {key: (round(v, 2) if isinstance(v, float) else v) for key, v in tot.items()}
tot["count_ok"] = tot["cliques"] == stars and (only or tot["star_members"] == members)
print(json.dumps({"total": tot}), flush=True)
