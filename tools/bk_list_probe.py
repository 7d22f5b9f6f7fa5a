"""GPU probe: Bron-Kerbosch LISTING on the BASELINE configs[3] graph (or `scale ef`), in one process: gmsx_bk_count, then per shard the sizing
call, the fill call (re-using the sizing pass) and the device-to-host copy, wall and HIP-event times, and the size histogram of the whole list.
usage: bk_list_probe.py [scale ef] [--nparts N]   (default 8 shards: the whole list of configs[3] does not fit a small host)"""
import ctypes as C
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi
argv = sys.argv[1:]
nparts = int(argv[argv.index("--nparts") + 1]) if "--nparts" in argv else 8
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--nparts")]
scale, ef = (int(pos[0]), int(pos[1])) if len(pos) > 1 else (21, 56)
capi.init(0)
csr = capi.HostCSR.generate_rmat(scale, ef, 0.45, 0.22, 0.22)
g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
counts = []
for _ in range(3):
    total, st = g.bk_count(stats=True)
    counts.append(round(st["kernel_ms"], 1))
print(json.dumps({"graph": [scale, ef], "bk_count": total, "count_kernel_ms": counts}), flush=True)
L = capi.lib()
hist = np.zeros(65, dtype=np.int64)
tot = {"cliques": 0, "members": 0, "sizing_ms": 0.0, "sizing_kernel_ms": 0.0, "fill_ms": 0.0, "fill_kernel_ms": 0.0}
for part in range(nparts):
    info, st = capi.BkListInfo(), capi.Stats()
    t0 = time.perf_counter()
    assert L.gmsx_bk_list(g._h, None, part, nparts, None, None, 0, 0, C.byref(info), C.byref(st)) == 0
    t1 = time.perf_counter()
    sizing_kernel = st.kernel_ms
    off = np.empty(info.cliques + 1, dtype=np.int64)
    mem = np.empty(max(info.members, 1), dtype=np.int32)
    off[:] = 0  # first touch outside the timed call
    mem[:] = 0
    t2 = time.perf_counter()
    assert L.gmsx_bk_list(g._h, None, part, nparts, off.ctypes.data_as(C.c_void_p), mem.ctypes.data_as(C.c_void_p), off.size, info.members,
                          C.byref(info), C.byref(st)) == 0
    t3 = time.perf_counter()
    hist += np.asarray(info.size_hist[:], dtype=np.int64)
    rec = {"part": part, "cliques": info.cliques, "members": info.members, "max_size": info.max_size, "sizing_ms": round(1e3 * (t1 - t0), 1),
           "sizing_kernel_ms": round(sizing_kernel, 1), "fill_ms": round(1e3 * (t3 - t2), 1), "fill_kernel_ms": round(st.kernel_ms, 1),
           "copy_and_host_ms": round(1e3 * (t3 - t2) - st.kernel_ms, 1), "launches": st.launches}
    print(json.dumps(rec), flush=True)
    tot["cliques"] += info.cliques
    tot["members"] += info.members
    tot["sizing_ms"] += 1e3 * (t1 - t0)
    tot["sizing_kernel_ms"] += sizing_kernel
    tot["fill_ms"] += 1e3 * (t3 - t2)
    tot["fill_kernel_ms"] += st.kernel_ms
    del off, mem
tot = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in tot.items()}
tot["mean_size"] = round(tot["members"] / max(tot["cliques"], 1), 3)
tot["count_ok"] = tot["cliques"] == total
tot["size_hist"] = {int(s): int(c) for s, c in enumerate(hist) if c}
print(json.dumps({"total": tot}), flush=True)
