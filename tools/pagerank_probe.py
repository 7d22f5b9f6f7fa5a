"""GPU probe: gmsx_pagerank on one handle, in one process (run it under `timeout`).  Per graph one JSON line.  For either storage type (double,
and float under GMSX_PR_FLOAT32) the call runs --sweeps sweeps (default 20) at tolerance 0, --reps times warm (default 5); reported are the
MEDIAN of kernel_ms / sweeps by the call's own HIP events with the smallest and the largest beside it (the run-to-run spread), the algorithmic
bytes of one sweep with no reuse assumed

    4 nnz                       the ids of the CSR
  + S nnz                       one gathered contribution per id (S = 8 or 4 bytes)
  + (8 + 4 + 8) n               per vertex: its row offset, its entry of the class list, its teleport entry
  + 3 S n                       … its old score read, its new score and its new contribution written

(so bytes = (4 + S) nnz + (20 + 3 S) n), the GB/s these bytes give at the median time, and the fraction of the rate gmsx_hbm_read_probe reports
in this process.  `setup_first_ms` is the setup_ms of the first call on the handle (it builds the row classes), `setup_ms` the median afterwards.

usage: pagerank_probe.py [--reps N] [--sweeps K] GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
sweeps = int(argv[argv.index("--sweeps") + 1]) if "--sweeps" in argv else 20
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--reps", "--sweeps"))]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]))
    return capi.HostCSR.load(name)


capi.init(0)
read_gbs = capi.hbm_read_probe()
for name in names:
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    deg = np.diff(np.asarray(csr.offsets(), dtype=np.int64))
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    out = {"graph": name, "n": n, "nnz": nnz, "max_degree": int(deg.max()), "rows_lane_group_long": [int(((deg > 0) & (deg <= 16)).sum()),
           int(((deg > 16) & (deg <= 1024)).sum()), int((deg > 1024).sum())], "read_gbs": round(read_gbs, 1), "sweeps": sweeps, "reps": reps}
    t0 = time.perf_counter()
    _, info, st = g.pagerank(max_iters=1, tolerance=0, stats=True)  # builds the classes; the first launches of the kernels
    out["setup_first_ms"] = round(st["setup_ms"], 3)
    out["first_call_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    for label, float32, size in (("double", False, 8), ("float32", True, 4)):
        per, setup, wall = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, info, st = g.pagerank(max_iters=sweeps, tolerance=0, float32=float32, stats=True)
            wall.append(1e3 * (time.perf_counter() - t0))
            assert info["iterations"] == sweeps
            per.append(st["kernel_ms"] / sweeps)
            setup.append(st["setup_ms"])
        nbytes = (4 + size) * nnz + (20 + 3 * size) * n
        med = float(np.median(per))
        out[label] = {"sweep_ms_median_min_max": [round(med, 4), round(min(per), 4), round(max(per), 4)], "setup_ms": round(float(np.median(setup)), 3),
                      "wall_ms": round(float(np.median(wall)), 3), "bytes_per_sweep": nbytes, "gbs": round(nbytes / (med * 1e6), 1),
                      "fraction_of_read_probe": round(nbytes / (med * 1e6) / read_gbs, 3), "arcs_per_s": round(nnz / (med * 1e-3), 0),
                      "launches": st["launches"], "error": info["error"], "sum": info["sum"]}
    print(json.dumps(out), flush=True)
    g.free()
    del csr
