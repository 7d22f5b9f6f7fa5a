"""GPU probe: gmsx_link_prediction per graph and metric, in one process.  Per (graph, metric) one JSON line, best of --reps (default 3) by
kernel time:
  q = m / 4, the reference driver's choice (link_prediction.cc:36): kernel / wall ms, launches, found, scored, positive, chunks, classes;
  for the five common-neighbour metrics also q = positive + m / 4 — the POS class whole plus a ZERO fill of m / 4 pairs — and the difference
  of the two, which is what the ZERO class costs;
  hub_share: the share of the two-hop walk (sum over w in N(u) of deg(w), entries one workgroup reads alone) that belongs to the heaviest
  source — the known tail of the per-source formulation; computed on the host from the CSR.
usage: link_prediction_probe.py [--reps R] [--metrics jaccard,adamic_adar,...] GRAPH…
       GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | a file the loader reads"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gms_amd import capi

argv = sys.argv[1:]


def flag(name, default):
    return argv[argv.index(name) + 1] if name in argv else default


reps = int(flag("--reps", 3))
metrics = flag("--metrics", "jaccard,adamic_adar").split(",")
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--reps", "--metrics"))]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]))
    return capi.HostCSR.load(name)


def timed(fn):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall = 1e3 * (time.perf_counter() - t0)
        if best is None or r[4]["kernel_ms"] < best[0][4]["kernel_ms"]:
            best = (r, wall)
    (u, v, s, info, st), wall = best
    return {"kernel_ms": round(st["kernel_ms"], 3), "wall_ms": round(wall, 3), "launches": st["launches"], **info}


capi.init(0)
for name in names:
    csr = load(name)
    off, adj = np.asarray(csr.offsets()), np.asarray(csr.neighbors())
    deg = np.diff(off)
    walk = np.add.reduceat(deg[adj], off[:-1][deg > 0]) if adj.size else np.zeros(1, dtype=np.int64)  # per non-isolated source: entries of its two-hop walk
    hub_share = float(walk.max()) / float(max(int(walk.sum()), 1))
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    q = max(1, csr.num_edges // 4)
    for metric in metrics:
        g.link_prediction(metric, 1)  # warm-up: first launches of the kernels, rocPRIM's temporary sizes
        rec = {"graph": name, "n": csr.num_nodes, "m": csr.num_edges, "metric": metric, "q": q, "hub_share": round(hub_share, 5),
               "isolated": int(np.count_nonzero(deg == 0)), "q_m4": timed(lambda: g.link_prediction(metric, q, stats=True))}
        p = rec["q_m4"]["positive"]
        if 0 <= p and p + q <= 1 << 24:  # (beyond: the result arrays alone are gigabytes; the q = m / 4 line stands alone)
            q2 = p + q
            rec["q_pos_plus_m4"] = dict(timed(lambda: g.link_prediction(metric, q2, stats=True)), q=q2)
            q1 = max(p, 1)
            rec["q_pos"] = dict(timed(lambda: g.link_prediction(metric, q1, stats=True)), q=q1)
            rec["zero_fill_kernel_ms"] = round(rec["q_pos_plus_m4"]["kernel_ms"] - rec["q_pos"]["kernel_ms"], 3)
        print(json.dumps(rec), flush=True)
    g.free()
    del csr
