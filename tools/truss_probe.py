"""GPU probe: gmsx_truss_decomposition and gmsx_edge_support on one handle, in one process.  Per graph one JSON line: max truss, levels, rounds,
triangles; kernel / setup / wall time and launches of the decomposition (best of --reps, default 3) at the default (TRUSS_WG_FRONTIER=0: every
round a kernel boundary), and again with the one-workgroup tail taking the frontiers of up to 512 edges (TRUSS_WG_FRONTIER=512) — the measured
answer to what the tail saves —; the mean time per round of both; and gmsx_edge_support beside the earlier route to the same numbers, gmsx_intersect_count_batch over all 2 m arcs with its
host pair arrays, the two calls alternating (wall time of both: the batch's kernel time leaves out its copies).
usage: truss_probe.py GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | rmat-SCALE-DEGREE (a = .45, b = c = .22) | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 3
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--reps")]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]))
    if len(parts) >= 3 and parts[0] == "rmat":
        return capi.HostCSR.generate_rmat(int(parts[1]), int(parts[2]), 0.45, 0.22, 0.22)
    return capi.HostCSR.load(name)


def timed(fn):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        wall = 1e3 * (time.perf_counter() - t0)
        st = r[-1]
        if best is None or st["kernel_ms"] + st["setup_ms"] < best[1]["kernel_ms"] + best[1]["setup_ms"]:
            best = (r, st, wall)
    return best


def figures(st, wall, rounds):
    return {"kernel_ms": round(st["kernel_ms"], 3), "setup_ms": round(st["setup_ms"], 3), "wall_ms": round(wall, 3), "launches": st["launches"],
            "us_per_round": round(1e3 * st["kernel_ms"] / max(rounds, 1), 2)}


capi.init(0)
for name in names:
    csr = load(name)
    off, adj = csr.offsets(), csr.neighbors()
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    g.truss_decomposition()  # warm-up: first launches of the kernels, rocPRIM's temporary sizes
    (truss, info, _), st, wall = timed(lambda: g.truss_decomposition(stats=True))
    with capi.options(TRUSS_WG_FRONTIER=512):
        (truss0, info0, _), st0, wall0 = timed(lambda: g.truss_decomposition(stats=True))
    assert info0 == info and truss0.tobytes() == truss.tobytes()
    # edge support beside one intersect_count per arc, alternating
    src = np.repeat(np.arange(off.size - 1, dtype=np.int32), np.diff(off))
    dst = np.ascontiguousarray(adj, dtype=np.int32)
    g.edge_support(), g.intersect_count_batch(src[:1024], dst[:1024])
    sup_wall, sup_kernel, batch_wall, batch_kernel = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        sup, tri, sst = g.edge_support(stats=True)
        sup_wall.append(1e3 * (time.perf_counter() - t0))
        sup_kernel.append(sst["kernel_ms"])
        t0 = time.perf_counter()
        cnt, bst = g.intersect_count_batch(src, dst, stats=True)
        batch_wall.append(1e3 * (time.perf_counter() - t0))
        batch_kernel.append(bst["kernel_ms"])
    assert np.array_equal(cnt.astype(np.int32), sup) and tri == info["triangles"]
    print(json.dumps({
        "graph": name, "n": csr.num_nodes, "m": csr.num_edges, **info,
        "truss": figures(st, wall, info["rounds"]), "truss_tail_512": figures(st0, wall0, info["rounds"]),
        "edge_support": {"wall_ms": round(min(sup_wall), 3), "kernel_ms": round(min(sup_kernel), 3)},
        "intersect_count_batch_all_arcs": {"wall_ms": round(min(batch_wall), 3), "kernel_ms": round(min(batch_kernel), 3)},
    }), flush=True)
    g.free()
    del csr
