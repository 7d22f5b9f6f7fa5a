"""GPU probe: gmsx_sssp over the bucket width delta, on one handle per graph, in one process (run it under `timeout`) — the measurement behind
the default rule of delta = 0.  Per (graph, source, delta) one JSON line: --calls calls (default 5) by their own HIP events
(kernel_ms + setup_ms), the MIDDLE THREE of them as [median, smallest, largest]; buckets, rounds, relaxations and launches of the last call; the
bytes the next-bucket passes read (buckets * 2 * n * word bytes) and, per relaxation, the bytes a walker touches (4 id + 4 weight + word).  A
call that takes longer than --slow-ms (default 2000) is not repeated: its line carries "calls": 1.  Before the deltas of a source one line
with gmsx_bfs's time on the same graph and source: the floor.  dist and parent must be the same bytes under every delta.

usage: sssp_probe.py [--calls N] [--sources N] [--deltas a,b,..] [--slow-ms MS] GRAPH…
GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE (generated weights 1 … 255) | grid-ROWS-COLS (weights 1 … 255, numpy RandomState(1)) |
a file gmsx_csr_load_weighted reads.  delta 0 = the library's rule; "one" = one bucket (2^62)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
VALUED = ("--calls", "--sources", "--deltas", "--slow-ms")


def arg(name, default):
    return argv[argv.index(name) + 1] if name in argv else default


calls, n_sources, slow_ms = int(arg("--calls", 5)), int(arg("--sources", 4)), float(arg("--slow-ms", 2000))
deltas = [2 ** 62 if x == "one" else int(x) for x in arg("--deltas", "1,2,4,8,16,32,64,128,256,one,0").split(",")]
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in VALUED)]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate_weighted(parts[0], int(parts[1]), int(parts[2]), capi.RELABEL_NEVER)
    if len(parts) == 3 and parts[0] == "grid":
        rows, cols = int(parts[1]), int(parts[2])
        ids = np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)
        src = np.concatenate([ids[:, :-1].ravel(), ids[:-1].ravel()])
        dst = np.concatenate([ids[:, 1:].ravel(), ids[1:].ravel()])
        return capi.HostCSR.from_weighted_edges(src, dst, np.random.RandomState(1).randint(1, 256, size=src.size), num_nodes=rows * cols)
    return capi.HostCSR.load_weighted(name)


def timed(fn):
    """(last result, [median, smallest, largest] of the middle three device times, calls made)"""
    dev, r = [], None
    for i in range(calls):
        r = fn()
        dev.append(r[-1]["kernel_ms"] + r[-1]["setup_ms"])
        if dev[-1] > slow_ms:
            break
    mid = sorted(dev)[1:-1] if len(dev) >= 5 else sorted(dev)
    return r, [round(float(np.median(mid)), 4), round(min(mid), 4), round(max(mid), 4)], len(dev)


capi.init(0)
for name in names:
    t0 = time.perf_counter()
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    w = csr.weights()
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    g.set_weights(w)
    head = {"graph": name, "n": n, "nnz": nnz, "mean_weight": round(float(np.mean(w)), 3), "mean_degree": round(nnz / n, 3),
            "load_s": round(time.perf_counter() - t0, 1)}
    print(json.dumps(head), flush=True)
    for source in csr.pick_sources(n_sources).tolist():
        g.bfs(source, want_depth=False, want_parent=False)
        (_, _, bi, _), dev, made = timed(lambda: g.bfs(source, want_depth=False, want_parent=False, stats=True))
        print(json.dumps({"graph": name, "source": source, "bfs_ms": dev, "reached": bi["reached"], "levels": bi["levels"]}), flush=True)
        first = None
        for delta in deltas:
            (dist, parent, info, st), dev, made = timed(lambda: g.sssp(source, delta, stats=True))
            first = first if first is not None else (dist.tobytes(), parent.tobytes())
            assert (dist.tobytes(), parent.tobytes()) == first
            word = 8 if info["wide"] else 4
            print(json.dumps({"graph": name, "source": source, "delta": "auto" if delta == 0 else ("one" if delta == 2 ** 62 else delta),
                              "delta_used": info["delta"], "ms": dev, "calls": made, "buckets": info["buckets"], "rounds": info["rounds"],
                              "relaxations": info["relaxations"], "launches": st["launches"], "max_dist": info["max_dist"],
                              "sweep_bytes": info["buckets"] * 2 * n * word, "bytes_per_relaxation": 8 + word}), flush=True)
    g.free()
    del csr
