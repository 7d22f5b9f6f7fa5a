"""GPU probe: gmsx_greedy_matching on one handle per graph, in one process (run it under `timeout`) — the measurement of DESIGN.md §5.4p.
Per (graph, unweighted / weighted, MATCH_WAVE_ROW / MATCH_WG_ROW, MATCH_KEEP 0 / 1) one JSON line: --calls calls (default 5) by their own HIP
events, kernel_ms and kernel_ms + setup_ms, the MIDDLE THREE of them as [median, smallest, largest]; rounds, pairs, launches and alg_elements
(the arcs the search pass examined) of the last call; and "rounds_detail", the library's own per-round lines of one further call under the
option TIMING: [live vertices, arcs examined, pairs] per round.  After them one line with gmsx_matching_verify's time on the result.  Every
output must be the same bytes under every setting.  --bins adds the two ends of MATCH_WAVE_ROW / MATCH_WG_ROW to the defaults and (64, 1024).

usage: matching_probe.py [--calls N] [--bins] [--unweighted-only] GRAPH…
GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE (generated weights 1 … 255) | grid-ROWS-COLS (weights 1 … 255, numpy RandomState(1)) |
a file gmsx_csr_load_weighted reads."""
import json, os, re, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 5
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--calls")]
HUGE = 2 ** 31 - 1
BINS = [(256, 4096), (64, 1024)] + ([(1, 1), (1, HUGE), (HUGE, HUGE)] if "--bins" in argv else [])
WEIGHTED = (False,) if "--unweighted-only" in argv else (False, True)


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


def middle(values):
    mid = sorted(values)[1:-1] if len(values) >= 5 else sorted(values)
    return [round(float(np.median(mid)), 4), round(min(mid), 4), round(max(mid), 4)]


def rounds_detail(fn):
    """the [gmsx matching] lines one call under TIMING writes to the C library's stderr"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            with capi.options(TIMING=1):
                fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return [[int(x) for x in m.groups()] for m in re.finditer(r"\[gmsx matching\] round \d+: (\d+) live vertices, (\d+) arcs examined, (\d+) pairs", text)]


capi.init(0)
for name in names:
    t0 = time.perf_counter()
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    g.set_weights(csr.weights())
    print(json.dumps({"graph": name, "n": n, "nnz": nnz, "load_s": round(time.perf_counter() - t0, 1)}), flush=True)
    for weighted in WEIGHTED:
        first = None
        for wave_row, wg_row in BINS:
            for keep in (1, 0):
                with capi.options(MATCH_KEEP=keep, MATCH_WAVE_ROW=wave_row, MATCH_WG_ROW=wg_row):
                    run = lambda: g.greedy_matching(weighted=weighted, want_edges=True, stats=True)  # noqa: E731
                    run()
                    rs = [run() for _ in range(calls)]
                    detail = rounds_detail(run)
                r = rs[-1]
                same = tuple(a.tobytes() for a in r[:4]) + (json.dumps(r[4], sort_keys=True),)
                first = first if first is not None else same
                assert same == first, (name, weighted, keep, wave_row, wg_row)
                print(json.dumps({"graph": name, "weighted": weighted, "keep": keep, "wave_row": wave_row, "wg_row": wg_row,
                                  "kernel_ms": middle([x[5]["kernel_ms"] for x in rs]),
                                  "ms": middle([x[5]["kernel_ms"] + x[5]["setup_ms"] for x in rs]), "calls": calls,
                                  "rounds": r[4]["rounds"], "pairs": r[4]["pairs"], "total_weight": r[4]["total_weight"], "exposed": r[4]["exposed"],
                                  "launches": r[5]["launches"], "arcs_examined": r[5]["alg_elements"], "rounds_detail": detail}), flush=True)
        mate = np.frombuffer(first[0], dtype=np.int32)
        vs = [g.matching_verify(mate, weighted=weighted, stats=True) for _ in range(calls)]
        print(json.dumps({"graph": name, "weighted": weighted, "verify_kernel_ms": middle([v[1]["kernel_ms"] for v in vs]), "check": vs[-1][0]}), flush=True)
    g.free()
    del csr
