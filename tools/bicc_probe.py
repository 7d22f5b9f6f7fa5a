"""GPU probe: gmsx_biconnected_components on one handle per graph, in one process (run it under `timeout`) — the measurement of DESIGN.md §5.4q.
Per graph first one line with the times of gmsx_connected_components and gmsx_bfs (source 0) on the same handle, the yardsticks.  Then per
option setting one JSON line: one warm-up, then --calls calls (default 5) by their own HIP events, kernel_ms and kernel_ms + setup_ms as
[median, smallest, largest]; launches, levels, alg_elements (the arcs the arc passes examined) and the info block of the last call; and
"phases_ms", the library's own line of one further call under the option TIMING: the wall time of the roots, the forest, the three sweeps by
level (nd, preorder, lowhigh), the arc passes and the ids (under TIMING every phase ends in a synchronize, so their sum exceeds kernel_ms).
Every output must be the same bytes under every setting.  --no-arrays asks for the info block only (no block, no arc_keep).
--options adds the ends of BCC_WG_LEVEL and BCC_WG_FRONTIER and the two ends of BCC_WAVE_ROW / BCC_WG_ROW to the defaults.

usage: bicc_probe.py [--calls N] [--options] [--no-arrays] GRAPH…
GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | grid-ROWS-COLS | path-N | a file gmsx_csr_load reads (never relabelled)."""
import json, os, re, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 5
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--calls")]
arrays = "--no-arrays" not in argv
HUGE = 2 ** 31 - 1
DEFAULTS = {"BCC_WAVE_ROW": 256, "BCC_WG_ROW": 4096, "BCC_WG_FRONTIER": 512, "BCC_WG_LEVEL": 1024}
SETTINGS = [{}]
if "--options" in argv:
    SETTINGS += [{"BCC_WG_LEVEL": 0}, {"BCC_WG_LEVEL": 64}, {"BCC_WG_LEVEL": 16384}, {"BCC_WG_FRONTIER": 0}, {"BCC_WG_FRONTIER": 4096},
                 {"BCC_WAVE_ROW": 1, "BCC_WG_ROW": HUGE}, {"BCC_WAVE_ROW": 64, "BCC_WG_ROW": 1024}, {"BCC_WAVE_ROW": HUGE, "BCC_WG_ROW": HUGE}]


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate(parts[0], int(parts[1]), int(parts[2]), capi.RELABEL_NEVER)
    if len(parts) == 3 and parts[0] == "grid":
        rows, cols = int(parts[1]), int(parts[2])
        ids = np.arange(rows * cols, dtype=np.int32).reshape(rows, cols)
        return capi.HostCSR.from_edges(np.concatenate([ids[:, :-1].ravel(), ids[:-1].ravel()]), np.concatenate([ids[:, 1:].ravel(), ids[1:].ravel()]),
                                       num_nodes=rows * cols)
    if len(parts) == 2 and parts[0] == "path":
        return capi.HostCSR.from_edges(np.arange(int(parts[1]) - 1, dtype=np.int32), np.arange(1, int(parts[1]), dtype=np.int32), num_nodes=int(parts[1]))
    return capi.HostCSR.load(name, relabel=capi.RELABEL_NEVER)


def spread(values):
    return [round(float(np.median(values)), 4), round(min(values), 4), round(max(values), 4)]


def phases(fn):
    """the [gmsx bicc] line one call under TIMING writes to the C library's stderr"""
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
    m = re.search(r"\[gmsx bicc\] roots ([\d.]+) forest ([\d.]+) nd ([\d.]+) preorder ([\d.]+) lowhigh ([\d.]+) arcs ([\d.]+) ids ([\d.]+) ms", text)
    return dict(zip(("roots", "forest", "nd", "preorder", "lowhigh", "arcs", "ids"), (float(x) for x in m.groups()))) if m else None


capi.init(0)
for name in names:
    t0 = time.perf_counter()
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    print(json.dumps({"graph": name, "n": n, "nnz": nnz, "load_s": round(time.perf_counter() - t0, 1)}), flush=True)
    g.connected_components()
    cc = [g.connected_components(stats=True) for _ in range(calls)]
    g.bfs(0)
    bfs = [g.bfs(0, stats=True) for _ in range(calls)]
    print(json.dumps({"graph": name, "cc_kernel_ms": spread([c[2]["kernel_ms"] for c in cc]), "cc_ms": spread([c[2]["kernel_ms"] + c[2]["setup_ms"] for c in cc]),
                      "components": cc[-1][1]["components"], "bfs_kernel_ms": spread([b[3]["kernel_ms"] for b in bfs]),
                      "bfs_ms": spread([b[3]["kernel_ms"] + b[3]["setup_ms"] for b in bfs]), "bfs_levels": bfs[-1][2]["levels"]}), flush=True)
    first = None
    for setting in SETTINGS:
        with capi.options(**setting):
            run = lambda: g.biconnected_components(want_block=arrays, want_blocks_at=True, want_mask=arrays, stats=True)  # noqa: E731
            run()
            rs = [run() for _ in range(calls)]
            detail = phases(run)
        r = rs[-1]
        same = tuple(a.tobytes() if a is not None else b"" for a in r[:3]) + (json.dumps(r[3], sort_keys=True),)
        first = first if first is not None else same
        assert same == first, (name, setting)
        print(json.dumps({"graph": name, "options": dict(DEFAULTS, **setting), "arrays": arrays, "kernel_ms": spread([x[4]["kernel_ms"] for x in rs]),
                          "ms": spread([x[4]["kernel_ms"] + x[4]["setup_ms"] for x in rs]), "calls": calls, "launches": r[4]["launches"],
                          "levels": r[3]["levels"], "arcs_examined": r[4]["alg_elements"], "info": r[3], "phases_ms": detail}), flush=True)
    g.free()
    del csr
