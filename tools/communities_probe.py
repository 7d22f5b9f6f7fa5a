"""GPU probe: gmsx_label_propagation and gmsx_modularity on one handle per graph, in one process (run it under `timeout`) — the measurement of
DESIGN.md §5.4o.  Per graph, JSON lines:
  * "hbm_read_gbs": gmsx_hbm_read_probe on the same device, the stream the gather is held against;
  * per (weighted, LP_WG_WORK default / 0 / the values of --wg-work, LP_ACTIVE 0 / 1): --calls calls (default 5) by their own HIP events, kernel_ms (the sweeps) and
    kernel_ms + setup_ms, the MIDDLE THREE of them as [median, smallest, largest]; sweeps, launches, rows and arcs of the last call; every
    output must be the same bytes under all of them;
  * "sweeps_detail" (defaults only): the library's own per-sweep lines of one further call under the option TIMING, where every launch is waited
    for: [changes, rows, arcs, launches, ms, ms of the four bins (16-lane group, wave, LDS table, global table), ms of the one-workgroup launches];
  * "sweep1": one call with max_sweeps = 1 and LP_ACTIVE = 0: its kernel_ms, and the gathered bytes per second, nnz * (4 + 4 [+ 4 weighted])
    over that time;
  * gmsx_modularity of the result: kernel_ms and the integers.
--bins adds the forced bins (every row long, every row up to 4096 entries in LDS); --wg-work A,B,… adds values of LP_WG_WORK (a huge one puts the
whole graph through one workgroup: seconds per call at scale 20).

usage: communities_probe.py [--calls N] [--bins] [--wg-work A,B,…] GRAPH…
GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE (generated weights 1 … 255) | a file gmsx_csr_load_weighted reads."""
import json, os, re, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gms_amd import capi

argv = sys.argv[1:]
calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 5
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--calls", "--wg-work"))]
WG_WORK = [None, 0] + ([int(x) for x in argv[argv.index("--wg-work") + 1].split(",")] if "--wg-work" in argv else [])
BINS = [None] + ([(0, 0), (0, 4096)] if "--bins" in argv else [])


def load(name):
    parts = name.split("-")
    if len(parts) == 3 and parts[0] in ("kronecker", "uniform"):
        return capi.HostCSR.generate_weighted(parts[0], int(parts[1]), int(parts[2]), capi.RELABEL_NEVER)
    return capi.HostCSR.load_weighted(name)


def middle(values):
    mid = sorted(values)[1:-1] if len(values) >= 5 else sorted(values)
    return [round(float(np.median(mid)), 4), round(min(mid), 4), round(max(mid), 4)]


def sweeps_detail(fn):
    """the [gmsx communities] lines one call under TIMING writes to the C library's stderr"""
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
    pat = (r"\[gmsx communities\] sweep \d+: (\d+) changes, (\d+) rows, (\d+) arcs, (\d+) launches, ([\d.]+) ms \(every launch waited for: "
           r"bins ([\d.]+) ([\d.]+) ([\d.]+) ([\d.]+), one workgroup ([\d.]+)\)")
    return [[int(x) for x in m.groups()[:4]] + [float(x) for x in m.groups()[4:]] for m in re.finditer(pat, text)]


capi.init(0)
for name in names:
    t0 = time.perf_counter()
    csr = load(name)
    n, nnz = csr.num_nodes, csr.nnz
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    g.set_weights(csr.weights())
    print(json.dumps({"graph": name, "n": n, "nnz": nnz, "load_s": round(time.perf_counter() - t0, 1),
                      "hbm_read_gbs": round(capi.hbm_read_probe(1 << 30, 10), 1)}), flush=True)
    col = [g.coloring_jp(stats=True) for _ in range(3)]
    print(json.dumps({"graph": name, "coloring_ms": middle([c[2]["kernel_ms"] for c in col]), "colors": col[-1][1]["colors"]}), flush=True)
    for weighted in (False, True):
        first = None
        for bins in BINS:
            for wg_work in WG_WORK:
                for active in (1, 0):
                    opts = {"LP_ACTIVE": active}
                    if wg_work is not None:
                        opts["LP_WG_WORK"] = wg_work
                    if bins is not None:
                        opts["LP_WAVE_ROW"], opts["LP_LDS_ROW"] = bins
                    with capi.options(**opts):
                        run = lambda: g.label_propagation(weighted=weighted, stats=True)  # noqa: E731
                        run()
                        rs = [run() for _ in range(calls)]
                        detail = sweeps_detail(run) if wg_work is None and bins is None else None
                    r = rs[-1]
                    same = (r[0].tobytes(), json.dumps(r[1], sort_keys=True))
                    first = first if first is not None else same
                    assert same == first, (name, weighted, opts)
                    line = {"graph": name, "weighted": weighted, "wg_work": wg_work, "active": active, "bins": bins,
                            "kernel_ms": middle([x[2]["kernel_ms"] for x in rs]), "ms": middle([x[2]["kernel_ms"] + x[2]["setup_ms"] for x in rs]),
                            "calls": calls, "sweeps": r[1]["sweeps"], "changes": r[1]["changes"], "communities": r[1]["communities"],
                            "launches": r[2]["launches"], "rows": r[2]["units"], "arcs": r[2]["alg_elements"]}
                    if detail is not None:
                        line["sweeps_detail"] = detail
                    print(json.dumps(line), flush=True)
        with capi.options(LP_ACTIVE=0):
            one = [g.label_propagation(weighted=weighted, max_sweeps=1, want_labels=False, stats=True) for _ in range(calls)]
        ms = middle([x[2]["kernel_ms"] for x in one])
        print(json.dumps({"graph": name, "weighted": weighted, "sweep1_kernel_ms": ms, "sweep1_launches": one[-1][2]["launches"],
                          "sweep1_gather_gbs": round(nnz * (12 if weighted else 8) / (ms[0] * 1e-3) / 1e9, 1)}), flush=True)
        label = g.label_propagation(weighted=weighted)[0]
        mods = [g.modularity(label, weighted=weighted, stats=True) for _ in range(calls)]
        m = mods[-1][0]
        print(json.dumps({"graph": name, "weighted": weighted, "modularity_kernel_ms": middle([x[1]["kernel_ms"] for x in mods]),
                          "modularity_ms": middle([x[1]["kernel_ms"] + x[1]["setup_ms"] for x in mods]),
                          "modularity": {k: m[k] for k in ("total_weight", "intra_weight", "communities", "largest", "unstable", "modularity")}}), flush=True)
    g.free()
    del csr
