"""GPU probe: gmsx_coloring_jp under the colouring heuristics, in one process.  Per graph and heuristic one JSON line: colors, rounds, max_pred,
first_round; kernel / wall time and launches of the colouring (best of --reps, default 3) with the one-workgroup rounds at their default,
and again with them disabled (COLOR_WG_FRONTIER=0: every round a kernel boundary) — the comparison the one-workgroup rounds must win —; the
mean time per round of both; the kernel / wall time of the order's producer; the verifier's time and verdict.
usage: coloring_probe.py [--reps N] [--orders id,lf,sl,adg] GRAPH…
GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | rmat-SCALE-DEGREE (a = .45, b = c = .22) | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gms_amd import capi

argv = sys.argv[1:]
reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 3
orders = argv[argv.index("--orders") + 1].split(",") if "--orders" in argv else ["id", "lf", "sl", "adg"]
names = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--reps", "--orders"))]


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
        if best is None or st["kernel_ms"] < best[1]["kernel_ms"]:
            best = (r, st, wall)
    return best


def producer(g, heuristic):
    """(rank or None, stats of the producer or None, wall ms)"""
    if heuristic in ("id", "ff"):
        t0 = time.perf_counter()
        rank = g.color_order(heuristic)
        return rank, None, 1e3 * (time.perf_counter() - t0)
    if heuristic == "lf":
        (rank, _), st, wall = timed(lambda: g.degree_rank(stats=True))
    elif heuristic == "sl":
        (_, rank, _, _), st, wall = timed(lambda: g.core_decomposition(stats=True))
    else:
        (rank, _, _), st, wall = timed(lambda: g.adg_rank(0.001, stats=True))
    return rank, st, wall


capi.init(0)
for name in names:
    csr = load(name)
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    g.coloring_jp()  # warm-up: first launches of the kernels
    for heuristic in orders:
        rank, pst, pwall = producer(g, heuristic)
        (col, info, _), st, wall = timed(lambda: g.coloring_jp(rank, stats=True))
        with capi.options(COLOR_WG_FRONTIER=0):
            (col0, info0, _), st0, wall0 = timed(lambda: g.coloring_jp(rank, stats=True))
        assert info0 == info and col0.tobytes() == col.tobytes()
        (chk, _), vst, vwall = timed(lambda: g.coloring_verify(col, stats=True))
        rounds = max(info["rounds"], 1)
        print(json.dumps({
            "graph": name, "order": heuristic, "n": csr.num_nodes, "m": csr.num_edges, **info,
            "coloring": {"kernel_ms": round(st["kernel_ms"], 3), "wall_ms": round(wall, 3), "launches": st["launches"],
                         "us_per_round": round(1e3 * st["kernel_ms"] / rounds, 2)},
            "coloring_every_round_a_launch": {"kernel_ms": round(st0["kernel_ms"], 3), "wall_ms": round(wall0, 3), "launches": st0["launches"],
                                              "us_per_round": round(1e3 * st0["kernel_ms"] / rounds, 2)},
            "producer": {"kernel_ms": round(pst["kernel_ms"], 3) if pst else None, "wall_ms": round(pwall, 3)},
            "verify": {"kernel_ms": round(vst["kernel_ms"], 3), "wall_ms": round(vwall, 3),
                       "pass": chk["conflicts"] == 0 and chk["invalid"] == 0 and chk["max_color"] == chk["distinct"] == info["colors"]},
        }), flush=True)
    g.free()
    del csr
