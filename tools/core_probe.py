"""GPU probe: gmsx_core_decomposition beside gmsx_adg_rank on the same handle, in one process, and the quality of the ADG, degree and exact
orders.  Per graph one JSON line: degeneracy, levels, rounds; kernel / wall time and launches of the core decomposition (best of --reps,
default 3) with the one-workgroup tail at its default, and again with it disabled (CORE_WG_FRONTIER=0: every round a kernel boundary) — the
measured answer to what the tail saves —; the mean time per round of both; the same figures of gmsx_adg_rank; core_number_of_order of the three
orders against the exact degeneracy.
usage: core_probe.py GRAPH…   GRAPH = kronecker-SCALE-DEGREE | uniform-SCALE-DEGREE | rmat-SCALE-DEGREE (a = .45, b = c = .22) | a file the loader reads"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
        if best is None or st["kernel_ms"] < best[1]["kernel_ms"]:
            best = (r, st, wall)
    return best


capi.init(0)
for name in names:
    csr = load(name)
    g = capi.DeviceGraph.from_csr(csr, flags=capi.UPLOAD_TRUSTED)
    g.core_decomposition(order=False)  # warm-up: first launches of the kernels, rocPRIM's temporary sizes
    (core, rank, info, _), st, wall = timed(lambda: g.core_decomposition(stats=True))
    with capi.options(CORE_WG_FRONTIER=0):
        (core0, rank0, info0, _), st0, wall0 = timed(lambda: g.core_decomposition(stats=True))
    assert info0 == info and rank0.tobytes() == rank.tobytes() and core0.tobytes() == core.tobytes()
    _, peel, peel_wall = timed(lambda: g.core_decomposition(order=False, stats=True))
    (adg, adg_rounds, _), ast, awall = timed(lambda: g.adg_rank(0.001, stats=True))
    (deg, _), dst, dwall = timed(lambda: g.degree_rank(stats=True))
    d = info["degeneracy"]
    q = {tag: g.order_quality(r, core_number=d) for tag, r in (("adg", adg), ("degree", deg), ("exact", rank))}
    (_, qst), _, qwall = timed(lambda: g.order_quality(adg, core_number=d, stats=True))
    rounds = max(info["rounds"], 1)
    print(json.dumps({
        "graph": name, "n": csr.num_nodes, "m": csr.num_edges, **info,
        "core": {"kernel_ms": round(st["kernel_ms"], 3), "wall_ms": round(wall, 3), "launches": st["launches"], "us_per_round": round(1e3 * st["kernel_ms"] / rounds, 2)},
        "core_peel_only": {"kernel_ms": round(peel["kernel_ms"], 3), "wall_ms": round(peel_wall, 3), "launches": peel["launches"]},
        "core_no_tail": {"kernel_ms": round(st0["kernel_ms"], 3), "wall_ms": round(wall0, 3), "launches": st0["launches"],
                         "us_per_round": round(1e3 * st0["kernel_ms"] / rounds, 2)},
        "adg": {"kernel_ms": round(ast["kernel_ms"], 3), "wall_ms": round(awall, 3), "launches": ast["launches"], "rounds": adg_rounds},
        "degree_rank": {"kernel_ms": round(dst["kernel_ms"], 3), "wall_ms": round(dwall, 3)},
        "order_quality": {"kernel_ms": round(qst["kernel_ms"], 3), "wall_ms": round(qwall, 3)},
        "core_number_of_order": {tag: v["core_number_of_order"] for tag, v in q.items()},
        "faulty": {tag: v["faulty"] for tag, v in q.items()},
        "relative_error": {tag: round(v["relative_error"], 4) for tag, v in q.items()},
    }), flush=True)
    g.free()
    del csr
