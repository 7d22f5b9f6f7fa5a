"""GPU: the light edges of the triangle count as packed blocks (GMSX_TC_LIGHT_PACKED = 1, k_tc_lpack) — one block of whole 16-byte units
per edge, laid out size class by size class, compared by binary search in LDS — against the CPU oracle and against the pointer records
of GMSX_TC_LIGHT_PACKED = 0 (k_tc_light).  Light edges exist on small graphs only with the hub-limit hook of the upload flags and
INLINE_LIMIT, as in test_tc_gpu.py::test_inline_limit."""
import numpy as np
import pytest

from conftest import host_graph

pytestmark = pytest.mark.gpu
HEAVY = 64
# capacities of the size classes in ids: u's hub part, u's tail part in front of v, v's hub part, v's tail part (device_graph.hpp, light_shape)
SHAPES = [(16, 12, 16, 16), (8, 8, 40, 32), (16, 16, 40, 36), (24, 32, 32, 36), (48, 32, 48, 40), (64, 64, 64, 64)]
_CASES = {}


def light_class(ah, at, bh, bt):
    for c, (ca, cb, cc, cd) in enumerate(SHAPES):
        if ah <= ca and at <= cb and bh <= cc and bt <= cd:
            return c
    raise AssertionError((ah, at, bh, bt))


def generated(gpu, oracle, name):
    """(csr, triangles) of the two generated graphs, built once per session and left unchanged."""
    if name not in _CASES:
        kind, scale, deg = {"kron13_16": ("kronecker", 13, 16), "uniform12_20": ("uniform", 12, 20)}[name]
        csr = host_graph(gpu, kind, scale, deg, True)
        _CASES[name] = (csr, oracle.tc_total(csr.offsets(), csr.neighbors()))
    return _CASES[name]


def cpu_light_edges(csr, hub_limit, inline_limit):
    """A lower bound, from degrees and limits alone, of the edges that stay with the light-edge kernel: oriented edges (u, v) — towards
    the higher degree — with 2 <= d+(u) < 64, d+(v) < 64, rank(v) >= max(hub limit, inline limit), rank(u) >= hub limit (the core never
    reaches beyond the hub ids).  Only pairs of strictly different degree are counted, so the tie rule of the ranking does not matter."""
    off, adj = np.asarray(csr.offsets()), np.asarray(csr.neighbors())
    n = len(off) - 1
    deg = np.diff(off)
    src = np.repeat(np.arange(n), deg)
    rank = np.empty(n, dtype=np.int64)
    rank[np.lexsort((np.arange(n), -deg))] = np.arange(n)
    up = rank[adj] < rank[src]  # src -> adj is an oriented edge
    dplus = np.bincount(src[up], minlength=n)
    limit = min(n, max(hub_limit, inline_limit))
    u, v = src[up], adj[up]
    keep = (dplus[u] >= 2) & (dplus[u] < HEAVY) & (dplus[v] < HEAVY) & (rank[v] >= limit) & (rank[u] >= hub_limit) & (deg[u] != deg[v])
    return int(keep.sum())


def run(gpu, csr, hub_limit, shard=None):
    """(count, stats, breakdown) of one upload under the options in force."""
    kw = {"shard": shard} if shard else {}
    g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8), **kw)
    try:
        t, st = g.tc_partial(shard[0], shard[1], stats=True) if shard else g.tc_total(stats=True)
        return t, st, g.tc_stream_breakdown()
    finally:
        g.free()


def check_both(gpu, csr, want, hub_limit, min_light=1):
    """Packed and pointer records: the oracle's count, units = m, the byte fields add up, the same light edges."""
    seen = {}
    for packed in (1, 0):
        gpu.set_option("TC_LIGHT_PACKED", packed)
        t, st, b = run(gpu, csr, hub_limit)
        print(f"packed={packed} hub_limit={hub_limit}: total={t} want={want} units={st['units']} light={b['count_light_streamed_members']} "
              f"launches={st['launches']} stream_bytes={st['stream_bytes']}")
        assert t == want
        assert st["units"] == csr.num_edges
        assert sum(b[x] for x in gpu.DeviceGraph.BREAKDOWN_BYTES) == st["stream_bytes"]
        assert b["count_light_streamed_members"] >= min_light
        seen[packed] = b
    assert seen[1]["count_light_streamed_members"] == seen[0]["count_light_streamed_members"]
    assert seen[1]["light_pivot_lists_and_descriptors"] == 0  # a block has no record and no header
    assert seen[1]["light_streamed_hub_rows"] % 16 == 0 and seen[1]["light_streamed_tail_rows"] % 16 == 0
    return seen


@pytest.mark.parametrize("hub_limit,inline_limit", [(16, 0), (16, 40), (300, 301)])
@pytest.mark.parametrize("name", ["kron13_16", "uniform12_20"])
def test_generated_graphs(gpu, oracle, name, hub_limit, inline_limit):
    csr, want = generated(gpu, oracle, name)
    expect = cpu_light_edges(csr, hub_limit, inline_limit)
    print(f"{name} hub_limit={hub_limit} inline_limit={inline_limit}: at least {expect} light edges by degrees and limits")
    assert expect > 0
    gpu.set_option("INLINE_LIMIT", str(inline_limit))
    try:
        check_both(gpu, csr, want, hub_limit)  # (the light-edge count itself must be positive: check_both)
    finally:
        gpu.reset_options()


# ---- hand-made graph: light pairs (u, v) whose four parts have chosen lengths -----------------------------------------------------------
NH = NW = 64  # hubs (the 64 highest degrees: hub limit 64) and "top tail" vertices (the next 64 degrees: tail ids in front of every u and v)
EDGE_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 62]
TAILS = [(0, 0), (1, 0), (0, 1), (4, 4), (5, 4), (4, 5), (8, 8), (9, 8), (8, 9), (15, 16), (16, 17), (17, 16), (31, 1), (1, 31), (33, 20), (20, 33), (0, 62), (62, 0)]


def pair_specs():
    """(ah, at, bh, bt) of the hand-made pairs: every combination of the hub lengths, the tail lengths cycling (cut down to d+ < 64: u has
    ah + at + 1 ids — v itself —, v has bh + bt)."""
    specs, i = [], 0
    for ah in EDGE_LENGTHS:
        for bh in EDGE_LENGTHS:
            at, bt = TAILS[i % len(TAILS)]
            i += 1
            specs.append((ah, min(at, 62 - ah), bh, min(bt, 63 - bh)))
    # small hub parts against every tail pair, an empty hub part against an empty tail part, the largest blocks
    specs += [(1, min(a, 61), 1, min(b, 62)) for a, b in TAILS] + [(0, 3, 5, 0), (5, 0, 0, 3), (0, 62, 63, 0), (62, 0, 0, 63), (31, 31, 31, 32)]
    # every class filled to the brim, and one id more in each of its four parts (cut down to d+ < 64)
    for ca, cb, cc, cd in SHAPES[:-1]:
        full = (ca, min(cb, 62 - ca), cc, min(cd, 63 - cc))
        specs.append(full)
        for k in range(4):
            more = list(full)
            more[k] += 1
            if more[0] + more[1] <= 62 and more[2] + more[3] <= 63:
                specs.append(tuple(more))
        specs += [(ca, 0, cc, 0), (ca + 1, 0, cc, 0), (ca, 0, cc + 1, 0), (0, cb, 0, cd), (0, cb + 1, 0, cd), (0, cb, 0, cd + 1)]
    return specs


def handmade(gpu, oracle):
    """Hubs h (degree 3000 + i), top-tail vertices w (1000 + j), per pair a v (degree 600) and a u (degree 400); private leaves of degree 1 pad
    every degree.  u is adjacent to ah hubs, at top-tail vertices and v; v to bh hubs and bt top-tail vertices.  u's row is therefore ah hub
    ids + at tail ids in front of v, v's row bh + bt ids; every w is a far light member as well (d+ = 0), which adds edges of further shapes.
    Odd pairs take their hubs / top-tail vertices from the upper end, even ones from the lower end: the common neighbours are then the first
    ids of a part, the last ones, or lie in both parts."""
    if "handmade" not in _CASES:
        specs = pair_specs()
        assert {light_class(*s) for s in specs} == set(range(len(SHAPES)))
        hubs, tops = np.arange(NH), NH + np.arange(NW)
        nxt = NH + NW
        src, dst, target = [], [], {}
        for i in range(NH):
            target[int(hubs[i])] = 3000 + i
        for j in range(NW):
            target[int(tops[j])] = 1000 + j
        for p, (ah, at, bh, bt) in enumerate(specs):
            v, u = nxt, nxt + 1
            nxt += 2
            target[v], target[u] = 600, 400
            pick = (lambda a, k, low: a[:k] if low else a[len(a) - k:])
            for x in pick(hubs, ah, p % 2 == 0):
                src.append(u), dst.append(int(x))
            for x in pick(tops, at, p % 3 == 0):
                src.append(u), dst.append(int(x))
            for x in pick(hubs, bh, p % 4 < 2):
                src.append(v), dst.append(int(x))
            for x in pick(tops, bt, p % 5 < 3):
                src.append(v), dst.append(int(x))
            src.append(u), dst.append(v)
        deg = np.bincount(np.array(src + dst), minlength=nxt)
        for x, want_deg in target.items():
            k = want_deg - int(deg[x])
            assert k >= 0
            src += [x] * k
            dst += list(range(nxt, nxt + k))
            nxt += k
        csr = gpu.HostCSR.from_edges(np.array(src, dtype=np.int32), np.array(dst, dtype=np.int32))
        _CASES["handmade"] = (csr, oracle.tc_total(csr.offsets(), csr.neighbors()), len(specs))
    return _CASES["handmade"]


def test_handmade_class_edges(gpu, oracle):
    csr, want, npairs = handmade(gpu, oracle)
    assert want > 0
    gpu.set_option("INLINE_LIMIT", "0")
    try:
        seen = check_both(gpu, csr, want, NH, min_light=npairs - 2)  # (two pairs have a u with d+ = 1: no pivot)
        # every block is at least the smallest class and at most the largest one
        light = seen[1]["count_light_streamed_members"]
        blocks = seen[1]["light_streamed_hub_rows"] + seen[1]["light_streamed_tail_rows"]
        strides = [16 * (a // 8 + b // 4 + c // 8 + d // 4) for a, b, c, d in SHAPES]  # bytes per block
        assert min(strides) * light <= blocks <= max(strides) * light
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("name", ["kron13_16", "handmade"])
def test_shards_of_a_full_upload(gpu, oracle, name):
    csr, want = generated(gpu, oracle, name) if name != "handmade" else handmade(gpu, oracle)[:2]
    hub_limit = NH if name == "handmade" else 16
    gpu.set_option("INLINE_LIMIT", "0")
    try:
        g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8))
        t, st = g.tc_total(stats=True)
        assert t == want and st["units"] == csr.num_edges
        assert g.tc_stream_breakdown()["count_light_streamed_members"] > 0
        for nparts in (2, 3, 5, 8):
            parts = [g.tc_partial(p, nparts, stats=True) for p in range(nparts)]
            assert sum(p[0] for p in parts) == want, nparts
            assert sum(p[1]["units"] for p in parts) == csr.num_edges, nparts
            assert sum(p[1]["stream_bytes"] for p in parts) == st["stream_bytes"], nparts
        g.free()
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("name", ["kron13_16", "handmade"])
def test_sharded_uploads(gpu, oracle, name, nparts):
    csr, want = generated(gpu, oracle, name) if name != "handmade" else handmade(gpu, oracle)[:2]
    hub_limit = NH if name == "handmade" else 16
    gpu.set_option("INLINE_LIMIT", "0")
    try:
        total = units = 0
        for p in range(nparts):
            t, st, _ = run(gpu, csr, hub_limit, shard=(p, nparts))
            total += t
            units += st["units"]
        assert total == want and units == csr.num_edges
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("knobs", [{"TC_CORE": "1024"}, {"TC_OVERLAP": "1"}, {"TC_PERSIST": "0"}, {"TC_PERSIST": "0", "TC_OVERLAP": "1"}])
def test_knobs_beside_it(gpu, oracle, knobs):
    """A forced core (clamped to the 300 hub ids: the light pivots' hub members are core pivots), the light edges on a side stream, the
    one-workgroup-per-item kernels: the counts stay."""
    csr, want = generated(gpu, oracle, "kron13_16")
    try:
        for name, value in knobs.items():
            gpu.set_option(name, value)
        gpu.set_option("INLINE_LIMIT", "301")
        seen = check_both(gpu, csr, want, 300)
        if "TC_CORE" in knobs:
            assert seen[1]["core_k"] == 300
    finally:
        gpu.reset_options()
