"""GPU: the dense core of the triangle count (GMSX_TC_CORE, k_tc_core).  The oriented edges whose pivot-side endpoint has a rank id below
K are counted as one masked bit-GEMM on the matrix cores and leave the streamed path — no task entry, no inline copy, no light-edge record.
Every such edge must be counted exactly once whatever K is: the totals are compared with the oracle or a closed form, the bookkeeping
(units = m, the breakdown adds up to stream_bytes, slot 16 = the clamped K) and the shard sums with what they must be."""
import numpy as np
import pytest

from conftest import edges_to_csr, host_graph, load_golden

pytestmark = pytest.mark.gpu
GRAPHS = load_golden("graphs.json")
CORE_CAP = 32768
HUB_IDS = 65535

# kronecker 13/16 and 13/40: a dense top, heavy and light pivots, reverse entries, inline rows; uniform 10/120: a dense core without a
# degree skew; K200: every edge is a core edge at K = 200; a path: no triangle, every row one id
SHAPES = ["kron13_16", "kron13_40", "uniform10_120", "k200", "path"]
# 1, 2: rows clamped at K - 1 inside one block; 63 / 64 / 65: a last partial block, one full block, the first second block; 100, 129: the
# 2-word and 4-word tails (nw = 2 (bj + 1) = 4, 6); 1000: first full 8-word chunks (bj >= 3); 5000: many chunks, rounds over the XCDs;
# 10 ** 6: above n and above the cap
KS = [1, 2, 63, 64, 65, 100, 129, 1000, 5000, 10 ** 6]
_CASES = {}


def case(gpu, oracle, shape):
    """(csr, triangles): built once per session and left unchanged."""
    if shape not in _CASES:
        if shape == "k200":
            iu = np.triu_indices(200, 1)
            csr = gpu.HostCSR.from_edges(iu[0].astype(np.int32), iu[1].astype(np.int32))
            want = 200 * 199 * 198 // 6
        elif shape == "path":
            csr = edges_to_csr(gpu, [(i, i + 1) for i in range(1000)])
            want = 0
        else:
            kind, scale, deg = {"kron13_16": ("kronecker", 13, 16), "kron13_40": ("kronecker", 13, 40), "uniform10_120": ("uniform", 10, 120)}[shape]
            csr = host_graph(gpu, kind, scale, deg, True)
            want = oracle.tc_total(csr.offsets(), csr.neighbors())
        _CASES[shape] = (csr, want)
    return _CASES[shape]


def clamped(k, n, hub_limit=0):
    return min(k, hub_limit or HUB_IDS, n, CORE_CAP)


def check(gpu, csr, want, k, hub_limit=0, shards=(3, 5)):
    """Upload under the options in force and assert everything the core must keep."""
    g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8))
    try:
        t, st = g.tc_total(stats=True)
        b = g.tc_stream_breakdown()
        print(f"K={k} hub_limit={hub_limit}: total={t} want={want} units={st['units']} m={csr.num_edges} core_k={b['core_k']} "
              f"core_bytes={b['core_matrix']} launches={st['launches']} items={b['count_work_items']}")
        assert t == want
        assert st["units"] == csr.num_edges
        assert sum(b[x] for x in gpu.DeviceGraph.BREAKDOWN_BYTES) == st["stream_bytes"]
        assert b["core_k"] == clamped(k, g.num_nodes, hub_limit)
        assert (b["core_matrix"] > 0) == (b["core_k"] > 0)
        for nparts in shards:
            parts = [g.tc_partial(p, nparts, stats=True) for p in range(nparts)]
            assert sum(p[0] for p in parts) == want, nparts
            assert sum(p[1]["units"] for p in parts) == csr.num_edges, nparts
            assert sum(p[1]["stream_bytes"] for p in parts) == st["stream_bytes"], nparts  # items, light edges and core blocks are each dealt out exactly once
        return st, b
    finally:
        g.free()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forced_core(gpu, oracle, shape, k):
    csr, want = case(gpu, oracle, shape)
    gpu.set_option("TC_CORE", k)
    try:
        st, b = check(gpu, csr, want, k)
        if shape == "k200" and k >= 200:  # the graph lies inside the core: no work item, no light edge, one launch
            assert b["count_work_items"] == 0 and b["count_entries"] == 0 and b["count_light_streamed_members"] == 0 and st["launches"] == 1
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("hub_limit", [16, 300])
@pytest.mark.parametrize("shape", ["kron13_16", "kron13_40", "uniform10_120"])
def test_core_clamps_to_the_hub_limit(gpu, oracle, shape, hub_limit):
    """A core row holds hub ids only: with 16 / 300 hub ids K = 1000 and K = 5000 come out as 16 / 300, a smaller K stays."""
    csr, want = case(gpu, oracle, shape)
    try:
        for k in (10, 1000, 5000):
            gpu.set_option("TC_CORE", k)
            check(gpu, csr, want, k, hub_limit=hub_limit)
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("knobs", [{"TC_TWO_SIDED": "0"}, {"TC_PERSIST": "0"}, {"TC_INLINE_FIRST": "5"}, {"INLINE_LIMIT": "0"}])
def test_core_beside_the_task_list_knobs(gpu, oracle, knobs):
    try:
        for name, value in knobs.items():
            gpu.set_option(name, value)
        for shape in ("kron13_40", "uniform10_120"):
            csr, want = case(gpu, oracle, shape)
            for k in (65, 1000):
                gpu.set_option("TC_CORE", k)
                check(gpu, csr, want, k, shards=(3,))
    finally:
        gpu.reset_options()


def test_core_on_a_sharded_upload(gpu, oracle):
    """Every rank of a sharded upload builds the whole matrix and counts every third block of it."""
    csr, want = case(gpu, oracle, "kron13_40")
    gpu.set_option("TC_CORE", 1000)
    try:
        total = units = 0
        for p in range(3):
            g = gpu.DeviceGraph.from_csr(csr, shard=(p, 3))
            t, st = g.tc_partial(p, 3, stats=True)
            assert g.tc_stream_breakdown()["core_k"] == 1000
            total += t
            units += st["units"]
            g.free()
        assert total == want and units == csr.num_edges
    finally:
        gpu.reset_options()


def test_core_scale_18_passes_default_and_off(gpu):
    """Kronecker scale 18 against its golden count: the default, GMSX_TC_CORE = 0, the rule's own K (-1: 0 or a multiple of 1 024), and a forced
    core under a container budget that needs several passes (the core runs in the first pass only)."""
    rec = GRAPHS["kronecker-18-16-relabel"]
    csr = host_graph(gpu, rec["generator"], rec["scale"], rec["degree"], rec["relabel"])
    try:
        for core in (None, 0, -1):
            if core is not None:
                gpu.set_option("TC_CORE", core)
            g = gpu.DeviceGraph.from_csr(csr)
            t, st = g.tc_total(stats=True)
            k = g.tc_stream_breakdown()["core_k"]
            print(f"TC_CORE={core}: core_k={k} kernel_ms={st['kernel_ms']:.3f}")
            assert t == rec["triangles"] and st["units"] == rec["m"]
            assert k % 1024 == 0 and (core != 0 or k == 0)
            g.free()
        gpu.set_option("TC_CORE", 1000)
        gpu.set_option("TC_MEM_LIMIT_MB", "64")
        g = gpu.DeviceGraph.from_csr(csr)
        t, st = g.tc_total(stats=True)
        assert g.tc_passes >= 2
        assert t == rec["triangles"] and st["units"] == rec["m"]
        parts = [g.tc_partial(p, 3, stats=True) for p in range(3)]
        assert sum(p[0] for p in parts) == rec["triangles"] and sum(p[1]["units"] for p in parts) == rec["m"]
        assert g.tc_total() == rec["triangles"]
        g.free()
    finally:
        gpu.reset_options()
