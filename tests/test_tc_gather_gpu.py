"""GPU: gathered rows of the triangle count (GMSX_TC_GATHER = R; device_graph.hpp, host/tc_gather_plan.hpp) — the units behind a stream row's
last 128-byte line boundary move to a densely packed row of the receiving pivot — against the CPU oracle, for R = 0, 1, 3, 7: the count, the
units, the byte fields of the breakdown, the shard sums; and what the diagnostics say about lines (row_line_bytes, partial_line_entries,
gathered_rows).  Two generated graphs and a hand-made one whose heavy receivers get member rows of chosen lengths."""
import numpy as np
import pytest

from conftest import host_graph

pytestmark = pytest.mark.gpu
RS = (0, 1, 3, 7)
ROW_SLOTS = ("hub_rows_list", "hub_rows_bitset", "hub_rows_delta", "tail_rows_list", "tail_rows_delta")
_CASES = {}


def generated(gpu, oracle, name):
    """(csr, triangles, hub limit) of the two generated graphs, built once per session and left unchanged."""
    if name not in _CASES:
        kind, scale, deg = {"kron13_16": ("kronecker", 13, 16), "uniform12_20": ("uniform", 12, 20)}[name]
        csr = host_graph(gpu, kind, scale, deg, True)
        _CASES[name] = (csr, oracle.tc_total(csr.offsets(), csr.neighbors()), 300)
    return _CASES[name]


# ---- hand-made graph ----------------------------------------------------------------------------------------------------------------------
# Degrees descend hubs > tops > members > receivers, all distinct, so the ranking is known: the NH hubs are the hub ids (hub limit NH), the
# NW tops the first tail ids, a member's row is exactly the hubs and tops it is adjacent to, and a receiver (adjacent to members, hubs and
# tops) is a heavy pivot whose members' rows are streamed against it.
NH, NW = 480, 56
LENGTHS = [7, 8, 9, 15, 16, 17, 23, 24, 25, 33]


def member_specs():
    """name -> (hub ids, top ids) of every member."""
    m = {}
    for L in LENGTHS:
        m[f"l{L}"] = (8 * L, 0)      # a list row of L units (TC_DELTA=0); ceil(8 L / 14) delta units under TC_DELTA=2
        m[f"d{L}"] = (14 * L, 0)     # a byte-delta row of L units under TC_DELTA=2 (consecutive ids: 14 per unit)
    for k in range(1, 10):
        m[f"t{k}"] = (0, 4 * k)      # a tail list row of k units
        m[f"td{k}"] = (0, 6 * k)     # a tail delta row of k units under TC_TAIL_DELTA=2 (rows of >= 8 ids)
    for j in range(9):
        m[f"f{j}"] = (120, 0)        # 15 units: 7 behind the last line boundary
    for j in range(520):
        m[f"s{j}"] = (8 + j % 41, j % 5)  # small rows of 1 … 6 hub units (packed, so they straddle lines) and 0 … 1 tail units
    return m


def receiver_specs():
    """name -> (hubs it is adjacent to, tops, members).  A receiver adjacent to all hubs streams every member's row itself (its own hub row is
    the longer one); `rev` has a short hub row, so its heavy members take the edge and stream ITS rows, cut at their ids (reverse entries)."""
    every = [f"l{L}" for L in LENGTHS] + [f"d{L}" for L in LENGTHS] + [f"t{k}" for k in range(1, 10)] + [f"td{k}" for k in range(1, 10)]
    return {
        "all": (NH, NW, every),
        "all2": (NH - 7, NW - 3, every[::-1]),
        "rev": (70, 5, every),
        "zero": (NH, 0, ["l8", "l16", "l24"]),                                 # list rows of whole lines only: nothing to gather
        "g64": (NH, 0, [f"f{j}" for j in range(9)] + ["l9", "l8"]),           # 9 x 7 + 1 = 64 units gathered at R = 7
        "g65": (NH, 0, [f"f{j}" for j in range(9)] + ["l9", "l17", "l16"]),   # … and one more: a second chunk of one unit
        "big": (100, 9, [f"s{j}" for j in range(520)]),                       # more than 512 entries: two work items
    }


def handmade(gpu, oracle, only=None):
    """(csr, triangles, hub limit): the graph of all receivers, or of the one receiver `only`."""
    key = ("handmade", only)
    if key not in _CASES:
        members, receivers = member_specs(), receiver_specs()
        if only:
            receivers = {only: receivers[only]}
        used = sorted({m for _, _, ms in receivers.values() for m in ms}, key=lambda s: (s[0], len(s), s))
        hubs, tops = np.arange(NH), NH + np.arange(NW)
        nxt = NH + NW
        src, dst, target, ids = [], [], {}, {}
        for i in range(NH):
            target[i] = 1700 + i
        for j in range(NW):
            target[NH + j] = 1600 + j
        for k, name in enumerate(used):
            ids[name] = nxt
            target[nxt] = 1000 + k
            nh, nw = members[name]
            lo = (7 * k) % (NH - nh + 1) if name[0] in "fs" else 0  # consecutive hub ids (delta units stay full); shifted for the small and filler rows
            for x in hubs[lo:lo + nh]:
                src.append(nxt), dst.append(int(x))
            for x in tops[:nw] if k % 2 else tops[NW - nw:]:
                src.append(nxt), dst.append(int(x))
            nxt += 1
        for k, (name, (nh, nw, ms)) in enumerate(receivers.items()):
            target[nxt] = 700 + k
            for x in hubs[:nh]:
                src.append(nxt), dst.append(int(x))
            for x in tops[:nw]:
                src.append(nxt), dst.append(int(x))
            for m in ms:
                src.append(nxt), dst.append(ids[m])
            nxt += 1
        deg = np.bincount(np.array(src + dst), minlength=nxt)
        pad_src, pad_dst = [], []
        for x, want_deg in target.items():
            k = want_deg - int(deg[x])
            assert k >= 0, (x, want_deg, int(deg[x]))
            pad_src.append(np.full(k, x, dtype=np.int32))
            pad_dst.append(np.arange(nxt, nxt + k, dtype=np.int32))
            nxt += k
        csr = gpu.HostCSR.from_edges(np.concatenate([np.array(src, dtype=np.int32)] + pad_src), np.concatenate([np.array(dst, dtype=np.int32)] + pad_dst))
        _CASES[key] = (csr, oracle.tc_total(csr.offsets(), csr.neighbors()), NH)
    return _CASES[key]


def case(gpu, oracle, name):
    return handmade(gpu, oracle) if name == "handmade" else generated(gpu, oracle, name)


def run(gpu, csr, hub_limit, shard=None, hist=False):
    """(count, stats, breakdown[, row histogram]) of one upload under the options in force."""
    kw = {"shard": shard} if shard else {}
    g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8), **kw)
    try:
        t, st = g.tc_partial(shard[0], shard[1], stats=True) if shard else g.tc_total(stats=True)
        out = (t, st, g.tc_stream_breakdown())
        return out + (g.tc_row_histogram()[0],) if hist else out
    finally:
        g.free()


def sweep(gpu, csr, want, hub_limit, rs=RS, label="", gathers=True):
    """One upload per R: the oracle's count, units = m, the byte fields add up; then the relations between the R."""
    seen = {}
    for r in rs:
        gpu.set_option("TC_GATHER", r)
        t, st, b = run(gpu, csr, hub_limit)
        print(f"{label} R={r}: total={t} want={want} units={st['units']} stream_bytes={st['stream_bytes']} entries={b['count_entries']} items={b['count_work_items']} "
              f"inline_entries={b['count_inline_entries']} gathered={b['gathered_rows']} row_line_bytes={b['row_line_bytes']} partial={b['partial_line_entries']}")
        assert t == want
        assert st["units"] == csr.num_edges
        assert sum(b[x] for x in gpu.DeviceGraph.BREAKDOWN_BYTES) == st["stream_bytes"]
        assert b["entries"] == 6 * b["count_entries"] and b["gathered_rows"] % 16 == 0
        assert b["gather_limit"] == r  # an explicit R is taken as given
        assert b["row_line_bytes"] >= sum(b[x] for x in ROW_SLOTS)  # every unit lies in a line
        seen[r] = (st, b)
    if 0 in seen:
        st0, b0 = seen[0]
        assert b0["gathered_rows"] == 0
        for r, (st, b) in seen.items():
            # units only move: the row bytes as a whole stay (list units stay list units, delta units delta units); bitset rows are untouched
            assert b["hub_rows_bitset"] == b0["hub_rows_bitset"]
            for x in ROW_SLOTS:
                assert b[x] == b0[x], (r, x)
            assert b["gathered_rows"] <= sum(b[x] for x in ROW_SLOTS)
            # stream_bytes: no region rounding (a gathered row's last chunk names its units, not its lines), 6 bytes per entry added (a chunk per
            # 64 gathered units and a last one per gathered row: at most 2 rows per list, a list with entries has a work item) or dropped (each
            # dropped entry moved at least one unit); the pivots' containers are read once per work item
            delta = (st["stream_bytes"] - b["pivot_containers"]) - (st0["stream_bytes"] - b0["pivot_containers"])
            assert delta == 6 * (b["count_entries"] - b0["count_entries"])
            assert -6 * (b["gathered_rows"] // 16) <= delta <= 6 * (b["gathered_rows"] // (16 * 64) + 2 * b["count_work_items"])
        if 7 in seen:
            b7 = seen[7][1]
            assert b7["row_line_bytes"] <= b0["row_line_bytes"]
            if gathers:
                assert b7["gathered_rows"] > 0
            # R = 7: every list / delta row that ends inside a line has lost its remainder (a row of >= 8 units, a cut row and the second slot of a
            # hybrid row start on line boundaries or are small; a small row moves whole or up to the boundary it straddles).  What is left, per
            # list (a receiver's hub list or tail list): the last chunk of its one inline row — with gathered rows the inline region and every
            # receiver's inline row start on line boundaries and a full chunk is 64 units = 8 lines, so no other chunk ends inside a line — and the
            # last chunk of its gathered rows, at most two (list units, delta units).  A list with entries has at least one work item: 3 per item.
            assert b7["partial_line_entries"] <= 3 * b7["count_work_items"]
    return seen


@pytest.mark.parametrize("name", ["kron13_16", "uniform12_20", "handmade"])
def test_counts_and_lines(gpu, oracle, name):
    csr, want, hub_limit = case(gpu, oracle, name)
    assert want > 0
    try:
        if name == "handmade":
            gpu.set_option("INLINE_LIMIT", "0")
        sweep(gpu, csr, want, hub_limit, label=name, gathers=name != "uniform12_20")  # (uniform12_20 has no pivot of d+ >= 64: every entry is an inline chunk)
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("name", ["kron13_16", "uniform12_20", "handmade"])
def test_row_line_bytes_drop(gpu, oracle, name):
    """row_line_bytes(R = 7) < row_line_bytes(R = 0) on every graph.  uniform12_20 has no pivot of d+ >= 64 and therefore no forward or
    reverse entry, nothing to gather: all its entries are chunks of inline rows, and what drops there is the lines of the inline rows, which
    start on line boundaries when rows are gathered."""
    csr, want, hub_limit = case(gpu, oracle, name)
    try:
        if name == "handmade":
            gpu.set_option("INLINE_LIMIT", "0")
        lines = {}
        for r in (0, 7):
            gpu.set_option("TC_GATHER", r)
            t, _, b = run(gpu, csr, hub_limit)
            assert t == want
            lines[r] = b["row_line_bytes"]
        print(f"{name}: row_line_bytes {lines[0]} -> {lines[7]}")
        assert lines[7] < lines[0]
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("delta", [0, 2])
def test_handmade_forms(gpu, oracle, delta):
    """The member rows forced out of the delta forms (the list rows have the chosen lengths) and into them (the delta rows have)."""
    csr, want, hub_limit = handmade(gpu, oracle)
    try:
        gpu.set_option("INLINE_LIMIT", "0")
        gpu.set_option("TC_DELTA", delta)
        gpu.set_option("TC_TAIL_DELTA", delta)
        gpu.set_option("TC_GATHER", 0)
        hist = run(gpu, csr, hub_limit, hist=True)[3]  # [hub list, bitset, delta, tail list, tail delta][bin][rows, units]; bin = units - 1 up to 16, then 17-32, 33-64
        hub, tail = hist[2 if delta else 0], hist[4 if delta else 3]
        for L in LENGTHS:
            assert hub[L - 1 if L <= 16 else 16 if L <= 32 else 17][0] >= 2, L  # at least the receivers `all` and `all2` stream it
        for k in range(1 if not delta else 2, 10):
            assert tail[k - 1][0] >= 2, k
        seen = sweep(gpu, csr, want, hub_limit, label=f"handmade delta={delta}")
        assert seen[7][1]["hub_rows_delta" if delta else "hub_rows_list"] > 0 and seen[7][1]["tail_rows_delta" if delta else "tail_rows_list"] > 0
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("only,units", [("zero", 0), ("g64", 64), ("g65", 65)])
def test_handmade_gathered_totals(gpu, oracle, only, units):
    """One receiver alone, list rows only: its gathered row holds exactly the remainders of its members' rows — none, one full chunk, one chunk
    and a unit — and takes one entry per chunk, while every member row that lost a remainder keeps its entry."""
    csr, want, hub_limit = handmade(gpu, oracle, only)
    try:
        gpu.set_option("INLINE_LIMIT", "0")
        gpu.set_option("TC_DELTA", 0)
        gpu.set_option("TC_TAIL_DELTA", 0)
        seen = sweep(gpu, csr, want, hub_limit, rs=(0, 7), label=only, gathers=units > 0)
        b0, b7 = seen[0][1], seen[7][1]
        assert b7["gathered_rows"] == 16 * units
        assert b7["count_entries"] - b0["count_entries"] == (units + 63) // 64
        # list rows only: the one gathered row ends inside a line unless it is whole lines; every list has at most one inline row, whose last
        # chunk may end inside a line, and at least one work item
        assert b7["partial_line_entries"] <= (1 if units % 8 else 0) + b7["count_work_items"]
    finally:
        gpu.reset_options()


def test_handmade_covers_long_lists_and_reverse_entries(gpu, oracle):
    """The two cases of the hand-made graph that nothing else would miss if the ranking or the inline rules changed, each on the graph of
    its receiver alone, without gathered rows and with list rows only.  `big`: its hub list has more than 512 entries, i.e. two work items.
    Every entry that is no inline chunk is a forward entry of `big` (no member of it is heavy, so none takes an edge back): one per member
    for the hub rows, one per member with tops for the tail rows.  `rev`: its heavy members whose hub row is longer than its own 9 units take
    the edge and stream ITS hub row — whole, they are tail members — so rows of exactly 9 list units appear, many more than the one member
    (`l9`) that owns such a row."""
    try:
        gpu.set_option("INLINE_LIMIT", "0")
        gpu.set_option("TC_DELTA", 0)
        gpu.set_option("TC_TAIL_DELTA", 0)
        gpu.set_option("TC_GATHER", 0)
        members, receivers = member_specs(), receiver_specs()
        csr, want, hub_limit = handmade(gpu, oracle, "big")
        t, st, b = run(gpu, csr, hub_limit)
        with_tail = sum(1 for m in receivers["big"][2] if members[m][1] > 0)
        hub_entries = b["count_entries"] - b["count_inline_entries"] - with_tail  # at least: the tail list has at most one entry per member with tops
        print(f"big: entries={b['count_entries']} inline={b['count_inline_entries']} members with a tail row={with_tail} items={b['count_work_items']}")
        assert t == want and st["units"] == csr.num_edges
        assert hub_entries > 512 and b["count_work_items"] >= 3  # two hub items and a tail item
        csr, want, hub_limit = handmade(gpu, oracle, "rev")
        t, st, b, hist = run(gpu, csr, hub_limit, hist=True)
        longer = sum(1 for m in receivers["rev"][2] if members[m][1] == 0 and (members[m][0] + 7) // 8 > 9)  # heavy, no tail part, more than 9 units
        print(f"rev: hub list rows of 9 units={hist[0][8][0]} members with a longer hub row={longer}")
        assert t == want and st["units"] == csr.num_edges
        assert longer >= 10 and hist[0][8][0] >= 3
        gpu.reset_options()  # no option: the default R, which nothing here is too large for
        assert run(gpu, csr, hub_limit)[2]["gather_limit"] == 7
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("name", ["kron13_16", "uniform12_20", "handmade"])
def test_shards(gpu, oracle, name, r):
    """The shard sums of a full upload (2, 3, 5, 8 parts) and of sharded uploads (2, 3) equal the whole."""
    csr, want, hub_limit = case(gpu, oracle, name)
    try:
        if name == "handmade":
            gpu.set_option("INLINE_LIMIT", "0")
        gpu.set_option("TC_GATHER", r)
        g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8))
        try:
            t, st = g.tc_total(stats=True)
            assert t == want and st["units"] == csr.num_edges
            for nparts in (2, 3, 5, 8):
                parts = [g.tc_partial(p, nparts, stats=True) for p in range(nparts)]
                assert sum(p[0] for p in parts) == want, nparts
                assert sum(p[1]["units"] for p in parts) == csr.num_edges, nparts
                assert sum(p[1]["stream_bytes"] for p in parts) == st["stream_bytes"], nparts
        finally:
            g.free()
        for nparts in (2, 3):
            got = [run(gpu, csr, hub_limit, shard=(p, nparts)) for p in range(nparts)]
            assert sum(x[0] for x in got) == want and sum(x[1]["units"] for x in got) == csr.num_edges, nparts
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("knobs", [{"TC_PERSIST": "0"}, {"TC_HOT_WINDOWS": "2", "TC_HOT_KB": "1", "TC_HOT_MIN": "1"}, {"TC_HOT_WINDOWS": "2"}, {"TC_CORE": "128"},
                                   {"TC_HYBRID": "2"}, {"TC_HYBRID": "2", "TC_PERSIST": "0"}])
@pytest.mark.parametrize("name", ["kron13_16", "handmade"])
def test_knobs_beside_it(gpu, oracle, name, knobs):
    """The one-workgroup-per-item kernels (their one-step classes need the class of the shrunk length), hot windows (windows of 1 KB: the
    gathered regions lie behind them; the default 2 MB: the whole pool lies inside window 0), a forced core, hybrid rows."""
    csr, want, hub_limit = case(gpu, oracle, name)
    try:
        for k, v in knobs.items():
            gpu.set_option(k, v)
        seen = sweep(gpu, csr, want, hub_limit, label=f"{name} {knobs}")
        if "TC_CORE" in knobs:
            assert seen[7][1]["core_k"] == 128
    finally:
        gpu.reset_options()


@pytest.mark.parametrize("r", RS)
def test_passes(gpu, oracle, r):
    """A container budget (GMSX_TC_MEM_LIMIT_MB) of half of what kron13_16 needs: the build — pool growth included — is accounted, falls back to
    passes, and the count stays."""
    csr, want, hub_limit = generated(gpu, oracle, "kron13_16")
    try:
        gpu.set_option("TC_GATHER", r)
        g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8))
        base = g.device_bytes
        assert g.tc_total() == want and g.tc_passes == 1
        containers = g.device_bytes - base
        g.free()
        limit = max(1, (containers // 2) >> 20)
        print(f"R={r}: containers {containers} bytes, budget {limit} MB")
        assert containers > (limit << 20)
        gpu.set_option("TC_MEM_LIMIT_MB", limit)
        g = gpu.DeviceGraph.from_csr(csr, flags=gpu.UPLOAD_DEFAULT | (hub_limit << 8))
        try:
            t, st = g.tc_total(stats=True)
            assert t == want and st["units"] == csr.num_edges and g.tc_passes >= 2
            assert sum(g.tc_partial(p, 3) for p in range(3)) == want
        finally:
            g.free()
    finally:
        gpu.reset_options()
