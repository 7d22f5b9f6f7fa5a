// The row classes of the library, stated once: how a pass over CSR rows gives every row the lanes its length deserves.  Connected components
// (components.hip), biconnected components (bicc.hip), the Borůvka rounds (msf.hip) and the greedy matching rounds (matching.hip) schedule
// through it; what an arc MEANS stays in their files.
//
// THE CLASSES.  Class 0: a lane per row, rows of fewer than short_row = min(kShortRow, wave_row) entries; class 1: a kGroup-lane group, rows
// below wave_row; class 2: a wave, rows below wg_row; class 3: the 256 threads of a workgroup from there on — no lane walks a long row alone
// (a hub of 10^5 to 10^6 entries is not one wave's job).  wave_row and wg_row are options of each algorithm (row_bounds) and first guesses,
// not tuned values.  A class above 0 is a vertex list that k_row_classify fills once per call; the order inside a list is the arrival order
// of atomics and reaches no output.
// THREE SHAPES OF USE.
//   whole-graph passes (components, bicc): three lists in one buffer; class 0 is taken straight from the vertex range 0 .. n - 1 by its
//       degree.  launch_rows runs k_rows<Op, WIDTH> once per class: Op::row<kLanes>(v, j0, j1, lane, width) is called by all WIDTH lanes of a
//       non-empty row (kLanes of them share a wave) and returns the arcs this lane looked at; Op::begin() by every thread before its first
//       row, Op::finish() after its last, both converged.
//   two-width whole-graph passes (msf, matching, bicc, sssp): no list at all.  launch_rows_two_width runs the same k_rows twice over the
//       vertex range: a kGroup-lane group per row of at most kLongRow entries, EMPTY ROWS INCLUDED (an Op with nothing to do there falls
//       through its own loop), and, only where the graph has one, a wave per longer row.  Both widths fit a wave (kLanes == WIDTH), so a
//       row's lanes may ballot (RowGroup<kLanes>) and keep its CSR order, or fold one result per row; the Op is the kernel's by-value
//       argument: begin() sets its per-thread sums and does every read that belongs before the row loop, finish() folds and adds them.
//   live-list rounds (msf, matching): four lists in each of two buffers, rows without an arc in none; a round reads buffer cur and may append
//       to the other.  launch_live_rows runs k_live_rows<Op, WIDTH> over the non-empty classes: a wave (WIDTH = 256: the workgroup) takes
//       its rows together and stays converged, so Op::row<WIDTH>(v, active, lane), called by every thread whether its row exists or not, may
//       use ballots, wave folds and — WIDTH = 256 — barriers.  It returns the arcs this lane looked at.
// Every append is bounds-checked and raises the caller's flag word; every count read on the device is clamped to its capacity before it
// bounds a loop (RowLists::rows), and live_count checks the host's mirror of it.
#pragma once
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // wave_append, kGroup
#include "wave_ops.hpp"

#include <algorithm>
#include <climits>

namespace gmsx {
namespace {

constexpr int kShortRow = 16;                                         // rows below this: one lane
constexpr long long kWaveRowDefault = 256, kWgRowDefault = 4096;      // first guesses (gmsx.h, OPTIONS)
constexpr int kRowsPerCu[4] = {16, 32, 32, 8};                        // workgroups per compute unit a live-list class is launched with, at most

// the shortest row of class 1, 2, 3
struct RowBounds {
    int64_t short_row, wave_row, wg_row;
};

// an algorithm's …_WAVE_ROW and …_WG_ROW options (test hooks), clamped: 1 <= wave_row <= wg_row <= INT_MAX
inline RowBounds row_bounds(const char *wave_name, const char *wg_name) {
    const int64_t wave_row = std::max<long long>(1, std::min<long long>(opt_int(wave_name, kWaveRowDefault), INT_MAX));
    const int64_t wg_row = std::max<long long>(wave_row, std::min<long long>(opt_int(wg_name, kWgRowDefault), INT_MAX));
    return {std::min<int64_t>(kShortRow, wave_row), wave_row, wg_row};
}

// THE GRIDS: workgroups of 256 threads for `rows` rows of `width` lanes each, at most per_cu of them per compute unit.  In use: a lane per
// row and 16, a kGroup-lane group and 32, a wave and 8 (whole-graph passes); kRowsPerCu (live lists).
inline unsigned row_grid(int64_t rows, int width, int cus, int per_cu) {
    return unsigned(std::min<int64_t>((rows * width + 255) / 256, int64_t(cus) * per_cu));
}

// the lists: list b of buffer i is buf[i] + base[b], at most cap[b] entries; count[b] (four device words per buffer, in the caller's control
// block) says how many it holds.  Without a class-0 list cap[0] is 0.
struct RowLists {
    int32_t *buf[2];
    int64_t base[4], cap[4];
    __device__ __forceinline__ int32_t *list(int i, int b) const { return buf[i] + base[b]; }
    // entries of list b under its count word, never more than were allocated
    __device__ __forceinline__ int64_t rows(const int32_t *count, int b) const { return min(int64_t(count[b]), cap[b]); }
};

// … and their owner
struct RowListStore {
    DevBuf b0, b1;
    RowLists l;
    // THE CAPACITY RULE: rows of at least `bound` entries number at most min(n, nnz / bound + 1).  two_buffers = false: both names mean b0.
    int alloc(int64_t n, int64_t nnz, const RowBounds &r, bool lane_list, bool two_buffers) {
        const int64_t bound[4] = {1, r.short_row, r.wave_row, r.wg_row};
        int64_t total = 0;
        for (int b = 0; b < 4; ++b) {
            l.base[b] = total;
            l.cap[b] = b > 0 || lane_list ? std::min<int64_t>(n, nnz / bound[b] + 1) : 0;
            total += l.cap[b];
        }
        if (int rc = dalloc<int32_t>(b0, total)) return rc;
        if (two_buffers)
            if (int rc = dalloc<int32_t>(b1, total)) return rc;
        l.buf[0] = b0.as<int32_t>();
        l.buf[1] = two_buffers ? b1.as<int32_t>() : l.buf[0];
        return GMSX_OK;
    }
};

// every vertex with an arc into the list of its class in buffer 0 (whole waves stay converged for the ballots); kLaneList = false: class 0
// has no list.  The last guard matters when wg_row is clamped to 1.
template <bool kLaneList>
__global__ __launch_bounds__(256) void k_row_classify(int64_t n, const int64_t *__restrict__ off, RowBounds r, RowLists l, int32_t *__restrict__ count,
                                                      int32_t *__restrict__ error) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        const int64_t d = v < n ? off[v + 1] - off[v] : 0;
        if (kLaneList) wave_append(d >= 1 && d < r.short_row, int32_t(v), l.list(0, 0), &count[0], l.cap[0], error);
        wave_append(d >= r.short_row && d < r.wave_row, int32_t(v), l.list(0, 1), &count[1], l.cap[1], error);
        wave_append(d >= r.wave_row && d < r.wg_row, int32_t(v), l.list(0, 2), &count[2], l.cap[2], error);
        wave_append(d >= r.wg_row && d >= 1, int32_t(v), l.list(0, 3), &count[3], l.cap[3], error);
    }
}
template <bool kLaneList>
void classify_rows(const gmsx_graph *g, const RowBounds &r, const RowLists &l, int32_t *count, int32_t *error, int cus, hipStream_t s, int *launches) {
    hipLaunchKernelGGL(k_row_classify<kLaneList>, dim3(row_grid(g->n, 1, cus, 16)), dim3(256), 0, s, g->n, g->off, r, l, count, error);
    ++*launches;
}

// A WHOLE-GRAPH ROW PASS: WIDTH lanes per row of dmin <= entries < dmax.  list == nullptr: the rows are the vertices 0 .. n - 1; else
// list[0 .. *count), clamped to list_cap.  The arcs looked at are added to *examined.
template <class Op, int WIDTH>
__global__ __launch_bounds__(256) void k_rows(Op op, int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ list,
                                              const int32_t *__restrict__ count, int64_t list_cap, int64_t dmin, int64_t dmax,
                                              unsigned long long *__restrict__ examined_all) {
    constexpr int kLanes = WIDTH > 64 ? 64 : WIDTH;
    const int lane = threadIdx.x & (WIDTH - 1);
    const int64_t row0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / WIDTH;
    const int64_t rows_step = (int64_t(gridDim.x) * blockDim.x) / WIDTH;
    const int64_t rows = list ? min(int64_t(*count), list_cap) : n;
    unsigned long long examined = 0;
    op.begin();
    for (int64_t i = row0; i < rows; i += rows_step) {
        const int32_t v = list ? list[i] : int32_t(i);
        const int64_t j0 = off[v], j1 = off[v + 1];
        if (j1 - j0 >= dmax || j1 - j0 < dmin) continue;
        examined += op.template row<kLanes>(v, j0, j1, lane, WIDTH);
    }
    op.finish();
    examined = wave_sum(examined);
    if ((threadIdx.x & 63) == 0 && examined) atomicAdd(examined_all, examined);
}
// one pass over every row: class 0 over all vertices, the three lists (of buffer 0, counted by count[1 .. 3]) above it
template <class Op>
void launch_rows(const Op &op, const gmsx_graph *g, const RowBounds &r, const RowLists &l, const int32_t *count, unsigned long long *examined, int cus,
                 hipStream_t s, int *launches) {
    const int64_t n = g->n;
    const unsigned lanes = row_grid(n, 1, cus, 16), grid = unsigned(cus) * 8;
    const int64_t one = 1, all = INT64_MAX;
    hipLaunchKernelGGL((k_rows<Op, 1>), dim3(lanes), dim3(256), 0, s, op, n, g->off, (const int32_t *)nullptr, count, int64_t(0), one, r.short_row, examined);
    hipLaunchKernelGGL((k_rows<Op, kGroup>), dim3(grid), dim3(256), 0, s, op, n, g->off, l.buf[0] + l.base[1], count + 1, l.cap[1], one, all, examined);
    hipLaunchKernelGGL((k_rows<Op, 64>), dim3(grid), dim3(256), 0, s, op, n, g->off, l.buf[0] + l.base[2], count + 2, l.cap[2], one, all, examined);
    hipLaunchKernelGGL((k_rows<Op, 256>), dim3(grid), dim3(256), 0, s, op, n, g->off, l.buf[0] + l.base[3], count + 3, l.cap[3], one, all, examined);
    *launches += 4;
}
// THE TWO-WIDTH PLAN over the same kernel, no lists: a kGroup-lane group for every vertex with at most kLongRow entries, then — only where
// the graph has such a row — a wave for every longer one.  An Op that counts no arcs returns 0 from row and may leave examined null.
template <class Op>
void launch_rows_two_width(const Op &op, const gmsx_graph *g, unsigned long long *examined, int cus, hipStream_t s, int *launches) {
    const int64_t n = g->n, wide = int64_t(kLongRow) + 1;
    hipLaunchKernelGGL((k_rows<Op, kGroup>), dim3(row_grid(n, kGroup, cus, 32)), dim3(256), 0, s, op, n, g->off, (const int32_t *)nullptr,
                       (const int32_t *)nullptr, int64_t(0), int64_t(0), wide, examined);
    if (g->max_deg > kLongRow)
        hipLaunchKernelGGL((k_rows<Op, 64>), dim3(row_grid(n, 64, cus, 8)), dim3(256), 0, s, op, n, g->off, (const int32_t *)nullptr,
                           (const int32_t *)nullptr, int64_t(0), wide, int64_t(INT64_MAX), examined);
    *launches += g->max_deg > kLongRow ? 2 : 1;
}

// A LIVE-LIST ROW PASS: WIDTH lanes per row of list[0 .. *count), clamped to list_cap.  A wave takes 64 / WIDTH consecutive rows at a time and
// stays together (its appends are one atomic, and a next list keeps runs of the order of this one); WIDTH = 256: a row per workgroup, whose
// barriers the loop passes.
template <class Op, int WIDTH>
__global__ __launch_bounds__(256) void k_live_rows(Op op, const int32_t *__restrict__ list, const int32_t *__restrict__ count, int64_t list_cap,
                                                   unsigned long long *__restrict__ examined_all) {
    constexpr int kUnit = WIDTH > 64 ? WIDTH : 64;  // threads that go through the row loop together: the wave, or the workgroup
    const int lane = threadIdx.x & (WIDTH - 1);
    const int64_t first = ((int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kUnit) * (kUnit / WIDTH);
    const int64_t rows_step = (int64_t(gridDim.x) * blockDim.x) / WIDTH;
    const int64_t rows = min(int64_t(*count), list_cap);
    unsigned long long examined = 0;
    for (int64_t base = first; base < rows; base += rows_step) {
        const int64_t i = base + (threadIdx.x & (kUnit - 1)) / WIDTH;
        const bool active = i < rows;
        examined += op.template row<WIDTH>(active ? list[i] : 0, active, lane);
    }
    examined = wave_sum(examined);
    if ((threadIdx.x & 63) == 0 && examined) atomicAdd(examined_all, examined);
}
// … over list b of buffer cur, `rows` entries by the host's mirror of its count: no launch for an empty class, at most kRowsPerCu[b] workgroups
// per compute unit
template <int WIDTH, class Op>
void launch_live_class(const Op &op, const RowLists &l, int cur, int b, const int32_t *count, int64_t rows, unsigned long long *examined, int cus,
                       hipStream_t s, int *launches) {
    if (rows <= 0) return;
    const unsigned grid = row_grid(rows, WIDTH, cus, kRowsPerCu[b]);
    hipLaunchKernelGGL((k_live_rows<Op, WIDTH>), dim3(grid), dim3(256), 0, s, op, l.buf[cur] + l.base[b], count + b, l.cap[b], examined);
    ++*launches;
}
// … and over the four lists of buffer cur; op_for(b) is the Op of class b
template <class OpFor>
void launch_live_rows(const OpFor &op_for, const RowLists &l, int cur, const int32_t *count, const int32_t *rows, unsigned long long *examined, int cus,
                      hipStream_t s, int *launches) {
    launch_live_class<1>(op_for(0), l, cur, 0, count, rows[0], examined, cus, s, launches);
    launch_live_class<kGroup>(op_for(1), l, cur, 1, count, rows[1], examined, cus, s, launches);
    launch_live_class<64>(op_for(2), l, cur, 2, count, rows[2], examined, cus, s, launches);
    launch_live_class<256>(op_for(3), l, cur, 3, count, rows[3], examined, cus, s, launches);
}

// the host's mirror of one buffer's counts: their sum, or -1 where one is out of its range (GMSX_ERR_KERNEL)
inline int64_t live_count(const int32_t *count, const RowLists &l) {
    int64_t live = 0;
    for (int b = 0; b < 4; ++b) {
        if (count[b] < 0 || int64_t(count[b]) > l.cap[b]) return -1;
        live += count[b];
    }
    return live;
}

}  // namespace
}  // namespace gmsx
