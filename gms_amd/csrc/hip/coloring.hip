// Jones–Plassmann graph colouring under a caller-given priority, and the verifier of a colouring, on gfx950:
//   gmsx_coloring_jp      GMS::Coloring::JonesV3::graph_coloring_jones (non_set_based/coloring/coloring_jones_v3.h:38-68): u is a predecessor of v
//                         iff order[u] > order[v] (:52); a vertex takes the smallest colour >= 1 none of its predecessors holds (:12-21).  That is
//                         the greedy colouring of the vertices taken by descending order[], whatever the thread count; with order[v] = n-1-v it
//                         is graph_coloring_naive_sequential (coloring_sequential.h:17-42).
//   gmsx_coloring_verify  GCVerifierMaxColor / GCVerifierDeltaPlusOne and uniqueColorsCount (coloring_common.h:102-157, 205-209) as integers
//
// THE ROUNDS.  cnt[v] = predecessors of v not coloured yet (k_oq_later of order_rank.hpp: the neighbours of higher rank).  The frontier of a
// round is cnt == 0, and it is an INDEPENDENT SET: of two adjacent vertices one is the other's predecessor.  So while v is in the frontier
// every neighbour's colour is stable — a predecessor holds a colour >= 1, a successor holds 0 — and ONE pass over v's row does both jobs:
// a non-zero colour is marked in v's forbidden bitmap, a zero one is a successor whose counter drops, and the ONE decrement that returns 1
// queues it for the next round.  Then v takes the first free colour in 1..p+1 (p = its predecessor count; a colour above p+1 cannot block
// it and is dropped).  No rank[] gather in the rounds; every CSR entry is touched once per endpoint over the whole run.  Which vertices a
// round colours, and with what, is a fact about the integers; the order inside the queues and the slab offsets are not, and reach no output.
//
// COST SHAPE.  That of the peel in core.hip — hundreds to thousands of rounds, most of them tiny — and its solution: the rounds are those of the
// frontier engine (frontier_rounds.hpp: the row binning, the one-workgroup tail under COLOR_WG_FRONTIER and its hand-back rule); this file
// supplies the per-vertex work (ColorJp), the setup and the final checks.  A short row keeps its bitmap in the group's LDS words; a long row is
// parked with a piece of a zeroed global slab (its note) and takes its colour at the round boundary, so no graph is refused for a wide
// neighbourhood.
#include "coloring_device.hpp"
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"
#include "order_rank.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

constexpr int kBitWords = kLongRow / 32 + 1;  // bitmap of a short row: colours 1..p+1, p <= kLongRow

// control block of one run: the engine's, plus what the colours need
struct ColorCtrl : FrontierCtrl {  // (done = vertices coloured in finished rounds; error: also the slab or a first-free search hit its bound)
    int32_t colors;                // largest colour given so far
    int32_t max_pred;              // most predecessors of any vertex
    unsigned long long slab_used;  // words of the slab handed to long rows so far (every vertex is parked at most once)
};

// the lanes of a wave run in program order: this only keeps the compiler from moving LDS accesses across the phases of a group
__device__ __forceinline__ void group_phase() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// pred[v] = cnt[v] (the counters fall, the bitmap widths stay), max_pred, and the first frontier: cnt == 0 (one wave-aggregated append per wave)
__global__ __launch_bounds__(256) void k_color_select(int64_t n, const int32_t *__restrict__ cnt, int32_t *__restrict__ pred, ColorCtrl *__restrict__ ctrl,
                                                      int32_t *__restrict__ frontier) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;  // whole waves stay converged for the ballot
    int32_t mx = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        bool take = false;
        if (v < n) {
            const int32_t p = cnt[v];
            pred[v] = p;
            mx = max(mx, p);
            take = p == 0;
        }
        wave_append(take, int32_t(v), frontier, &ctrl->count, n, &ctrl->error);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctrl->max_pred, mx);
}

// first zero bit of slab[0 .. p/32] by all threads of the workgroup (every thread must call it); 0-based, INT_MAX if none
__device__ __forceinline__ int32_t first_free_long(const uint32_t *__restrict__ slab, int32_t p, int tid, int threads) {
    __shared__ int32_t s_best;
    if (tid == 0) s_best = INT_MAX;
    __syncthreads();
    const int32_t words = p / 32 + 1;
    for (int32_t w = tid; w < words; w += threads) {
        const uint32_t free = ~load_now(&slab[w]);
        if (free) {
            atomicMin(&s_best, w * 32 + __ffs(free) - 1);
            break;  // (this thread's later words are higher)
        }
    }
    __syncthreads();
    const int32_t best = s_best;
    __syncthreads();
    return best;
}

// Jones–Plassmann as a policy of the engine: one pass over the row of frontier vertex x marks the colours of its predecessors and releases its
// successors; then x takes the first free colour
struct ColorJp {
    static constexpr int kGroupWords = kBitWords;
    static constexpr bool kNotes = true;  // a parked row's note = where its bitmap starts in the slab
    int64_t n;
    const int64_t *off;
    const int32_t *adj, *pred;
    int32_t *color, *round_of, *cnt;
    uint32_t *slab;
    unsigned long long slab_cap, *slab_used;  // (slab_used, colors: the words of the control block)
    int32_t *colors;
    int32_t top;  // largest colour this thread gave (the kernel argument is every thread's own copy)

    __device__ __forceinline__ void give(int32_t x, int32_t c, int32_t round, int32_t *error) {
        if (c == 0) *error = 1;
        store_now(&color[x], c);
        round_of[x] = round;
        top = max(top, c);
    }
    // row entry w: a colour is a predecessor's, and is marked by `mark`; 0 is a successor — its counter drops, and the decrement that brings it
    // to 0 queues it
    template <class Mark>
    __device__ __forceinline__ void visit(int32_t w, int32_t p, const NextQueue &q, Mark mark) const {
        const int32_t c = load_now(&color[w]);
        if (c != 0) {
            if (c - 1 >= 0 && c - 1 <= p) mark(c - 1);
        } else if (atomicSub(&cnt[w], 1) == 1) {
            q.push(w);
        }
    }
    // SHORT row: the forbidden bitmap in `bits` (kBitWords words of LDS, the group's own); cannot find none: at most p of the p + 1 bits are set
    __device__ __forceinline__ void short_row(int32_t x, int64_t j0, int64_t j1, int lane, int32_t round, uint32_t *bits, const NextQueue &q) {
        const int32_t p = pred[x];
        const int words = min(p / 32 + 1, kBitWords);  // bits 0..p = colours 1..p+1
        for (int w = lane; w < words; w += kGroup) bits[w] = 0;
        group_phase();
        for (int64_t j = j0 + lane; j < j1; j += kGroup)
            visit(adj[j], p, q, [&](int32_t b) {
                if ((b >> 5) < words) atomicOr(&bits[b >> 5], 1u << (b & 31));
            });
        group_phase();
        int32_t best = INT_MAX;
        for (int w = lane; w < words; w += kGroup) {
            const uint32_t free = ~bits[w];
            if (free) best = min(best, w * 32 + __ffs(free) - 1);
        }
        best = wave_min_all<kGroup>(best);
        group_phase();  // (the next vertex of this group zeroes the same words)
        if (lane == 0) give(x, best <= p ? best + 1 : 0, round, q.error);
    }
    // LONG row: its piece of the slab, pred/32 + 1 zeroed words …
    __device__ __forceinline__ void park(int32_t x, int32_t, unsigned long long *notes, int64_t pos, int32_t *error) const {
        const unsigned long long words = (unsigned long long)(pred[x] / 32 + 1);
        const unsigned long long at = atomicAdd(slab_used, words);
        if (at + words <= slab_cap) notes[pos] = at;
        else *error = 1;
    }
    // … set by idempotent ORs of many threads together …
    __device__ __forceinline__ void long_walk(int32_t x, unsigned long long note, int64_t tid, int64_t threads, const NextQueue &q) const {
        uint32_t *bits = slab + note;
        const int32_t p = pred[x];
        const int64_t j1 = off[x + 1];
        for (int64_t j = off[x] + tid; j < j1; j += threads)
            visit(adj[j], p, q, [&](int32_t b) {
                const uint32_t bit = 1u << (b & 31);
                if (!(load_now(&bits[b >> 5]) & bit)) atomicOr(&bits[b >> 5], bit);  // (a stale read costs an atomic, never the result)
            });
    }
    // … and searched when they are complete
    __device__ __forceinline__ void settle(int32_t x, unsigned long long note, int32_t round, int tid, int32_t *error) {
        const int32_t p = pred[x];
        const int32_t best = first_free_long(slab + note, p, tid, kTailThreads);
        if (tid == 0) give(x, best > p ? 0 : best + 1, round, error);
    }
    __device__ __forceinline__ void finish() const {
        if (top) atomicMax(colors, top);
    }
};

// ---- verify -------------------------------------------------------------------------------------------------------------------------

// acc[0] arcs whose endpoints hold equal colours, [1] vertices of colour < 1, [2] largest colour + 2^31, [3] largest degree, [4] set bits of `present`
constexpr int kAccArcs = 0, kAccInvalid = 1, kAccMax = 2, kAccDeg = 3, kAccDistinct = 4;

// one pass over the CSR, a 16-lane group per vertex; rows above kLongRow parked for k_cv_long.  present: one bit per colour in [0, n]
__global__ __launch_bounds__(256) void k_cv_rows(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                 const int32_t *__restrict__ color, uint32_t *__restrict__ present, int32_t *__restrict__ longs,
                                                 int64_t long_cap, int32_t *__restrict__ ctl /* [0] long rows, [1] error */,
                                                 unsigned long long *__restrict__ acc) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    unsigned long long arcs = 0, invalid = 0, mx = 0, deg = 0;
    for (int64_t v = group0; v < n; v += groups) {
        const int64_t j0 = off[v], j1 = off[v + 1];
        const int32_t c = color[v];
        if (lane == 0) {
            if (c < 1) ++invalid;
            mx = max(mx, (unsigned long long)(int64_t(c) + (1ll << 31)));
            deg = max(deg, (unsigned long long)(j1 - j0));
            if (c >= 0 && int64_t(c) <= n) {
                const uint32_t bit = 1u << (c & 31);
                if (!(present[c >> 5] & bit)) atomicOr(&present[c >> 5], bit);
            }
        }
        if (j1 - j0 > kLongRow) {
            if (lane == 0) {
                append_checked(longs, &ctl[0], long_cap, int32_t(v), &ctl[1]);
            }
            continue;
        }
        for (int64_t j = j0 + lane; j < j1; j += kGroup) arcs += color[adj[j]] == c ? 1 : 0;
    }
    arcs = wave_sum(arcs);
    invalid = wave_sum(invalid);
    mx = wave_max(mx);
    deg = wave_max(deg);
    if ((threadIdx.x & 63) == 0) {
        if (arcs) atomicAdd(&acc[kAccArcs], arcs);
        if (invalid) atomicAdd(&acc[kAccInvalid], invalid);
        if (mx) atomicMax(&acc[kAccMax], mx);
        if (deg) atomicMax(&acc[kAccDeg], deg);
    }
}
__global__ __launch_bounds__(256) void k_cv_long(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const int32_t *__restrict__ color,
                                                 const int32_t *__restrict__ longs, int64_t long_cap, const int32_t *__restrict__ ctl,
                                                 unsigned long long *__restrict__ acc) {
    const int64_t nlong = min(int64_t(ctl[0]), long_cap);
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, threads = int64_t(gridDim.x) * blockDim.x;
    unsigned long long arcs = 0;
    for (int64_t i = 0; i < nlong; ++i) {
        const int32_t v = longs[i];
        const int32_t c = color[v];
        const int64_t j1 = off[v + 1];
        for (int64_t j = off[v] + tid; j < j1; j += threads) arcs += color[adj[j]] == c ? 1 : 0;
    }
    arcs = wave_sum(arcs);
    if ((threadIdx.x & 63) == 0 && arcs) atomicAdd(&acc[kAccArcs], arcs);
}
__global__ __launch_bounds__(256) void k_cv_distinct(int64_t words, const uint32_t *__restrict__ present, unsigned long long *__restrict__ acc) {
    unsigned long long c = 0;
    for (int64_t w = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < words; w += int64_t(gridDim.x) * blockDim.x) c += __popc(present[w]);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&acc[kAccDistinct], c);
}

}  // namespace

// The colouring on the device: color and round_of stay in the two buffers (n words each), res and *launches_out are filled, and the rounds lie
// between the events ev[0] and ev[1] of the context.  gmsx_coloring_jp copies the arrays out; label propagation (communities.hip) keeps them
// where they are.  n > 0.
int coloring_jp_device(const gmsx_graph *g, const int32_t *ordering, int rank_format, DevBuf &d_color, DevBuf &d_round, gmsx_coloring_info &res,
                       int *launches_out) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const unsigned tb = unsigned((n + 255) / 256);
    DevBuf d_in, d_rank, d_seen, d_cnt, d_pred, d_slab, d_ctl, d_ctrl;
    FrontierStore store;  // (a parked row's note: where its bitmap starts in the slab)
    if (int rc = dalloc<int32_t>(d_in, n)) return rc;
    if (int rc = dalloc<int32_t>(d_cnt, n)) return rc;
    if (int rc = dalloc<int32_t>(d_pred, n)) return rc;
    if (int rc = dalloc<int32_t>(d_color, n)) return rc;
    if (int rc = dalloc<int32_t>(d_round, n)) return rc;
    if (int rc = store.alloc(n, g->nnz, true)) return rc;
    const int64_t long_cap = store.long_cap;
    // every long row is parked once in the whole run and takes pred/32 + 1 <= degree/32 + 1 words
    const unsigned long long slab_cap = (unsigned long long)(g->nnz / 32 + long_cap);
    if (int rc = dalloc<uint32_t>(d_slab, int64_t(slab_cap))) return rc;
    if (int rc = dalloc<int32_t>(d_ctl, 4)) return rc;
    if (int rc = dalloc<ColorCtrl>(d_ctrl, 1)) return rc;
    const bool own_rank = ordering && !rank_format;
    if (ordering)
        if (int rc = dalloc<int32_t>(d_seen, n)) return rc;
    if (own_rank)
        if (int rc = dalloc<int32_t>(d_rank, n)) return rc;
    ColorCtrl *ctrl = d_ctrl.as<ColorCtrl>();
    int32_t *rank = own_rank ? d_rank.as<int32_t>() : d_in.as<int32_t>();
    int32_t *cnt = d_cnt.as<int32_t>(), *pred = d_pred.as<int32_t>(), *color = d_color.as<int32_t>(), *rnd = d_round.as<int32_t>();
    uint32_t *slab = d_slab.as<uint32_t>();
    const FrontierBufs bufs = store.bufs();
    const ColorJp jp{n, g->off, g->adj, pred, color, rnd, cnt, slab, slab_cap, &ctrl->slab_used, &ctrl->colors, 0};
    const long long wg_frontier = frontier_wg_option("COLOR_WG_FRONTIER", kWgFrontierDefault);

    GMSX_HIP(hipMemsetAsync(d_ctl.p, 0, 4 * sizeof(int32_t), s));
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(ColorCtrl), s));
    GMSX_HIP(hipMemsetAsync(color, 0, size_t(n) * sizeof(int32_t), s));
    GMSX_HIP(hipMemsetAsync(slab, 0, size_t(std::max<unsigned long long>(slab_cap, 1)) * sizeof(uint32_t), s));
    int &launches = *launches_out;
    launches = 0;
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (ordering) {
        GMSX_HIP(hipMemcpyAsync(d_in.p, ordering, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        GMSX_HIP(hipMemsetAsync(d_seen.p, 0, size_t(n) * sizeof(int32_t), s));
        // a permutation of 0..n-1, checked before anything reads rank[] as an index; the reference mis-colours on ties
        hipLaunchKernelGGL(k_oq_rank, dim3(tb), dim3(256), 0, s, n, d_in.as<int32_t>(), rank_format ? 1 : 0, rank, d_seen.as<int32_t>(),
                           d_ctl.as<int32_t>() + 2);
        int32_t ctl[4] = {0, 0, 0, 0};
        GMSX_HIP(hipMemcpyAsync(ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (ctl[2]) return GMSX_ERR_INVALID;
    } else {
        hipLaunchKernelGGL(k_iota, dim3(tb), dim3(256), 0, s, n, rank);  // getSimpleIdOrdering: what coloring.cc:25-30 hands to JonesV3
    }
    const unsigned lb = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    const unsigned long_grid = unsigned(cus) * 4;
    hipLaunchKernelGGL(k_oq_later, dim3(lb), dim3(256), 0, s, n, g->off, g->adj, rank, cnt, bufs.longs, long_cap, d_ctl.as<int32_t>());
    hipLaunchKernelGGL(k_oq_later_long, dim3(long_grid), dim3(256), 0, s, g->off, g->adj, rank, cnt, bufs.longs, long_cap, d_ctl.as<int32_t>());
    hipLaunchKernelGGL(k_color_select, dim3(sweep), dim3(256), 0, s, n, cnt, pred, ctrl, bufs.f[0]);
    launches += 4;
    ColorCtrl h;
    std::memset(&h, 0, sizeof h);
    int32_t ctl[4] = {0, 0, 0, 0};
    GMSX_HIP(hipMemcpyAsync(ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (ctl[1] || h.error || h.count <= 0 || h.count > n) return GMSX_ERR_KERNEL;  // (a permutation has a maximum: the first frontier is not empty)
    res.first_round = h.count;
    res.max_pred = h.max_pred;
    if (int rc = run_frontier_rounds(jp, bufs, ctrl, h, wg_frontier, &launches)) return rc;
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (h.done != n || h.colors < 1 || h.colors > h.max_pred + 1 || h.slab_used > slab_cap) return GMSX_ERR_KERNEL;
    res.colors = h.colors;
    res.rounds = h.round;
    return GMSX_OK;
}

int coloring_verify_device(const gmsx_graph *g, const int32_t *d_color, unsigned long long acc[8], int32_t ctl[4], float *ms) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const int64_t long_cap = frontier_long_cap(n, g->nnz);
    const int64_t words = n / 32 + 1;  // colours 0..n
    DevBuf d_present, d_long, d_ctl, d_acc;
    if (int rc = dalloc<uint32_t>(d_present, words)) return rc;
    if (int rc = dalloc<int32_t>(d_long, long_cap)) return rc;
    if (int rc = dalloc<int32_t>(d_ctl, 4)) return rc;
    if (int rc = dalloc<unsigned long long>(d_acc, 8)) return rc;
    GMSX_HIP(hipMemsetAsync(d_present.p, 0, size_t(words) * sizeof(uint32_t), s));
    GMSX_HIP(hipMemsetAsync(d_ctl.p, 0, 4 * sizeof(int32_t), s));
    GMSX_HIP(hipMemsetAsync(d_acc.p, 0, 8 * sizeof(unsigned long long), s));
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    const unsigned lb = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
    const unsigned sweep = unsigned(std::min<int64_t>((words + 255) / 256, int64_t(cus) * 16));
    hipLaunchKernelGGL(k_cv_rows, dim3(lb), dim3(256), 0, s, n, g->off, g->adj, d_color, d_present.as<uint32_t>(), d_long.as<int32_t>(), long_cap,
                       d_ctl.as<int32_t>(), d_acc.as<unsigned long long>());
    hipLaunchKernelGGL(k_cv_long, dim3(unsigned(cus) * 4), dim3(256), 0, s, g->off, g->adj, d_color, d_long.as<int32_t>(), long_cap, d_ctl.as<int32_t>(),
                       d_acc.as<unsigned long long>());
    hipLaunchKernelGGL(k_cv_distinct, dim3(sweep), dim3(256), 0, s, words, d_present.as<uint32_t>(), d_acc.as<unsigned long long>());
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    GMSX_HIP(hipMemcpyAsync(acc, d_acc.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(ctl, d_ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    GMSX_HIP(hipEventElapsedTime(ms, c.ev[0], c.ev[1]));
    return GMSX_OK;
}

}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_coloring_jp(const gmsx_graph *g, const int32_t *ordering, int rank_format, int32_t *coloring, int32_t *round_of, gmsx_coloring_info *info,
                     gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        const int64_t n = g->n;
        gmsx_coloring_info res;
        std::memset(&res, 0, sizeof res);
        if (n == 0) {
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        DevBuf d_color, d_round;
        int launches = 0;
        if (int rc = coloring_jp_device(g, ordering, rank_format, d_color, d_round, res, &launches)) return rc;
        const int32_t *color = d_color.as<const int32_t>(), *rnd = d_round.as<const int32_t>();
        // the outputs are written only now, when nothing can fail but the copies themselves
        std::vector<int32_t> h_color, h_round;
        if (coloring) {
            h_color.resize(size_t(n));
            GMSX_HIP(hipMemcpy(h_color.data(), color, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        if (round_of) {
            h_round.resize(size_t(n));
            GMSX_HIP(hipMemcpy(h_round.data(), rnd, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        float ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        if (coloring) std::memcpy(coloring, h_color.data(), size_t(n) * sizeof(int32_t));
        if (round_of) std::memcpy(round_of, h_round.data(), size_t(n) * sizeof(int32_t));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), 0.0, uint64_t(n), 0, uint64_t(res.rounds), launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_coloring_verify(const gmsx_graph *g, const int32_t *coloring, gmsx_coloring_check *out, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !out || (g->n > 0 && !coloring)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int64_t n = g->n;
        gmsx_coloring_check res;
        std::memset(&res, 0, sizeof res);
        if (n == 0) {
            *out = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        DevBuf d_color;
        if (int rc = dalloc<int32_t>(d_color, n)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_color.p, coloring, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int32_t ctl[4] = {0, 0, 0, 0};
        float ms = 0.f;
        if (int rc = coloring_verify_device(g, d_color.as<const int32_t>(), acc, ctl, &ms)) return rc;
        if (ctl[1] || (acc[kAccArcs] & 1ull)) return GMSX_ERR_KERNEL;  // (the CSR is symmetric: every equal pair is met from both ends)
        // the colours the bitmap does not cover — negative, or above n — are counted here; a colouring of any algorithm has none
        std::vector<int32_t> outliers;
        for (int64_t v = 0; v < n; ++v)
            if (coloring[v] < 0 || int64_t(coloring[v]) > n) outliers.push_back(coloring[v]);
        std::sort(outliers.begin(), outliers.end());
        const int64_t extra = int64_t(std::unique(outliers.begin(), outliers.end()) - outliers.begin());
        res.conflicts = int64_t(acc[kAccArcs] / 2);
        res.invalid = int64_t(acc[kAccInvalid]);
        res.max_color = int32_t(int64_t(acc[kAccMax]) - (1ll << 31));
        res.distinct = int32_t(int64_t(acc[kAccDistinct]) + extra);
        res.max_degree = int32_t(acc[kAccDeg]);
        *out = res;
        if (stats) *stats = gmsx_stats{double(ms), 0.0, uint64_t(n), 0, 0, 3, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
