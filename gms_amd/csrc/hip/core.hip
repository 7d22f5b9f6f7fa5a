// Exact k-core decomposition, the degree order and the quality of an order, on gfx950:
//   gmsx_core_decomposition  the exact counterpart of PpSequential::getDegeneracyOrderingMatula (preprocessing/sequential/degeneracy_matula.h:13-66;
//                            PpParallel's is the same serial loop behind a parallel degree pass) — BK-GMS-DGR of the Bron–Kerbosch driver
//                            (maximal_clique_enum_bron_kerbosch.cc:50-56)
//   gmsx_degree_rank         PpParallel::getDegreeOrdering (preprocessing/parallel/degree.h:15-61) — BK-GMS-DEG (:43-49)
//   gmsx_order_quality       CoreNumberEvaluator::getCoreNumberOfOrder / evaluateCoreNrAccuracy (preprocessing/util/core_number_evaluator.h:73-139)
//
// THE PEEL.  Matula's loop removes ONE vertex per step — the minimum of (remaining degree, id) — and is serial by construction.  The core
// numbers it implies (the running maximum of the removal degrees) do not depend on that sequence, and the level-synchronous peel yields them
// in a few hundred rounds: k := the smallest remaining degree; then rounds until none applies — in a round every remaining vertex of
// remaining degree <= k leaves at once (core number k, round = the running round index) and PUSHes a decrement to each neighbour, as
// k_adg_push does: every CSR entry is touched once over the whole run.  deg[] alone carries the membership: deg[w] <= k <=> w has left, is
// leaving or is queued for the next round, and the ONE decrement that takes deg[w] from k+1 to k (atomicSub returns k+1) queues w.  Which
// vertices a round removes is a fact about the integers, not about the arrival order of the atomics; the order inside the queues is not, and
// never reaches an output: the result is sorted by (round, id) at the end.
//
// COST SHAPE.  Hundreds of rounds, almost all of a handful of vertices: the fixed cost per round decides.  The rounds are those of the frontier
// engine (frontier_rounds.hpp: the row binning, the one-workgroup tail under CORE_WG_FRONTIER and its hand-back rule); this file supplies the
// per-vertex work (CorePeel), the level sweep and the final checks.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"
#include "order_rank.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

namespace gmsx {

namespace {

// control block of one peel: the engine's, plus the level
struct CoreCtrl : FrontierCtrl {  // (done = vertices that have left in finished rounds)
    int32_t k;        // current level
    int32_t min_deg;  // level sweep: smallest remaining degree
};

__global__ void k_core_init(int64_t n, const int64_t *__restrict__ off, int32_t *__restrict__ deg, int32_t *__restrict__ round_of) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) {
        deg[v] = int32_t(off[v + 1] - off[v]);
        round_of[v] = -1;
    }
}

// level sweep, first half: ctrl->min_deg = min deg over the remaining vertices (deg > the level just finished)
__global__ __launch_bounds__(256) void k_core_min(int64_t n, const int32_t *__restrict__ deg, int32_t k_done, CoreCtrl *__restrict__ ctrl) {
    int32_t m = INT_MAX;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += int64_t(gridDim.x) * blockDim.x) {
        const int32_t d = deg[v];
        if (d > k_done) m = min(m, d);
    }
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0 && m != INT_MAX) atomicMin(&ctrl->min_deg, m);
}

// … second half: the remaining vertices of that degree are the level's first frontier (one wave-aggregated append per wave)
__global__ __launch_bounds__(256) void k_core_select(int64_t n, const int32_t *__restrict__ deg, int32_t k_done, CoreCtrl *__restrict__ ctrl,
                                                     int32_t *__restrict__ frontier) {
    const int32_t k = ctrl->min_deg;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->k = k;  // (the others read min_deg, not k)
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;  // whole waves stay converged for the ballot
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        bool take = false;
        if (v < n) {
            const int32_t d = deg[v];
            take = d > k_done && d <= k;
        }
        wave_append(take, int32_t(v), frontier, &ctrl->count, n, &ctrl->error);
    }
}

// the peel as a policy of the engine: a frontier vertex leaves (core number k, this round) and PUSHes a decrement along its row
struct CorePeel {
    static constexpr int kGroupWords = 0;
    static constexpr bool kNotes = false;
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    int32_t *deg, *round_of, *core;
    int32_t k;  // the level (the host sets it from the control block it read)

    __device__ __forceinline__ void leave(int32_t x, int32_t round) const {
        round_of[x] = round;
        core[x] = k;
    }
    // row part [j0, j1) by `width` lanes: a neighbour still above k loses one; the decrement that brings it to k queues it
    __device__ __forceinline__ void walk(int64_t j0, int64_t j1, int64_t lane, int64_t width, const NextQueue &q) const {
        for (int64_t j = j0 + lane; j < j1; j += width) {
            const int32_t w = adj[j];
            if (load_now(&deg[w]) <= k) continue;  // has left, is leaving or is queued (deg only ever falls: a stale value costs an atomic, never the result)
            if (atomicSub(&deg[w], 1) == k + 1) q.push(w);
        }
    }
    __device__ __forceinline__ void short_row(int32_t x, int64_t j0, int64_t j1, int lane, int32_t round, uint32_t *, const NextQueue &q) const {
        if (lane == 0) leave(x, round);
        walk(j0, j1, lane, kGroup, q);
    }
    __device__ __forceinline__ void park(int32_t x, int32_t round, unsigned long long *, int64_t, int32_t *) const { leave(x, round); }
    __device__ __forceinline__ void long_walk(int32_t x, unsigned long long, int64_t tid, int64_t threads, const NextQueue &q) const {
        walk(off[x], off[x + 1], tid, threads, q);
    }
    __device__ __forceinline__ void finish() const {}
};

__global__ void k_core_keys(int64_t n, const int32_t *__restrict__ hi, unsigned long long *__restrict__ keys) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) keys[v] = ((unsigned long long)uint32_t(hi[v]) << 32) | (unsigned long long)uint32_t(v);
}
__global__ void k_degree_keys(int64_t n, const int64_t *__restrict__ off, unsigned long long *__restrict__ keys) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) keys[v] = ((unsigned long long)uint32_t(off[v + 1] - off[v]) << 32) | (unsigned long long)uint32_t(v);
}
__global__ void k_core_emit(int64_t n, const unsigned long long *__restrict__ sorted, int rank_format, int32_t *__restrict__ out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) {
        const int32_t v = int32_t(uint32_t(sorted[i] & 0xffffffffull));
        if (rank_format) out[v] = int32_t(i);
        else out[i] = v;
    }
}

int bits_for(uint64_t max_value) {
    int b = 1;
    while (b < 32 && (max_value >> b) != 0) ++b;
    return b;
}

// sorts n keys (hi << 32 | id) whose high halves are <= max_hi and writes the rank or order vector they imply into d_out
int sort_and_emit(int64_t n, DevBuf &d_keys, uint64_t max_hi, int rank_format, int32_t *d_out, hipStream_t s, int *launches) {
    DevBuf d_sorted, d_tmp;
    if (int rc = dalloc<unsigned long long>(d_sorted, n)) return rc;
    const unsigned end_bit = 32u + unsigned(bits_for(max_hi));
    size_t tmp_bytes = 0;
    GMSX_HIP(rocprim::radix_sort_keys(nullptr, tmp_bytes, d_keys.as<unsigned long long>(), d_sorted.as<unsigned long long>(), size_t(n), 0, end_bit, s));
    if (int rc = dalloc<char>(d_tmp, int64_t(tmp_bytes))) return rc;
    GMSX_HIP(rocprim::radix_sort_keys(d_tmp.p, tmp_bytes, d_keys.as<unsigned long long>(), d_sorted.as<unsigned long long>(), size_t(n), 0, end_bit, s));
    hipLaunchKernelGGL(k_core_emit, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, n, d_sorted.as<unsigned long long>(), rank_format, d_out);
    GMSX_HIP(hipStreamSynchronize(s));  // d_sorted / d_tmp are freed on return
    *launches += 2;
    return GMSX_OK;
}

// The peel.  On success d_core / d_round (n each, device) hold the core number and the round of every vertex.
int core_peel(const gmsx_graph *g, DevBuf &d_core, DevBuf &d_round, gmsx_core_info *info, int *launches_out) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    DevBuf d_deg, d_ctrl;
    FrontierStore store;
    if (int rc = dalloc<int32_t>(d_deg, n)) return rc;
    if (int rc = dalloc<int32_t>(d_core, n)) return rc;
    if (int rc = dalloc<int32_t>(d_round, n)) return rc;
    if (int rc = store.alloc(n, g->nnz, false)) return rc;
    if (int rc = dalloc<CoreCtrl>(d_ctrl, 1)) return rc;
    CoreCtrl *ctrl = d_ctrl.as<CoreCtrl>();
    int32_t *deg = d_deg.as<int32_t>();
    const FrontierBufs bufs = store.bufs();
    CorePeel peel{n, g->off, g->adj, deg, d_round.as<int32_t>(), d_core.as<int32_t>(), 0};
    const long long wg_frontier = frontier_wg_option("CORE_WG_FRONTIER", kWgFrontierDefault);

    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const unsigned tb = unsigned((n + 255) / 256);
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    int launches = 1;
    hipLaunchKernelGGL(k_core_init, dim3(tb), dim3(256), 0, s, n, g->off, deg, peel.round_of);
    CoreCtrl h;
    std::memset(&h, 0, sizeof h);
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(CoreCtrl), s));
    int32_t k_done = -1, levels = 0;
    int64_t top_core = 0;
    while (h.done < n) {
        // ---- the next level: k = smallest remaining degree, first frontier = the vertices that have it
        GMSX_HIP(hipMemsetAsync(&ctrl->min_deg, 0x7f, sizeof(int32_t), s));
        hipLaunchKernelGGL(k_core_min, dim3(sweep), dim3(256), 0, s, n, deg, k_done, ctrl);
        hipLaunchKernelGGL(k_core_select, dim3(sweep), dim3(256), 0, s, n, deg, k_done, ctrl, bufs.f[h.cur]);
        launches += 2;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.error || h.count <= 0 || h.count > n - h.done || h.min_deg <= k_done || h.k != h.min_deg) return GMSX_ERR_KERNEL;
        const int64_t removed_before = h.done;
        // ---- rounds of this level
        peel.k = h.k;
        if (int rc = run_frontier_rounds(peel, bufs, ctrl, h, wg_frontier, &launches)) return rc;
        top_core = h.done - removed_before;
        k_done = h.k;
        ++levels;
    }
    GMSX_HIP(hipGetLastError());
    if (h.done != n) return GMSX_ERR_KERNEL;
    info->degeneracy = k_done;
    info->levels = levels;
    info->rounds = h.round;
    info->reserved = 0;
    info->top_core = top_core;
    *launches_out = launches;
    return GMSX_OK;
}

// ---- order quality ------------------------------------------------------------------------------------------------------------------

// ordering -> rank[] with its validation (k_oq_rank) and later[] (k_oq_later / k_oq_later_long): order_rank.hpp, shared with coloring.hip

// acc[0] = max later, acc[1] = #(later > core_number), acc[2] = Σ (later - core_number) over those; core_number < 0: the maximum only
__global__ __launch_bounds__(256) void k_oq_reduce(int64_t n, const int32_t *__restrict__ later, int32_t core_number, unsigned long long *__restrict__ acc) {
    unsigned long long mx = 0, faulty = 0, excess = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += int64_t(gridDim.x) * blockDim.x) {
        const int32_t l = later[v];
        mx = max(mx, (unsigned long long)l);
        if (core_number >= 0 && l > core_number) {
            ++faulty;
            excess += (unsigned long long)(l - core_number);
        }
    }
    mx = wave_max(mx);
    faulty = wave_sum(faulty);
    excess = wave_sum(excess);
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(&acc[0], mx);
        if (faulty) atomicAdd(&acc[1], faulty);
        if (excess) atomicAdd(&acc[2], excess);
    }
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_core_decomposition(const gmsx_graph *g, int32_t *core, int32_t *ordering, int rank_format, gmsx_core_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int64_t n = g->n;
        gmsx_core_info res;
        std::memset(&res, 0, sizeof res);
        if (n == 0) {
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        DevBuf d_core, d_round, d_keys, d_out;
        int launches = 0;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = core_peel(g, d_core, d_round, &res, &launches)) return rc;
        if (ordering) {
            if (int rc = dalloc<unsigned long long>(d_keys, n)) return rc;
            if (int rc = dalloc<int32_t>(d_out, n)) return rc;
            hipLaunchKernelGGL(k_core_keys, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, n, d_round.as<int32_t>(), d_keys.as<unsigned long long>());
            launches += 1;
            if (int rc = sort_and_emit(n, d_keys, uint64_t(res.rounds), rank_format ? 1 : 0, d_out.as<int32_t>(), s, &launches)) return rc;
        }
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        // the outputs are written only now, when nothing can fail but the copies themselves
        std::vector<int32_t> h_core, h_ord;
        if (core) {
            h_core.resize(size_t(n));
            GMSX_HIP(hipMemcpy(h_core.data(), d_core.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        if (ordering) {
            h_ord.resize(size_t(n));
            GMSX_HIP(hipMemcpy(h_ord.data(), d_out.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        float ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        if (core) std::memcpy(core, h_core.data(), size_t(n) * sizeof(int32_t));
        if (ordering) std::memcpy(ordering, h_ord.data(), size_t(n) * sizeof(int32_t));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), 0.0, uint64_t(n), 0, uint64_t(res.rounds), launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_degree_rank(const gmsx_graph *g, int rank_format, int32_t *out, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !out) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int64_t n = g->n;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        if (n == 0) return GMSX_OK;
        DevBuf d_keys, d_out;
        if (int rc = dalloc<unsigned long long>(d_keys, n)) return rc;
        if (int rc = dalloc<int32_t>(d_out, n)) return rc;
        int launches = 1;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        // compare_degree (degree.h:16-22): v before w iff (deg v, v) < (deg w, w) — a strict total order, so the sort has one result
        hipLaunchKernelGGL(k_degree_keys, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, n, g->off, d_keys.as<unsigned long long>());
        if (int rc = sort_and_emit(n, d_keys, 0x7fffffffull /* any degree */, rank_format ? 1 : 0, d_out.as<int32_t>(), s, &launches))
            return rc;
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        GMSX_HIP(hipMemcpyAsync(out, d_out.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (stats) {
            float ms = 0.f;
            GMSX_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
            *stats = gmsx_stats{double(ms), 0.0, uint64_t(n), 0, 0, launches, 0, 0};
        }
        return GMSX_OK;
    });
}

int gmsx_order_quality(const gmsx_graph *g, const int32_t *ordering, int rank_format, int32_t core_number, int32_t *later,
                       gmsx_order_quality_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || (g->n > 0 && !ordering)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int64_t n = g->n;
        gmsx_order_quality_info res;
        std::memset(&res, 0, sizeof res);
        if (n == 0) {
            res.core_number = std::max<int32_t>(core_number, 0);
            res.core_number_of_order = res.core_number;
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        const unsigned tb = unsigned((n + 255) / 256);
        const int64_t long_cap = frontier_long_cap(n, g->nnz);
        DevBuf d_in, d_rank, d_seen, d_later, d_long, d_ctl, d_acc;
        if (int rc = dalloc<int32_t>(d_in, n)) return rc;
        if (int rc = dalloc<int32_t>(d_seen, n)) return rc;
        if (int rc = dalloc<int32_t>(d_later, n)) return rc;
        if (int rc = dalloc<int32_t>(d_long, long_cap)) return rc;
        if (int rc = dalloc<int32_t>(d_ctl, 4)) return rc;
        if (int rc = dalloc<unsigned long long>(d_acc, 4)) return rc;
        if (!rank_format)
            if (int rc = dalloc<int32_t>(d_rank, n)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_in.p, ordering, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        GMSX_HIP(hipMemsetAsync(d_seen.p, 0, size_t(n) * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(d_ctl.p, 0, 4 * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(d_acc.p, 0, 4 * sizeof(unsigned long long), s));
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        int32_t *rank = rank_format ? d_in.as<int32_t>() : d_rank.as<int32_t>();
        // a permutation of 0..n-1, checked before anything reads rank[] as an index (the BK entry points refuse the same inputs)
        hipLaunchKernelGGL(k_oq_rank, dim3(tb), dim3(256), 0, s, n, d_in.as<int32_t>(), rank_format ? 1 : 0, rank, d_seen.as<int32_t>(), d_ctl.as<int32_t>() + 2);
        int32_t ctl[4] = {0, 0, 0, 0};
        GMSX_HIP(hipMemcpyAsync(ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (ctl[2]) return GMSX_ERR_INVALID;  // n in-range entries, none hit twice: every value once
        int launches = 3;
        const unsigned lb = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
        hipLaunchKernelGGL(k_oq_later, dim3(lb), dim3(256), 0, s, n, g->off, g->adj, rank, d_later.as<int32_t>(), d_long.as<int32_t>(), long_cap, d_ctl.as<int32_t>());
        hipLaunchKernelGGL(k_oq_later_long, dim3(unsigned(cus) * 4), dim3(256), 0, s, g->off, g->adj, rank, d_later.as<int32_t>(), d_long.as<int32_t>(), long_cap,
                           d_ctl.as<int32_t>());
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        GMSX_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        if (core_number < 0) {  // graded against the true degeneracy: the peel of gmsx_core_decomposition
            DevBuf d_core, d_round;
            gmsx_core_info ci;
            int peel_launches = 0;
            GMSX_HIP(hipEventRecord(c.ev[0], s));
            if (int rc = core_peel(g, d_core, d_round, &ci, &peel_launches)) return rc;
            GMSX_HIP(hipEventRecord(c.ev[1], s));
            GMSX_HIP(hipStreamSynchronize(s));
            float pms = 0.f;
            GMSX_HIP(hipEventElapsedTime(&pms, c.ev[0], c.ev[1]));
            ms += pms;
            launches += peel_launches;
            core_number = ci.degeneracy;
        }
        const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        hipLaunchKernelGGL(k_oq_reduce, dim3(sweep), dim3(256), 0, s, n, d_later.as<int32_t>(), core_number, d_acc.as<unsigned long long>());
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        unsigned long long acc[4] = {0, 0, 0, 0};
        GMSX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (ctl[1]) return GMSX_ERR_KERNEL;
        float rms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&rms, c.ev[0], c.ev[1]));
        std::vector<int32_t> h_later;
        if (later) {
            h_later.resize(size_t(n));
            GMSX_HIP(hipMemcpy(h_later.data(), d_later.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        res.max_later = int32_t(acc[0]);
        res.core_number = core_number;
        res.core_number_of_order = std::max(core_number, res.max_later);
        res.faulty = int64_t(acc[1]);
        res.excess = int64_t(acc[2]);
        if (core_number > 0) {
            // core_number_evaluator.h:105-110, operand order as written there (size_t difference first, then the division by the double)
            const size_t core_of_order = size_t(res.core_number_of_order), actual = size_t(core_number);
            res.relative_error = (core_of_order - actual) / (double)actual;
            res.fault_rate = (double)acc[1] / (double)n;
            res.relative_mean_difference = (acc[1] == 0) ? 0 : ((double)acc[2] / (double)acc[1]) / (double)actual;
        }
        if (later) std::memcpy(later, h_later.data(), size_t(n) * sizeof(int32_t));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms + rms), 0.0, uint64_t(n), 0, 0, launches + 1, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
