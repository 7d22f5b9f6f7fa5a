// The frontier-rounds engine: level-synchronous rounds over a frontier of vertices, written once for the k-core peel (core.hip), Jones–Plassmann
// colouring (coloring.hip), the truss peel (truss.hip: its items are edges), top-down BFS (traversal.hip) and delta-stepping shortest paths
// (sssp.hip).  A round walks the row of every frontier vertex; what a row entry means is the POLICY's business (the peel pushes a decrement,
// colouring marks a bitmap, releases successors and picks a colour, BFS claims, SSSP relaxes), and whatever the walk appends to the next
// frontier is the next round's work.  The kernels, the host's round loop (run_frontier_rounds: nothing else launches a k_frontier_* kernel), the
// owner of the buffers (FrontierStore) and the two device pieces the users share around the rounds (k_frontier_collect, RowGroup) are here and
// nowhere else.  The rule all share:
//   binning     a kGroup-lane group per frontier vertex up to kLongRow entries; longer rows are PARKED with a bounds-checked append and walked
//               by all workgroups together (all threads of the workgroup in the tail) — no lane walks a long row alone
//   boundary    a round boundary is a kernel boundary (k_frontier_round + k_frontier_round_long + k_frontier_advance, then the host reads the
//               control block) or, while the frontier holds at most wg_frontier vertices, a __syncthreads() of k_frontier_tail: ONE workgroup
//               that runs round after round until the frontier empties or outgrows the threshold
//   hand-back   the tail weighs every round first (tail_too_heavy): a row above kWgRowMax, more than kTailLong long rows or more than kWgWorkMax
//               entries in all set ctrl->bail and the round goes to the grid-wide kernels — else every other CU would idle behind this one
// No workgroup ever waits for another one.  Every append is bounds-checked and raises ctrl->error.
//
// A POLICY is a small struct passed by value as a kernel argument (so every thread owns a copy and may keep per-thread state in it):
//   n, off                                    the engine reads the row bounds and the frontier capacity from it
//   kGroupWords                               LDS words a group gets for a short row (0: none)
//   kNotes                                    parked rows carry a 64-bit note and are settled at the round boundary
//   short_row(x, j0, j1, lane, round, words, q)   the kGroup lanes of a group, row [j0, j1) of frontier vertex x
//   park(x, round, notes, pos, error)         lane 0, when x was parked at `pos`
//   long_walk(x, note, tid, threads, q)       the part of the parked row x that thread tid of `threads` walks
//   settle(x, note, round, tid, error)        kNotes only: every thread of ONE workgroup of kTailThreads, behind the walks (may hold barriers)
//   finish()                                  every thread, converged, at the end of each of the four kernels (k_frontier_advance: kNotes only)
//   kStops, round_stop()                      optional: ONE thread at every round boundary, behind all appends of the round; true ends the step
//                                             there (the tail returns, and the policy tells the host through its own control block)
//   kReenters                                 optional: a vertex may enter more than one frontier, so the host does not read ctrl->done
#pragma once
#include "device_buffer.hpp"
#include "device_graph.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <type_traits>

namespace gmsx {
namespace {

// does policy P decide at a round boundary whether the rounds go on (P::kStops, P::round_stop)?
template <class P, class = void>
struct policy_stops : std::false_type {};
template <class P>
struct policy_stops<P, std::void_t<decltype(P::kStops)>> : std::true_type {};
// may a vertex enter more than one frontier under policy P (P::kReenters)?
template <class P, class = void>
struct policy_reenters : std::false_type {};
template <class P>
struct policy_reenters<P, std::void_t<decltype(P::kReenters)>> : std::true_type {};

// UNMEASURED: none of these bounds is tuned yet (tools/core_probe.py and tools/coloring_probe.py are the measurement).  They
// follow the round table of the peel on R-MAT graphs (almost every round holds fewer than 256 vertices) and the row shapes named there.
constexpr int kGroup = 16;           // lanes per vertex of a short row
constexpr int kLongRow = 1024;       // longer rows are walked by many waves together
constexpr int kWgRowMax = 32768;     // the tail hands a frontier with a longer row back to the grid-wide kernels
constexpr int kTailThreads = 1024;
constexpr int kTailLong = 256;       // long rows one round of the tail can park; more: the round goes back to the grid
constexpr int kWgWorkMax = 1 << 18;  // CSR entries one round of the tail may walk (256 per thread); more: the round goes back to the grid
constexpr long long kWgFrontierDefault = 512;

// control block of one run (device, mirrored to the host after every step); an algorithm derives its own from it
struct FrontierCtrl {
    int32_t count;  // vertices in the current frontier
    int32_t next;   // appended to the next one so far
    int32_t round;  // index of the round the current frontier is worked in
    int32_t done;   // vertices of finished rounds (kReenters: frontier entries, may pass n and wrap; the host does not read it)
    int32_t error;  // an append (or a policy) hit its bound
    int32_t nlong;  // long rows parked by k_frontier_round
    int32_t bail;   // the tail met a round too heavy for one workgroup: it belongs to the grid-wide kernels
    int32_t cur;    // which of the two frontier buffers is the current one
};

// the buffers of one run: two frontiers of n entries, the parked rows and (kNotes) their notes
struct FrontierBufs {
    int32_t *f[2];
    int32_t *longs;
    unsigned long long *notes;
    int64_t long_cap;
};

// how many rows above kLongRow `items` rows of `entries` entries in all can hold (also for the passes that only bin rows and run no rounds)
inline int64_t frontier_long_cap(int64_t items, int64_t entries) { return std::min<int64_t>(items, entries / kLongRow + 1); }

// … and their owner
struct FrontierStore {
    DevBuf f0, f1, longs, notes;
    int64_t long_cap = 0;
    int alloc(int64_t items, int64_t entries, bool with_notes) {
        long_cap = frontier_long_cap(items, entries);
        if (int rc = dalloc<int32_t>(f0, items)) return rc;
        if (int rc = dalloc<int32_t>(f1, items)) return rc;
        if (int rc = dalloc<int32_t>(longs, long_cap)) return rc;
        return with_notes ? dalloc<unsigned long long>(notes, long_cap) : GMSX_OK;
    }
    FrontierBufs bufs() const { return {{f0.as<int32_t>(), f1.as<int32_t>()}, longs.as<int32_t>(), notes.as<unsigned long long>(), long_cap}; }
};

// an algorithm's …_WG_FRONTIER option: 0 = every round a kernel boundary, large = every round the tail may take
inline long long frontier_wg_option(const char *name, long long dflt) {
    return std::max<long long>(0, std::min<long long>(opt_int(name, dflt), INT_MAX));
}

__device__ __forceinline__ int32_t load_now(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t load_now(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long load_now(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_now(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// buf[(*count)++] = v if that is below cap (the position is returned), else *error = 1 (-1); count in LDS or in global memory
__device__ __forceinline__ int64_t append_checked(int32_t *buf, int32_t *count, int64_t cap, int32_t v, int32_t *error) {
    const int64_t pos = int64_t(atomicAdd(count, 1));
    if (pos < cap) {
        buf[pos] = v;
        return pos;
    }
    *error = 1;
    return -1;
}

// the same for the lanes of a converged wave that `take`: one atomic per wave
__device__ __forceinline__ void wave_append(bool take, int32_t v, int32_t *buf, int32_t *count, int64_t cap, int32_t *error) {
    const unsigned long long m = __ballot(take);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    int32_t base = 0;
    if (lane == 0) base = atomicAdd(count, int32_t(__popcll(m)));
    base = __shfl(base, 0);
    if (take) {
        const int64_t pos = int64_t(base) + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < cap) buf[pos] = v;
        else *error = 1;
    }
}

// every v < n that `pred` (passed by value) holds of into a frontier list of n entries
template <class Pred>
__global__ __launch_bounds__(256) void k_frontier_collect(int64_t n, Pred pred, int32_t *__restrict__ list, int32_t *__restrict__ count,
                                                          int32_t *__restrict__ error) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;  // whole waves stay converged for the ballot
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride)
        wave_append(v < n && pred(v), int32_t(v), list, count, n, error);
}
template <class Pred>
void frontier_collect(int64_t n, Pred pred, int32_t *list, int32_t *count, int32_t *error) {
    const int cus = ctx().compute_units > 0 ? ctx().compute_units : 256;
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    hipLaunchKernelGGL(k_frontier_collect<Pred>, dim3(sweep), dim3(256), 0, ctx().stream, n, pred, list, count, error);
}

// a group of WIDTH lanes (a power of two) that scans a row chunk by chunk, a ballot per chunk
template <int WIDTH>
struct RowGroup {
    static constexpr unsigned long long mask = WIDTH == 64 ? ~0ull : ((1ull << (WIDTH & 63)) - 1ull);
    const int lane, shift;  // shift: where the group's lanes sit in the wave's ballot
    __device__ __forceinline__ RowGroup() : lane(threadIdx.x & (WIDTH - 1)), shift((threadIdx.x & 63) & ~(WIDTH - 1)) {}
    __device__ __forceinline__ unsigned long long ballot(bool b) const { return (__ballot(b) >> shift) & mask; }
    // the lowest lane of `hits`: in an ascending row it holds the smallest id
    __device__ static __forceinline__ int first(unsigned long long hits) { return __ffsll((long long)hits) - 1; }
};

// the next frontier as a policy sees it
struct NextQueue {
    int32_t *buf, *count;
    int64_t cap;
    int32_t *error;
    __device__ __forceinline__ void push(int32_t w) const { append_checked(buf, count, cap, w, error); }
};

[[maybe_unused]] __global__ void k_iota(int64_t n, int32_t *__restrict__ ids) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = int32_t(i);
}

// one round, grid-wide: a kGroup-lane group per frontier vertex; rows above kLongRow are parked for k_frontier_round_long
template <class P>
__global__ __launch_bounds__(256) void k_frontier_round(P p, const int32_t *__restrict__ cur, int32_t *__restrict__ next, int32_t *__restrict__ longs,
                                                        unsigned long long *__restrict__ notes, int64_t long_cap, FrontierCtrl *__restrict__ ctrl) {
    __shared__ uint32_t s_words[256 / kGroup][P::kGroupWords ? P::kGroupWords : 1];
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    const int32_t count = ctrl->count, round = ctrl->round;
    const NextQueue q{next, &ctrl->next, p.n, &ctrl->error};
    for (int64_t i = group0; i < count; i += groups) {  // (a group is on its own from here: its shuffles and its LDS words stay inside it)
        const int32_t x = cur[i];
        const int64_t j0 = p.off[x], j1 = p.off[x + 1];
        if (j1 - j0 > kLongRow) {
            if (lane == 0) {
                const int64_t pos = append_checked(longs, &ctrl->nlong, long_cap, x, &ctrl->error);
                if (pos >= 0) p.park(x, round, notes, pos, &ctrl->error);
            }
            continue;
        }
        p.short_row(x, j0, j1, lane, round, s_words[threadIdx.x / kGroup], q);
    }
    p.finish();
}

// … its long rows: all workgroups walk each of them together
template <class P>
__global__ __launch_bounds__(256) void k_frontier_round_long(P p, int32_t *__restrict__ next, const int32_t *__restrict__ longs,
                                                             const unsigned long long *__restrict__ notes, int64_t long_cap,
                                                             FrontierCtrl *__restrict__ ctrl) {
    if (P::kNotes && ctrl->error) return;  // (a parked row without its note)
    const int64_t nlong = min(int64_t(ctrl->nlong), long_cap);
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, threads = int64_t(gridDim.x) * blockDim.x;
    const NextQueue q{next, &ctrl->next, p.n, &ctrl->error};
    for (int64_t i = 0; i < nlong; ++i) p.long_walk(longs[i], P::kNotes ? notes[i] : 0ull, tid, threads, q);
    // SsspRelax flushes its walks' counts here.  ColorJp::finish() publishes `top`, which only give() raises and long_walk never calls: it stays
    // the 0 the host passed, and the hook costs that policy one compare.
    p.finish();
}

// … and the round boundary: the parked rows are settled (kNotes: ONE workgroup of kTailThreads — their walks are complete only behind the
// kernel boundary; else one thread) and the next frontier becomes the current one
template <class P>
__global__ __launch_bounds__(kTailThreads) void k_frontier_advance(P p, const int32_t *__restrict__ longs, const unsigned long long *__restrict__ notes,
                                                                   int64_t long_cap, FrontierCtrl *__restrict__ ctrl) {
    if constexpr (P::kNotes) {
        const int64_t nlong = ctrl->error ? 0 : min(int64_t(ctrl->nlong), long_cap);
        const int32_t round = ctrl->round;
        int32_t bad = 0;
        for (int64_t i = 0; i < nlong; ++i) p.settle(longs[i], notes[i], round, int(threadIdx.x), &bad);
        if (bad) ctrl->error = 1;
        p.finish();
    }
    if (threadIdx.x == 0) {
        ctrl->done += ctrl->count;
        ctrl->count = ctrl->next;
        ctrl->next = 0;
        ctrl->nlong = 0;
        ctrl->round += 1;
        ctrl->cur ^= 1;
        if constexpr (policy_stops<P>::value) p.round_stop();
    }
}

// what the round would cost the tail (every thread must call it; one barrier): one workgroup takes it only if no row is above kWgRowMax, its
// long rows fit the list and all its rows together hold at most kWgWorkMax entries
__device__ __forceinline__ bool tail_too_heavy(const int32_t *cur, int32_t count, const int64_t *__restrict__ off, int tid, int32_t *s_flag,
                                               int32_t *s_nlong_seen, unsigned long long *s_work) {
    unsigned long long work = 0;
    int32_t nl = 0;
    for (int32_t i = tid; i < count; i += kTailThreads) {
        const int32_t x = load_now(&cur[i]);
        const int64_t len = off[x + 1] - off[x];
        if (len > kWgRowMax) *s_flag = 1;
        if (len > kLongRow) ++nl;
        work += (unsigned long long)len;
    }
    if (work) atomicAdd(s_work, work);
    if (nl) atomicAdd(s_nlong_seen, nl);
    __syncthreads();
    return *s_flag || *s_nlong_seen > kTailLong || *s_work > (unsigned long long)kWgWorkMax;
}

// rounds inside ONE workgroup: the round boundary is a __syncthreads().  Runs while 0 < frontier <= wg_frontier; returns with the control block
// describing the state it stopped in (frontier empty: done; larger than wg_frontier, or ctrl->bail: the grid-wide kernels go on).  The two
// frontier buffers stay in global memory (they are bounds-checked against n there and may be handed back at any round), read with loads that
// bypass the vector cache; the counters, the parked rows and the groups' words live in LDS.
template <class P>
__global__ __launch_bounds__(kTailThreads) void k_frontier_tail(P p, int32_t *__restrict__ f0, int32_t *__restrict__ f1, int32_t wg_frontier,
                                                                FrontierCtrl *__restrict__ ctrl) {
    __shared__ int32_t s_count, s_next, s_error, s_flag, s_nlong, s_nlong_seen;
    __shared__ unsigned long long s_work;
    __shared__ int32_t s_long[kTailLong];
    __shared__ unsigned long long s_notes[P::kNotes ? kTailLong : 1];
    __shared__ uint32_t s_words[kTailThreads / kGroup][P::kGroupWords ? P::kGroupWords : 1];
    const int tid = threadIdx.x, lane = tid & (kGroup - 1), group = tid / kGroup;
    constexpr int groups = kTailThreads / kGroup;
    int32_t round = ctrl->round, done = ctrl->done, curi = ctrl->cur, bail = 0;
    if (tid == 0) {
        s_count = ctrl->count;
        s_next = 0;
        s_error = 0;
        s_flag = 0;
        s_nlong = 0;
        s_nlong_seen = 0;
        s_work = 0;
    }
    __syncthreads();
    for (;;) {
        const int32_t count = s_count;
        if (count == 0 || count > wg_frontier) break;
        const int32_t *cur = curi ? f1 : f0;
        const NextQueue q{curi ? f0 : f1, &s_next, p.n, &s_error};
        if (tail_too_heavy(cur, count, p.off, tid, &s_flag, &s_nlong_seen, &s_work)) {
            bail = 1;
            break;
        }
        for (int32_t i = group; i < count; i += groups) {
            const int32_t x = load_now(&cur[i]);
            const int64_t j0 = p.off[x], j1 = p.off[x + 1];
            if (j1 - j0 > kLongRow) {
                if (lane == 0) {  // at most kTailLong of them: weighed above
                    const int64_t pos = append_checked(s_long, &s_nlong, kTailLong, x, &s_error);
                    if (pos >= 0) p.park(x, round, s_notes, pos, &s_error);
                }
                continue;
            }
            p.short_row(x, j0, j1, lane, round, s_words[group], q);
        }
        __syncthreads();
        const int32_t nlong = (P::kNotes && s_error) ? 0 : min(s_nlong, kTailLong);
        // every thread has read s_error before a walk may set it: settle() holds barriers, the trip count must be uniform
        if constexpr (P::kNotes) __syncthreads();
        for (int32_t i = 0; i < nlong; ++i) p.long_walk(s_long[i], P::kNotes ? s_notes[i] : 0ull, tid, kTailThreads, q);
        __syncthreads();
        if constexpr (P::kNotes) {
            for (int32_t i = 0; i < nlong; ++i) p.settle(s_long[i], s_notes[i], round, tid, &s_error);
            __syncthreads();
        }
        done += count;
        round += 1;
        curi ^= 1;
        if (tid == 0) {
            s_count = s_error ? 0 : min(s_next, int32_t(min(p.n, int64_t(INT_MAX))));
            s_next = 0;
            s_nlong = 0;
            s_nlong_seen = 0;
            s_work = 0;
        }
        __syncthreads();
        if constexpr (policy_stops<P>::value) {  // (s_stop is written again only behind the barriers of the next round)
            __shared__ int32_t s_stop;
            if (tid == 0) s_stop = p.round_stop() ? 1 : 0;
            __syncthreads();
            if (s_stop) break;
        }
    }
    p.finish();
    if (tid == 0) {
        ctrl->count = s_count;
        ctrl->next = 0;
        ctrl->nlong = 0;
        ctrl->round = round;
        ctrl->done = done;
        ctrl->cur = curi;
        ctrl->bail = bail;
        if (s_error) ctrl->error = 1;
    }
}

// The host's round loop: steps until the frontier that the mirror h (Ctrl: derived from FrontierCtrl, read back whole after every step)
// describes is empty, or until `stop` says so of the mirror (asked before every step).  A step is the tail or the three grid-wide launches.
struct NeverStop {
    template <class Ctrl> bool operator()(const Ctrl &) const { return false; }
};
template <class P, class Ctrl, class Stop = NeverStop>
int run_frontier_rounds(const P &p, const FrontierBufs &b, Ctrl *ctrl, Ctrl &h, long long wg_frontier, int *launches, Stop stop = Stop{}) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const int64_t n = p.n;
    constexpr bool once = !policy_reenters<P>::value;  // every vertex enters one frontier: `done` bounds the frontier and grows with every step
    while (h.count > 0 && !stop(h)) {
        if (h.count <= wg_frontier && !h.bail) {
            hipLaunchKernelGGL(k_frontier_tail<P>, dim3(1), dim3(kTailThreads), 0, s, p, b.f[0], b.f[1], int32_t(wg_frontier), ctrl);
            *launches += 1;
        } else {
            const unsigned rb = unsigned(std::min<int64_t>((int64_t(h.count) * kGroup + 255) / 256, int64_t(cus) * 32));
            hipLaunchKernelGGL(k_frontier_round<P>, dim3(rb), dim3(256), 0, s, p, b.f[h.cur], b.f[h.cur ^ 1], b.longs, b.notes, b.long_cap, ctrl);
            hipLaunchKernelGGL(k_frontier_round_long<P>, dim3(unsigned(cus) * 4), dim3(256), 0, s, p, b.f[h.cur ^ 1], b.longs, b.notes, b.long_cap, ctrl);
            hipLaunchKernelGGL(k_frontier_advance<P>, dim3(1), dim3(P::kNotes ? kTailThreads : 1), 0, s, p, b.longs, b.notes, b.long_cap, ctrl);
            *launches += 3;
            if (h.bail) {
                h.bail = 0;
                GMSX_HIP(hipMemsetAsync(&ctrl->bail, 0, sizeof(int32_t), s));
            }
        }
        const int32_t done_was = h.done, round_was = h.round;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.error || h.count < 0 || (once ? h.done > n || h.count > n - h.done : h.count > n)) return GMSX_ERR_KERNEL;
        if (!h.bail && ((once && h.done <= done_was) || h.round <= round_was)) return GMSX_ERR_KERNEL;  // a step that made no progress
    }
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx
