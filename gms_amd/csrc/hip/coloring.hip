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
// COST SHAPE.  That of the peel in core.hip — hundreds to thousands of rounds, most of them tiny — and its solutions: a round boundary is a
// kernel boundary (k_color_round + k_color_round_long + k_color_pick_advance, then the host reads the control block) or, while the frontier holds at
// most COLOR_WG_FRONTIER vertices that are light enough, a __syncthreads() of k_color_tail, ONE workgroup that runs round after round.  No
// workgroup ever waits for another one.  Rows are binned as there: a 16-lane group per vertex up to kLongRow entries with its bitmap in
// LDS; longer rows by all workgroups together (all threads of the workgroup in k_color_tail) with the bitmap in a zeroed global slab, so
// no graph is refused for a wide neighbourhood.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "order_rank.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

// UNMEASURED: none of these bounds has a timing behind it yet (tools/coloring_probe.py is the measurement).  They are
// core.hip's, for the same reasons; kGroup and kLongRow are shared with it (order_rank.hpp).
constexpr int kBitWords = kLongRow / 32 + 1;  // bitmap of a short row: colours 1..p+1, p <= kLongRow
constexpr int kWgRowMax = 32768;              // k_color_tail hands a frontier with a longer row back to the grid-wide kernels
constexpr int kTailThreads = 1024;
constexpr int kTailLong = 256;                // long rows one round of k_color_tail can park; more: the round goes back to the grid
constexpr int kWgWorkMax = 1 << 18;           // CSR entries one round of k_color_tail may walk; more: the round goes back to the grid
constexpr long long kWgFrontierDefault = 512;

// control block of one run (device, mirrored to the host after every step)
struct ColorCtrl {
    int32_t count;      // vertices in the current frontier
    int32_t next;       // appended to the next one so far
    int32_t round;      // index of the round the current frontier is coloured in
    int32_t colored;    // vertices coloured in finished rounds
    int32_t error;      // an append, the slab or a first-free search hit its bound
    int32_t nlong;      // long rows parked by k_color_round
    int32_t bail;       // k_color_tail met a round too heavy for one workgroup
    int32_t cur;        // which of the two frontier buffers is the current one
    int32_t colors;     // largest colour given so far
    int32_t max_pred;   // most predecessors of any vertex
    unsigned long long slab_used;  // words of the slab handed to long rows so far (every vertex is parked at most once)
};

__device__ __forceinline__ int32_t load_now(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t load_now(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_now(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the lanes of a wave run in program order: this only keeps the compiler from moving LDS accesses across the phases of a group
__device__ __forceinline__ void group_phase() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ void k_color_iota(int64_t n, int32_t *__restrict__ rank) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) rank[v] = int32_t(v);  // getSimpleIdOrdering: what coloring.cc:25-30 hands to JonesV3
}

// pred[v] = cnt[v] (the counters fall, the bitmap widths stay), max_pred, and the first frontier: cnt == 0 (one wave-aggregated append per wave)
__global__ __launch_bounds__(256) void k_color_select(int64_t n, const int32_t *__restrict__ cnt, int32_t *__restrict__ pred, ColorCtrl *__restrict__ ctrl,
                                                      int32_t *__restrict__ frontier) {
    const int lane = threadIdx.x & 63;
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
        const unsigned long long m = __ballot(take);
        if (m == 0) continue;
        int32_t base = 0;
        if (lane == 0) base = atomicAdd(&ctrl->count, int32_t(__popcll(m)));
        base = __shfl(base, 0);
        if (take) {
            const int64_t pos = int64_t(base) + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < n) frontier[pos] = int32_t(v);
            else ctrl->error = 1;
        }
    }
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_down(mx, o));
    if (lane == 0 && mx) atomicMax(&ctrl->max_pred, mx);
}

// a successor of the frontier vertex: its counter drops, and the decrement that brings it to 0 queues it
template <class Counter>
__device__ __forceinline__ void release_successor(int32_t w, int32_t *__restrict__ cnt, int32_t *__restrict__ next, Counter *next_count, int64_t cap,
                                                  int32_t *error) {
    if (atomicSub(&cnt[w], 1) == 1) {
        const int64_t pos = int64_t(atomicAdd(next_count, 1));
        if (pos < cap) next[pos] = w;
        else *error = 1;
    }
}

// one SHORT row [j0, j1) of frontier vertex x by the kGroup lanes of a group, forbidden bitmap `bits` (kBitWords words of LDS, the group's own):
// returns x's colour (every lane of the group), 0 if the search found none (cannot happen: at most p of the p + 1 bits are set)
template <class Counter>
__device__ __forceinline__ int32_t color_short_row(int64_t j0, int64_t j1, int32_t p, int lane, uint32_t *bits, const int32_t *__restrict__ adj,
                                                   const int32_t *__restrict__ color, int32_t *__restrict__ cnt, int32_t *__restrict__ next,
                                                   Counter *next_count, int64_t cap, int32_t *error) {
    const int words = min(p / 32 + 1, kBitWords);  // bits 0..p = colours 1..p+1
    for (int w = lane; w < words; w += kGroup) bits[w] = 0;
    group_phase();
    for (int64_t j = j0 + lane; j < j1; j += kGroup) {
        const int32_t w = adj[j];
        const int32_t c = load_now(&color[w]);
        if (c != 0) {
            const int32_t b = c - 1;
            if (b >= 0 && b <= p && (b >> 5) < words) atomicOr(&bits[b >> 5], 1u << (b & 31));
        } else {
            release_successor(w, cnt, next, next_count, cap, error);
        }
    }
    group_phase();
    int32_t best = INT_MAX;
    for (int w = lane; w < words; w += kGroup) {
        const uint32_t free = ~bits[w];
        if (free) best = min(best, w * 32 + __ffs(free) - 1);
    }
    for (int o = kGroup / 2; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, kGroup));
    group_phase();  // (the next vertex of this group zeroes the same words)
    return best <= p ? best + 1 : 0;
}

// the part of one LONG row that `threads` threads walk together: the bitmap is slab[0 .. p/32], zeroed, set by idempotent ORs
template <class Counter>
__device__ __forceinline__ void color_long_walk(int64_t j0, int64_t j1, int32_t p, int64_t tid, int64_t threads, uint32_t *__restrict__ slab,
                                                const int32_t *__restrict__ adj, const int32_t *__restrict__ color, int32_t *__restrict__ cnt,
                                                int32_t *__restrict__ next, Counter *next_count, int64_t cap, int32_t *error) {
    for (int64_t j = j0 + tid; j < j1; j += threads) {
        const int32_t w = adj[j];
        const int32_t c = load_now(&color[w]);
        if (c != 0) {
            const int32_t b = c - 1;
            if (b >= 0 && b <= p) {
                const uint32_t bit = 1u << (b & 31);
                if (!(load_now(&slab[b >> 5]) & bit)) atomicOr(&slab[b >> 5], bit);  // (a stale read costs an atomic, never the result)
            }
        } else {
            release_successor(w, cnt, next, next_count, cap, error);
        }
    }
}

// first zero bit of slab[0 .. p/32] by all threads of the workgroup (every thread must call it); 0-based, INT_MAX if none
__device__ __forceinline__ int32_t first_free_long(const uint32_t *__restrict__ slab, int32_t p, int tid, int threads, int32_t *s_best) {
    if (tid == 0) *s_best = INT_MAX;
    __syncthreads();
    const int32_t words = p / 32 + 1;
    for (int32_t w = tid; w < words; w += threads) {
        const uint32_t free = ~load_now(&slab[w]);
        if (free) {
            atomicMin(s_best, w * 32 + __ffs(free) - 1);
            break;  // (this thread's later words are higher)
        }
    }
    __syncthreads();
    const int32_t best = *s_best;
    __syncthreads();
    return best;
}

// one round, grid-wide: a 16-lane group per frontier vertex; rows above kLongRow are parked for k_color_round_long, each with its piece of the slab
__global__ __launch_bounds__(256) void k_color_round(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                     const int32_t *__restrict__ pred, int32_t *__restrict__ color, int32_t *__restrict__ round_of,
                                                     int32_t *__restrict__ cnt, const int32_t *__restrict__ cur, int32_t *__restrict__ next,
                                                     int32_t *__restrict__ longs, unsigned long long *__restrict__ long_slab, int64_t long_cap,
                                                     unsigned long long slab_cap, ColorCtrl *__restrict__ ctrl) {
    __shared__ uint32_t s_bits[256 / kGroup][kBitWords];
    const int lane = threadIdx.x & (kGroup - 1);
    uint32_t *bits = s_bits[threadIdx.x / kGroup];
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    const int32_t count = ctrl->count, round = ctrl->round;
    int32_t top = 0;
    for (int64_t i = group0; i < count; i += groups) {  // (a group is on its own from here: its shuffles and its bitmap stay inside it)
        const int32_t x = cur[i];
        const int64_t j0 = off[x], j1 = off[x + 1];
        const int32_t p = pred[x];
        if (j1 - j0 > kLongRow) {
            if (lane == 0) {
                const unsigned long long words = (unsigned long long)(p / 32 + 1);
                const int64_t pos = int64_t(atomicAdd(&ctrl->nlong, 1));
                const unsigned long long at = atomicAdd(&ctrl->slab_used, words);
                if (pos < long_cap && at + words <= slab_cap) {
                    longs[pos] = x;
                    long_slab[pos] = at;
                } else {
                    ctrl->error = 1;
                }
            }
            continue;
        }
        const int32_t c = color_short_row(j0, j1, p, lane, bits, adj, color, cnt, next, &ctrl->next, n, &ctrl->error);
        if (lane == 0) {
            if (c == 0) ctrl->error = 1;
            store_now(&color[x], c);
            round_of[x] = round;
            top = max(top, c);
        }
    }
    if (top) atomicMax(&ctrl->colors, top);
}

// … its long rows: all workgroups walk each of them together
__global__ __launch_bounds__(256) void k_color_round_long(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                          const int32_t *__restrict__ pred, const int32_t *__restrict__ color,
                                                          int32_t *__restrict__ cnt, int32_t *__restrict__ next, const int32_t *__restrict__ longs,
                                                          const unsigned long long *__restrict__ long_slab, int64_t long_cap,
                                                          uint32_t *__restrict__ slab, ColorCtrl *__restrict__ ctrl) {
    if (ctrl->error) return;  // (a parked row without its piece of the slab)
    const int64_t nlong = min(int64_t(ctrl->nlong), long_cap);
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, threads = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = 0; i < nlong; ++i) {
        const int32_t x = longs[i];
        color_long_walk(off[x], off[x + 1], pred[x], tid, threads, slab + long_slab[i], adj, color, cnt, next, &ctrl->next, n, &ctrl->error);
    }
}

// … their colours (ONE workgroup: the bitmaps are complete only behind the kernel boundary), and the round boundary: the next frontier becomes
// the current one
__global__ __launch_bounds__(kTailThreads) void k_color_pick_advance(const int32_t *__restrict__ pred, int32_t *__restrict__ color,
                                                                     int32_t *__restrict__ round_of, const int32_t *__restrict__ longs,
                                                                     const unsigned long long *__restrict__ long_slab, int64_t long_cap,
                                                                     const uint32_t *__restrict__ slab, ColorCtrl *__restrict__ ctrl) {
    __shared__ int32_t s_best;
    const int tid = threadIdx.x;
    const int64_t nlong = ctrl->error ? 0 : min(int64_t(ctrl->nlong), long_cap);
    const int32_t round = ctrl->round;
    int32_t top = 0, bad = 0;
    for (int64_t i = 0; i < nlong; ++i) {
        const int32_t x = longs[i];
        const int32_t p = pred[x];
        const int32_t best = first_free_long(slab + long_slab[i], p, tid, kTailThreads, &s_best);
        if (tid == 0) {
            if (best > p) bad = 1;
            const int32_t c = best > p ? 0 : best + 1;
            store_now(&color[x], c);
            round_of[x] = round;
            top = max(top, c);
        }
    }
    if (tid == 0) {
        if (bad) ctrl->error = 1;
        if (top > ctrl->colors) ctrl->colors = top;  // (the only workgroup of the only kernel that runs now)
        ctrl->colored += ctrl->count;
        ctrl->count = ctrl->next;
        ctrl->next = 0;
        ctrl->nlong = 0;
        ctrl->round += 1;
        ctrl->cur ^= 1;
    }
}

// rounds inside ONE workgroup: the round boundary is a __syncthreads().  Runs while 0 < frontier <= wg_frontier; returns with the control block
// describing the state it stopped in (frontier empty: done; larger than wg_frontier, or ctrl->bail — a round too heavy for one workgroup —:
// the grid-wide kernels go on).  color[], cnt[], the slab and the two frontier buffers stay in global memory and are read with loads that
// bypass the vector cache; the counters and the short rows' bitmaps live in LDS.
__global__ __launch_bounds__(kTailThreads) void k_color_tail(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                             const int32_t *__restrict__ pred, int32_t *__restrict__ color,
                                                             int32_t *__restrict__ round_of, int32_t *__restrict__ cnt, int32_t *__restrict__ f0,
                                                             int32_t *__restrict__ f1, uint32_t *__restrict__ slab, unsigned long long slab_cap,
                                                             int32_t wg_frontier, ColorCtrl *__restrict__ ctrl) {
    __shared__ int32_t s_count, s_next, s_error, s_flag, s_nlong, s_nlong_seen, s_best, s_top;
    __shared__ unsigned long long s_work;
    __shared__ int32_t s_long[kTailLong];
    __shared__ unsigned long long s_long_slab[kTailLong];
    __shared__ uint32_t s_bits[kTailThreads / kGroup][kBitWords];
    const int tid = threadIdx.x, lane = tid & (kGroup - 1), group = tid / kGroup;
    constexpr int groups = kTailThreads / kGroup;
    uint32_t *bits = s_bits[group];
    int32_t round = ctrl->round, colored = ctrl->colored, curi = ctrl->cur, bail = 0;
    if (tid == 0) {
        s_count = ctrl->count;
        s_next = 0;
        s_error = 0;
        s_flag = 0;
        s_nlong = 0;
        s_nlong_seen = 0;
        s_work = 0;
        s_top = 0;
    }
    __syncthreads();
    for (;;) {
        const int32_t count = s_count;
        if (count == 0 || count > wg_frontier) break;
        const int32_t *cur = curi ? f1 : f0;
        int32_t *next = curi ? f0 : f1;
        // what the round would cost here (core.hip's rule): one workgroup takes it only if no row is above kWgRowMax, its long rows fit the
        // list and all its rows together hold at most kWgWorkMax entries — else every other CU would idle behind this one
        unsigned long long work = 0;
        int32_t nl = 0;
        for (int32_t i = tid; i < count; i += kTailThreads) {
            const int32_t x = load_now(&cur[i]);
            const int64_t len = off[x + 1] - off[x];
            if (len > kWgRowMax) s_flag = 1;
            if (len > kLongRow) ++nl;
            work += (unsigned long long)len;
        }
        if (work) atomicAdd(&s_work, work);
        if (nl) atomicAdd(&s_nlong_seen, nl);
        __syncthreads();
        if (s_flag || s_nlong_seen > kTailLong || s_work > (unsigned long long)kWgWorkMax) {
            bail = 1;
            break;
        }
        int32_t top = 0;
        for (int32_t i = group; i < count; i += groups) {
            const int32_t x = load_now(&cur[i]);
            const int64_t j0 = off[x], j1 = off[x + 1];
            const int32_t p = pred[x];
            if (j1 - j0 > kLongRow) {
                if (lane == 0) {  // at most kTailLong of them: checked above
                    const unsigned long long words = (unsigned long long)(p / 32 + 1);
                    const int32_t pos = atomicAdd(&s_nlong, 1);
                    const unsigned long long at = atomicAdd(&ctrl->slab_used, words);
                    if (pos < kTailLong && at + words <= slab_cap) {
                        s_long[pos] = x;
                        s_long_slab[pos] = at;
                    } else {
                        s_error = 1;
                    }
                }
                continue;
            }
            const int32_t c = color_short_row(j0, j1, p, lane, bits, adj, color, cnt, next, &s_next, n, &s_error);
            if (lane == 0) {
                if (c == 0) s_error = 1;
                store_now(&color[x], c);
                round_of[x] = round;
                top = max(top, c);
            }
        }
        if (top) atomicMax(&s_top, top);
        __syncthreads();
        const int32_t nlong = s_error ? 0 : min(s_nlong, kTailLong);
        __syncthreads();  // every thread has read s_error before the walk may set it: the loops below hold barriers, their trip count must be uniform
        for (int32_t i = 0; i < nlong; ++i) {
            const int32_t x = s_long[i];
            color_long_walk(off[x], off[x + 1], pred[x], tid, kTailThreads, slab + s_long_slab[i], adj, color, cnt, next, &s_next, n, &s_error);
        }
        __syncthreads();
        for (int32_t i = 0; i < nlong; ++i) {
            const int32_t x = s_long[i];
            const int32_t p = pred[x];
            const int32_t best = first_free_long(slab + s_long_slab[i], p, tid, kTailThreads, &s_best);
            if (tid == 0) {
                if (best > p) s_error = 1;
                const int32_t c = best > p ? 0 : best + 1;
                store_now(&color[x], c);
                round_of[x] = round;
                if (c > s_top) s_top = c;
            }
        }
        __syncthreads();
        colored += count;
        round += 1;
        curi ^= 1;
        if (tid == 0) {
            s_count = s_error ? 0 : min(s_next, int32_t(min(n, int64_t(INT_MAX))));
            s_next = 0;
            s_nlong = 0;
            s_nlong_seen = 0;
            s_work = 0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        ctrl->count = s_count;
        ctrl->next = 0;
        ctrl->nlong = 0;
        ctrl->round = round;
        ctrl->colored = colored;
        ctrl->cur = curi;
        ctrl->bail = bail;
        if (s_top > ctrl->colors) ctrl->colors = s_top;
        if (s_error) ctrl->error = 1;
    }
}

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
                const int64_t pos = int64_t(atomicAdd(&ctl[0], 1));
                if (pos < long_cap) longs[pos] = int32_t(v);
                else ctl[1] = 1;
            }
            continue;
        }
        for (int64_t j = j0 + lane; j < j1; j += kGroup) arcs += color[adj[j]] == c ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        arcs += __shfl_down(arcs, o);
        invalid += __shfl_down(invalid, o);
        mx = max(mx, (unsigned long long)__shfl_down((long long)mx, o));
        deg = max(deg, (unsigned long long)__shfl_down((long long)deg, o));
    }
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
    for (int o = 32; o > 0; o >>= 1) arcs += __shfl_down(arcs, o);
    if ((threadIdx.x & 63) == 0 && arcs) atomicAdd(&acc[kAccArcs], arcs);
}
__global__ __launch_bounds__(256) void k_cv_distinct(int64_t words, const uint32_t *__restrict__ present, unsigned long long *__restrict__ acc) {
    unsigned long long c = 0;
    for (int64_t w = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < words; w += int64_t(gridDim.x) * blockDim.x) c += __popc(present[w]);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&acc[kAccDistinct], c);
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_coloring_jp(const gmsx_graph *g, const int32_t *ordering, int rank_format, int32_t *coloring, int32_t *round_of, gmsx_coloring_info *info,
                     gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int64_t n = g->n;
        gmsx_coloring_info res;
        std::memset(&res, 0, sizeof res);
        if (n == 0) {
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        const unsigned tb = unsigned((n + 255) / 256);
        const int64_t long_cap = std::min<int64_t>(n, g->nnz / kLongRow + 1);
        // every long row is parked once in the whole run and takes pred/32 + 1 <= degree/32 + 1 words
        const unsigned long long slab_cap = (unsigned long long)(g->nnz / 32 + long_cap);
        DevBuf d_in, d_rank, d_seen, d_cnt, d_pred, d_color, d_round, d_f0, d_f1, d_long, d_long_slab, d_slab, d_ctl, d_ctrl;
        if (int rc = dalloc<int32_t>(d_in, n)) return rc;
        if (int rc = dalloc<int32_t>(d_cnt, n)) return rc;
        if (int rc = dalloc<int32_t>(d_pred, n)) return rc;
        if (int rc = dalloc<int32_t>(d_color, n)) return rc;
        if (int rc = dalloc<int32_t>(d_round, n)) return rc;
        if (int rc = dalloc<int32_t>(d_f0, n)) return rc;
        if (int rc = dalloc<int32_t>(d_f1, n)) return rc;
        if (int rc = dalloc<int32_t>(d_long, long_cap)) return rc;
        if (int rc = dalloc<unsigned long long>(d_long_slab, long_cap)) return rc;
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
        int32_t *f[2] = {d_f0.as<int32_t>(), d_f1.as<int32_t>()};
        uint32_t *slab = d_slab.as<uint32_t>();
        long long wg_frontier = opt_int("COLOR_WG_FRONTIER", kWgFrontierDefault);  // test hook: 0 = every round a kernel boundary
        wg_frontier = std::max<long long>(0, std::min<long long>(wg_frontier, INT_MAX));

        GMSX_HIP(hipMemsetAsync(d_ctl.p, 0, 4 * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(ColorCtrl), s));
        GMSX_HIP(hipMemsetAsync(color, 0, size_t(n) * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(slab, 0, size_t(std::max<unsigned long long>(slab_cap, 1)) * sizeof(uint32_t), s));
        int launches = 0;
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
            hipLaunchKernelGGL(k_color_iota, dim3(tb), dim3(256), 0, s, n, rank);
        }
        const unsigned lb = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
        const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
        const unsigned long_grid = unsigned(cus) * 4;
        hipLaunchKernelGGL(k_oq_later, dim3(lb), dim3(256), 0, s, n, g->off, g->adj, rank, cnt, d_long.as<int32_t>(), long_cap, d_ctl.as<int32_t>());
        hipLaunchKernelGGL(k_oq_later_long, dim3(long_grid), dim3(256), 0, s, g->off, g->adj, rank, cnt, d_long.as<int32_t>(), long_cap,
                           d_ctl.as<int32_t>());
        hipLaunchKernelGGL(k_color_select, dim3(sweep), dim3(256), 0, s, n, cnt, pred, ctrl, f[0]);
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
        while (h.count > 0) {
            if (h.count <= wg_frontier && !h.bail) {
                hipLaunchKernelGGL(k_color_tail, dim3(1), dim3(kTailThreads), 0, s, n, g->off, g->adj, pred, color, rnd, cnt, f[0], f[1], slab, slab_cap,
                                   int32_t(wg_frontier), ctrl);
                launches += 1;
            } else {
                const unsigned rb = unsigned(std::min<int64_t>((int64_t(h.count) * kGroup + 255) / 256, int64_t(cus) * 32));
                hipLaunchKernelGGL(k_color_round, dim3(rb), dim3(256), 0, s, n, g->off, g->adj, pred, color, rnd, cnt, f[h.cur], f[h.cur ^ 1],
                                   d_long.as<int32_t>(), d_long_slab.as<unsigned long long>(), long_cap, slab_cap, ctrl);
                hipLaunchKernelGGL(k_color_round_long, dim3(long_grid), dim3(256), 0, s, n, g->off, g->adj, pred, color, cnt, f[h.cur ^ 1],
                                   d_long.as<int32_t>(), d_long_slab.as<unsigned long long>(), long_cap, slab, ctrl);
                hipLaunchKernelGGL(k_color_pick_advance, dim3(1), dim3(kTailThreads), 0, s, pred, color, rnd, d_long.as<int32_t>(),
                                   d_long_slab.as<unsigned long long>(), long_cap, slab, ctrl);
                launches += 3;
                if (h.bail) {
                    h.bail = 0;
                    GMSX_HIP(hipMemsetAsync(&ctrl->bail, 0, sizeof(int32_t), s));
                }
            }
            const int32_t colored_was = h.colored, round_was = h.round;
            GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            if (h.error || h.count < 0 || h.colored > n || h.count > n - h.colored) return GMSX_ERR_KERNEL;
            if (!h.bail && (h.colored <= colored_was || h.round <= round_was)) return GMSX_ERR_KERNEL;  // a step that made no progress
        }
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (h.colored != n || h.colors < 1 || h.colors > h.max_pred + 1 || h.slab_used > slab_cap) return GMSX_ERR_KERNEL;
        res.colors = h.colors;
        res.rounds = h.round;
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
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        const int64_t long_cap = std::min<int64_t>(n, g->nnz / kLongRow + 1);
        const int64_t words = n / 32 + 1;  // colours 0..n
        DevBuf d_color, d_present, d_long, d_ctl, d_acc;
        if (int rc = dalloc<int32_t>(d_color, n)) return rc;
        if (int rc = dalloc<uint32_t>(d_present, words)) return rc;
        if (int rc = dalloc<int32_t>(d_long, long_cap)) return rc;
        if (int rc = dalloc<int32_t>(d_ctl, 4)) return rc;
        if (int rc = dalloc<unsigned long long>(d_acc, 8)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_color.p, coloring, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        GMSX_HIP(hipMemsetAsync(d_present.p, 0, size_t(words) * sizeof(uint32_t), s));
        GMSX_HIP(hipMemsetAsync(d_ctl.p, 0, 4 * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(d_acc.p, 0, 8 * sizeof(unsigned long long), s));
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        const unsigned lb = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
        const unsigned sweep = unsigned(std::min<int64_t>((words + 255) / 256, int64_t(cus) * 16));
        hipLaunchKernelGGL(k_cv_rows, dim3(lb), dim3(256), 0, s, n, g->off, g->adj, d_color.as<int32_t>(), d_present.as<uint32_t>(), d_long.as<int32_t>(),
                           long_cap, d_ctl.as<int32_t>(), d_acc.as<unsigned long long>());
        hipLaunchKernelGGL(k_cv_long, dim3(unsigned(cus) * 4), dim3(256), 0, s, g->off, g->adj, d_color.as<int32_t>(), d_long.as<int32_t>(), long_cap,
                           d_ctl.as<int32_t>(), d_acc.as<unsigned long long>());
        hipLaunchKernelGGL(k_cv_distinct, dim3(sweep), dim3(256), 0, s, words, d_present.as<uint32_t>(), d_acc.as<unsigned long long>());
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int32_t ctl[4] = {0, 0, 0, 0};
        GMSX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (ctl[1] || (acc[kAccArcs] & 1ull)) return GMSX_ERR_KERNEL;  // (the CSR is symmetric: every equal pair is met from both ends)
        // the colours the bitmap does not cover — negative, or above n — are counted here; a colouring of any algorithm has none
        std::vector<int32_t> outliers;
        for (int64_t v = 0; v < n; ++v)
            if (coloring[v] < 0 || int64_t(coloring[v]) > n) outliers.push_back(coloring[v]);
        std::sort(outliers.begin(), outliers.end());
        const int64_t extra = int64_t(std::unique(outliers.begin(), outliers.end()) - outliers.begin());
        float ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
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
