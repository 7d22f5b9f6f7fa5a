// Batched multi-source breadth-first search on gfx950, over the uploaded CSR: gmsx_bfs_multi (the definitions are those of include/gmsx.h).
// Bit-parallel: W 64-bit words per vertex, one bit per source of the pass, so one sweep of the CSR advances 64 W traversals at once.  Per vertex
//   seen   the sources that have reached it
//   front  … that reached it at the last level (zero outside the active list)
//   next   … that reach it at this level
// `all` is the mask of the pass's live bits (the last pass is partial).  Every output is an exact integer, or a double the HOST computes from exact
// integers in a fixed order; the only atomics on the words are integer ORs of the push, so arrival order reaches no output.
//
// PULL LEVEL (k_ms_pull, k_ms_pull_rows): one owner per vertex, no atomic on the words.  v with need = all & ~seen[v] != 0 ORs front[u] over its
// row and stops as soon as (acc & need) == need.  A lane per row of at most kLaneRow entries; a longer row is appended to a list and walked by a
// kGroup-lane group (a wave above kLongRow) chunk by chunk, the lanes' words OR-combined by a fixed butterfly, out at the first chunk whose ballot
// says the row is complete.  No lane walks a long row alone, every loop is bounded by the row length.  k_ms_pull stores next[v] for EVERY v, so a
// pull needs no cleared array; it leaves the old front behind in the array that becomes `next` (the host clears it before a push).
//
// PUSH LEVEL (k_ms_push, k_ms_push_long, k_ms_finish): for x in the active list and w in N(x): m = front[x] & ~seen[w]; old = atomicOr(&next[w],
// m), and the thread that saw old == 0 appends the word to the touched list (bounded by n W).  seen is constant during the push.  Rows above
// kLongRow are parked and cut across all waves.  Then `next` IS the new front: k_ms_finish gives every touched vertex ONE owner (the entry of its
// lowest non-zero word), which does what the pull does per vertex, and clears the old front over the old active list.
//
// ACCOUNTING (ms_account, in the pull kernels, in k_ms_finish and in the seeding of level 0): per vertex dist_sum += level * popcount(new),
// reach += popcount(new), far = max(far, level) — one writer, plain stores.  Per source: a wave whose lanes hold new bits walks those lanes (at
// most 64 turns, none for a wave with nothing new); in every turn lane b of word k looks at bit 64 k + b of the broadcast words and keeps the
// count and the degree sum of its source in registers across its grid-stride loop — the transposition the bit-wise ballots would give, but with the
// owner's degree at hand — and adds them with one integer atomic per lane per wave at the end of the kernel.  The host reads the 64 W counter
// pairs once per level: termination, reached, depth_sum, reached_arcs, levels and the harmonic sum come from them.  The vertex is appended to the
// next active list and its degree added to a 64-bit sum: the operand of the direction rule (push when that sum <= nnz / MSBFS_ALPHA).
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

using u64 = unsigned long long;

constexpr long long kMsAlphaDefault = 15;  // a first guess, not a tuned value (gmsx.h, OPTIONS)
constexpr int kLaneRow = 16;               // longest row a single lane ORs in the pull
constexpr int kMsMaxWords = 2;

// control block of one level (device, zeroed before every level, read back whole behind it)
struct MsCtrl {
    int32_t error;
    int32_t act;      // vertices appended to the next active list
    int32_t touched;  // push: words that went from zero to non-zero
    int32_t rows;     // pull: rows left to the groups and waves
    int32_t nlong;    // push: parked rows
    int32_t reserved;
    u64 act_deg;      // degrees of the next active list
    u64 pairs[64 * kMsMaxWords][2];  // per source of the pass: vertices it reached at this level, their degrees
};

// what the final pass over the per-vertex arrays adds up
struct MsSums {
    u64 reach_sum;
    int32_t max_far, error;
};

template <int W>
struct MsArgs {
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    u64 *seen, *front, *next;
    int64_t *dist_sum;
    int32_t *reach, *far;
    int32_t *depth;  // 64 W rows of n, or nullptr
    int32_t *act_next;
    MsCtrl *ctrl;
    u64 all[W];
    int32_t level;
};

// the registers a lane keeps across its loop: bit `lane` of every word
template <int W>
struct MsRegs {
    u64 cnt[W], arcs[W], act_deg;
    __device__ __forceinline__ MsRegs() : act_deg(0) {
        for (int k = 0; k < W; ++k) cnt[k] = arcs[k] = 0;
    }
};

// Every lane of a CONVERGED wave calls this; nw = the new bits of vertex v (all zero: nothing to do for this lane), deg = v's degree.
template <int W>
__device__ __forceinline__ void ms_account(const MsArgs<W> &a, MsRegs<W> &r, int64_t v, const u64 (&nw)[W], int64_t deg) {
    u64 any = 0;
    for (int k = 0; k < W; ++k) any |= nw[k];
    u64 todo = __ballot(any != 0);
    if (todo == 0) return;
    const int lane = threadIdx.x & 63;
    if (any) {
        int pc = 0;
        for (int k = 0; k < W; ++k) pc += __popcll(nw[k]);
        a.dist_sum[v] += int64_t(a.level) * pc;
        a.reach[v] += pc;
        a.far[v] = max(a.far[v], a.level);
        if (a.depth) {
            for (int k = 0; k < W; ++k) {
                u64 bits = nw[k];
                while (bits) {  // at most 64 turns
                    const int b = __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    a.depth[int64_t(k * 64 + b) * a.n + v] = a.level;
                }
            }
        }
    }
    wave_append(any != 0, int32_t(v), a.act_next, &a.ctrl->act, a.n, &a.ctrl->error);
    while (todo) {  // at most 64 turns: one per lane that holds new bits
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const u64 dl = u64(__shfl((long long)deg, l));
        for (int k = 0; k < W; ++k) {
            const u64 w = __shfl(nw[k], l);
            if ((w >> lane) & 1ull) {
                ++r.cnt[k];
                r.arcs[k] += dl;
            }
        }
        r.act_deg += dl;  // (the same in every lane; lane 0 adds it)
    }
}

// … and at the end of the kernel: one integer atomic per lane and word that counted something
template <int W>
__device__ __forceinline__ void ms_flush(const MsArgs<W> &a, const MsRegs<W> &r) {
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < W; ++k)
        if (r.cnt[k]) {
            atomicAdd(&a.ctrl->pairs[k * 64 + lane][0], r.cnt[k]);
            atomicAdd(&a.ctrl->pairs[k * 64 + lane][1], r.arcs[k]);
        }
    if (lane == 0 && r.act_deg) atomicAdd(&a.ctrl->act_deg, r.act_deg);
}

// level 0 of a pass: ONE workgroup of 64 W threads, thread i owns source i of the pass.  The first occurrence of a vertex in the list owns the
// vertex and sets the bits of every occurrence (a source listed twice is two rows); seen, front and next were zeroed by the host.
template <int W>
__global__ __launch_bounds__(64 * W) void k_ms_seed(MsArgs<W> a, const int32_t *__restrict__ src, int32_t count) {
    const int i = threadIdx.x;
    MsRegs<W> r;
    u64 nw[W];
    for (int k = 0; k < W; ++k) nw[k] = 0;
    int64_t v = 0, deg = 0;
    if (i < count) {
        const int32_t s = src[i];
        bool first = true;
        for (int j = 0; j < count; ++j) {
            if (src[j] != s) continue;
            if (j < i) first = false;
            nw[j >> 6] |= 1ull << (j & 63);
        }
        if (first) {
            v = s;
            deg = a.off[s + 1] - a.off[s];
            for (int k = 0; k < W; ++k) a.seen[int64_t(s) * W + k] = a.front[int64_t(s) * W + k] = nw[k];
        } else {
            for (int k = 0; k < W; ++k) nw[k] = 0;
        }
    }
    ms_account<W>(a, r, v, nw, deg);
    ms_flush<W>(a, r);
}

// pull, pass 1: a lane per vertex; rows above kLaneRow go to the list
template <int W>
__global__ __launch_bounds__(256) void k_ms_pull(MsArgs<W> a, int32_t *__restrict__ rows) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((a.n + 63) / 64) * 64;  // whole waves stay converged for the ballots
    MsRegs<W> r;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        u64 nw[W];
        for (int k = 0; k < W; ++k) nw[k] = 0;
        int64_t deg = 0;
        bool more = false;
        if (v < a.n) {
            u64 need[W], rest = 0;
            for (int k = 0; k < W; ++k) {
                need[k] = a.all[k] & ~a.seen[v * W + k];
                rest |= need[k];
            }
            if (rest) {
                const int64_t j0 = a.off[v], j1 = a.off[v + 1];
                deg = j1 - j0;
                if (deg > kLaneRow) {
                    more = true;
                } else {
                    u64 acc[W];
                    for (int k = 0; k < W; ++k) acc[k] = 0;
                    for (int64_t j = j0; j < j1; ++j) {
                        const int64_t u = a.adj[j];
                        rest = 0;
                        for (int k = 0; k < W; ++k) {
                            acc[k] |= a.front[u * W + k];
                            rest |= need[k] & ~acc[k];
                        }
                        if (!rest) break;
                    }
                    for (int k = 0; k < W; ++k) {
                        nw[k] = acc[k] & need[k];
                        if (nw[k]) a.seen[v * W + k] |= nw[k];
                    }
                }
            }
            for (int k = 0; k < W; ++k) a.next[v * W + k] = nw[k];
        }
        wave_append(more, int32_t(v), rows, &a.ctrl->rows, a.n, &a.ctrl->error);
        ms_account<W>(a, r, v, nw, deg);
    }
    ms_flush<W>(a, r);
}

// pull, pass 2: the listed rows, WIDTH lanes per row (kGroup: rows up to kLongRow; 64: the longer ones); per chunk of WIDTH entries the lanes'
// words are OR-combined by a butterfly, and a ballot tells the group whether the row is complete
template <int W, int WIDTH>
__global__ __launch_bounds__(256) void k_ms_pull_rows(MsArgs<W> a, const int32_t *__restrict__ rows) {
    constexpr int kPerWave = 64 / WIDTH;
    const RowGroup<WIDTH> grp;
    const int wl = threadIdx.x & 63, lane = grp.lane;
    const int64_t wave0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const int64_t count = min(int64_t(a.ctrl->rows), a.n);
    MsRegs<W> r;
    for (int64_t base = wave0 * kPerWave; base < count; base += waves * kPerWave) {  // (uniform in the wave)
        const int64_t i = base + wl / WIDTH;
        u64 nw[W];
        for (int k = 0; k < W; ++k) nw[k] = 0;
        int64_t v = 0, deg = 0;
        if (i < count) {
            v = rows[i];
            const int64_t j0 = a.off[v], j1 = a.off[v + 1];
            if ((j1 - j0 > kLongRow) == (WIDTH == 64)) {
                u64 need[W], acc[W];
                for (int k = 0; k < W; ++k) {
                    need[k] = a.all[k] & ~a.seen[v * W + k];
                    acc[k] = 0;
                }
                for (int64_t c = j0; c < j1; c += WIDTH) {  // (uniform in the group: its lanes leave together)
                    const int64_t j = c + lane;
                    if (j < j1) {
                        const int64_t u = a.adj[j];
                        for (int k = 0; k < W; ++k) acc[k] |= a.front[u * W + k];
                    }
                    u64 rest = 0;
                    for (int k = 0; k < W; ++k) {
                        acc[k] = wave_or_all<WIDTH>(acc[k]);
                        rest |= need[k] & ~acc[k];
                    }
                    if (grp.ballot(rest == 0) & 1ull) break;
                }
                if (lane == 0) {
                    deg = j1 - j0;
                    for (int k = 0; k < W; ++k) {
                        nw[k] = acc[k] & need[k];
                        if (nw[k]) {
                            a.next[v * W + k] = nw[k];
                            a.seen[v * W + k] |= nw[k];
                        }
                    }
                }
            }
        }
        ms_account<W>(a, r, v, nw, deg);
    }
    ms_flush<W>(a, r);
}

// what entry w of x's row gets in the push
template <int W>
__device__ __forceinline__ void ms_push_visit(const MsArgs<W> &a, const u64 (&fx)[W], int64_t w, int32_t *touched, int64_t tcap) {
    for (int k = 0; k < W; ++k) {
        const u64 m = fx[k] & ~a.seen[w * W + k];
        if (!m) continue;
        u64 *p = &a.next[w * W + k];
        if ((__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) == m) continue;  // (someone brought these bits already)
        if (atomicOr(p, m) == 0) append_checked(touched, &a.ctrl->touched, tcap, int32_t(w * W + k), &a.ctrl->error);
    }
}

// push: a kGroup-lane group per active vertex; rows above kLongRow are parked
template <int W>
__global__ __launch_bounds__(256) void k_ms_push(MsArgs<W> a, const int32_t *__restrict__ act, int32_t count, int32_t *__restrict__ touched,
                                                 int64_t tcap, int32_t *__restrict__ longs, int64_t long_cap) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    for (int64_t i = group0; i < count; i += groups) {
        const int64_t x = act[i];
        const int64_t j0 = a.off[x], j1 = a.off[x + 1];
        if (j1 - j0 > kLongRow) {
            if (lane == 0) append_checked(longs, &a.ctrl->nlong, long_cap, int32_t(x), &a.ctrl->error);
            continue;
        }
        u64 fx[W];
        for (int k = 0; k < W; ++k) fx[k] = a.front[x * W + k];
        for (int64_t j = j0 + lane; j < j1; j += kGroup) ms_push_visit<W>(a, fx, a.adj[j], touched, tcap);
    }
}

// … its parked rows: every one cut across all the waves of the grid
template <int W>
__global__ __launch_bounds__(256) void k_ms_push_long(MsArgs<W> a, int32_t *__restrict__ touched, int64_t tcap, const int32_t *__restrict__ longs,
                                                      int64_t long_cap) {
    const int64_t nlong = min(int64_t(a.ctrl->nlong), long_cap);
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, threads = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = 0; i < nlong; ++i) {
        const int64_t x = longs[i];
        u64 fx[W];
        for (int k = 0; k < W; ++k) fx[k] = a.front[x * W + k];
        const int64_t j1 = a.off[x + 1];
        for (int64_t j = a.off[x] + tid; j < j1; j += threads) ms_push_visit<W>(a, fx, a.adj[j], touched, tcap);
    }
}

// behind a push (a.front = the array the push ORed into, a.next = the front it read): the touched vertices get their owner — the entry of the
// vertex's lowest non-zero word — and the old front is cleared over the old active list
template <int W>
__global__ __launch_bounds__(256) void k_ms_finish(MsArgs<W> a, const int32_t *__restrict__ act, int32_t count, const int32_t *__restrict__ touched,
                                                   int64_t tcap) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t nt = min(int64_t(a.ctrl->touched), tcap);
    const int64_t end = ((max(nt, int64_t(count)) + 63) / 64) * 64;
    MsRegs<W> r;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < end; i += stride) {
        if (i < count) {
            const int64_t x = act[i];
            for (int k = 0; k < W; ++k) a.next[x * W + k] = 0;
        }
        u64 nw[W];
        for (int k = 0; k < W; ++k) nw[k] = 0;
        int64_t v = 0, deg = 0;
        if (i < nt) {
            const int64_t e = touched[i];
            v = e / W;
            const int k0 = int(e % W);
            bool owner = true;
            for (int k = 0; k < W; ++k) {
                nw[k] = a.front[v * W + k];
                if (k < k0 && nw[k]) owner = false;
            }
            if (owner) {
                deg = a.off[v + 1] - a.off[v];
                for (int k = 0; k < W; ++k)
                    if (nw[k]) a.seen[v * W + k] |= nw[k];
            } else {
                for (int k = 0; k < W; ++k) nw[k] = 0;
            }
        }
        ms_account<W>(a, r, v, nw, deg);
    }
    ms_flush<W>(a, r);
}

__global__ __launch_bounds__(256) void k_ms_vertex_init(int64_t n, int64_t *__restrict__ dist_sum, int32_t *__restrict__ reach, int32_t *__restrict__ far) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    dist_sum[v] = 0;
    reach[v] = 0;
    far[v] = -1;
}

// the sum of reach[] (against the sum of the sources' reached) and the largest far[]
__global__ __launch_bounds__(256) void k_ms_sums(int64_t n, const int32_t *__restrict__ reach, const int32_t *__restrict__ far, MsSums *__restrict__ out) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    u64 sum = 0;
    int32_t mx = -1;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t rv = reach[v], fv = far[v];
        if (rv < 0 || fv < -1 || (rv == 0) != (fv == -1)) out->error = 1;
        sum += u64(max(rv, 0));
        mx = max(mx, fv);
    }
    sum = wave_sum(sum);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&out->reach_sum, sum);
        atomicMax(&out->max_far, mx);
    }
}

// ---- the host ------------------------------------------------------------------------------------------------------------------------------

struct MsOptions {
    long long direction, alpha, words;
};

MsOptions ms_options() {
    MsOptions o;
    o.direction = opt_int("MSBFS_DIRECTION", 0);
    if (o.direction < 0 || o.direction > 2) o.direction = 0;
    o.alpha = std::max<long long>(1, std::min<long long>(opt_int("MSBFS_ALPHA", kMsAlphaDefault), INT_MAX));
    o.words = opt_int("MSBFS_WORDS", 0);  // 0: by the length of the source list (gmsx_bfs_multi)
    if (o.words != 1 && o.words != 2) o.words = 0;
    return o;
}

struct MsBufs {
    DevBuf words, dist_sum, reach, far, depth, act0, act1, rows, touched, longs, src, ctrl, sums;
    int64_t long_cap = 0, tcap = 0;
};

struct MsTotals {
    int64_t passes = 0, push_levels = 0, pull_levels = 0;
    uint64_t level_sum = 0;
    int launches = 0;
};

// The passes of one call, n > 0 and n_sources > 0, every id in range: per_source complete, the per-vertex arrays on the device, h_depth filled
// pass by pass when wanted.
template <int W>
int ms_run(const gmsx_graph *g, int64_t n_sources, const MsOptions &o, const MsBufs &b, std::vector<gmsx_bfs_source> &per_source,
           std::vector<int32_t> *h_depth, MsTotals &t) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    const unsigned group_grid = unsigned(cus) * 8;
    const bool has_long = g->max_deg > kLongRow;
    const bool timing = opt_on("TIMING");  // one line per level on stderr: its direction and what the rule weighed
    constexpr int kBits = 64 * W;
    MsCtrl *ctrl = b.ctrl.as<MsCtrl>();
    u64 *words = b.words.as<u64>();
    int32_t *act[2] = {b.act0.as<int32_t>(), b.act1.as<int32_t>()};
    MsArgs<W> a;
    a.n = n;
    a.off = g->off;
    a.adj = g->adj;
    a.dist_sum = b.dist_sum.as<int64_t>();
    a.reach = b.reach.as<int32_t>();
    a.far = b.far.as<int32_t>();
    a.depth = h_depth ? b.depth.as<int32_t>() : nullptr;
    a.ctrl = ctrl;
    MsCtrl h;
    for (int64_t base = 0; base < n_sources; base += kBits) {
        const int32_t count = int32_t(std::min<int64_t>(kBits, n_sources - base));
        for (int k = 0; k < W; ++k) {
            const int live = std::max(0, std::min(64, count - 64 * k));
            a.all[k] = live == 64 ? ~0ull : ((1ull << live) - 1ull);
        }
        a.seen = words;
        a.front = words + n * W;
        a.next = words + 2 * n * W;
        GMSX_HIP(hipMemsetAsync(words, 0, size_t(3 * n * W) * sizeof(u64), s));
        if (a.depth) GMSX_HIP(hipMemsetAsync(a.depth, 0xff, size_t(kBits) * size_t(n) * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(MsCtrl), s));
        int cur = 0;
        a.level = 0;
        a.act_next = act[cur];
        hipLaunchKernelGGL(k_ms_seed<W>, dim3(1), dim3(kBits), 0, s, a, b.src.as<const int32_t>() + base, count);
        ++t.launches;
        bool next_dirty = false, pushed = false;
        int32_t pass_levels = 0;
        for (int32_t level = 0;; ++level) {
            // ---- behind level `level`: its counter pairs
            GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            if (h.error || h.act < 0 || h.act > n || h.touched < 0 || h.rows < 0 || h.rows > n || h.nlong < 0) return GMSX_ERR_KERNEL;
            uint64_t found = 0;
            for (int i = 0; i < count; ++i) {
                const uint64_t cnt = h.pairs[i][0], arcs = h.pairs[i][1];
                if (!cnt) continue;
                gmsx_bfs_source &ps = per_source[size_t(base + i)];
                if (ps.levels != level || cnt > uint64_t(n) || arcs > uint64_t(g->nnz)) return GMSX_ERR_KERNEL;  // (a source's levels have no gap)
                ps.reached += int64_t(cnt);
                ps.reached_arcs += int64_t(arcs);
                ps.depth_sum += int64_t(level) * int64_t(cnt);
                ps.levels = level + 1;
                if (level > 0) ps.harmonic += double(cnt) / double(level);
                found += cnt;
            }
            for (int i = count; i < kBits; ++i)
                if (h.pairs[i][0]) return GMSX_ERR_KERNEL;
            if ((found == 0) != (h.act == 0) || found < uint64_t(h.act)) return GMSX_ERR_KERNEL;
            if (level > 0 && found) {  // (the last level of a pass finds nothing and is not counted: Σ = the largest levels - 1)
                ++pass_levels;
                ++(pushed ? t.push_levels : t.pull_levels);
            }
            if (h.act == 0) break;
            if (int64_t(level) + 1 > n) return GMSX_ERR_KERNEL;
            // ---- level `level + 1`
            const bool push = o.direction == 1 || (o.direction == 0 && (long long)h.act_deg <= (long long)(g->nnz / o.alpha));
            const int32_t active = h.act;
            pushed = push;
            if (timing)
                std::fprintf(stderr, "msbfs pass %lld level %d: %s, %d active vertices, degree sum %llu of %lld arcs\n", (long long)t.passes, int(level) + 1,
                             push ? "push" : "pull", int(active), h.act_deg, (long long)g->nnz);
            GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(MsCtrl), s));
            a.level = level + 1;
            a.act_next = act[cur ^ 1];
            if (push) {
                if (next_dirty) {
                    GMSX_HIP(hipMemsetAsync(a.next, 0, size_t(n * W) * sizeof(u64), s));
                    next_dirty = false;
                }
                const unsigned pb = unsigned(std::min<int64_t>((int64_t(active) * kGroup + 255) / 256, int64_t(cus) * 32));
                hipLaunchKernelGGL(k_ms_push<W>, dim3(pb), dim3(256), 0, s, a, act[cur], active, b.touched.as<int32_t>(), b.tcap, b.longs.as<int32_t>(),
                                   b.long_cap);
                ++t.launches;
                if (has_long) {
                    hipLaunchKernelGGL(k_ms_push_long<W>, dim3(unsigned(cus) * 4), dim3(256), 0, s, a, b.touched.as<int32_t>(), b.tcap,
                                       b.longs.as<const int32_t>(), b.long_cap);
                    ++t.launches;
                }
                std::swap(a.front, a.next);
                hipLaunchKernelGGL(k_ms_finish<W>, dim3(sweep), dim3(256), 0, s, a, act[cur], active, b.touched.as<const int32_t>(), b.tcap);
                ++t.launches;
            } else {
                hipLaunchKernelGGL(k_ms_pull<W>, dim3(sweep), dim3(256), 0, s, a, b.rows.as<int32_t>());
                hipLaunchKernelGGL((k_ms_pull_rows<W, kGroup>), dim3(group_grid), dim3(256), 0, s, a, b.rows.as<const int32_t>());
                t.launches += 2;
                if (has_long) {
                    hipLaunchKernelGGL((k_ms_pull_rows<W, 64>), dim3(group_grid), dim3(256), 0, s, a, b.rows.as<const int32_t>());
                    ++t.launches;
                }
                std::swap(a.front, a.next);
                next_dirty = true;
            }
            cur ^= 1;
        }
        ++t.passes;
        t.level_sum += uint64_t(pass_levels) + 1;
        if (h_depth)
            GMSX_HIP(hipMemcpyAsync(h_depth->data() + size_t(base) * size_t(n), a.depth, size_t(count) * size_t(n) * sizeof(int32_t),
                                    hipMemcpyDeviceToHost, s));
    }
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_bfs_multi(const gmsx_graph *g, int64_t n_sources, const int32_t *sources, gmsx_bfs_source *per_source, int32_t *depth, int64_t *dist_sum,
                   int32_t *reach, int32_t *far, gmsx_bfs_multi_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || n_sources < 0 || (n_sources > 0 && !sources)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        for (int64_t i = 0; i < n_sources; ++i)
            if (sources[i] < 0 || int64_t(sources[i]) >= n) return GMSX_ERR_INVALID;
        gmsx_bfs_multi_info res;
        std::memset(&res, 0, sizeof res);
        if (n == 0 || n_sources == 0) {
            for (int64_t v = 0; v < n; ++v) {
                if (dist_sum) dist_sum[v] = 0;
                if (reach) reach[v] = 0;
                if (far) far[v] = -1;
            }
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        MsOptions o = ms_options();
        // measured: up to 64 sources the second word only costs (4 - 8 %); beyond, one pass of 16-byte words beats two passes of
        // 8-byte words (1.3 - 1.8 x)
        if (o.words == 0) o.words = n_sources > 64 ? 2 : 1;
        if (n * o.words > int64_t(INT_MAX)) o.words = 1;  // (the touched list names a word by a 32-bit index)
        const int64_t W = o.words;
        MsBufs b;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        b.long_cap = frontier_long_cap(n, g->nnz);
        b.tcap = n * W;
        if (int rc = dalloc<u64>(b.words, 3 * n * W)) return rc;
        if (int rc = dalloc<int64_t>(b.dist_sum, n)) return rc;
        if (int rc = dalloc<int32_t>(b.reach, n)) return rc;
        if (int rc = dalloc<int32_t>(b.far, n)) return rc;
        if (depth)
            if (int rc = dalloc<int32_t>(b.depth, 64 * W * n)) return rc;
        if (int rc = dalloc<int32_t>(b.act0, n)) return rc;
        if (int rc = dalloc<int32_t>(b.act1, n)) return rc;
        if (int rc = dalloc<int32_t>(b.rows, n)) return rc;
        if (int rc = dalloc<int32_t>(b.touched, b.tcap)) return rc;
        if (int rc = dalloc<int32_t>(b.longs, b.long_cap)) return rc;
        if (int rc = dalloc<int32_t>(b.src, n_sources)) return rc;
        if (int rc = dalloc<MsCtrl>(b.ctrl, 1)) return rc;
        if (int rc = dalloc<MsSums>(b.sums, 1)) return rc;
        GMSX_HIP(hipMemcpyAsync(b.src.p, sources, size_t(n_sources) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_ms_vertex_init, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, n, b.dist_sum.as<int64_t>(), b.reach.as<int32_t>(),
                           b.far.as<int32_t>());
        GMSX_HIP(hipMemsetAsync(b.sums.p, 0, sizeof(MsSums), s));
        GMSX_HIP(hipMemsetAsync(&b.sums.as<MsSums>()->max_far, 0xff, sizeof(int32_t), s));
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        std::vector<gmsx_bfs_source> ps;
        ps.resize(size_t(n_sources));
        std::memset(ps.data(), 0, ps.size() * sizeof(gmsx_bfs_source));
        std::vector<int32_t> h_depth;
        if (depth) h_depth.resize(size_t(n_sources) * size_t(n));
        MsTotals t;
        t.launches = 1;
        if (int rc = W == 2 ? ms_run<2>(g, n_sources, o, b, ps, depth ? &h_depth : nullptr, t)
                            : ms_run<1>(g, n_sources, o, b, ps, depth ? &h_depth : nullptr, t))
            return rc;
        hipLaunchKernelGGL(k_ms_sums, dim3(unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16))), dim3(256), 0, s, n,
                           b.reach.as<const int32_t>(), b.far.as<const int32_t>(), b.sums.as<MsSums>());
        ++t.launches;
        GMSX_HIP(hipEventRecord(c.ev[2], s));
        MsSums sums;
        GMSX_HIP(hipMemcpyAsync(&sums, b.sums.p, sizeof sums, hipMemcpyDeviceToHost, s));
        // the caller's arrays go through host staging and are written only after the flag words were read as zero
        std::vector<int64_t> h_dist;
        std::vector<int32_t> h_reach, h_far;
        if (dist_sum) {
            h_dist.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_dist.data(), b.dist_sum.p, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        }
        if (reach) {
            h_reach.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_reach.data(), b.reach.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (far) {
            h_far.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_far.data(), b.far.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        uint64_t arcs = 0;
        for (gmsx_bfs_source &x : ps) {
            if (x.reached < 1 || x.levels < 1 || int64_t(x.levels) > n) return GMSX_ERR_KERNEL;
            x.closeness = x.depth_sum ? double(x.reached - 1) / double(x.depth_sum) : 0.0;
            res.reached_total += x.reached;
            res.max_levels = std::max(res.max_levels, x.levels);
            arcs += uint64_t(x.reached_arcs);
        }
        if (sums.error || sums.reach_sum != uint64_t(res.reached_total) || sums.max_far != res.max_levels - 1) return GMSX_ERR_KERNEL;
        res.sources = n_sources;
        res.passes = t.passes;
        res.max_far = sums.max_far;
        res.push_levels = int32_t(t.push_levels);
        res.pull_levels = int32_t(t.pull_levels);
        float up_ms = 0.f, ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
        if (per_source) std::memcpy(per_source, ps.data(), ps.size() * sizeof(gmsx_bfs_source));
        if (depth) std::memcpy(depth, h_depth.data(), h_depth.size() * sizeof(int32_t));
        if (dist_sum) std::memcpy(dist_sum, h_dist.data(), size_t(n) * sizeof(int64_t));
        if (reach) std::memcpy(reach, h_reach.data(), size_t(n) * sizeof(int32_t));
        if (far) std::memcpy(far, h_far.data(), size_t(n) * sizeof(int32_t));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), double(up_ms), arcs, 0, t.level_sum, t.launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
