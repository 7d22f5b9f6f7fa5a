// 4-cycle counting and the 3- / 4-vertex motif census on gfx950.
//   gmsx_cycle4_count / gmsx_cycle4_partial   the 4-cycles of the uploaded graph (and, whole graph only, the 4-cycles through every vertex)
//   gmsx_motif_census4                        wedge, triangle, 3-star, 4-path, tailed triangle, 4-cycle, diamond, 4-clique: non-induced and induced
// No counterpart in the reference; the definitions are those of include/gmsx.h.  Every result is an exact integer and a fact about the graph.
//
// THE RULE.  In rank ids (decreasing (degree, id), rank 0 = the biggest hub; gmsx_graph::newid) every 4-cycle u - v - w - v' - u is counted once,
// at its vertex u of the SMALLEST rank id, against the opposite vertex w: for a source u, every neighbour v with rank(v) > rank(u) and every
// w in N(v) with rank(w) > rank(u) is one WEDGE (u, v, w) and one cnt[w]++; the cycles of u are Σ_w C(cnt[w], 2).  Neighbour ranks are newid[]
// lookups on the uploaded CSR (as k_oq_later reads its rank array): no call-local rank-id CSR is built, so at_vertex needs no translation and a
// call allocates nothing of the order of nnz.  A source with fewer than two later neighbours closes no cycle and is not walked at all.
//
// THREE WALKS over the same wedges of a source (c4_walk), a barrier or a kernel boundary between them:
//   1 count     cnt[w]++                                                  (no-return atomics)
//   2 middle    at_vertex[v] += Σ_w (cnt[w] - 1), one atomic per (u, v)   (only when the caller asked for at_vertex)
//   3 clean     old = exchange(cnt[w], 0); the ONE wedge per w that gets old != 0 harvests C(old, 2): into the call's cycles, and into
//               at_vertex[w] and at_vertex[u]
// The clean walk returns every counter to zero, so a span is zeroed exactly once, when it is allocated, and never by a memset between sources.
// Σ old over the harvests must equal the wedges the count walk added: a span that was not zero, or a walk that lost a wedge, makes the two sums
// differ and the call returns GMSX_ERR_KERNEL.  A counter index is checked against its span before it is used; a violation raises the flag word.
//
// WHERE THE COUNTERS LIVE.  The counter of w for source u is cnt[rank(w) - rank(u) - 1]: a dense span of n - rank(u) - 1 words, short for the
// many light sources at the end of the order, long for the hubs.  k_c4_classify computes per source the later neighbours and the wedge BOUND
// Σ_{later v} deg(v) (a sufficient upper bound of its wedges), k_c4_bin puts it on one of three lists:
//   LDS    span <= C4_LDS_SPAN (at most kC4LdsMax words of a workgroup's LDS): LDS atomics, one source per workgroup at a time (k_c4_block<true>)
//   slab   a span of n words per WORKGROUP in a global slab, global atomics; a workgroup keeps its span for all the sources it takes
//          (k_c4_block<false>).  C4_SLAB_MB bounds the slab: a smaller budget = fewer workgroups, never more launches
//   split  bound > C4_SPLIT_WEDGES: the source is walked by MANY workgroups into ONE global span of its own; the three walks are three launches
//          (k_c4_split<phase>), batched over as many such sources as fit the budget (launch_plan.hpp: task = source, slab = its span).  No
//          workgroup waits for another inside a kernel.
// Within a workgroup the later neighbours' rows are binned by the source's mean row length: a lane, a 16-lane group or a wave per row.
// Counters in global memory are read with agent-scope loads: the count walk's atomics land in L2, a plain load could be served from a stale
// line of the CU's L1.
//
// THE OTHER SEVEN COUNTS are integer identities over the degrees, the per-edge support (truss.hip's numbering and support pass, truss_edges.hpp)
// and the k = 4 clique count (kclique.hip).  The reductions keep 128-bit sums per wave (two 64-bit halves) and the host finishes in
// unsigned __int128, so the overflow answer is exact: C(d, 3) of one hub of 4.9 M neighbours alone passes 2^64.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // load_now, wave_append, kGroup, kLongRow
#include "launch_plan.hpp"
#include "truss_edges.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

constexpr int kC4LdsMax = 8192;  // counters of the LDS path: 32 KB of a workgroup's LDS
constexpr long long kC4LdsSpanDefault = kC4LdsMax, kC4SlabMbDefault = 1024, kC4SplitWedgesDefault = 1 << 18;  // first guesses (gmsx.h, OPTIONS)
constexpr int kC4BlocksPerCu = 8;
constexpr int64_t kC4SplitBatch = 32768;  // sources of one split launch (gridDim.y)

struct C4Graph {
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    const int32_t *newid;
};

// the call's small device block, zeroed per call
struct C4Acc {
    int32_t error;     // the flag word: a counter index outside its span, a list past its bound, a counter read as zero inside its own wedge
    int32_t max_cod;   // largest counter value harvested
    int32_t nlist[3];  // sources on the LDS / slab / split list
    int32_t pad[3];
    unsigned long long cycles, wedges, harvested;
};

// what a thread gathers over all the sources it works on
struct C4Thread {
    unsigned long long cycles = 0, wedges = 0, harvested = 0;
    uint32_t mx = 0;
};

template <bool LDS>
__device__ __forceinline__ uint32_t c4_read(const uint32_t *p) {
    if (LDS) return *p;
    return load_now(p);
}

// One of the three walks over the wedges of source u (rank ru, counters cnt[0 .. span)).  1 << wshift lanes share a later neighbour's row; the
// calling threads take the positions g0 + (thread >> wshift), + gstep, … of u's row.
template <bool LDS, int PHASE, bool AT>
__device__ __forceinline__ void c4_walk(const C4Graph &G, int32_t u, int32_t ru, int64_t span, int wshift, int64_t g0, int64_t gstep, uint32_t *cnt,
                                        unsigned long long *__restrict__ at, C4Thread &t, int32_t *error) {
    const int width = 1 << wshift, lane = int(threadIdx.x) & (width - 1);
    const int64_t j0 = G.off[u], d = G.off[u + 1] - j0;
    for (int64_t i = g0 + (int64_t(threadIdx.x) >> wshift); i < d; i += gstep) {
        const int32_t v = G.adj[j0 + i];
        if (G.newid[v] <= ru) continue;
        const int64_t k1 = G.off[v + 1];
        unsigned long long s = 0;
        for (int64_t k = G.off[v] + lane; k < k1; k += width) {
            const int32_t w = G.adj[k];
            const int64_t idx = int64_t(G.newid[w]) - ru - 1;
            if (idx < 0) continue;
            if (idx >= span) {
                *error = 1;
                continue;
            }
            if (PHASE == 1) {
                atomicAdd(&cnt[idx], 1u);
                ++t.wedges;
            } else if (PHASE == 2) {
                const uint32_t c = c4_read<LDS>(&cnt[idx]);
                if (c == 0) *error = 1;  // (this wedge itself was counted)
                else s += c - 1;
            } else {
                const uint32_t old = atomicExch(&cnt[idx], 0u);
                if (old) {
                    const unsigned long long pairs = (unsigned long long)old * (old - 1) / 2;
                    t.cycles += pairs;
                    t.harvested += old;
                    t.mx = max(t.mx, old);
                    if (AT && pairs) atomicAdd(&at[w], pairs);
                }
            }
        }
        if (PHASE == 2) {
            s = wave_sum(s, width);
            if (lane == 0 && s) atomicAdd(&at[v], s);
        }
    }
}

// the thread sums of a kernel into the call's block: one 64-bit atomic per wave and value
__device__ __forceinline__ void c4_flush(C4Thread t, C4Acc *__restrict__ acc) {
    t.cycles = wave_sum(t.cycles);
    t.wedges = wave_sum(t.wedges);
    t.harvested = wave_sum(t.harvested);
    t.mx = wave_max(t.mx);
    if ((threadIdx.x & 63) == 0) {
        if (t.cycles) atomicAdd(&acc->cycles, t.cycles);
        if (t.wedges) atomicAdd(&acc->wedges, t.wedges);
        if (t.harvested) atomicAdd(&acc->harvested, t.harvested);
        if (t.mx) atomicMax(&acc->max_cod, int32_t(min(t.mx, uint32_t(INT_MAX))));
    }
}

// at[u] += the pairs this source harvested (cycles before / after its clean walk): one atomic per wave
__device__ __forceinline__ void c4_source_share(unsigned long long pairs, int32_t u, unsigned long long *__restrict__ at) {
    pairs = wave_sum(pairs);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(&at[u], pairs);
}

// per source: later neighbours and the wedge bound Σ_{later v} deg(v).  A kGroup-lane group per row of at most kLongRow entries …
__global__ __launch_bounds__(256) void k_c4_classify(C4Graph G, int32_t *__restrict__ later, int64_t *__restrict__ bound) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    for (int64_t u = group0; u < G.n; u += groups) {
        const int64_t j0 = G.off[u], j1 = G.off[u + 1];
        if (j1 - j0 > kLongRow) continue;
        const int32_t ru = G.newid[u];
        int32_t l = 0;
        int64_t b = 0;
        for (int64_t j = j0 + lane; j < j1; j += kGroup) {
            const int32_t v = G.adj[j];
            if (G.newid[v] > ru) {
                ++l;
                b += G.off[v + 1] - G.off[v];
            }
        }
        l = wave_sum<kGroup>(l);
        b = wave_sum<kGroup>(b);
        if (lane == 0) {
            later[u] = l;
            bound[u] = b;
        }
    }
}

// … and a whole workgroup per longer row (every workgroup scans the degrees of its stripe of the vertices)
__global__ __launch_bounds__(256) void k_c4_classify_long(C4Graph G, int32_t *__restrict__ later, int64_t *__restrict__ bound) {
    __shared__ int32_t s_l[4];
    __shared__ int64_t s_b[4];
    for (int64_t u = blockIdx.x; u < G.n; u += gridDim.x) {
        const int64_t j0 = G.off[u], j1 = G.off[u + 1];
        if (j1 - j0 <= kLongRow) continue;
        const int32_t ru = G.newid[u];
        int32_t l = 0;
        int64_t b = 0;
        for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
            const int32_t v = G.adj[j];
            if (G.newid[v] > ru) {
                ++l;
                b += G.off[v + 1] - G.off[v];
            }
        }
        l = wave_sum(l);
        b = wave_sum(b);
        if ((threadIdx.x & 63) == 0) {
            s_l[threadIdx.x >> 6] = l;
            s_b[threadIdx.x >> 6] = b;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            later[u] = s_l[0] + s_l[1] + s_l[2] + s_l[3];
            bound[u] = s_b[0] + s_b[1] + s_b[2] + s_b[3];
        }
        __syncthreads();
    }
}

// the three lists (whole waves stay converged for the ballots) and the lanes per row of every source.  The split list carries the rank of
// its sources: the host plans their spans from it.
__global__ __launch_bounds__(256) void k_c4_bin(C4Graph G, const int32_t *__restrict__ later, const int64_t *__restrict__ bound, int64_t lds_span,
                                                int64_t split_wedges, int part, int nparts, int32_t *__restrict__ l_lds, int32_t *__restrict__ l_slab,
                                                int32_t *__restrict__ l_split, int32_t *__restrict__ split_rank, uint8_t *__restrict__ wcode,
                                                C4Acc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((G.n + 63) / 64) * 64;
    const int lane = threadIdx.x & 63;
    for (int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; u < end; u += stride) {
        int which = -1;
        int32_t ru = 0;
        if (u < G.n) {
            ru = G.newid[u];
            const int32_t l = later[u];
            const int64_t b = bound[u];
            if (l >= 2 && shard_of(ru, nparts) == part) {
                which = b > split_wedges ? 2 : (G.n - ru - 1 <= lds_span ? 0 : 1);
                const int64_t mean = b / l;  // entries of a later neighbour's row
                wcode[u] = uint8_t((mean <= 4 && l >= 64) ? 0 : mean <= 64 ? 4 : 6);
            }
        }
        wave_append(which == 0, int32_t(u), l_lds, &acc->nlist[0], G.n, &acc->error);
        wave_append(which == 1, int32_t(u), l_slab, &acc->nlist[1], G.n, &acc->error);
        // (the split list and its ranks share their positions)
        const unsigned long long m = __ballot(which == 2);
        if (m) {
            int32_t base = 0;
            if (lane == 0) base = atomicAdd(&acc->nlist[2], int32_t(__popcll(m)));
            base = __shfl(base, 0);
            if (which == 2) {
                const int64_t pos = int64_t(base) + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < G.n) {
                    l_split[pos] = int32_t(u);
                    split_rank[pos] = ru;
                } else {
                    acc->error = 1;
                }
            }
        }
    }
}

// LDS and slab path: a workgroup takes one source at a time and runs the three walks with barriers between them
template <bool LDS, bool AT>
__global__ __launch_bounds__(256) void k_c4_block(C4Graph G, const int32_t *__restrict__ list, int which, const uint8_t *__restrict__ wcode, int64_t cap,
                                                  uint32_t *__restrict__ slab, unsigned long long *__restrict__ at, C4Acc *__restrict__ acc) {
    __shared__ uint32_t s_cnt[LDS ? kC4LdsMax : 1];
    uint32_t *cnt = LDS ? s_cnt : slab + int64_t(blockIdx.x) * cap;
    if (LDS) {
        for (int i = threadIdx.x; i < kC4LdsMax; i += 256) s_cnt[i] = 0;
        __syncthreads();
    }
    const int64_t nsrc = min(int64_t(acc->nlist[which]), G.n);
    C4Thread t;
    for (int64_t s = blockIdx.x; s < nsrc; s += gridDim.x) {
        const int32_t u = list[s];
        const int32_t ru = G.newid[u];
        const int64_t span = G.n - ru - 1;
        if (span > cap) {  // (uniform: the whole workgroup skips the source)
            if (threadIdx.x == 0) acc->error = 1;
            continue;
        }
        const int wshift = wcode[u];
        const int64_t gstep = 256 >> wshift;
        c4_walk<LDS, 1, AT>(G, u, ru, span, wshift, 0, gstep, cnt, at, t, &acc->error);
        __threadfence();
        __syncthreads();
        if (AT) {
            c4_walk<LDS, 2, AT>(G, u, ru, span, wshift, 0, gstep, cnt, at, t, &acc->error);
            __syncthreads();
        }
        const unsigned long long before = t.cycles;
        c4_walk<LDS, 3, AT>(G, u, ru, span, wshift, 0, gstep, cnt, at, t, &acc->error);
        if (AT) c4_source_share(t.cycles - before, u, at);
        __threadfence();
        __syncthreads();
    }
    c4_flush(t, acc);
}

// split path, one launch per walk: workgroup (x, y) takes the positions x, x + gridDim.x, … (in groups) of the row of source ids[t0 + y]
template <int PHASE, bool AT>
__global__ __launch_bounds__(256) void k_c4_split(C4Graph G, const int32_t *__restrict__ ids, const int64_t *__restrict__ soff, int64_t t0,
                                                  const uint8_t *__restrict__ wcode, uint32_t *__restrict__ slab, int64_t slab_words,
                                                  unsigned long long *__restrict__ at, C4Acc *__restrict__ acc) {
    const int64_t s = t0 + blockIdx.y;
    const int32_t u = ids[s];
    const int32_t ru = G.newid[u];
    const int64_t span = G.n - ru - 1, first = soff[s] - soff[t0];
    if (first < 0 || first + span > slab_words || soff[s + 1] - soff[s] != span) {
        if (threadIdx.x == 0) acc->error = 1;
        return;
    }
    const int wshift = wcode[u];
    const int64_t ngrp = 256 >> wshift;
    C4Thread t;
    c4_walk<false, PHASE, AT>(G, u, ru, span, wshift, int64_t(blockIdx.x) * ngrp, int64_t(gridDim.x) * ngrp, slab + first, at, t, &acc->error);
    if (PHASE == 3 && AT) c4_source_share(t.cycles, u, at);
    c4_flush(t, acc);
}

// what one 4-cycle call returns to its entry point
struct C4Result {
    uint64_t cycles = 0, wedges = 0, sources = 0;
    int32_t max_cod = 0;
    int launches = 0;
    float setup_ms = 0.f, kernel_ms = 0.f;
};

// The 4-cycles of shard (part, nparts); d_at (n words, device, zeroed here) gets the per-vertex counts when given.
int cycle4_run(const gmsx_graph *g, int part, int nparts, unsigned long long *d_at, C4Result &r) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    // test hooks, first guesses
    const int64_t lds_span = std::max<long long>(0, std::min<long long>(opt_int("C4_LDS_SPAN", kC4LdsSpanDefault), kC4LdsMax));
    const long long slab_mb = std::max<long long>(1, std::min<long long>(opt_int("C4_SLAB_MB", kC4SlabMbDefault), 1 << 20));
    const int64_t split_wedges = std::max<long long>(1, opt_int("C4_SPLIT_WEDGES", kC4SplitWedgesDefault));
    const unsigned long long budget_words = ((unsigned long long)slab_mb << 20) / 4;
    const C4Graph G{n, g->off, g->adj, g->newid};
    DevBuf d_later, d_bound, d_lds, d_slabl, d_split, d_rank, d_wcode, d_acc, d_slab, d_soff, d_arena;
    // ---- setup: classify and bin the sources, allocate (and zero, once) the counter spans
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_later, n)) return rc;
    if (int rc = dalloc<int64_t>(d_bound, n)) return rc;
    if (int rc = dalloc<int32_t>(d_lds, n)) return rc;
    if (int rc = dalloc<int32_t>(d_slabl, n)) return rc;
    if (int rc = dalloc<int32_t>(d_split, n)) return rc;
    if (int rc = dalloc<int32_t>(d_rank, n)) return rc;
    if (int rc = dalloc<uint8_t>(d_wcode, n)) return rc;
    if (int rc = dalloc<C4Acc>(d_acc, 1)) return rc;
    C4Acc *acc = d_acc.as<C4Acc>();
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(C4Acc), s));
    GMSX_HIP(hipMemsetAsync(d_wcode.p, 0, size_t(n), s));
    if (d_at) GMSX_HIP(hipMemsetAsync(d_at, 0, size_t(n) * sizeof(unsigned long long), s));
    const unsigned groups = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    hipLaunchKernelGGL(k_c4_classify, dim3(groups), dim3(256), 0, s, G, d_later.as<int32_t>(), d_bound.as<int64_t>());
    if (g->max_deg > kLongRow)
        hipLaunchKernelGGL(k_c4_classify_long, dim3(unsigned(std::min<int64_t>(n, int64_t(cus) * 8))), dim3(256), 0, s, G, d_later.as<int32_t>(),
                           d_bound.as<int64_t>());
    hipLaunchKernelGGL(k_c4_bin, dim3(sweep), dim3(256), 0, s, G, d_later.as<const int32_t>(), d_bound.as<const int64_t>(), lds_span, split_wedges, part, nparts,
                       d_lds.as<int32_t>(), d_slabl.as<int32_t>(), d_split.as<int32_t>(), d_rank.as<int32_t>(), d_wcode.as<uint8_t>(), acc);
    r.launches = 3;
    C4Acc h;
    GMSX_HIP(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    const int64_t n_lds = h.nlist[0], n_slab = h.nlist[1], n_split = h.nlist[2];
    if (h.error || n_lds < 0 || n_slab < 0 || n_split < 0 || n_lds + n_slab + n_split > n) return GMSX_ERR_KERNEL;
    r.sources = uint64_t(n_lds + n_slab + n_split);
    // slab path: a span of n words per workgroup
    int64_t slab_wgs = 0;
    if (n_slab > 0) {
        slab_wgs = std::max<int64_t>(1, std::min<int64_t>({n_slab, int64_t(cus) * kC4BlocksPerCu, int64_t(budget_words / (unsigned long long)n)}));
        if (int rc = dalloc<uint32_t>(d_slab, slab_wgs * n)) return rc;
        GMSX_HIP(hipMemsetAsync(d_slab.p, 0, size_t(slab_wgs * n) * sizeof(uint32_t), s));
    }
    // split path: a span per source, as many sources per launch as fit the budget
    std::vector<Launch> plan;
    unsigned long long arena_words = 0;
    if (n_split > 0) {
        std::vector<int32_t> ranks(size_t(n_split), 0);
        GMSX_HIP(hipMemcpyAsync(ranks.data(), d_rank.p, size_t(n_split) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        std::vector<int64_t> soff(size_t(n_split) + 1, 0);
        for (int64_t t = 0; t < n_split; ++t) {
            if (ranks[size_t(t)] < 0 || ranks[size_t(t)] >= n) return GMSX_ERR_KERNEL;
            soff[size_t(t) + 1] = soff[size_t(t)] + (n - ranks[size_t(t)] - 1);
        }
        plan = plan_launches(soff, n_split, budget_words, kC4SplitBatch, &arena_words);
        if (int rc = dalloc<int64_t>(d_soff, n_split + 1)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_soff.p, soff.data(), soff.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (int rc = dalloc<uint32_t>(d_arena, int64_t(arena_words))) return rc;
        GMSX_HIP(hipMemsetAsync(d_arena.p, 0, size_t(std::max<unsigned long long>(arena_words, 1)) * sizeof(uint32_t), s));
        GMSX_HIP(hipStreamSynchronize(s));  // (soff is a local)
    }
    // ---- the wedge kernels
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    const uint8_t *wcode = d_wcode.as<const uint8_t>();
    if (n_lds > 0) {
        const unsigned blocks = unsigned(std::min<int64_t>(n_lds, int64_t(cus) * kC4BlocksPerCu));
        if (d_at)
            hipLaunchKernelGGL((k_c4_block<true, true>), dim3(blocks), dim3(256), 0, s, G, d_lds.as<const int32_t>(), 0, wcode, lds_span, (uint32_t *)nullptr, d_at, acc);
        else
            hipLaunchKernelGGL((k_c4_block<true, false>), dim3(blocks), dim3(256), 0, s, G, d_lds.as<const int32_t>(), 0, wcode, lds_span, (uint32_t *)nullptr, d_at, acc);
        ++r.launches;
    }
    if (n_slab > 0) {
        if (d_at)
            hipLaunchKernelGGL((k_c4_block<false, true>), dim3(unsigned(slab_wgs)), dim3(256), 0, s, G, d_slabl.as<const int32_t>(), 1, wcode, n, d_slab.as<uint32_t>(), d_at, acc);
        else
            hipLaunchKernelGGL((k_c4_block<false, false>), dim3(unsigned(slab_wgs)), dim3(256), 0, s, G, d_slabl.as<const int32_t>(), 1, wcode, n, d_slab.as<uint32_t>(), d_at, acc);
        ++r.launches;
    }
    for (const Launch &l : plan) {
        const int64_t tasks = l.t1 - l.t0;
        const unsigned px = unsigned(std::max<int64_t>(1, std::min<int64_t>(int64_t(cus) * 16 / tasks, int64_t(cus) * 4)));
        const dim3 grid(px, unsigned(tasks));
        const int32_t *ids = d_split.as<const int32_t>();
        const int64_t *so = d_soff.as<const int64_t>();
        uint32_t *arena = d_arena.as<uint32_t>();
        const int64_t aw = int64_t(arena_words);
        if (d_at) {
            hipLaunchKernelGGL((k_c4_split<1, true>), grid, dim3(256), 0, s, G, ids, so, l.t0, wcode, arena, aw, d_at, acc);
            hipLaunchKernelGGL((k_c4_split<2, true>), grid, dim3(256), 0, s, G, ids, so, l.t0, wcode, arena, aw, d_at, acc);
            hipLaunchKernelGGL((k_c4_split<3, true>), grid, dim3(256), 0, s, G, ids, so, l.t0, wcode, arena, aw, d_at, acc);
            r.launches += 3;
        } else {
            hipLaunchKernelGGL((k_c4_split<1, false>), grid, dim3(256), 0, s, G, ids, so, l.t0, wcode, arena, aw, d_at, acc);
            hipLaunchKernelGGL((k_c4_split<3, false>), grid, dim3(256), 0, s, G, ids, so, l.t0, wcode, arena, aw, d_at, acc);
            r.launches += 2;
        }
    }
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    GMSX_HIP(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    // a counter left behind, or one that was not zero when its source began, makes the harvest differ from the count
    if (h.error || h.harvested != h.wedges) return GMSX_ERR_KERNEL;
    // the 64-bit sum of the cycles cannot have wrapped: Σ_w C(cnt[w], 2) <= wedges * max counter / 2 (sufficient, far from tight; a graph
    // that fails it has more than 2^34 wedges)
    if ((unsigned __int128)h.wedges * (unsigned __int128)std::max(h.max_cod, 1) / 2 > (unsigned __int128)UINT64_MAX) return GMSX_ERR_OVERFLOW;
    GMSX_HIP(hipEventElapsedTime(&r.setup_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&r.kernel_ms, c.ev[1], c.ev[2]));
    r.cycles = h.cycles;
    r.wedges = h.wedges;
    r.max_cod = h.max_cod;
    return GMSX_OK;
}

// ---- the other seven counts ------------------------------------------------------------------------------------------------------------

// a 128-bit sum in two halves
struct U128 {
    unsigned long long lo = 0, hi = 0;
    __device__ __forceinline__ void add(unsigned long long x_lo, unsigned long long x_hi = 0) {
        lo += x_lo;
        hi += x_hi + (lo < x_lo ? 1ull : 0ull);
    }
};
__device__ __forceinline__ void wave_store(U128 v, unsigned long long *__restrict__ out) {
    wave_fold2(v.lo, v.hi, [&v](unsigned long long &, unsigned long long &, unsigned long long lo, unsigned long long hi) { v.add(lo, hi); });
    if ((threadIdx.x & 63) == 0) {
        out[0] = v.lo;
        out[1] = v.hi;
    }
}

constexpr int kEdgeSums = 4, kDegSums = 2;

// per wave: Σ sup, Σ C(sup, 2), Σ sup (d_u + d_v - 4), Σ (d_u - 1)(d_v - 1) over the edges, as 128-bit partials (out[wave][sum][lo, hi])
__global__ __launch_bounds__(256) void k_motif_edges(int64_t m, const int64_t *__restrict__ off, const int32_t *__restrict__ eu, const int32_t *__restrict__ ev,
                                                     const int32_t *__restrict__ sup, unsigned long long *__restrict__ out) {
    U128 a[kEdgeSums];
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < m; e += int64_t(gridDim.x) * blockDim.x) {
        const int32_t u = eu[e], v = ev[e];
        const unsigned long long du = (unsigned long long)(off[u + 1] - off[u]), dv = (unsigned long long)(off[v + 1] - off[v]);
        const unsigned long long sp = (unsigned long long)max(sup[e], 0);
        a[0].add(sp);
        if (sp) {  // (an edge in a triangle has both degrees >= 2)
            a[1].add(sp * (sp - 1) / 2);
            a[2].add(sp * (du + dv - 4));
        }
        if (du && dv) a[3].add((du - 1) * (dv - 1));
    }
    const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    for (int k = 0; k < kEdgeSums; ++k) wave_store(a[k], out + (wave * kEdgeSums + k) * 2);
}

// per wave: Σ C(d, 2) and Σ C(d, 3) over the vertices.  C(d, 3) = (d (d - 1) / 2) (d - 2) / 3: the first factor fits 64 bits for d < 2^31 and one
// of the two is a multiple of 3, so the product of the reduced factors is exact in 128 bits.
__global__ __launch_bounds__(256) void k_motif_degrees(int64_t n, const int64_t *__restrict__ off, unsigned long long *__restrict__ out) {
    U128 a[kDegSums];
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += int64_t(gridDim.x) * blockDim.x) {
        const unsigned long long d = (unsigned long long)(off[v + 1] - off[v]);
        if (d < 2) continue;
        unsigned long long x = d * (d - 1) / 2, y = d - 2;
        a[0].add(x);
        if (y % 3 == 0) y /= 3;
        else x /= 3;
        a[1].add(x * y, __umul64hi(x, y));
    }
    const int64_t wave = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    for (int k = 0; k < kDegSums; ++k) wave_store(a[k], out + (wave * kDegSums + k) * 2);
}

using u128 = unsigned __int128;

void sum_partials(const std::vector<unsigned long long> &p, int sums, u128 *out) {
    for (int k = 0; k < sums; ++k) out[k] = 0;
    for (size_t w = 0; w + size_t(sums) * 2 <= p.size(); w += size_t(sums) * 2)
        for (int k = 0; k < sums; ++k) out[k] += (u128(p[w + size_t(k) * 2 + 1]) << 64) | u128(p[w + size_t(k) * 2]);
}

const gmsx_stats kNoStats{0.0, 0.0, 0, 0, 0, 0, 0, 0};

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_cycle4_count(const gmsx_graph *g, uint64_t *cycles, int64_t *at_vertex, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !cycles) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        const int64_t n = g->n;
        if (n == 0 || g->nnz == 0) {
            if (at_vertex && n > 0) std::memset(at_vertex, 0, size_t(n) * sizeof(int64_t));
            *cycles = 0;
            if (stats) *stats = kNoStats;
            return GMSX_OK;
        }
        DevBuf d_at;
        if (at_vertex)
            if (int rc = dalloc<unsigned long long>(d_at, n)) return rc;
        C4Result r;
        if (int rc = cycle4_run(g, 0, 1, d_at.as<unsigned long long>(), r)) return rc;
        if (at_vertex) {  // the flag word was read as zero: the caller's array is written now, through host staging
            std::vector<unsigned long long> h_at(size_t(n), 0);
            hipStream_t s = ctx().stream;
            GMSX_HIP(hipMemcpyAsync(h_at.data(), d_at.p, size_t(n) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            unsigned __int128 sum = 0;
            for (unsigned long long x : h_at) sum += x;
            if (sum != (unsigned __int128)r.cycles * 4) return GMSX_ERR_KERNEL;  // every cycle is met at its four vertices
            std::memcpy(at_vertex, h_at.data(), size_t(n) * sizeof(int64_t));
        }
        *cycles = r.cycles;
        if (stats) *stats = gmsx_stats{double(r.kernel_ms), double(r.setup_ms), r.sources, r.wedges, 0, r.launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_cycle4_partial(const gmsx_graph *g, int part, int nparts, uint64_t *partial, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !partial || nparts < 1 || part < 0 || part >= nparts) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        if (g->n == 0 || g->nnz == 0) {
            *partial = 0;
            if (stats) *stats = kNoStats;
            return GMSX_OK;
        }
        C4Result r;
        if (int rc = cycle4_run(g, part, nparts, nullptr, r)) return rc;
        *partial = r.cycles;
        if (stats) *stats = gmsx_stats{double(r.kernel_ms), double(r.setup_ms), r.sources, r.wedges, 0, r.launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_motif_census4(const gmsx_graph *g, gmsx_motif_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        gmsx_motif_info res;
        std::memset(&res, 0, sizeof res);
        if (g->n == 0 || g->nnz == 0) {
            *info = res;
            if (stats) *stats = kNoStats;
            return GMSX_OK;
        }
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int64_t n = g->n;
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        // ---- the 4-cycles
        C4Result r;
        if (int rc = cycle4_run(g, 0, 1, nullptr, r)) return rc;
        // ---- support of every edge, then the two reductions
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        TrussEdges t;
        if (int rc = truss_edges(g, t, nullptr)) return rc;
        const int64_t m = t.m;
        const unsigned eb = unsigned(std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, int64_t(cus) * 8)));
        const unsigned vb = unsigned(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, int64_t(cus) * 8)));
        const size_t ew = size_t(eb) * 4 * kEdgeSums * 2, vw = size_t(vb) * 4 * kDegSums * 2;  // four waves per workgroup
        DevBuf d_part;
        if (int rc = dalloc<unsigned long long>(d_part, int64_t(ew + vw))) return rc;
        hipLaunchKernelGGL(k_motif_edges, dim3(eb), dim3(256), 0, s, m, g->off, t.eu.as<const int32_t>(), t.ev.as<const int32_t>(), t.sup.as<const int32_t>(),
                           d_part.as<unsigned long long>());
        hipLaunchKernelGGL(k_motif_degrees, dim3(vb), dim3(256), 0, s, n, g->off, d_part.as<unsigned long long>() + ew);
        std::vector<unsigned long long> h_part(ew + vw, 0);
        GMSX_HIP(hipMemcpyAsync(h_part.data(), d_part.p, h_part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        float red_ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&red_ms, c.ev[0], c.ev[1]));
        // ---- the 4-cliques: the existing count driver
        uint64_t k4_ordered = 0, k4 = 0;
        gmsx_stats kst = kNoStats;
        if (int rc = gmsx_kclique_count(g, 4, &k4_ordered, &k4, &kst)) return rc;
        // ---- the identities, in 128 bits
        u128 es[kEdgeSums], ds[kDegSums];
        sum_partials(std::vector<unsigned long long>(h_part.begin(), h_part.begin() + long(ew)), kEdgeSums, es);
        sum_partials(std::vector<unsigned long long>(h_part.begin() + long(ew), h_part.end()), kDegSums, ds);
        if (es[0] != u128(t.h.sum) || es[0] % 3 != 0 || es[2] % 2 != 0) return GMSX_ERR_KERNEL;
        const u128 tri = es[0] / 3;
        if (es[3] < 3 * tri) return GMSX_ERR_KERNEL;
        u128 sub[GMSX_MOTIF_KINDS];
        sub[GMSX_MOTIF_WEDGE] = ds[0];
        sub[GMSX_MOTIF_TRIANGLE] = tri;
        sub[GMSX_MOTIF_STAR3] = ds[1];
        sub[GMSX_MOTIF_PATH4] = es[3] - 3 * tri;
        sub[GMSX_MOTIF_PAW] = es[2] / 2;
        sub[GMSX_MOTIF_CYCLE4] = r.cycles;
        sub[GMSX_MOTIF_DIAMOND] = es[1];
        sub[GMSX_MOTIF_CLIQUE4] = k4;
        for (int k = 0; k < GMSX_MOTIF_KINDS; ++k)
            if (sub[k] > u128(UINT64_MAX)) return GMSX_ERR_OVERFLOW;  // nothing was written
        using i128 = __int128;
        i128 ind[GMSX_MOTIF_KINDS];
        const i128 K4 = i128(k4);
        ind[GMSX_MOTIF_CLIQUE4] = K4;
        ind[GMSX_MOTIF_DIAMOND] = i128(sub[GMSX_MOTIF_DIAMOND]) - 6 * K4;
        ind[GMSX_MOTIF_CYCLE4] = i128(sub[GMSX_MOTIF_CYCLE4]) - ind[GMSX_MOTIF_DIAMOND] - 3 * K4;
        ind[GMSX_MOTIF_PAW] = i128(sub[GMSX_MOTIF_PAW]) - 4 * ind[GMSX_MOTIF_DIAMOND] - 12 * K4;
        ind[GMSX_MOTIF_STAR3] = i128(sub[GMSX_MOTIF_STAR3]) - ind[GMSX_MOTIF_PAW] - 2 * ind[GMSX_MOTIF_DIAMOND] - 4 * K4;
        ind[GMSX_MOTIF_PATH4] = i128(sub[GMSX_MOTIF_PATH4]) - 2 * ind[GMSX_MOTIF_PAW] - 4 * ind[GMSX_MOTIF_CYCLE4] - 6 * ind[GMSX_MOTIF_DIAMOND] - 12 * K4;
        ind[GMSX_MOTIF_TRIANGLE] = i128(tri);
        ind[GMSX_MOTIF_WEDGE] = i128(sub[GMSX_MOTIF_WEDGE]) - 3 * i128(tri);
        for (int k = 0; k < GMSX_MOTIF_KINDS; ++k) {
            if (ind[k] < 0 || ind[k] > i128(sub[k])) return GMSX_ERR_KERNEL;  // an induced count is a part of its non-induced one
            res.subgraphs[k] = uint64_t(sub[k]);
            res.induced[k] = uint64_t(ind[k]);
        }
        res.wedges_walked = r.wedges;
        res.max_codegree = r.max_cod;
        *info = res;
        if (stats)
            *stats = gmsx_stats{double(r.kernel_ms), double(r.setup_ms) + double(red_ms) + kst.kernel_ms + kst.setup_ms, r.sources, r.wedges, 0,
                                r.launches + t.launches + 2 + kst.launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
