// Link prediction on gfx950: the exact top-q similarity over the NON-edges of the graph, and the precision / recall step behind it.
//   gmsx_link_prediction            GMS::LinkPrediction::link_prediction_similarity<Metric> (set_based/link_prediction/link_prediction.h:42-101)
//   gmsx_link_prediction_precision  score_link_prediction_precision (set_based/link_prediction/evaluation.h:99-124)
//
// THE RULE the reference's insertion loop amounts to (gmsx.h): candidates = the non-edges u < v whose score is not NaN; order = decreasing
// score, ties by ascending (u, v); result = the first min(q, candidates) of that order, returned worst first.
//
// CLASSES.  For the five common-neighbour metrics a non-edge is ONE (Jaccard only: both endpoints isolated, score 1.0), POS (a common
// neighbour, score > 0; Jaccard <= 1/3) or ZERO (none, score exactly 0.0; Overlap: both endpoints non-isolated, else 0/0) and the rule orders
// ONE, POS, ZERO, with ONE and ZERO purely lexicographic.  So only POS — the pairs at distance two — is ever scored and sorted; ZERO is
// generated in order and cut where q is reached.  TotalNeighbors / PrefAttachment rank every non-edge: one class, ALL, O(n^2) scores like
// the reference.
//
// CANDIDATES.  A task is a source vertex u of the shard (u mod nparts == part), a workgroup takes one source at a time.  It marks two bitmaps
// over [0, n): the two-hop bits (a wave per w in N(u), lanes over N(w), only v > u; atomicOr is idempotent, so what the bitmap holds after the
// barrier is a fact about the graph) and the adjacency bits of N(u).  POS = twohop & ~adj, ZERO = ~twohop & ~adj, ALL = ~adj, all cut to
// u < v < n.  Word popcounts + a workgroup scan compact the candidates of a source in ascending v.  Pass 1 counts per source, an exclusive scan
// gives every source its base, pass 2 marks again and writes (u, v) there; a wave per pair then scores them through wave_pair_similarity,
// the function gmsx_vertex_similarity_batch runs (pair_similarity.hpp): the scores are its bits.
//
// SELECTION.  The candidates of a chunk of sources are in lexicographic order by construction, and chunks run in ascending u.  The running
// best (at most q entries, already in the rule's order) followed by the new chunk is sorted by ONE STABLE radix sort, descending on the
// order-preserving 64-bit image of the score, and cut to q: equal scores keep their lexicographic order, which is the rule.  No atomic
// arrival order reaches an output.
//
// KNOWN LIMIT.  One workgroup walks the whole two-hop neighbourhood of a hub source alone (the tail gmsx_bk_list has too);
// tools/link_prediction_probe.py prints that source's share of the walk.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "launch_plan.hpp"
#include "pair_similarity.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

namespace gmsx {

namespace {

// FIRST GUESSES, all of them: no device timing stands behind any of these bounds yet (tools/link_prediction_probe.py is the
// measurement).
constexpr int kThreads = 256;                          // one workgroup per source
constexpr int64_t kLdsMaxN = 131072;                   // both bitmaps of a source in LDS up to this n (2 x 16 KB); beyond: the workgroup's global slab
constexpr unsigned long long kChunkCapBytes = 1ull << 30;  // chunk budget = min(free / 4, this)
constexpr int kCandWords = 8;                          // 32-bit words a candidate takes in a chunk: key + pair, in and out of the sort
constexpr int kLanesPerRow = 64;                       // lanes that walk one N(w) of the two-hop marking (a wave per w)
constexpr int64_t kAllMaxN = 131072;                   // the ALL class is refused above this n (n^2 / 2 scores)
constexpr int64_t kZeroBlock = 4096;                   // sources the ZERO fill counts ahead before it fills (it stops as soon as q is reached)
constexpr int kGridPerCu = 4;

enum { kClsPos = 0, kClsZero = 1, kClsAll = 2 };
enum { kBitOne = 1, kBitPos = 2, kBitZero = 4, kBitAll = 8 };
// flag word: 1 = a write outside its span, 2 = a fill that disagrees with its count, 4 = an id outside [0, n), 8 = a NaN among the candidates
using Flags = unsigned long long;

__device__ __forceinline__ uint32_t load_word(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive scan of c over the workgroup (kThreads = 4 waves); *total = the sum.  Every thread calls it.
__device__ __forceinline__ int block_excl_scan(int c, int *s_w, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = wave_incl_scan(c, lane);
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) base += s_w[w];
        sum += s_w[w];
    }
    __syncthreads();
    *total = sum;
    return base + x - c;
}

// Sources i in [i0, i1) of the shard (u = part + i * nparts), one per workgroup at a time.  FILL = false: cnt[i - c0] = candidates of the
// source.  FILL = true: the pairs (u << 32 | v), ascending v, at pairs[cbase[i - c0] + shift ...), never at or past pairs_cap.
template <bool FILL>
__global__ __launch_bounds__(kThreads) void k_lp_sources(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int64_t n, int metric, int cls,
                                                         int part, int nparts, int64_t i0, int64_t i1, int64_t c0, int64_t words, int use_lds,
                                                         uint32_t *__restrict__ arena, const uint32_t *__restrict__ iso, int64_t *__restrict__ cnt,
                                                         const int64_t *__restrict__ cbase, int64_t shift, unsigned long long *__restrict__ pairs,
                                                         int64_t pairs_cap, Flags *__restrict__ flags) {
    extern __shared__ uint32_t lds_bm[];
    __shared__ int s_w[kThreads / 64];
    uint32_t *bm_two = use_lds ? lds_bm : arena + size_t(blockIdx.x) * size_t(2 * words);
    uint32_t *bm_adj = bm_two + words;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t i = i0 + blockIdx.x; i < i1; i += gridDim.x) {
        const int64_t u = int64_t(part) + i * nparts;
        const int64_t r0 = off[u], r1 = off[u + 1];
        for (int64_t w = tid; w < 2 * words; w += kThreads) bm_two[w] = 0;
        __syncthreads();
        for (int64_t j = r0 + tid; j < r1; j += kThreads) {
            const int32_t x = adj[j];
            if (x > u && x < n) atomicOr(&bm_adj[x >> 5], 1u << (x & 31));
        }
        if (cls != kClsAll) {
            for (int64_t j = r0 + wave; j < r1; j += kThreads / 64) {
                const int32_t w = adj[j];
                if (w < 0 || w >= n) continue;
                const int64_t k1 = off[w + 1];
                for (int64_t k = off[w] + lane; k < k1; k += kLanesPerRow) {
                    const int32_t v = adj[k];
                    if (v > u && v < n) atomicOr(&bm_two[v >> 5], 1u << (v & 31));
                }
            }
        }
        __syncthreads();
        const bool u_iso = r1 == r0;
        const bool none = cls == kClsZero && metric == GMSX_SIM_OVERLAP && u_iso;                               // 0/0: not a candidate
        const bool mask_iso = cls == kClsZero && (metric == GMSX_SIM_OVERLAP || (metric == GMSX_SIM_JACCARD && u_iso));  // NaN / the ONE class
        int64_t run = 0;
        const int64_t at = FILL ? cbase[i - c0] + shift : 0;
        for (int64_t t0 = 0; t0 < words; t0 += kThreads) {
            const int64_t wd = t0 + tid;
            uint32_t m = 0;
            if (wd < words && !none) {
                const uint32_t a = load_word(&bm_adj[wd]), t = load_word(&bm_two[wd]);
                m = cls == kClsPos ? (t & ~a) : cls == kClsZero ? (~t & ~a) : ~a;
                const int64_t lo = wd * 32;
                if (lo + 31 <= u) m = 0;
                else if (lo <= u) m &= ~((2u << uint32_t(u - lo)) - 1u);     // only v > u
                if (lo + 32 > n) m &= (1u << uint32_t(n - lo)) - 1u;         // only v < n
                if (mask_iso) m &= ~iso[wd];
            }
            int total = 0;
            const int ex = block_excl_scan(__popc(m), s_w, &total);
            if (FILL) {
                int64_t p = at + run + ex;
                while (m) {
                    const int b = __ffs(int(m)) - 1;
                    m &= m - 1;
                    if (p >= 0 && p < pairs_cap) pairs[p] = ((unsigned long long)uint32_t(u) << 32) | (unsigned long long)uint32_t(wd * 32 + b);
                    else atomicOr(&flags[0], 1ull);
                    ++p;
                }
            }
            run += total;
        }
        if (tid == 0) {
            if (!FILL) cnt[i - c0] = run;
            else if (run != cbase[i - c0 + 1] - cbase[i - c0]) atomicOr(&flags[0], 2ull);
        }
        __syncthreads();
    }
}

// the order-preserving 64-bit image of a double: a < b  <=>  image(a) < image(b)
__host__ __device__ inline unsigned long long score_image(double x) {
    unsigned long long b;
    memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
inline double image_score(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    double x;
    std::memcpy(&x, &b, 8);
    return x;
}

// keys[p] = image of the score of pairs[p]: a wave per pair through the function gmsx_vertex_similarity_batch runs
__global__ __launch_bounds__(256) void k_lp_score(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int64_t n, int metric, int64_t count,
                                                  const unsigned long long *__restrict__ pairs, unsigned long long *__restrict__ keys,
                                                  Flags *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t p = wave0; p < count; p += nwaves) {
        const unsigned long long e = pairs[p];
        const int32_t u = int32_t(uint32_t(e >> 32)), v = int32_t(uint32_t(e));
        if (u < 0 || v < 0 || u >= n || v >= n) {
            if (lane == 0) {
                keys[p] = 0;
                atomicOr(&flags[0], 4ull);
            }
            continue;
        }
        const double r = wave_pair_similarity(off, adj, metric, u, v, lane);
        if (lane == 0) {
            if (r != r) atomicOr(&flags[0], 8ull);
            keys[p] = score_image(r);
        }
    }
}

// isolated vertices: flag[v] (n + 1 entries, the last 0) for the scan and the bitmap the ZERO class masks with
__global__ void k_lp_iso_flags(int64_t n, const int64_t *__restrict__ off, int64_t *__restrict__ flag, uint32_t *__restrict__ iso) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v > n) return;
    const bool is = v < n && off[v + 1] == off[v];
    flag[v] = is ? 1 : 0;
    if (is) atomicOr(&iso[v >> 5], 1u << (v & 31));
}
__global__ void k_lp_iso_compact(int64_t n, const int64_t *__restrict__ flag, const int64_t *__restrict__ pos, int32_t *__restrict__ list, int64_t cap,
                                 Flags *__restrict__ flags) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n || !flag[v]) return;
    if (pos[v] >= 0 && pos[v] < cap) list[pos[v]] = int32_t(v);
    else atomicOr(&flags[0], 1ull);
}

// ---- precision ----------------------------------------------------------------------------------------------------------------------
// keys[i] = min << 32 | max of predicted pair i; a pair with u == v or an id outside [0, n) raises the flag
__global__ void k_lp_norm(int64_t n, int64_t n_pred, const int32_t *__restrict__ pu, const int32_t *__restrict__ pv, unsigned long long *__restrict__ keys,
                          Flags *__restrict__ flags) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_pred) return;
    const int32_t u = pu[i], v = pv[i];
    if (u < 0 || v < 0 || u >= n || v >= n || u == v) {
        keys[i] = 0;
        atomicOr(&flags[0], 4ull);
        return;
    }
    keys[i] = ((unsigned long long)uint32_t(u < v ? u : v) << 32) | (unsigned long long)uint32_t(u < v ? v : u);
}
// one lane per SORTED predicted pair; a pair equal to its predecessor is the same edge and counts once; binary search of the larger id in the
// smaller id's row of g_test
__global__ __launch_bounds__(256) void k_lp_contains(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int64_t n, int64_t n_pred,
                                                     const unsigned long long *__restrict__ keys, unsigned long long *__restrict__ tp) {
    const int64_t end = ((n_pred + 63) / 64) * 64;  // whole waves stay together for the ballot
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < end; i += int64_t(gridDim.x) * blockDim.x) {
        bool hit = false;
        if (i < n_pred && (i == 0 || keys[i] != keys[i - 1])) {
            const int32_t a = int32_t(uint32_t(keys[i] >> 32)), b = int32_t(uint32_t(keys[i]));
            if (a >= 0 && a < n) {
                int64_t lo = off[a], hi = off[a + 1];
                const int64_t rend = hi;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (adj[mid] < b) lo = mid + 1; else hi = mid;
                }
                hit = lo < rend && adj[lo] == b;
            }
        }
        const unsigned long long m = __ballot(hit);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(tp, (unsigned long long)__popcll(m));
    }
}

// ---- the class driver ---------------------------------------------------------------------------------------------------------------
struct LpCall {
    const gmsx_graph *g = nullptr;
    int metric = 0, part = 0, nparts = 1;
    int64_t q = 0, n_src = 0, words = 0;
    bool use_lds = true;
    unsigned max_blocks = 1;
    unsigned long long budget_words = 0;
    DevBuf arena, iso, flags;
    int launches = 0, chunks = 0;
    int64_t scored = 0;
};

struct Entry {
    int32_t u, v;
    double score;
};

int lp_flags_clear(LpCall &c) {
    Flags f = 1;
    GMSX_HIP(hipMemcpyAsync(&f, c.flags.p, sizeof f, hipMemcpyDeviceToHost, ctx().stream));
    GMSX_HIP(hipStreamSynchronize(ctx().stream));
    GMSX_HIP(hipGetLastError());
    return f ? GMSX_ERR_KERNEL : GMSX_OK;
}

void lp_launch(LpCall &c, bool fill, int cls, int64_t i0, int64_t i1, int64_t c0, int64_t *cnt, const int64_t *cbase, int64_t shift,
               unsigned long long *pairs, int64_t pairs_cap) {
    const gmsx_graph *g = c.g;
    const unsigned blocks = unsigned(std::max<int64_t>(1, std::min<int64_t>(i1 - i0, c.max_blocks)));
    const size_t lds = c.use_lds ? size_t(2 * c.words) * 4 : 0;
    if (fill)
        hipLaunchKernelGGL(k_lp_sources<true>, dim3(blocks), dim3(kThreads), lds, ctx().stream, g->off, g->adj, g->n, c.metric, cls, c.part, c.nparts, i0, i1, c0,
                           c.words, c.use_lds ? 1 : 0, c.arena.as<uint32_t>(), c.iso.as<const uint32_t>(), cnt, cbase, shift, pairs, pairs_cap,
                           c.flags.as<Flags>());
    else
        hipLaunchKernelGGL(k_lp_sources<false>, dim3(blocks), dim3(kThreads), lds, ctx().stream, g->off, g->adj, g->n, c.metric, cls, c.part, c.nparts, i0, i1, c0,
                           c.words, c.use_lds ? 1 : 0, c.arena.as<uint32_t>(), c.iso.as<const uint32_t>(), cnt, cbase, shift, pairs, pairs_cap,
                           c.flags.as<Flags>());
    ++c.launches;
}

// pass 1 over the sources [i0, i1): hb = their exclusive bases (i1 - i0 + 1 entries, host), d_cbase the same on the device
int lp_count(LpCall &c, int cls, int64_t i0, int64_t i1, DevBuf &d_cbase, std::vector<int64_t> &hb) {
    hipStream_t s = ctx().stream;
    const int64_t nt = i1 - i0;
    DevBuf d_cnt;
    if (int rc = dalloc<int64_t>(d_cnt, nt + 1)) return rc;
    d_cbase.reset();
    if (int rc = dalloc<int64_t>(d_cbase, nt + 1)) return rc;
    GMSX_HIP(hipMemsetAsync(d_cnt.p, 0, size_t(nt + 1) * 8, s));
    lp_launch(c, false, cls, i0, i1, i0, d_cnt.as<int64_t>(), nullptr, 0, nullptr, 0);
    GMSX_HIP(hipGetLastError());
    if (int rc = exclusive_scan_i64(d_cnt.as<const int64_t>(), d_cbase.as<int64_t>(), nt + 1, s)) return rc;
    hb.resize(size_t(nt + 1));
    GMSX_HIP(hipMemcpyAsync(hb.data(), d_cbase.p, size_t(nt + 1) * 8, hipMemcpyDeviceToHost, s));
    if (int rc = lp_flags_clear(c)) return rc;
    for (int64_t t = 0; t < nt; ++t)
        if (hb[size_t(t + 1)] < hb[size_t(t)] || hb[size_t(t + 1)] - hb[size_t(t)] > c.g->n) return GMSX_ERR_KERNEL;
    return GMSX_OK;
}

// how pass 2 over those sources is cut: slab of a source = its candidates' chunk storage (launch_plan.hpp)
std::vector<Launch> lp_plan(const LpCall &c, const std::vector<int64_t> &hb, int64_t *max_cands) {
    std::vector<int64_t> soff(hb.size());
    for (size_t t = 0; t < hb.size(); ++t) soff[t] = hb[t] * kCandWords;
    unsigned long long widest = 0;
    std::vector<Launch> plan = plan_launches(soff, int64_t(hb.size()) - 1, std::max<unsigned long long>(c.budget_words, kCandWords), kNoTaskCap, &widest);
    *max_cands = int64_t(widest / kCandWords);
    return plan;
}

// POS or ALL: every source of the shard, scored, the best `need` kept.  *total = candidates of the class in the shard.
int lp_scored_class(LpCall &c, int cls, int64_t need, int64_t *total, std::vector<Entry> &out) {
    hipStream_t s = ctx().stream;
    const gmsx_graph *g = c.g;
    DevBuf d_cbase;
    std::vector<int64_t> hb;
    if (int rc = lp_count(c, cls, 0, c.n_src, d_cbase, hb)) return rc;
    *total = hb[size_t(c.n_src)];
    if (need <= 0 || *total == 0) return GMSX_OK;
    int64_t max_cands = 0;
    const std::vector<Launch> plan = lp_plan(c, hb, &max_cands);
    const int64_t keep = std::min(need, *total);
    const int64_t cap = keep + max_cands;
    if (cap >= (int64_t(1) << 32)) return GMSX_ERR_DEVICE_MEM;
    DevBuf kbuf[2], vbuf[2], d_tmp;
    for (int i = 0; i < 2; ++i) {
        if (int rc = dalloc<unsigned long long>(kbuf[i], cap)) return rc;
        if (int rc = dalloc<unsigned long long>(vbuf[i], cap)) return rc;
    }
    size_t tmp_bytes = 0;
    GMSX_HIP(rocprim::radix_sort_pairs_desc(nullptr, tmp_bytes, kbuf[0].as<unsigned long long>(), kbuf[1].as<unsigned long long>(),
                                            vbuf[0].as<unsigned long long>(), vbuf[1].as<unsigned long long>(), size_t(cap), 0, 64, s));
    if (int rc = dalloc<char>(d_tmp, int64_t(tmp_bytes))) return rc;
    int a = 0;
    int64_t nb = 0;
    const int cus = ctx().compute_units > 0 ? ctx().compute_units : 256;
    for (const Launch &l : plan) {
        const int64_t cc = hb[size_t(l.t1)] - hb[size_t(l.t0)];
        if (cc == 0) continue;
        if (nb + cc > cap) return GMSX_ERR_KERNEL;
        unsigned long long *keys = kbuf[a].as<unsigned long long>(), *vals = vbuf[a].as<unsigned long long>();
        lp_launch(c, true, cls, l.t0, l.t1, 0, nullptr, d_cbase.as<const int64_t>(), nb - hb[size_t(l.t0)], vals, nb + cc);
        const int64_t sb = std::min<int64_t>((cc + 3) / 4, int64_t(cus) * 32);
        hipLaunchKernelGGL(k_lp_score, dim3(unsigned(sb)), dim3(256), 0, s, g->off, g->adj, g->n, c.metric, cc, vals + nb, keys + nb, c.flags.as<Flags>());
        ++c.launches;
        if (int rc = lp_flags_clear(c)) return rc;
        c.scored += cc;
        size_t tb = tmp_bytes;
        GMSX_HIP(rocprim::radix_sort_pairs_desc(d_tmp.p, tb, keys, kbuf[a ^ 1].as<unsigned long long>(), vals, vbuf[a ^ 1].as<unsigned long long>(),
                                                size_t(nb + cc), 0, 64, s));
        GMSX_HIP(hipStreamSynchronize(s));
        ++c.launches;
        ++c.chunks;
        nb = std::min(keep, nb + cc);
        a ^= 1;
    }
    std::vector<unsigned long long> hk, hv;
    hk.resize(size_t(nb));
    hv.resize(size_t(nb));
    if (nb > 0) {
        GMSX_HIP(hipMemcpy(hk.data(), kbuf[a].p, size_t(nb) * 8, hipMemcpyDeviceToHost));
        GMSX_HIP(hipMemcpy(hv.data(), vbuf[a].p, size_t(nb) * 8, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < nb; ++i) {
        if (i > 0 && hk[size_t(i)] > hk[size_t(i - 1)]) return GMSX_ERR_KERNEL;
        out.push_back(Entry{int32_t(uint32_t(hv[size_t(i)] >> 32)), int32_t(uint32_t(hv[size_t(i)])), image_score(hk[size_t(i)])});
    }
    return GMSX_OK;
}

// ZERO: lexicographic, score 0.0, no sort; blocks of sources in ascending u until `need` pairs are there
int lp_zero_class(LpCall &c, int64_t need, std::vector<Entry> &out) {
    hipStream_t s = ctx().stream;
    DevBuf d_cbase, d_pairs;
    int64_t pairs_cap = 0;
    std::vector<int64_t> hb;
    std::vector<unsigned long long> hp;
    for (int64_t b0 = 0; b0 < c.n_src && need > 0; b0 += kZeroBlock) {
        const int64_t b1 = std::min(c.n_src, b0 + kZeroBlock);
        if (int rc = lp_count(c, kClsZero, b0, b1, d_cbase, hb)) return rc;
        int64_t max_cands = 0;
        const std::vector<Launch> plan = lp_plan(c, hb, &max_cands);
        if (max_cands > pairs_cap) {
            d_pairs.reset();
            if (int rc = dalloc<unsigned long long>(d_pairs, max_cands)) return rc;
            pairs_cap = max_cands;
        }
        for (const Launch &l : plan) {
            const int64_t cc = hb[size_t(l.t1)] - hb[size_t(l.t0)];
            if (cc == 0) continue;
            if (cc > pairs_cap) return GMSX_ERR_KERNEL;
            lp_launch(c, true, kClsZero, b0 + l.t0, b0 + l.t1, b0, nullptr, d_cbase.as<const int64_t>(), -hb[size_t(l.t0)], d_pairs.as<unsigned long long>(), cc);
            const int64_t take = std::min(need, cc);
            hp.resize(size_t(take));
            GMSX_HIP(hipMemcpyAsync(hp.data(), d_pairs.p, size_t(take) * 8, hipMemcpyDeviceToHost, s));
            if (int rc = lp_flags_clear(c)) return rc;
            ++c.chunks;
            for (int64_t i = 0; i < take; ++i) out.push_back(Entry{int32_t(uint32_t(hp[size_t(i)] >> 32)), int32_t(uint32_t(hp[size_t(i)])), 0.0});
            need -= take;
            if (need == 0) break;
        }
    }
    return GMSX_OK;
}

// ONE (Jaccard): the isolated vertices compacted on the device; the shard's isolated sources against all isolated v > u, lexicographic
int lp_isolated(LpCall &c, std::vector<int32_t> &list) {
    hipStream_t s = ctx().stream;
    const int64_t n = c.g->n;
    DevBuf d_flag, d_pos, d_list;
    if (int rc = dalloc<int64_t>(d_flag, n + 1)) return rc;
    if (int rc = dalloc<int64_t>(d_pos, n + 1)) return rc;
    if (int rc = dalloc<uint32_t>(c.iso, c.words)) return rc;
    GMSX_HIP(hipMemsetAsync(c.iso.p, 0, size_t(c.words) * 4, s));
    hipLaunchKernelGGL(k_lp_iso_flags, dim3(unsigned(n / 256 + 1)), dim3(256), 0, s, n, c.g->off, d_flag.as<int64_t>(), c.iso.as<uint32_t>());
    if (int rc = exclusive_scan_i64(d_flag.as<const int64_t>(), d_pos.as<int64_t>(), n + 1, s)) return rc;
    int64_t n_iso = 0;
    GMSX_HIP(hipMemcpy(&n_iso, d_pos.as<int64_t>() + n, 8, hipMemcpyDeviceToHost));
    if (n_iso < 0 || n_iso > n) return GMSX_ERR_KERNEL;
    if (int rc = dalloc<int32_t>(d_list, n_iso)) return rc;
    hipLaunchKernelGGL(k_lp_iso_compact, dim3(unsigned(n / 256 + 1)), dim3(256), 0, s, n, d_flag.as<const int64_t>(), d_pos.as<const int64_t>(), d_list.as<int32_t>(),
                       n_iso, c.flags.as<Flags>());
    c.launches += 2;
    list.resize(size_t(n_iso));
    if (n_iso > 0) GMSX_HIP(hipMemcpyAsync(list.data(), d_list.p, size_t(n_iso) * 4, hipMemcpyDeviceToHost, s));
    return lp_flags_clear(c);
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_link_prediction(const gmsx_graph *g, int metric, int64_t q, int part, int nparts, int32_t *u, int32_t *v, double *scores, int64_t capacity,
                         gmsx_link_prediction_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || !u || !v || !scores || q < 1 || metric < GMSX_SIM_JACCARD || metric > GMSX_SIM_PREF_ATTACHMENT || nparts < 1 || part < 0 ||
            part >= nparts || capacity < std::min<int64_t>(q, int64_t(1) << 62))
            return GMSX_ERR_INVALID;
        if (q > (int64_t(1) << 27)) return GMSX_ERR_UNSUPPORTED;
        if (int rc = ensure_init()) return rc;
        const bool all = metric == GMSX_SIM_TOTAL_NEIGHBORS || metric == GMSX_SIM_PREF_ATTACHMENT;
        const int64_t n = g->n;
        if (all && n > kAllMaxN) return GMSX_ERR_UNSUPPORTED;
        gmsx_link_prediction_info res;
        std::memset(&res, 0, sizeof res);
        res.positive = all ? -1 : 0;
        if (n < 2) {
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        Ctx &cx = ctx();
        hipStream_t s = cx.stream;
        LpCall c;
        c.g = g;
        c.metric = metric;
        c.part = part;
        c.nparts = nparts;
        c.q = q;
        c.n_src = part < n ? (n - part + nparts - 1) / nparts : 0;
        c.words = (n + 31) / 32;
        const long long lds_maxn = std::max<long long>(0, std::min<long long>(opt_int("LP_LDS_MAXN", kLdsMaxN), kLdsMaxN));  // test hook: 0 = every bitmap in the slab
        c.use_lds = n <= lds_maxn;
        c.max_blocks = unsigned(std::max<int64_t>(1, std::min<int64_t>(c.n_src, int64_t(cx.compute_units > 0 ? cx.compute_units : 256) * kGridPerCu)));
        if (int rc = dalloc<Flags>(c.flags, 1)) return rc;
        GMSX_HIP(hipMemsetAsync(c.flags.p, 0, sizeof(Flags), s));
        if (!c.use_lds)
            if (int rc = dalloc<uint32_t>(c.arena, int64_t(c.max_blocks) * 2 * c.words)) return rc;
        size_t free_b = 0, total_b = 0;
        GMSX_HIP(hipMemGetInfo(&free_b, &total_b));
        c.budget_words = std::min<unsigned long long>(free_b / 4, kChunkCapBytes) / 4;
        const long long mb = opt_int("LP_SLAB_MB", 0);  // test hook: a smaller budget = more chunks, the same output
        if (mb >= 1) c.budget_words = std::min<unsigned long long>(c.budget_words, ((unsigned long long)mb << 20) / 4);
        GMSX_HIP(hipEventRecord(cx.ev[0], s));

        std::vector<Entry> best;  // in the rule's order, best first
        if (c.n_src > 0) {
            if (all) {
                int64_t total = 0;
                if (int rc = lp_scored_class(c, kClsAll, q, &total, best)) return rc;
                if (!best.empty()) res.classes |= kBitAll;
            } else {
                std::vector<int32_t> iso_list;
                if (metric == GMSX_SIM_JACCARD || metric == GMSX_SIM_OVERLAP)
                    if (int rc = lp_isolated(c, iso_list)) return rc;
                if (metric == GMSX_SIM_JACCARD) {
                    for (size_t a = 0; a < iso_list.size() && int64_t(best.size()) < q; ++a) {
                        if (iso_list[a] % nparts != part) continue;
                        for (size_t b = a + 1; b < iso_list.size() && int64_t(best.size()) < q; ++b) best.push_back(Entry{iso_list[a], iso_list[b], 1.0});
                    }
                    if (!best.empty()) res.classes |= kBitOne;
                }
                const size_t before_pos = best.size();
                if (int rc = lp_scored_class(c, kClsPos, q - int64_t(best.size()), &res.positive, best)) return rc;
                if (best.size() > before_pos) res.classes |= kBitPos;
                const size_t before_zero = best.size();
                if (int64_t(best.size()) < q)
                    if (int rc = lp_zero_class(c, q - int64_t(best.size()), best)) return rc;
                if (best.size() > before_zero) res.classes |= kBitZero;
            }
        }
        GMSX_HIP(hipEventRecord(cx.ev[1], s));
        if (int rc = lp_flags_clear(c)) return rc;  // the caller's arrays are written only behind a zero flag word
        float ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&ms, cx.ev[0], cx.ev[1]));
        const int64_t found = int64_t(best.size());
        if (found > q || found > capacity) return GMSX_ERR_KERNEL;
        for (int64_t i = 0; i < found; ++i) {
            const Entry &e = best[size_t(i)];
            if (e.u < 0 || e.v <= e.u || e.v >= n || e.u % nparts != part) return GMSX_ERR_KERNEL;
        }
        for (int64_t i = 0; i < found; ++i) {  // worst first, as the reference returns them
            const Entry &e = best[size_t(found - 1 - i)];
            u[i] = e.u;
            v[i] = e.v;
            scores[i] = e.score;
        }
        res.found = found;
        res.scored = c.scored;
        res.chunks = c.chunks;
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), 0.0, uint64_t(c.scored), 0, 0, c.launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_link_prediction_precision(const gmsx_graph *g_test, int64_t n_pred, const int32_t *u, const int32_t *v, int64_t *true_positives, int64_t *true_count,
                                   double *precision, double *recall, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g_test || n_pred < 0 || (n_pred > 0 && (!u || !v)) || n_pred >= (int64_t(1) << 32)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &cx = ctx();
        hipStream_t s = cx.stream;
        unsigned long long tp = 0;
        float ms = 0.f;
        int launches = 0;
        if (n_pred > 0) {
            DevBuf du, dv, dk, ds, dtmp, dflags, dtp;
            if (int rc = dalloc<int32_t>(du, n_pred)) return rc;
            if (int rc = dalloc<int32_t>(dv, n_pred)) return rc;
            if (int rc = dalloc<unsigned long long>(dk, n_pred)) return rc;
            if (int rc = dalloc<unsigned long long>(ds, n_pred)) return rc;
            if (int rc = dalloc<Flags>(dflags, 1)) return rc;
            if (int rc = dalloc<unsigned long long>(dtp, 1)) return rc;
            GMSX_HIP(hipMemcpyAsync(du.p, u, size_t(n_pred) * 4, hipMemcpyHostToDevice, s));
            GMSX_HIP(hipMemcpyAsync(dv.p, v, size_t(n_pred) * 4, hipMemcpyHostToDevice, s));
            GMSX_HIP(hipMemsetAsync(dflags.p, 0, sizeof(Flags), s));
            GMSX_HIP(hipMemsetAsync(dtp.p, 0, 8, s));
            GMSX_HIP(hipEventRecord(cx.ev[0], s));
            hipLaunchKernelGGL(k_lp_norm, dim3(unsigned((n_pred + 255) / 256)), dim3(256), 0, s, g_test->n, n_pred, du.as<const int32_t>(), dv.as<const int32_t>(),
                               dk.as<unsigned long long>(), dflags.as<Flags>());
            Flags bad = 1;
            GMSX_HIP(hipMemcpyAsync(&bad, dflags.p, sizeof bad, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            GMSX_HIP(hipGetLastError());
            if (bad) return GMSX_ERR_INVALID;  // u == v or an id outside [0, n)
            size_t tmp_bytes = 0;
            GMSX_HIP(rocprim::radix_sort_keys(nullptr, tmp_bytes, dk.as<unsigned long long>(), ds.as<unsigned long long>(), size_t(n_pred), 0, 64, s));
            if (int rc = dalloc<char>(dtmp, int64_t(tmp_bytes))) return rc;
            GMSX_HIP(rocprim::radix_sort_keys(dtmp.p, tmp_bytes, dk.as<unsigned long long>(), ds.as<unsigned long long>(), size_t(n_pred), 0, 64, s));
            const int64_t blocks = std::min<int64_t>((n_pred + 255) / 256, int64_t(cx.compute_units > 0 ? cx.compute_units : 256) * 16);
            hipLaunchKernelGGL(k_lp_contains, dim3(unsigned(blocks)), dim3(256), 0, s, g_test->off, g_test->adj, g_test->n, n_pred, ds.as<const unsigned long long>(),
                               dtp.as<unsigned long long>());
            GMSX_HIP(hipEventRecord(cx.ev[1], s));
            GMSX_HIP(hipMemcpyAsync(&tp, dtp.p, 8, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            GMSX_HIP(hipGetLastError());
            GMSX_HIP(hipEventElapsedTime(&ms, cx.ev[0], cx.ev[1]));
            launches = 3;
        }
        const int64_t tc = g_test->nnz / 2;
        if (int64_t(tp) > tc || int64_t(tp) > n_pred) return GMSX_ERR_KERNEL;
        if (true_positives) *true_positives = int64_t(tp);
        if (true_count) *true_count = tc;
        // evaluation.h:119-121 as plain double divisions; the reference divides by zero where a denominator is 0 — 0.0 here
        if (precision) *precision = n_pred > 0 ? double(int64_t(tp)) / double(n_pred) : 0.0;
        if (recall) *recall = tc > 0 ? double(int64_t(tp)) / double(tc) : 0.0;
        if (stats) *stats = gmsx_stats{double(ms), 0.0, uint64_t(n_pred), 0, 0, launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
