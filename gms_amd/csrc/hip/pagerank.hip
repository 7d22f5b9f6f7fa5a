// PageRank on gfx950, over the uploaded CSR: gmsx_pagerank and gmsx_pagerank_residual (representations/graphs/log_graph/pr.cc: PageRankPull,
// PRVerifier).  The definitions are those of include/gmsx.h.  A sweep is one pull over the whole CSR:
//   new[u] = (1 - damping) t[u] + damping Σ_{v in N(u)} contrib[v]  (+ damping D t[u] under GMSX_PR_DANGLING),  contrib[v] = score[v] / deg(v)
// in the storage type S (double, or float under GMSX_PR_FLOAT32); every sum is taken in double.  No floating-point atomic is used.
//
// THE RULE.  A row's sum is a function of the row's length `len` alone:
//   len = 0                        nothing is summed (class 0); contrib of such a vertex is 0 and never divided
//   1 <= len <= kPrLaneRow         one lane adds the entries in ascending position (class 1)
//   kPrLaneRow < len <= kPrGroupRow   a 16-lane group: lane l adds the entries l, l + 16, … in ascending position, then the 16 partial sums
//                                  meet in the shuffle tree 8, 4, 2, 1 (class 2)
//   len > kPrGroupRow              the row is cut into chunks of kPrChunk entries (the last one shorter); a wave per chunk: lane l adds the
//                                  entries l, l + 64, … of the chunk, the shuffle tree 32, 16, … 1 gives the chunk's sum, which is stored to the
//                                  chunk's slot; ONE owner adds the slots in ascending chunk order (class 3)
// The three constants are part of the rule, not options.
//
// THE CLASSES are built once per handle (ensure_pr_bins: count per block of 256 vertices, scan, fill — every class ascending in the vertex id, no
// atomic cursor) and cached on the handle: `pr_bins` is the n vertices class by class; the long rows' chunks are numbered by a scan over the
// long class (pr_first), slot s belongs to long row pr_slot_row[s].
//
// THE REDUCTIONS.  A workgroup owns 256 consecutive positions of ONE class of pr_bins.  Its error partial Σ |new - old| is the tree of block_sum
// (per wave 32, 16, … 1, then the four waves in order) over its positions and goes to its own cell of `part`; k_pr_reduce — one workgroup —
// adds the cells (thread t the cells t, t + 1024, … ascending, then the same tree over 16 waves).  The dangling mass D of the next sweep is reduced
// the same way over the class-0 workgroups; sum, max_score and argmax of the result over blocks of 256 consecutive vertex ids.  Nothing of this
// depends on a grid size or on the order in which workgroups run, so scores and every info field are facts about (graph, arguments).
//
// A SWEEP is k_pr_zero, k_pr_lane, k_pr_group, k_pr_long + k_pr_long_sum (each only if its class is not empty) and k_pr_reduce.  The owner of u
// stores new[u] and the next sweep's contrib[u] (both arrays double-buffered) in its epilogue (pr_finish): the CSR is read once per sweep and
// there is no pass over the vertices beside it.  The host reads the control block (error, flag) behind every sweep.  gmsx_pagerank_residual is the
// same kernels with kStore = false: one sweep over the caller's scores, only the error is kept.
#include "device_buffer.hpp"
#include "device_graph.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

// first guesses, not tuned values; they are constants of the summation rule (see above), not options
constexpr int kPrLaneRow = 16;     // longest row one lane adds alone (msbfs.hip's lane limit)
constexpr int kPrGroupRow = 1024;  // longest row a 16-lane group adds (frontier_rounds.hpp's kLongRow)
constexpr int kPrChunk = 4096;     // entries of a long row one wave adds (traversal.hip's kBcChunk)
constexpr int kPrGroup = 16;
constexpr int kPrBlock = 256;      // positions (or vertices) one workgroup reduces

struct PrCtrl {
    int32_t flag;    // a position, vertex or slot outside its bound, or a non-finite score
    int32_t argmax;
    double error, dangling, sum, max_score;
};

__host__ __device__ inline int pr_class(int64_t len) { return len <= 0 ? 0 : len <= kPrLaneRow ? 1 : len <= kPrGroupRow ? 2 : 3; }

// ---- the classes ---------------------------------------------------------------------------------------------------------------------------

// cnt[c * nb + b] = vertices of class c among the 256 of block b
__global__ __launch_bounds__(256) void k_pr_count(int64_t n, const int64_t *__restrict__ off, int64_t nb, int64_t *__restrict__ cnt) {
    __shared__ int32_t s_c[4][4];
    const int64_t v = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    const int cls = v < n ? pr_class(off[v + 1] - off[v]) : -1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = 0; c < 4; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (lane == 0) s_c[wave][c] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int c = threadIdx.x;
        cnt[int64_t(c) * nb + blockIdx.x] = int64_t(s_c[0][c] + s_c[1][c] + s_c[2][c] + s_c[3][c]);
    }
}

// pos = the exclusive scan of cnt (4 nb + 1 values): vertex v goes to pos[cls * nb + block] + its rank among the block's vertices of its class
__global__ __launch_bounds__(256) void k_pr_fill(int64_t n, const int64_t *__restrict__ off, int64_t nb, const int64_t *__restrict__ pos,
                                                 int32_t *__restrict__ bins, PrCtrl *__restrict__ ctrl) {
    __shared__ int32_t s_c[4][4];
    const int64_t v = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    const int cls = v < n ? pr_class(off[v + 1] - off[v]) : -1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int rank = 0;
    for (int c = 0; c < 4; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (lane == 0) s_c[wave][c] = __popcll(m);
        if (cls == c) rank = __popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (cls < 0) return;
    for (int w = 0; w < wave; ++w) rank += s_c[w][cls];
    const int64_t p = pos[int64_t(cls) * nb + blockIdx.x] + rank;
    if (p >= 0 && p < n && p < pos[int64_t(cls + 1) * nb]) bins[p] = int32_t(v);
    else ctrl->flag = 1;
}

__global__ __launch_bounds__(256) void k_pr_long_chunks(int64_t n3, const int32_t *__restrict__ longs, const int64_t *__restrict__ off,
                                                        int64_t *__restrict__ chunks) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const int32_t u = longs[i];
    chunks[i] = (off[u + 1] - off[u] + kPrChunk - 1) / kPrChunk;
}

// slot_row[first[i] + c] = i for the chunks c of long row i: a 16-lane group per row
__global__ __launch_bounds__(256) void k_pr_slot_rows(int64_t n3, const int64_t *__restrict__ first, int64_t nslots, int32_t *__restrict__ slot_row,
                                                      PrCtrl *__restrict__ ctrl) {
    const int lane = threadIdx.x & (kPrGroup - 1);
    const int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kPrGroup;
    if (i >= n3) return;
    const int64_t s0 = first[i], s1 = first[i + 1];
    if (s0 < 0 || s1 < s0 || s1 > nslots) {
        ctrl->flag = 1;
        return;
    }
    for (int64_t s = s0 + lane; s < s1; s += kPrGroup) slot_row[s] = int32_t(i);
}

// ---- a sweep -------------------------------------------------------------------------------------------------------------------------------

template <class S>
struct PrArgs {
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    const int32_t *bins;   // the n vertices, class by class
    const double *t;       // the teleport vector, normalised
    const S *cur;          // scores of the last sweep
    S *nxt;
    const S *contrib;      // cur[v] / deg(v); 0 for deg(v) = 0
    S *cnext;
    double *part;          // a cell per workgroup of a sweep: its error partial
    double *dpart;         // … per class-0 workgroup: its share of the next sweep's dangling mass
    const int32_t *slot_row;
    const int64_t *first;  // [long rows + 1] first slot of a long row
    double *slots;
    int64_t nslots;
    PrCtrl *ctrl;
    double base, damping;  // base = 1 - damping
};

// u's single owner: the new score from the finished row sum, the stores, and the error term
template <class S, bool kDangling, bool kStore>
__device__ __forceinline__ double pr_finish(const PrArgs<S> &a, int32_t u, double sum, int64_t deg, double dd, double *nw_out) {
    // every product and sum is rounded on its own (no fused multiply-add): the value is the one the definition's operations give one by one
#pragma clang fp contract(off)
    const double tu = a.t[u];
    double nw = a.base * tu + a.damping * sum;
    if (kDangling) nw = nw + dd * tu;
    const S ns = S(nw);
    if (kStore) {
        a.nxt[u] = ns;
        a.cnext[u] = deg > 0 ? S(double(ns) / double(deg)) : S(0);
    }
    if (!(fabs(double(ns)) <= 1.7e308)) a.ctrl->flag = 1;  // (NaN or infinity)
    *nw_out = double(ns);
    return fabs(double(ns) - double(a.cur[u]));
}

// class 0, positions [lo, lo + cnt) of bins
template <class S, bool kDangling, bool kStore>
__global__ __launch_bounds__(256) void k_pr_zero(PrArgs<S> a, int64_t lo, int64_t cnt, int64_t pbase) {
    __shared__ double s_w[4];
    const int64_t p = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    const double dd = kDangling ? a.damping * a.ctrl->dangling : 0.0;
    double e = 0.0, nw = 0.0;
    if (p < cnt) {
        const int32_t u = a.bins[lo + p];
        if (u >= 0 && int64_t(u) < a.n) e = pr_finish<S, kDangling, kStore>(a, u, 0.0, 0, dd, &nw);
        else a.ctrl->flag = 1;
    }
    e = block_sum<4>(e, s_w);
    if (threadIdx.x == 0) a.part[pbase + blockIdx.x] = e;
    if (kDangling && kStore) {
        nw = block_sum<4>(nw, s_w);
        if (threadIdx.x == 0) a.dpart[blockIdx.x] = nw;
    }
}

// the dangling mass of the FIRST sweep: Σ cur over class 0, in the same cells
template <class S>
__global__ __launch_bounds__(256) void k_pr_zero_sum(PrArgs<S> a, int64_t lo, int64_t cnt) {
    __shared__ double s_w[4];
    const int64_t p = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    double x = 0.0;
    if (p < cnt) {
        const int32_t u = a.bins[lo + p];
        if (u >= 0 && int64_t(u) < a.n) x = double(a.cur[u]);
        else a.ctrl->flag = 1;
    }
    x = block_sum<4>(x, s_w);
    if (threadIdx.x == 0) a.dpart[blockIdx.x] = x;
}

// class 1: a lane per row
template <class S, bool kDangling, bool kStore>
__global__ __launch_bounds__(256) void k_pr_lane(PrArgs<S> a, int64_t lo, int64_t cnt, int64_t pbase) {
    __shared__ double s_w[4];
    const int64_t p = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    const double dd = kDangling ? a.damping * a.ctrl->dangling : 0.0;
    double e = 0.0, nw = 0.0;
    if (p < cnt) {
        const int32_t u = a.bins[lo + p];
        if (u >= 0 && int64_t(u) < a.n) {
            const int64_t j0 = a.off[u], j1 = a.off[u + 1];
            double sum = 0.0;
            for (int64_t j = j0; j < j1; ++j) sum += double(a.contrib[a.adj[j]]);
            e = pr_finish<S, kDangling, kStore>(a, u, sum, j1 - j0, dd, &nw);
        } else {
            a.ctrl->flag = 1;
        }
    }
    e = block_sum<4>(e, s_w);
    if (threadIdx.x == 0) a.part[pbase + blockIdx.x] = e;
}

// class 2: a 16-lane group per row; the 16 groups of a workgroup share its 256 positions, group g takes g, g + 16, …
template <class S, bool kDangling, bool kStore>
__global__ __launch_bounds__(256) void k_pr_group(PrArgs<S> a, int64_t lo, int64_t cnt, int64_t pbase) {
    __shared__ double s_w[4];
    const int lane = threadIdx.x & (kPrGroup - 1), grp = threadIdx.x / kPrGroup;
    const double dd = kDangling ? a.damping * a.ctrl->dangling : 0.0;
    double e = 0.0, nw = 0.0;
    for (int r = grp; r < kPrBlock; r += 256 / kPrGroup) {
        const int64_t p = int64_t(blockIdx.x) * kPrBlock + r;  // (uniform in the group)
        if (p >= cnt) break;
        const int32_t u = a.bins[lo + p];
        if (u < 0 || int64_t(u) >= a.n) {
            a.ctrl->flag = 1;
            continue;
        }
        const int64_t j0 = a.off[u], j1 = a.off[u + 1];
        double sum = 0.0;
        for (int64_t j = j0 + lane; j < j1; j += kPrGroup) sum += double(a.contrib[a.adj[j]]);
        sum = wave_sum<kPrGroup>(sum);
        if (lane == 0) e += pr_finish<S, kDangling, kStore>(a, u, sum, j1 - j0, dd, &nw);
    }
    e = block_sum<4>(e, s_w);
    if (threadIdx.x == 0) a.part[pbase + blockIdx.x] = e;
}

// class 3, the chunks: a wave per slot
template <class S>
__global__ __launch_bounds__(256) void k_pr_long(PrArgs<S> a, int64_t lo, int64_t cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t s = wave0; s < a.nslots; s += waves) {
        const int64_t i = a.slot_row[s];
        if (i < 0 || i >= cnt) {
            a.ctrl->flag = 1;
            continue;
        }
        const int32_t u = a.bins[lo + i];
        if (u < 0 || int64_t(u) >= a.n) {
            a.ctrl->flag = 1;
            continue;
        }
        const int64_t j0 = a.off[u], j1 = a.off[u + 1];
        const int64_t c = s - a.first[i];
        const int64_t c0 = j0 + c * kPrChunk, c1 = min(j1, c0 + kPrChunk);
        if (c < 0 || c0 >= j1) {
            a.ctrl->flag = 1;
            continue;
        }
        double sum = 0.0;
        for (int64_t j = c0 + lane; j < c1; j += 64) sum += double(a.contrib[a.adj[j]]);
        sum = wave_sum(sum);
        if (lane == 0) a.slots[s] = sum;
    }
}

// … and their owners: the slots of a row in ascending chunk order
template <class S, bool kDangling, bool kStore>
__global__ __launch_bounds__(256) void k_pr_long_sum(PrArgs<S> a, int64_t lo, int64_t cnt, int64_t pbase) {
    __shared__ double s_w[4];
    const int64_t p = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    const double dd = kDangling ? a.damping * a.ctrl->dangling : 0.0;
    double e = 0.0, nw = 0.0;
    if (p < cnt) {
        const int32_t u = a.bins[lo + p];
        const int64_t s0 = a.first[p], s1 = a.first[p + 1];
        if (u >= 0 && int64_t(u) < a.n && s0 >= 0 && s0 <= s1 && s1 <= a.nslots) {
            const int64_t len = a.off[u + 1] - a.off[u];
            if (s1 - s0 != (len + kPrChunk - 1) / kPrChunk) a.ctrl->flag = 1;
            double sum = 0.0;
            for (int64_t s = s0; s < s1; ++s) sum += a.slots[s];
            e = pr_finish<S, kDangling, kStore>(a, u, sum, len, dd, &nw);
        } else {
            a.ctrl->flag = 1;
        }
    }
    e = block_sum<4>(e, s_w);
    if (threadIdx.x == 0) a.part[pbase + blockIdx.x] = e;
}

// ONE workgroup: the cells of a sweep
__global__ __launch_bounds__(1024) void k_pr_reduce(const double *__restrict__ part, int64_t cells, const double *__restrict__ dpart, int64_t dcells,
                                                    bool want_error, bool want_dangling, PrCtrl *__restrict__ ctrl) {
    __shared__ double s_w[16];
    if (want_error) {
        double e = 0.0;
        for (int64_t i = threadIdx.x; i < cells; i += 1024) e += part[i];
        e = block_sum<16>(e, s_w);
        if (threadIdx.x == 0) ctrl->error = e;
    }
    if (want_dangling) {
        double d = 0.0;
        for (int64_t i = threadIdx.x; i < dcells; i += 1024) d += dpart[i];
        d = block_sum<16>(d, s_w);
        if (threadIdx.x == 0) ctrl->dangling = d;
    }
}

// the start: cur = S(in), contrib = cur / deg
template <class S>
__global__ __launch_bounds__(256) void k_pr_init(int64_t n, const int64_t *__restrict__ off, const double *__restrict__ in, S *__restrict__ cur,
                                                 S *__restrict__ contrib) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const S sc = S(in[v]);
    const int64_t deg = off[v + 1] - off[v];
    cur[v] = sc;
    contrib[v] = deg > 0 ? S(double(sc) / double(deg)) : S(0);
}

// the larger score; ties: the smaller id
__device__ __forceinline__ void pr_best(double &m, int32_t &at, double m2, int32_t at2) {
    if (at2 >= 0 && (at < 0 || m2 > m || (m2 == m && at2 < at))) {
        m = m2;
        at = at2;
    }
}

// the result: per block of 256 vertex ids the sum (block_sum's tree), the largest score and where
template <class S>
__global__ __launch_bounds__(256) void k_pr_final(int64_t n, const S *__restrict__ score, double *__restrict__ fsum, double *__restrict__ fmax,
                                                  int32_t *__restrict__ farg, PrCtrl *__restrict__ ctrl) {
    __shared__ double s_w[4];
    __shared__ double s_m[4];
    __shared__ int32_t s_a[4];
    const int64_t v = int64_t(blockIdx.x) * kPrBlock + threadIdx.x;
    double x = 0.0, m = 0.0;
    int32_t at = -1;
    if (v < n) {
        x = double(score[v]);
        if (!(fabs(x) <= 1.7e308)) ctrl->flag = 1;
        m = x;
        at = int32_t(v);
    }
    wave_fold2(m, at, pr_best);
    if ((threadIdx.x & 63) == 0) {
        s_m[threadIdx.x >> 6] = m;
        s_a[threadIdx.x >> 6] = at;
    }
    x = block_sum<4>(x, s_w);  // (its barriers publish s_m and s_a, too)
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) pr_best(m, at, s_m[w], s_a[w]);
        fsum[blockIdx.x] = x;
        fmax[blockIdx.x] = m;
        farg[blockIdx.x] = at;
    }
}

__global__ __launch_bounds__(1024) void k_pr_final_reduce(int64_t cells, const double *__restrict__ fsum, const double *__restrict__ fmax,
                                                          const int32_t *__restrict__ farg, PrCtrl *__restrict__ ctrl) {
    __shared__ double s_w[16];
    __shared__ double s_m[16];
    __shared__ int32_t s_a[16];
    double x = 0.0, m = 0.0;
    int32_t at = -1;
    for (int64_t i = threadIdx.x; i < cells; i += 1024) {
        x += fsum[i];
        pr_best(m, at, fmax[i], farg[i]);
    }
    wave_fold2(m, at, pr_best);
    if ((threadIdx.x & 63) == 0) {
        s_m[threadIdx.x >> 6] = m;
        s_a[threadIdx.x >> 6] = at;
    }
    x = block_sum<16>(x, s_w);
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) pr_best(m, at, s_m[w], s_a[w]);
        ctrl->sum = x;
        ctrl->max_score = m;
        ctrl->argmax = at;
    }
}

// ---- the host ------------------------------------------------------------------------------------------------------------------------------

inline unsigned blocks_of(int64_t count, int per = kPrBlock) { return unsigned((count + per - 1) / per); }

// the classes of g, built at its first call and kept on the handle
int ensure_pr_bins(const gmsx_graph *g, int *launches) {
    if (g->pr.ready) return GMSX_OK;
    hipStream_t s = ctx().stream;
    const int64_t n = g->n, nb = (n + kPrBlock - 1) / kPrBlock;
    DevBuf d_cnt, d_pos, d_ctrl, d_chunks;
    DevArr<int32_t> d_bins, d_slot_row;  // what the graph keeps
    DevArr<int64_t> d_first;
    if (int rc = dalloc<int64_t>(d_cnt, 4 * nb + 1)) return rc;
    if (int rc = dalloc<int64_t>(d_pos, 4 * nb + 1)) return rc;
    if (int rc = dalloc<int32_t>(d_bins, n)) return rc;
    if (int rc = dalloc<PrCtrl>(d_ctrl, 1)) return rc;
    GMSX_HIP(hipMemsetAsync(d_cnt.p, 0, size_t(4 * nb + 1) * sizeof(int64_t), s));
    GMSX_HIP(hipMemsetAsync(d_ctrl.p, 0, sizeof(PrCtrl), s));
    hipLaunchKernelGGL(k_pr_count, dim3(unsigned(nb)), dim3(256), 0, s, n, g->off, nb, d_cnt.as<int64_t>());
    ++*launches;
    if (int rc = exclusive_scan_i64(d_cnt.as<const int64_t>(), d_pos.as<int64_t>(), 4 * nb + 1, s)) return rc;
    int64_t base[5] = {0, 0, 0, 0, 0};
    for (int c = 0; c <= 4; ++c)
        GMSX_HIP(hipMemcpyAsync(&base[c], d_pos.as<int64_t>() + int64_t(c) * nb, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (base[0] != 0 || base[4] != n) return GMSX_ERR_KERNEL;  // (a bin total that is not n)
    for (int c = 0; c < 4; ++c)
        if (base[c + 1] < base[c]) return GMSX_ERR_KERNEL;
    hipLaunchKernelGGL(k_pr_fill, dim3(unsigned(nb)), dim3(256), 0, s, n, g->off, nb, d_pos.as<const int64_t>(), d_bins.as<int32_t>(),
                       d_ctrl.as<PrCtrl>());
    ++*launches;
    const int64_t n3 = n - base[3];
    int64_t nslots = 0;
    if (n3 > 0) {
        if (int rc = dalloc<int64_t>(d_chunks, n3 + 1)) return rc;
        if (int rc = dalloc<int64_t>(d_first, n3 + 1)) return rc;
        GMSX_HIP(hipMemsetAsync(d_chunks.p, 0, size_t(n3 + 1) * sizeof(int64_t), s));
        hipLaunchKernelGGL(k_pr_long_chunks, dim3(blocks_of(n3)), dim3(256), 0, s, n3, d_bins.as<const int32_t>() + base[3], g->off, d_chunks.as<int64_t>());
        ++*launches;
        if (int rc = exclusive_scan_i64(d_chunks.as<const int64_t>(), d_first.as<int64_t>(), n3 + 1, s)) return rc;
        GMSX_HIP(hipMemcpyAsync(&nslots, d_first.as<int64_t>() + n3, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (nslots < n3 || nslots > g->nnz / kPrChunk + n3) return GMSX_ERR_KERNEL;
        if (int rc = dalloc<int32_t>(d_slot_row, nslots)) return rc;
        hipLaunchKernelGGL(k_pr_slot_rows, dim3(blocks_of(n3 * kPrGroup)), dim3(256), 0, s, n3, d_first.as<const int64_t>(), nslots,
                           d_slot_row.as<int32_t>(), d_ctrl.as<PrCtrl>());
        ++*launches;
    }
    PrCtrl h;
    GMSX_HIP(hipMemcpyAsync(&h, d_ctrl.p, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (h.flag) return GMSX_ERR_KERNEL;  // (a bin list that would overflow)
    g->pr.bins = std::move(d_bins);
    g->pr.first = std::move(d_first);  // (both empty when there is no long row)
    g->pr.slot_row = std::move(d_slot_row);
    for (int c = 0; c <= 4; ++c) g->pr.base[c] = base[c];
    g->pr.slots = nslots;
    g->pr.ready = true;
    return GMSX_OK;
}

struct PrOut {
    gmsx_pagerank_info info;
    double kernel_ms = 0.0, setup_ms = 0.0;
    int launches = 0;
};

// one sweep on stream s; the cells of `part`: class by class, a cell per 256 positions
template <class S, bool kDangling, bool kStore>
void pr_sweep(const gmsx_graph *g, const PrArgs<S> &a, hipStream_t s, unsigned long_grid, int *launches) {
    const int64_t *b = g->pr.base;
    int64_t pbase = 0;
    const int64_t c0 = b[1] - b[0], c1 = b[2] - b[1], c2 = b[3] - b[2], c3 = b[4] - b[3];
    if (c0 > 0) {
        hipLaunchKernelGGL((k_pr_zero<S, kDangling, kStore>), dim3(blocks_of(c0)), dim3(256), 0, s, a, b[0], c0, pbase);
        ++*launches;
    }
    pbase += blocks_of(c0);
    if (c1 > 0) {
        hipLaunchKernelGGL((k_pr_lane<S, kDangling, kStore>), dim3(blocks_of(c1)), dim3(256), 0, s, a, b[1], c1, pbase);
        ++*launches;
    }
    pbase += blocks_of(c1);
    if (c2 > 0) {
        hipLaunchKernelGGL((k_pr_group<S, kDangling, kStore>), dim3(blocks_of(c2)), dim3(256), 0, s, a, b[2], c2, pbase);
        ++*launches;
    }
    pbase += blocks_of(c2);
    if (c3 > 0) {
        hipLaunchKernelGGL((k_pr_long<S>), dim3(long_grid), dim3(256), 0, s, a, b[3], c3);
        hipLaunchKernelGGL((k_pr_long_sum<S, kDangling, kStore>), dim3(blocks_of(c3)), dim3(256), 0, s, a, b[3], c3, pbase);
        *launches += 2;
    }
}

// start: the n scores the first sweep reads (the normalised teleport vector, or the caller's scores for the residual)
template <class S>
int pr_run(const gmsx_graph *g, const std::vector<double> &t, const double *start, double damping, int32_t max_iters, double tolerance, bool dangling,
           bool store, std::vector<S> *h_scores, PrOut *out) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = ensure_pr_bins(g, &out->launches)) return rc;
    const int64_t *b = g->pr.base;
    const int64_t cells = int64_t(blocks_of(b[1] - b[0])) + blocks_of(b[2] - b[1]) + blocks_of(b[3] - b[2]) + blocks_of(b[4] - b[3]);
    const int64_t dcells = blocks_of(b[1] - b[0]), vcells = blocks_of(n);
    DevBuf d_t, d_in, d_s0, d_s1, d_c0, d_c1, d_part, d_dpart, d_slots, d_fmax, d_farg, d_ctrl;
    if (int rc = dalloc<double>(d_t, n)) return rc;
    if (start)
        if (int rc = dalloc<double>(d_in, n)) return rc;
    if (int rc = dalloc<S>(d_s0, n)) return rc;
    if (int rc = dalloc<S>(d_s1, n)) return rc;
    if (int rc = dalloc<S>(d_c0, n)) return rc;
    if (int rc = dalloc<S>(d_c1, n)) return rc;
    if (int rc = dalloc<double>(d_part, std::max(cells, vcells))) return rc;
    if (int rc = dalloc<double>(d_dpart, dcells)) return rc;
    if (int rc = dalloc<double>(d_slots, g->pr.slots)) return rc;
    if (int rc = dalloc<double>(d_fmax, vcells)) return rc;
    if (int rc = dalloc<int32_t>(d_farg, vcells)) return rc;
    if (int rc = dalloc<PrCtrl>(d_ctrl, 1)) return rc;
    PrCtrl *ctrl = d_ctrl.as<PrCtrl>();
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(PrCtrl), s));
    GMSX_HIP(hipMemcpyAsync(d_t.p, t.data(), size_t(n) * sizeof(double), hipMemcpyHostToDevice, s));
    if (start) GMSX_HIP(hipMemcpyAsync(d_in.p, start, size_t(n) * sizeof(double), hipMemcpyHostToDevice, s));
    S *score[2] = {d_s0.as<S>(), d_s1.as<S>()}, *contrib[2] = {d_c0.as<S>(), d_c1.as<S>()};
    hipLaunchKernelGGL((k_pr_init<S>), dim3(blocks_of(n)), dim3(256), 0, s, n, g->off, start ? d_in.as<const double>() : d_t.as<const double>(), score[0],
                       contrib[0]);
    ++out->launches;
    PrArgs<S> a{n, g->off, g->adj, g->pr.bins, d_t.as<const double>(), score[0], score[1], contrib[0], contrib[1], d_part.as<double>(),
                d_dpart.as<double>(), g->pr.slot_row, g->pr.first, d_slots.as<double>(), g->pr.slots, ctrl, 1.0 - damping, damping};
    if (dangling) {  // D of the first sweep
        if (dcells > 0) {
            hipLaunchKernelGGL((k_pr_zero_sum<S>), dim3(unsigned(dcells)), dim3(256), 0, s, a, b[0], b[1] - b[0]);
            ++out->launches;
        }
        hipLaunchKernelGGL(k_pr_reduce, dim3(1), dim3(1024), 0, s, a.part, int64_t(0), a.dpart, dcells, false, true, ctrl);
        ++out->launches;
    }
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    const unsigned long_grid = unsigned(std::max<int64_t>(1, std::min<int64_t>((g->pr.slots + 3) / 4, int64_t(cus) * 8)));
    int cur = 0;
    int32_t iterations = 0;
    double error = 0.0;
    bool converged = false;
    PrCtrl h;
    std::memset(&h, 0, sizeof h);
    for (int32_t it = 0; it < max_iters; ++it) {
        a.cur = score[cur];
        a.nxt = score[cur ^ 1];
        a.contrib = contrib[cur];
        a.cnext = contrib[cur ^ 1];
        if (dangling) {
            if (store) pr_sweep<S, true, true>(g, a, s, long_grid, &out->launches);
            else pr_sweep<S, true, false>(g, a, s, long_grid, &out->launches);
        } else {
            if (store) pr_sweep<S, false, true>(g, a, s, long_grid, &out->launches);
            else pr_sweep<S, false, false>(g, a, s, long_grid, &out->launches);
        }
        hipLaunchKernelGGL(k_pr_reduce, dim3(1), dim3(1024), 0, s, a.part, cells, a.dpart, dcells, true, dangling && store, ctrl);
        ++out->launches;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.flag || !(h.error >= 0.0)) return GMSX_ERR_KERNEL;
        if (store) cur ^= 1;
        ++iterations;
        error = h.error;
        if (error < tolerance) {
            converged = true;
            break;
        }
    }
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    if (store) {  // the final reductions, over blocks of 256 vertex ids
        hipLaunchKernelGGL((k_pr_final<S>), dim3(unsigned(vcells)), dim3(256), 0, s, n, score[cur], d_part.as<double>(), d_fmax.as<double>(),
                           d_farg.as<int32_t>(), ctrl);
        hipLaunchKernelGGL(k_pr_final_reduce, dim3(1), dim3(1024), 0, s, vcells, d_part.as<const double>(), d_fmax.as<const double>(),
                           d_farg.as<const int32_t>(), ctrl);
        out->launches += 2;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        if (h_scores) {
            h_scores->resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_scores->data(), score[cur], size_t(n) * sizeof(S), hipMemcpyDeviceToHost, s));
        }
    }
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (h.flag) return GMSX_ERR_KERNEL;
    if (store && (h.argmax < 0 || int64_t(h.argmax) >= n || !(std::fabs(h.sum) <= 1.7e308))) return GMSX_ERR_KERNEL;
    float ms0 = 0.f, ms1 = 0.f, ms2 = 0.f;
    GMSX_HIP(hipEventElapsedTime(&ms0, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms1, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&ms2, c.ev[2], c.ev[3]));
    out->kernel_ms = double(ms1);
    out->setup_ms = double(ms0) + double(ms2);
    std::memset(&out->info, 0, sizeof out->info);
    out->info.iterations = iterations;
    out->info.converged = converged ? 1 : 0;
    out->info.argmax = store ? h.argmax : -1;
    out->info.error = error;
    out->info.sum = store ? h.sum : 0.0;
    out->info.max_score = store ? h.max_score : 0.0;
    out->info.isolated = b[1] - b[0];
    return GMSX_OK;
}

// the arguments that need no device and no handle
bool pr_args_ok(double damping, uint32_t flags) {
    if (!(damping >= 0.0 && damping <= 1.0)) return false;  // (NaN fails both)
    return (flags & ~uint32_t(GMSX_PR_DANGLING | GMSX_PR_FLOAT32)) == 0;
}

// t = teleport / Σ teleport (summed ascending, in double), or 1 / n; false: a negative, NaN or infinite entry, or sum 0
bool pr_teleport(int64_t n, const double *teleport, std::vector<double> &t) {
    t.resize(size_t(n));
    if (!teleport) {
        std::fill(t.begin(), t.end(), 1.0 / double(n));
        return true;
    }
    double sum = 0.0;
    for (int64_t v = 0; v < n; ++v) {
        if (!(teleport[v] >= 0.0) || std::isinf(teleport[v])) return false;
        sum += teleport[v];
    }
    if (!(sum > 0.0) || std::isinf(sum)) return false;
    for (int64_t v = 0; v < n; ++v) t[size_t(v)] = teleport[v] / sum;
    return true;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_pagerank(const gmsx_graph *g, double damping, int32_t max_iters, double tolerance, const double *teleport, uint32_t flags, double *scores,
                  gmsx_pagerank_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || !pr_args_ok(damping, flags) || max_iters < 0 || !(tolerance >= 0.0)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        if (n == 0) {
            std::memset(info, 0, sizeof *info);
            info->argmax = -1;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        std::vector<double> t;
        if (!pr_teleport(n, teleport, t)) return GMSX_ERR_INVALID;
        const bool dangling = (flags & GMSX_PR_DANGLING) != 0;
        PrOut out;
        std::vector<double> h64;
        std::vector<float> h32;
        if (flags & GMSX_PR_FLOAT32) {
            if (int rc = pr_run<float>(g, t, nullptr, damping, max_iters, tolerance, dangling, true, scores ? &h32 : nullptr, &out)) return rc;
        } else {
            if (int rc = pr_run<double>(g, t, nullptr, damping, max_iters, tolerance, dangling, true, scores ? &h64 : nullptr, &out)) return rc;
        }
        // the flag word was read as zero: the caller's arrays are written now
        if (scores) {
            if (flags & GMSX_PR_FLOAT32)
                for (int64_t v = 0; v < n; ++v) scores[v] = double(h32[size_t(v)]);
            else
                std::memcpy(scores, h64.data(), size_t(n) * sizeof(double));
        }
        *info = out.info;
        if (stats)
            *stats = gmsx_stats{out.kernel_ms, out.setup_ms, uint64_t(out.info.iterations) * uint64_t(g->nnz), 0, uint64_t(out.info.iterations),
                                out.launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_pagerank_residual(const gmsx_graph *g, const double *scores, double damping, const double *teleport, uint32_t flags, double *residual,
                           gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !residual || !pr_args_ok(damping, flags)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        if (n == 0) {
            *residual = 0.0;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        if (!scores) return GMSX_ERR_INVALID;
        std::vector<double> t;
        if (!pr_teleport(n, teleport, t)) return GMSX_ERR_INVALID;
        const bool dangling = (flags & GMSX_PR_DANGLING) != 0;
        PrOut out;
        if (flags & GMSX_PR_FLOAT32) {
            if (int rc = pr_run<float>(g, t, scores, damping, 1, 0.0, dangling, false, nullptr, &out)) return rc;
        } else {
            if (int rc = pr_run<double>(g, t, scores, damping, 1, 0.0, dangling, false, nullptr, &out)) return rc;
        }
        *residual = out.info.error;
        if (stats) *stats = gmsx_stats{out.kernel_ms, out.setup_ms, uint64_t(g->nnz), 0, 1, out.launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
