// Connected components and Jarvis–Patrick clustering on gfx950: one device union-find over the vertices of the uploaded CSR.
//   gmsx_connected_components   label[v] = smallest vertex id of v's component, over every edge or over the arcs a caller's byte mask keeps
//                               (the reference's ShiloachVishkin, representations/graphs/log_graph/cc.cc:40-72, converges to the same labels)
//   gmsx_jarvis_patrick         the same over the edges {u, v} with metric(N(u), N(v)) >= threshold; no reference counterpart
// The definitions are those of include/gmsx.h.
//
// THE UNION-FIND (cc_find, cc_link, the flatten and size kernels, their memory model and their caps) is union_find.hpp's: a root is only ever
// hooked under a SMALLER vertex id, so after a full flatten label[v] is the smallest vertex id of v's component.
//
// WORK DISTRIBUTION over CSR rows is row_classes.hpp's (a lane, a 16-lane group, a wave or a workgroup per row by its length; the bounds are
// CC_WAVE_ROW and CC_WG_ROW); CcLink, one template over the edge source, is the Op of its row pass.
//
// THE GIANT COMPONENT (Afforest's sampling; whole-graph call only).  Pass A links the first CC_SAMPLE neighbours of every vertex, a flatten
// follows, one workgroup reads the labels of 1024 seeded vertex ids and picks the most frequent label L (ties: the smaller), and pass B links the
// remaining neighbours of every vertex whose label is not L: the CSR is symmetric, so an edge from inside L to outside L is seen from its outside
// endpoint.  L changes how much work is skipped, never the result.  With an arc mask the kept arcs need not be visible from both sides, so pass
// B covers every vertex; Jarvis–Patrick is one pass over the edges.
//
// JARVIS–PATRICK (k_cc_jp).  Wave w of W takes the arcs w, w + W, w + 2 W, … — consecutive arcs of a hub's row, the dear ones, go to different
// waves, as the pairs of gmsx_vertex_similarity_batch do — 64 at a time: lane t finds the source of its arc by a binary search in off, then the
// wave works through the `u < v` arcs among them one after the other.  Such an arc is one wave_pair_similarity (pair_similarity.hpp, unchanged: the bits of
// gmsx_vertex_similarity_batch); score >= threshold (false for NaN) marks the arc for the lane that resolved it, and after the 64 arcs every lane
// links the endpoints of its own kept arc (up to 64 walks overlap instead of queueing on lane 0) and, where the caller asked for the mask,
// writes 1 to both arcs' bytes — the twin by a binary search of u in row v.  No score array and no edge list exist.  Every edge gets one wave:
// the workgroup-per-long-edge variant of truss.hip's support pass is not built here.
//
// INFO (k_cc_sizes of union_find.hpp, k_cc_info): the sizes per label; then per root: components, singletons, and the largest component as the
// maximum of size << 32 | ~label, i.e. ties go to the smaller label.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // load_now, store_now, wave_append, kGroup
#include "pair_similarity.hpp"
#include "row_classes.hpp"
#include "union_find.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace gmsx {

namespace {

constexpr int kCcSamples = 1024;   // vertex ids the giant-component vote reads
constexpr long long kCcSampleDefault = 2;  // a first guess (gmsx.h, OPTIONS)

// the call's small device block, zeroed per call and read once
struct CcAcc {
    int32_t error;   // the flag word: a cap was exceeded, an append hit its bound, an arc has no twin
    int32_t again;   // flatten: a walk ended below its root (behind error: union_find.hpp's flatten reads the two words together)
    int32_t giant;   // the label pass B skips, -1 = none
    int32_t pad;
    int32_t count[4];  // vertices in the group / wave / workgroup list: words 1 .. 3 (row_classes.hpp)
    unsigned long long examined;  // arcs the linking kernels looked at (Jarvis–Patrick: edges scored)
    unsigned long long kept;      // undirected edges the components are taken over
    unsigned long long comps, singles;
    unsigned long long best;      // size << 32 | ~label of the largest component
};

// edge sources of the row kernels
struct SrcAll {
    __device__ __forceinline__ bool keep(int64_t) const { return true; }
};
struct SrcMask {
    const uint8_t *mask;
    __device__ __forceinline__ bool keep(int64_t j) const { return mask[j] != 0; }
};

__global__ void k_cc_init(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ size) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) {
        parent[v] = int32_t(v);
        size[v] = 0;
    }
}

// The Op of the linking passes: links the arcs at positions [lo, min(degree, hi)) of a row that the source keeps.  A row whose label is *giant
// (giant != nullptr) is skipped.
template <class Src>
struct CcLink {
    Src src;
    int64_t lo, hi;
    const int32_t *giant;
    int32_t *parent;
    const int32_t *adj;
    uint32_t cap;
    int32_t *error;
    int32_t skip = -1;
    __device__ __forceinline__ void begin() { skip = giant ? *giant : -1; }
    template <int>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        const int64_t d = j1 - j0;
        if (d <= lo) return 0;
        if (skip >= 0 && load_now(&parent[v]) == skip) return 0;
        unsigned long long seen = 0;
        j1 = j0 + min(d, hi);
        for (int64_t j = j0 + lo + lane; j < j1; j += width, ++seen)
            if (src.keep(j)) cc_link(parent, v, adj[j], cap, error);
        return seen;
    }
    __device__ __forceinline__ void finish() {}
};

// Jarvis–Patrick: wave w takes the arcs w, w + W, …, 64 at a time (a lane resolves the source of each); one score per `u < v` arc, the kept
// ones linked (and marked on both arcs when mask != nullptr).  amdgpu_waves_per_eu(8, 8): the score loop is latency-bound and lives on resident
// waves; left alone the compiler takes 69 VGPRs = 7 waves per SIMD, held to 8 it takes 64 and spills nothing.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_cc_jp(int64_t n, int64_t nnz, const int64_t *__restrict__ off,
                                                                                          const int32_t *__restrict__ adj, int metric, double threshold,
                                                                                          int32_t *__restrict__ parent, uint8_t *__restrict__ mask,
                                                                                          CcAcc *__restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = uni64((int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6);
    const int64_t nwaves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const uint32_t cap = cc_walk_cap(n);
    unsigned long long scored = 0, kept = 0;  // (lane 0's are the wave's)
    for (int64_t k0 = 0; wave0 + k0 * nwaves < nnz; k0 += 64) {
        // lane t resolves arc wave0 + (k0 + t) nwaves: its source is the last u with off[u] <= j (off[n] = nnz > j, so u <= n - 1)
        const int64_t mine = wave0 + (k0 + lane) * nwaves;
        int32_t mu = -1, mv = -1;
        if (mine < nnz) {
            int64_t lo = 0, hi = n - 1;
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (off[mid] <= mine) lo = mid;
                else hi = mid - 1;
            }
            mv = adj[mine];
            if (int64_t(mv) > lo) mu = int32_t(lo);  // the edge is taken from its endpoint of the smaller id
        }
        // … the wave scores the `u < v` arcs among them one after the other …
        bool keep = false;
        for (unsigned long long todo = __ballot(mu >= 0); todo; todo &= todo - 1) {
            const int t = __ffsll((long long)todo) - 1;
            // (left in vector registers, as the pair batch has them: pinned to scalar registers — row bounds by scalar loads — the same
            // kernel measured 14 % slower)
            const int32_t u = __shfl(mu, t), v = __shfl(mv, t);
            const double score = wave_pair_similarity(off, adj, metric, u, v, lane);
            ++scored;
            if (score >= threshold && lane == t) keep = true;  // (a NaN score is never kept)
        }
        // … and every lane links the endpoints of its own arc, if that was kept: the walks of up to 64 links overlap instead of queueing on one lane
        kept += (unsigned long long)__popcll(__ballot(keep));
        if (keep) {
            cc_link(parent, mu, mv, cap, &acc->error);
            if (mask) {
                const int64_t twin = cc_find_in_row(adj, off[mv], off[mv + 1], mu);
                if (twin < 0) acc->error = 1;
                else {
                    mask[mine] = 1;
                    mask[twin] = 1;
                }
            }
        }
    }
    if (lane == 0) {
        if (scored) atomicAdd(&acc->examined, scored);
        if (kept) atomicAdd(&acc->kept, kept);
    }
}

// kept edges of a caller's mask, each once: a `u < v` arc with its byte set, or a `u > v` arc with its byte set whose twin's byte is zero.
// A kGroup-lane group per row.
__global__ __launch_bounds__(256) void k_cc_mask_edges(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                       const uint8_t *__restrict__ mask, CcAcc *__restrict__ acc) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    unsigned long long kept = 0;
    for (int64_t u = group0; u < n; u += groups)
        for (int64_t j = off[u] + lane; j < off[u + 1]; j += kGroup) {
            if (!mask[j]) continue;
            const int32_t v = adj[j];
            if (int64_t(v) > u) {
                ++kept;
            } else {
                const int64_t twin = cc_find_in_row(adj, off[v], off[v + 1], int32_t(u));
                if (twin < 0) acc->error = 1;
                else if (!mask[twin]) ++kept;
            }
        }
    kept = wave_sum(kept);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&acc->kept, kept);
}

// the giant-component vote: the labels of kCcSamples seeded vertex ids, the most frequent one (ties: the smaller label) into acc->giant.
// One workgroup of kCcSamples threads; 4 KB + 128 B of LDS.
__global__ __launch_bounds__(kCcSamples) void k_cc_vote(int64_t n, const int32_t *__restrict__ parent, CcAcc *__restrict__ acc) {
    __shared__ int32_t s_label[kCcSamples];
    __shared__ unsigned long long s_best[kCcSamples / 64];
    const int t = threadIdx.x;
    unsigned long long h = (unsigned long long)(t + 1) * 0x9E3779B97F4A7C15ull;  // the seeded set: a fixed hash of the slot
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    const int32_t mine = parent[int64_t(h % (unsigned long long)n)];
    s_label[t] = mine;
    __syncthreads();
    uint32_t c = 0;
    for (int i = 0; i < kCcSamples; ++i) c += s_label[i] == mine;
    unsigned long long key = ((unsigned long long)c << 32) | (0xffffffffu - uint32_t(mine));
    key = wave_max(key);
    if ((t & 63) == 0) s_best[t >> 6] = key;
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < kCcSamples / 64; ++i) key = max(key, s_best[i]);
        acc->giant = int32_t(0xffffffffu - uint32_t(key));
    }
}

// per root: components, singletons, the largest component (ties: the smaller label).  A label that is no root raises the flag.
__global__ __launch_bounds__(256) void k_cc_info(int64_t n, const int32_t *__restrict__ label, const int32_t *__restrict__ size, CcAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long comps = 0, singles = 0, best = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t l = label[v];
        if (l < 0 || l > v || label[l] != l) acc->error = 1;
        if (l != v) continue;
        const uint32_t s = uint32_t(size[v]);
        ++comps;
        singles += s == 1;
        best = max(best, ((unsigned long long)s << 32) | (0xffffffffu - uint32_t(v)));
    }
    comps = wave_sum(comps);
    singles = wave_sum(singles);
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0 && comps) {
        atomicAdd(&acc->comps, comps);
        if (singles) atomicAdd(&acc->singles, singles);
        atomicMax(&acc->best, best);
    }
}

enum { kSrcAll = 0, kSrcMask = 1, kSrcJp = 2 };

// Both entry points.  mask_in (host, nnz) for kSrcMask; mask_out (host, nnz, or null) for kSrcJp.
int components(const gmsx_graph *g, int source, const uint8_t *mask_in, int metric, double threshold, int32_t *label, uint8_t *mask_out,
               gmsx_components_info *info, gmsx_stats *stats) {
    gmsx_components_info res;
    std::memset(&res, 0, sizeof res);
    if (g->n == 0) {
        *info = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n, nnz = g->nnz;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    // test hooks, first guesses
    const int64_t sample = std::max<long long>(0, std::min<long long>(opt_int("CC_SAMPLE", kCcSampleDefault), INT_MAX));
    const RowBounds bounds = row_bounds("CC_WAVE_ROW", "CC_WG_ROW");
    RowListStore lists;
    DevBuf d_parent, d_size, d_acc, d_mask;
    const bool dev_mask = source == kSrcMask || (source == kSrcJp && mask_out);
    // ---- setup: the buffers and the caller's mask
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_parent, n)) return rc;
    if (int rc = dalloc<int32_t>(d_size, n)) return rc;
    if (int rc = dalloc<CcAcc>(d_acc, 1)) return rc;
    if (source != kSrcJp)
        if (int rc = lists.alloc(n, nnz, bounds, false, false)) return rc;
    if (dev_mask)
        if (int rc = dalloc<uint8_t>(d_mask, nnz)) return rc;
    CcAcc *acc = d_acc.as<CcAcc>();
    int32_t *parent = d_parent.as<int32_t>();
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(CcAcc), s));
    GMSX_HIP(hipMemsetAsync(&acc->giant, 0xff, sizeof(int32_t), s));
    if (source == kSrcMask && nnz > 0) GMSX_HIP(hipMemcpyAsync(d_mask.p, mask_in, size_t(nnz), hipMemcpyHostToDevice, s));
    if (source == kSrcJp && mask_out && nnz > 0) GMSX_HIP(hipMemsetAsync(d_mask.p, 0, size_t(nnz), s));
    // ---- linking and flatten
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    int launches = 0;
    const unsigned per_vertex = unsigned((n + 255) / 256);
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    hipLaunchKernelGGL(k_cc_init, dim3(per_vertex), dim3(256), 0, s, n, parent, d_size.as<int32_t>());
    ++launches;
    if (source == kSrcJp) {
        if (nnz > 0) {
            const unsigned blocks = unsigned(std::min<int64_t>((nnz + 7) / 8, int64_t(cus) * 32));  // a wave per edge while the grid lasts: the pair batch's shape
            hipLaunchKernelGGL(k_cc_jp, dim3(blocks), dim3(256), 0, s, n, nnz, g->off, g->adj, metric, threshold, parent, mask_out ? d_mask.as<uint8_t>() : nullptr,
                               acc);
            ++launches;
        }
    } else if (nnz > 0) {
        classify_rows<false>(g, bounds, lists.l, acc->count, &acc->error, cus, s, &launches);
        // pass A (the first `sample` entries of every row, a lane per row over all vertices), the vote where it is valid, pass B (the rest)
        auto link = [&](auto src) -> int {
            using Op = CcLink<decltype(src)>;
            const int64_t all = INT64_MAX;
            const int32_t *giant = nullptr;
            if (sample > 0) {
                hipLaunchKernelGGL((k_rows<Op, 1>), dim3(sweep), dim3(256), 0, s, Op{src, 0, sample, nullptr, parent, g->adj, cc_walk_cap(n), &acc->error}, n,
                                   g->off, (const int32_t *)nullptr, acc->count, int64_t(0), int64_t(1), all, &acc->examined);
                ++launches;
                if (source == kSrcAll) {  // the skip is valid only where every kept edge is visible from both sides
                    if (int rc = flatten(n, parent, &acc->error, cus, s, &launches, nullptr)) return rc;
                    hipLaunchKernelGGL(k_cc_vote, dim3(1), dim3(kCcSamples), 0, s, n, parent, acc);
                    ++launches;
                    giant = &acc->giant;
                }
            }
            launch_rows(Op{src, sample, all, giant, parent, g->adj, cc_walk_cap(n), &acc->error}, g, bounds, lists.l, acc->count, &acc->examined, cus, s,
                        &launches);
            return GMSX_OK;
        };
        if (int rc = source == kSrcAll ? link(SrcAll{}) : link(SrcMask{d_mask.as<const uint8_t>()})) return rc;
    }
    int32_t passes = 0;
    if (int rc = flatten(n, parent, &acc->error, cus, s, &launches, &passes)) return rc;
    // ---- the info reduction
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    hipLaunchKernelGGL(k_cc_sizes, dim3(sweep), dim3(256), 0, s, n, parent, d_size.as<int32_t>());
    hipLaunchKernelGGL(k_cc_info, dim3(sweep), dim3(256), 0, s, n, parent, d_size.as<int32_t>(), acc);
    if (source == kSrcMask && nnz > 0) {
        const unsigned groups = unsigned(std::min<int64_t>((n * kGroup + 255) / 256, int64_t(cus) * 32));
        hipLaunchKernelGGL(k_cc_mask_edges, dim3(groups), dim3(256), 0, s, n, g->off, g->adj, d_mask.as<const uint8_t>(), acc);
    }
    CcAcc h;
    GMSX_HIP(hipMemcpyAsync(&h, acc, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (h.error || h.comps < 1 || h.comps > (unsigned long long)n || (h.best >> 32) < 1) return GMSX_ERR_KERNEL;
    res.components = int64_t(h.comps);
    res.singletons = int64_t(h.singles);
    res.largest = int64_t(h.best >> 32);
    res.largest_label = int32_t(0xffffffffu - uint32_t(h.best));
    res.kept_edges = source == kSrcAll ? nnz / 2 : int64_t(h.kept);
    res.passes = passes;
    // the flag word was read as zero: the caller's arrays are written now, through host staging
    HostStage out;
    if (int rc = out.fetch(label, parent, size_t(n) * sizeof(int32_t), s)) return rc;
    if (source == kSrcJp)
        if (int rc = out.fetch(mask_out, d_mask.p, size_t(nnz), s)) return rc;
    GMSX_HIP(hipStreamSynchronize(s));
    float up_ms = 0.f, ms = 0.f, info_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&info_ms, c.ev[2], c.ev[3]));
    out.deliver();
    *info = res;
    if (stats)
        *stats = gmsx_stats{double(ms), double(up_ms) + double(info_ms), uint64_t(h.examined), source == kSrcJp ? g->alg_elements : 0, 0, launches, 0, 0};
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_connected_components(const gmsx_graph *g, const uint8_t *arc_keep, int32_t *label, gmsx_components_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        return components(g, arc_keep ? kSrcMask : kSrcAll, arc_keep, 0, 0.0, label, nullptr, info, stats);
    });
}

int gmsx_jarvis_patrick(const gmsx_graph *g, int metric, double threshold, int32_t *label, uint8_t *arc_keep, gmsx_components_info *info,
                        gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || metric < GMSX_SIM_JACCARD || metric > GMSX_SIM_PREF_ATTACHMENT || std::isnan(threshold)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        return components(g, kSrcJp, nullptr, metric, threshold, label, arc_keep, info, stats);
    });
}

}  // extern "C"
