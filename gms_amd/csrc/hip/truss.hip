// Per-edge triangle support and the exact k-truss decomposition on gfx950 — the edge counterpart of core.hip:
//   gmsx_edge_support          support(e) = |N(u) ∩ N(v)| on the full rows for every undirected edge e = {u, v}
//   gmsx_truss_decomposition   the trussness of every edge (and the round of the peel it leaves in)
// Neither has a counterpart in the reference; the definitions are those of include/gmsx.h.
//
// EDGE NUMBERING (per call, DevBufs only — the graph handle is not touched).  Edge ids are the `u < v` arcs in CSR order: up0[u] = position of
// the first entry above u in row u, ebase = exclusive scan of the per-row counts, id of arc j of row u = ebase[u] + (j - up0[u]).  eid[arc]
// carries the id on both arcs (the `u > v` arc finds its twin by a binary search in row v), eu / ev the endpoints, and coff is the prefix array
// over cost(e) = min(deg u, deg v) * bit length of max(deg u, deg v): the probes of one intersection — every entry of the shorter row is a binary
// search in the longer one, so an entry is an order of magnitude dearer than the row entry the engine's bounds were written for.
//
// SUPPORT.  A kGroup-lane group per edge streams the shorter full row and binary-searches the longer one (pairs.hip's formulation); an edge
// of more than kLongRow probes is parked with a bounds-checked append and gets a whole workgroup — no lane walks a long row alone.  (Hub-hub
// edges are many: all workgroups walking each of them together, as the engine does for the few long ROWS of a graph, costs a trip of the whole
// grid per edge.)  Integer sums only.
//
// THE PEEL is core.hip's, one level up: the frontier holds EDGE ids, the policy's n is m and its off is coff, so the engine's short / parked /
// hand-back binning (frontier_rounds.hpp, unchanged) bins by intersection cost in probes.  "Walk the row" becomes "intersect the two rows"; a leaving
// edge pushes a decrement to the two other edges of every triangle it destroys.  Per edge: sup[e] (remaining support) and rnd[e] — -1 while
// the edge is remaining and unqueued, else the round it is worked in, written at the moment it is queued.  For a frontier edge e = (u, v) of
// round r and a common neighbour w, with e1 = (u, w) and e2 = (v, w):
//   0 <= rnd[e1] < r or 0 <= rnd[e2] < r   the triangle died in an earlier round
//   neither e1 nor e2 in this frontier     (rnd != r) e decrements both
//   exactly one of them, say e2            the triangle has two leaving edges, both meet it: the one of the smaller id decrements e1
//   both                                   nobody is left to decrement
// so every destroyed triangle costs each edge that stays exactly one decrement.  A decrement applies only above the level l, and the one that
// lands on l queues the edge for round r + 1 (atomicSub returns l + 1 exactly once: sup only falls).  rnd[e1] can change under a reader only
// from -1 to r + 1, and both mean "not in this frontier, not dead": which edges a round removes is a fact about the integers, never about the
// arrival order of the atomics.  The order inside the queues is not, and reaches no output.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"
#include "truss_edges.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

// control block of one peel: the engine's, plus the level
struct TrussCtrl : FrontierCtrl {  // (done = edges that have left in finished rounds)
    int32_t l;        // current level: the edges leaving have trussness l + 2
    int32_t min_sup;  // level sweep: smallest remaining support
};

// (TrussAcc, the accumulators of the numbering and the support pass, and TrussEdges: truss_edges.hpp)

// position of x in the ascending row [lo, hi) of adj, or -1
__device__ __forceinline__ int64_t find_in_row(const int32_t *__restrict__ adj, int64_t lo, int64_t hi, int32_t x) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (adj[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && adj[lo] == x) ? lo : -1;
}

// up0[u] = first position of row u whose entry is above u; cnt[u] = entries from there on (cnt[n] = 0: the scan's last slot)
__global__ void k_truss_upper(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int64_t *__restrict__ up0,
                              int64_t *__restrict__ cnt) {
    const int64_t u = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u > n) return;
    if (u == n) {
        cnt[u] = 0;
        return;
    }
    int64_t lo = off[u], hi = off[u + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (adj[mid] <= int32_t(u)) lo = mid + 1;
        else hi = mid;
    }
    up0[u] = lo;
    cnt[u] = off[u + 1] - lo;
}

// one thread per arc j = (u -> v): eid[j]; the `u < v` arc also writes the endpoints and the cost of its edge.  Vertex ids are in [0, n): the
// upload refuses others even under GMSX_UPLOAD_TRUSTED.  Every EDGE id is checked against m before it is used: an input that breaks the rest of
// the canonical-row invariant (a self loop, an arc without its twin) raises acc->error and writes nothing out of bounds.
__global__ __launch_bounds__(256) void k_truss_number(int64_t n, int64_t nnz, int64_t m, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                      const int64_t *__restrict__ up0, const int64_t *__restrict__ ebase, int32_t *__restrict__ eid,
                                                      int32_t *__restrict__ eu, int32_t *__restrict__ ev, int64_t *__restrict__ cost,
                                                      TrussAcc *__restrict__ acc) {
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= nnz) return;
    int64_t lo = 0, hi = n;  // source vertex of arc j: last u with off[u] <= j
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    const int64_t u = lo;
    const int32_t v = adj[j];
    int64_t e = -1;
    if (u < v) {
        e = ebase[u] + (j - up0[u]);
        if (e >= 0 && e < m) {
            eu[e] = int32_t(u);
            ev[e] = v;
            const int64_t du = off[u + 1] - off[u], dv = off[v + 1] - off[v];
            cost[e] = min(du, dv) * int64_t(64 - __clzll((long long)max(du, dv)));
        }
    } else if (v < u && v >= 0) {
        const int64_t jj = find_in_row(adj, off[v], off[v + 1], int32_t(u));
        if (jj >= 0) e = ebase[v] + (jj - up0[v]);
    }
    if (e < 0 || e >= m) {
        acc->error = 1;
        e = 0;
    }
    eid[j] = int32_t(e);
}

// |N(a) ∩ N(b)| shares of one lane: the entries i = lane, lane + width, … of the shorter row are searched in the longer one
__device__ __forceinline__ uint32_t intersect_share(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int32_t u, int32_t v, int64_t lane,
                                                    int64_t width) {
    int64_t a0 = off[u], a1 = off[u + 1], b0 = off[v], b1 = off[v + 1];
    if (a1 - a0 > b1 - b0) {
        const int64_t t0 = a0, t1 = a1;
        a0 = b0, a1 = b1, b0 = t0, b1 = t1;
    }
    uint32_t c = 0;
    for (int64_t i = a0 + lane; i < a1; i += width)
        if (find_in_row(adj, b0, b1, adj[i]) >= 0) ++c;
    return c;
}

// support, short edges: a kGroup-lane group per edge; an edge of more than kLongRow probes (coff) is parked for k_truss_support_long
__global__ __launch_bounds__(256) void k_truss_support(int64_t m, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                       const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const int64_t *__restrict__ coff,
                                                       int32_t *__restrict__ sup, int32_t *__restrict__ longs, int64_t long_cap, TrussAcc *__restrict__ acc) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    for (int64_t e = group0; e < m; e += groups) {
        if (coff[e + 1] - coff[e] > kLongRow) {
            if (lane == 0) {
                sup[e] = 0;
                append_checked(longs, &acc->nlong, long_cap, int32_t(e), &acc->error);
            }
            continue;
        }
        uint32_t c = intersect_share(off, adj, eu[e], ev[e], lane, kGroup);
        c = wave_sum<kGroup>(c);
        if (lane == 0) sup[e] = int32_t(c);
    }
}

// … its parked edges: a workgroup per edge, one atomic per wave (sup[e] was zeroed when the edge was parked)
__global__ __launch_bounds__(256) void k_truss_support_long(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const int32_t *__restrict__ eu,
                                                            const int32_t *__restrict__ ev, int32_t *__restrict__ sup, const int32_t *__restrict__ longs,
                                                            int64_t long_cap, const TrussAcc *__restrict__ acc) {
    const int64_t nlong = min(int64_t(acc->nlong), long_cap);
    for (int64_t i = blockIdx.x; i < nlong; i += gridDim.x) {
        const int32_t e = longs[i];
        uint32_t c = intersect_share(off, adj, eu[e], ev[e], threadIdx.x, blockDim.x);
        c = wave_sum(c);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sup[e], int32_t(c));
    }
}

// Σ support and max support over the edges; rnd[e] = -1 (every edge remaining) when rnd is given
__global__ __launch_bounds__(256) void k_truss_reduce(int64_t m, const int32_t *__restrict__ sup, int32_t *__restrict__ rnd, TrussAcc *__restrict__ acc) {
    unsigned long long sum = 0;
    int32_t mx = 0;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < m; e += int64_t(gridDim.x) * blockDim.x) {
        const int32_t s = sup[e];
        sum += (unsigned long long)s;
        mx = max(mx, s);
        if (rnd) rnd[e] = -1;
    }
    sum = wave_sum(sum);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(&acc->sum, sum);
        if (mx) atomicMax(&acc->max_sup, mx);
    }
}

// out[arc] = val[eid[arc]]: the per-edge values on both arcs of every edge
__global__ void k_truss_gather(int64_t nnz, const int32_t *__restrict__ eid, const int32_t *__restrict__ val, int32_t *__restrict__ out) {
    const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j < nnz) out[j] = val[eid[j]];
}

// level sweep, first half: ctrl->min_sup = min sup over the remaining edges (rnd == -1)
__global__ __launch_bounds__(256) void k_truss_min(int64_t m, const int32_t *__restrict__ sup, const int32_t *__restrict__ rnd, TrussCtrl *__restrict__ ctrl) {
    int32_t mn = INT_MAX;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < m; e += int64_t(gridDim.x) * blockDim.x)
        if (rnd[e] < 0) mn = min(mn, sup[e]);
    mn = wave_min(mn);
    if ((threadIdx.x & 63) == 0 && mn != INT_MAX) atomicMin(&ctrl->min_sup, mn);
}

// … second half: the remaining edges of that support are the level's first frontier, worked in the round the control block names
__global__ __launch_bounds__(256) void k_truss_select(int64_t m, const int32_t *__restrict__ sup, int32_t *__restrict__ rnd, TrussCtrl *__restrict__ ctrl,
                                                      int32_t *__restrict__ frontier) {
    const int32_t l = ctrl->min_sup, round = ctrl->round;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->l = l;  // (the others read min_sup, not l)
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((m + 63) / 64) * 64;  // whole waves stay converged for the ballot
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < end; e += stride) {
        const bool take = e < m && rnd[e] < 0 && sup[e] <= l;
        if (take) rnd[e] = round;
        wave_append(take, int32_t(e), frontier, &ctrl->count, m, &ctrl->error);
    }
}

// the peel as a policy of the engine: a frontier edge leaves (trussness l + 2; its round was written when it was queued) and PUSHes a decrement
// to the two other edges of every triangle it destroys
struct TrussPeel {
    static constexpr int kGroupWords = 0;
    static constexpr bool kNotes = false;
    int64_t n;           // = m: the frontier holds edge ids
    const int64_t *off;  // = coff: prefix over the probes of every edge's intersection
    const int64_t *goff;
    const int32_t *adj, *eid, *eu, *ev;
    int32_t *sup, *rnd, *truss;
    int32_t l;  // the level (the host sets it from the control block it read)

    __device__ __forceinline__ void dec(int32_t f, int32_t round, const NextQueue &q) const {
        if (load_now(&sup[f]) <= l) return;  // has left, is leaving or is queued (sup only ever falls: a stale value costs an atomic, never the result)
        if (atomicSub(&sup[f], 1) == l + 1) {
            store_now(&rnd[f], round + 1);
            q.push(f);
        }
    }
    // the share of `width` lanes in the triangles of edge e
    __device__ __forceinline__ void walk(int32_t e, int32_t round, int64_t lane, int64_t width, const NextQueue &q) const {
        int32_t a = eu[e], b = ev[e];
        if (goff[a + 1] - goff[a] > goff[b + 1] - goff[b]) {
            const int32_t t = a;
            a = b, b = t;
        }
        const int64_t a0 = goff[a], a1 = goff[a + 1], b0 = goff[b], b1 = goff[b + 1];
        for (int64_t i = a0 + lane; i < a1; i += width) {
            const int64_t jb = find_in_row(adj, b0, b1, adj[i]);
            if (jb < 0) continue;
            const int32_t e1 = eid[i], e2 = eid[jb];
            const int32_t r1 = load_now(&rnd[e1]), r2 = load_now(&rnd[e2]);
            if ((r1 >= 0 && r1 < round) || (r2 >= 0 && r2 < round)) continue;  // the triangle died in an earlier round
            const bool in1 = r1 == round, in2 = r2 == round;
            if (!in1 && !in2) {
                dec(e1, round, q);
                dec(e2, round, q);
            } else if (in1 && !in2) {
                if (e < e1) dec(e2, round, q);
            } else if (in2 && !in1) {
                if (e < e2) dec(e1, round, q);
            }
        }
    }
    __device__ __forceinline__ void short_row(int32_t x, int64_t, int64_t, int lane, int32_t round, uint32_t *, const NextQueue &q) const {
        if (lane == 0) truss[x] = l + 2;
        walk(x, round, lane, kGroup, q);
    }
    __device__ __forceinline__ void park(int32_t x, int32_t, unsigned long long *, int64_t, int32_t *) const { truss[x] = l + 2; }
    // The engine hands a parked row to all threads it has.  In the tail that is one workgroup; grid-wide, the workgroup x picks walks the edge
    // and the others only read the list: a frontier parks many edges, and a trip of the whole grid per edge would cost more than its probes.
    __device__ __forceinline__ void long_walk(int32_t x, unsigned long long, int64_t tid, int64_t threads, const NextQueue &q) const {
        if (threads <= kTailThreads) {
            walk(x, load_now(&rnd[x]), tid, threads, q);  // (rnd[x] is the round x is worked in: this one)
        } else if (uint32_t(x) % uint32_t(threads / 256) == uint32_t(tid / 256)) {
            walk(x, load_now(&rnd[x]), tid % 256, 256, q);
        }
    }
    __device__ __forceinline__ void finish() const {}
};

}  // namespace

// Edge numbering and support (declared in truss_edges.hpp: motifs.hip calls it too).  rnd (m, device, or null) is set to -1.  Refuses
// m >= 2^31: edge ids are 32 bits.
int truss_edges(const gmsx_graph *g, TrussEdges &t, int32_t *rnd) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n, nnz = g->nnz;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    DevBuf d_up0, d_cnt, d_ebase, d_cost;
    if (int rc = dalloc<int64_t>(d_up0, n)) return rc;
    if (int rc = dalloc<int64_t>(d_cnt, n + 1)) return rc;
    if (int rc = dalloc<int64_t>(d_ebase, n + 1)) return rc;
    if (int rc = dalloc<TrussAcc>(t.acc, 1)) return rc;
    GMSX_HIP(hipMemsetAsync(t.acc.p, 0, sizeof(TrussAcc), s));
    hipLaunchKernelGGL(k_truss_upper, dim3(unsigned(n / 256 + 1)), dim3(256), 0, s, n, g->off, g->adj, d_up0.as<int64_t>(), d_cnt.as<int64_t>());
    if (int rc = exclusive_scan_i64(d_cnt.as<const int64_t>(), d_ebase.as<int64_t>(), n + 1, s)) return rc;
    int64_t m = 0;
    GMSX_HIP(hipMemcpyAsync(&m, d_ebase.as<int64_t>() + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (m >= (int64_t(1) << 31)) return GMSX_ERR_UNSUPPORTED;
    if (m * 2 != nnz) return GMSX_ERR_KERNEL;  // (a symmetric loop-free CSR has every edge once above the diagonal)
    t.m = m;
    if (int rc = dalloc<int32_t>(t.eid, nnz)) return rc;
    if (int rc = dalloc<int32_t>(t.eu, m)) return rc;
    if (int rc = dalloc<int32_t>(t.ev, m)) return rc;
    if (int rc = dalloc<int32_t>(t.sup, m)) return rc;
    if (int rc = dalloc<int64_t>(d_cost, m + 1)) return rc;
    if (int rc = dalloc<int64_t>(t.coff, m + 1)) return rc;
    GMSX_HIP(hipMemsetAsync(d_cost.p, 0, size_t(m + 1) * sizeof(int64_t), s));
    GMSX_HIP(hipMemsetAsync(t.eu.p, 0, size_t(m) * sizeof(int32_t), s));  // (an input that breaks the invariant leaves holes: they stay in range)
    GMSX_HIP(hipMemsetAsync(t.ev.p, 0, size_t(m) * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_truss_number, dim3(unsigned((nnz + 255) / 256)), dim3(256), 0, s, n, nnz, m, g->off, g->adj, d_up0.as<int64_t>(), d_ebase.as<int64_t>(),
                       t.eid.as<int32_t>(), t.eu.as<int32_t>(), t.ev.as<int32_t>(), d_cost.as<int64_t>(), t.acc.as<TrussAcc>());
    if (int rc = exclusive_scan_i64(d_cost.as<const int64_t>(), t.coff.as<int64_t>(), m + 1, s)) return rc;
    GMSX_HIP(hipMemcpyAsync(&t.total_cost, t.coff.as<int64_t>() + m, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(&t.h, t.acc.p, sizeof(TrussAcc), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (t.h.error) return GMSX_ERR_KERNEL;
    t.long_cap = frontier_long_cap(m, t.total_cost);
    if (int rc = dalloc<int32_t>(t.longs, t.long_cap)) return rc;
    const unsigned sb = unsigned(std::min<int64_t>((m * kGroup + 255) / 256, int64_t(cus) * 32));
    const unsigned sweep = unsigned(std::min<int64_t>((m + 255) / 256, int64_t(cus) * 16));
    hipLaunchKernelGGL(k_truss_support, dim3(sb), dim3(256), 0, s, m, g->off, g->adj, t.eu.as<int32_t>(), t.ev.as<int32_t>(), t.coff.as<int64_t>(),
                       t.sup.as<int32_t>(), t.longs.as<int32_t>(), t.long_cap, t.acc.as<TrussAcc>());
    hipLaunchKernelGGL(k_truss_support_long, dim3(unsigned(cus) * 4), dim3(256), 0, s, g->off, g->adj, t.eu.as<int32_t>(), t.ev.as<int32_t>(),
                       t.sup.as<int32_t>(), t.longs.as<int32_t>(), t.long_cap, t.acc.as<TrussAcc>());
    hipLaunchKernelGGL(k_truss_reduce, dim3(sweep), dim3(256), 0, s, m, t.sup.as<int32_t>(), rnd, t.acc.as<TrussAcc>());
    GMSX_HIP(hipMemcpyAsync(&t.h, t.acc.p, sizeof(TrussAcc), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (t.h.error || t.h.sum % 3 != 0) return GMSX_ERR_KERNEL;
    t.launches = 7;  // (two scans counted as one launch each)
    return GMSX_OK;
}

namespace {

// per-edge values -> the caller's per-arc array (host), through a host staging vector: written only after everything else succeeded
int gather_to_host(const TrussEdges &t, int64_t nnz, const int32_t *d_val, DevBuf &d_out, std::vector<int32_t> &h_out, hipStream_t s) {
    if (!d_out.p)
        if (int rc = dalloc<int32_t>(d_out, nnz)) return rc;
    hipLaunchKernelGGL(k_truss_gather, dim3(unsigned((nnz + 255) / 256)), dim3(256), 0, s, nnz, t.eid.as<int32_t>(), d_val, d_out.as<int32_t>());
    h_out.resize(size_t(nnz));
    GMSX_HIP(hipMemcpyAsync(h_out.data(), d_out.p, size_t(nnz) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_edge_support(const gmsx_graph *g, int32_t *support, uint64_t *triangles, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        if (g->nnz > 0 && !support) return GMSX_ERR_INVALID;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        if (g->n == 0 || g->nnz == 0) {
            if (triangles) *triangles = 0;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        TrussEdges t;
        DevBuf d_out;
        std::vector<int32_t> h_out;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = truss_edges(g, t, nullptr)) return rc;
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        if (int rc = gather_to_host(t, g->nnz, t.sup.as<int32_t>(), d_out, h_out, s)) return rc;
        float ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        std::memcpy(support, h_out.data(), size_t(g->nnz) * sizeof(int32_t));
        if (triangles) *triangles = uint64_t(t.h.sum / 3);
        if (stats) *stats = gmsx_stats{double(ms), 0.0, uint64_t(t.m), 0, 0, t.launches + 1, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_truss_decomposition(const gmsx_graph *g, int32_t *truss, int32_t *round_of, gmsx_truss_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        gmsx_truss_info res;
        std::memset(&res, 0, sizeof res);
        if (g->n == 0 || g->nnz == 0) {
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        const int64_t nnz = g->nnz;
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        TrussEdges t;
        DevBuf d_rnd, d_truss, d_ctrl, d_out;
        FrontierStore store;  // (the items are edges, their rows the cost ranges of coff; its longs list stands beside t.longs of the support pass)
        // ---- setup: numbering and support
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = dalloc<int32_t>(d_rnd, nnz / 2)) return rc;  // (the support pass's last kernel fills it; the numbering refuses m != nnz / 2)
        if (int rc = truss_edges(g, t, d_rnd.as<int32_t>())) return rc;
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        const int64_t m = t.m;
        if (int rc = dalloc<int32_t>(d_truss, m)) return rc;
        if (int rc = store.alloc(m, t.total_cost, false)) return rc;
        if (int rc = dalloc<TrussCtrl>(d_ctrl, 1)) return rc;
        TrussCtrl *ctrl = d_ctrl.as<TrussCtrl>();
        int32_t *sup = t.sup.as<int32_t>(), *rnd = d_rnd.as<int32_t>();
        const FrontierBufs bufs = store.bufs();
        TrussPeel peel{m, t.coff.as<int64_t>(), g->off, g->adj, t.eid.as<int32_t>(), t.eu.as<int32_t>(), t.ev.as<int32_t>(), sup, rnd, d_truss.as<int32_t>(), 0};
        // test hook: 0 = every round a kernel boundary, large = every round the tail may take.  The default is 0: a round here is an intersection per
        // frontier edge, and the one-workgroup tail measured slower than kernel boundaries at every size.
        const long long wg_frontier = frontier_wg_option("TRUSS_WG_FRONTIER", 0);
        res.max_support = t.h.max_sup;
        res.triangles = int64_t(t.h.sum / 3);
        // ---- the peel
        const unsigned sweep = unsigned(std::min<int64_t>((m + 255) / 256, int64_t(cus) * 16));
        int launches = 0;
        TrussCtrl h;
        std::memset(&h, 0, sizeof h);
        GMSX_HIP(hipEventRecord(c.ev[2], s));
        GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(TrussCtrl), s));
        int32_t l_done = -1, levels = 0;
        int64_t top_edges = 0;
        while (h.done < m) {
            // ---- the next level: l = smallest remaining support, first frontier = the remaining edges that have it
            GMSX_HIP(hipMemsetAsync(&ctrl->min_sup, 0x7f, sizeof(int32_t), s));
            hipLaunchKernelGGL(k_truss_min, dim3(sweep), dim3(256), 0, s, m, sup, rnd, ctrl);
            hipLaunchKernelGGL(k_truss_select, dim3(sweep), dim3(256), 0, s, m, sup, rnd, ctrl, bufs.f[h.cur]);
            launches += 2;
            GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            if (h.error || h.count <= 0 || h.count > m - h.done || h.min_sup <= l_done || h.l != h.min_sup) return GMSX_ERR_KERNEL;
            const int64_t removed_before = h.done;
            // ---- rounds of this level
            peel.l = h.l;
            if (int rc = run_frontier_rounds(peel, bufs, ctrl, h, wg_frontier, &launches)) return rc;
            top_edges = h.done - removed_before;
            l_done = h.l;
            ++levels;
        }
        GMSX_HIP(hipEventRecord(c.ev[3], s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (h.done != m) return GMSX_ERR_KERNEL;
        res.max_truss = l_done + 2;
        res.levels = levels;
        res.rounds = h.round;
        res.top_edges = top_edges;
        float setup_ms = 0.f, ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&setup_ms, c.ev[0], c.ev[1]));
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
        // the outputs are written only now, when nothing can fail but the copies themselves
        std::vector<int32_t> h_truss, h_round;
        if (truss) {
            if (int rc = gather_to_host(t, nnz, d_truss.as<int32_t>(), d_out, h_truss, s)) return rc;
            launches += 1;
        }
        if (round_of) {
            if (int rc = gather_to_host(t, nnz, rnd, d_out, h_round, s)) return rc;
            launches += 1;
        }
        if (truss) std::memcpy(truss, h_truss.data(), size_t(nnz) * sizeof(int32_t));
        if (round_of) std::memcpy(round_of, h_round.data(), size_t(nnz) * sizeof(int32_t));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), double(setup_ms), uint64_t(m), 0, uint64_t(res.rounds), launches + t.launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
