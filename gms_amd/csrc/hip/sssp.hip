// Edge weights on the device and delta-stepping single-source shortest paths on gfx950, over the uploaded CSR.
//   gmsx_graph_set_weights  int32 weights[nnz] parallel to adj (two parallel arrays), validated on the device: every weight >= 1, and
//                           w(u→v) == w(v→u) unless the upload was TRUSTED; wmax and Σw are recorded
//   gmsx_sssp               DeltaStep (representations/graphs/log_graph/sssp.cc:54-134): dist[v], then parent[v] = the SMALLEST-id neighbour u
//                           with dist[u] + w(u,v) == dist[v] by a pull pass — facts about (graph, weights, source)
//   gmsx_sssp_verify        the same pull pass over a caller's array: SSSPVerifier (sssp.cc:145-175) as integer counts
// The definitions are those of include/gmsx.h.
//
// BUCKETS.  Bucket i holds the tentative distances in [i delta, (i + 1) delta).  The state is dist[n] (32- or 64-bit words by the handle's
// (n - 1) wmax), two frontier buffers of n entries and a stamp per vertex: memory beyond the weights is O(n), there is no nnz-sized queue.
// The buckets are worked in ascending order; when bucket i is done every vertex below (i + 1) delta is final.
//
// A ROUND of a bucket relaxes every arc of every frontier vertex and is a policy (SsspRelax) of the frontier-rounds engine's kernels
// (frontier_rounds.hpp: a 16-lane group per short row, rows above kLongRow parked and walked by all workgroups, the one-workgroup tail under
// SSSP_WG_FRONTIER with its hand-back) and of its host loop.  Shortest paths re-enter vertices, so the policy declares kReenters: the loop then
// leaves the once-per-vertex checks on `done` out and keeps the others.  A walker of frontier vertex x reads dist[x] with load_now,
// reads dist[w] with a plain load and issues the integer atomicMin only when dist[x] + w(x,w) would improve it.  The walker whose atomicMin
// improved w appends w to the next round's frontier iff the new distance lies in the current bucket and it is the first to set w's stamp to
// this round's number (atomicExch): a vertex enters a round's frontier at most once, so a frontier never exceeds n.  The appends of a wave go
// out as one add of its active-lane count (the compiler aggregates atomicAdd(count, 1)).  Vertices that fall into later buckets are not queued.
//
// THE INVARIANT.  Distances only fall, and only by atomicMin, so a stale read of dist[w] is too LARGE: it can cost a superfluous atomic, never
// a missed one.  A stale read of the frontier vertex's own distance could only make its relaxations weaker, never wrong — and it is not stale:
// x was queued by the walker that improved it, behind that atomic, and load_now reads the L2 where the atomics are performed, behind a round
// boundary (a kernel boundary or the tail's barrier).  Whatever improves a vertex inside the current bucket queues it again, so when a bucket's
// frontier empties every arc out of every vertex of the bucket has been relaxed with that vertex's final distance.
//
// THE NEXT BUCKET.  When the frontier empties, one streaming pass over dist finds the smallest tentative distance at or above (i + 1) delta —
// it is final, as in Dijkstra's algorithm —, and a second one collects the vertices of its bucket into the frontier.  Both are plain coalesced
// reads of n words: the cost is O(buckets * n) on top of the relaxations.  The far pile that would avoid it is not built.
//
// BOUNDS.  Every loop is bounded and no workgroup waits for another.  A bucket is done after at most n rounds (Bellman–Ford inside the bucket:
// round k finishes every vertex whose lightest path uses at most k arcs of the bucket); the host gives up with GMSX_ERR_KERNEL after n + 1.
// Every bucket the host opens holds a final distance, so there are at most min(n, (n - 1) wmax / delta + 2) of them; beyond: GMSX_ERR_KERNEL.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"
#include "row_classes.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

constexpr long long kSsspDeltaAutoDefault = 16;  // measured once on four graphs and still a first guess (gmsx.h, OPTIONS)

template <class D> struct DistInf;
template <> struct DistInf<int32_t> { static constexpr int32_t value = INT_MAX; };
template <> struct DistInf<long long> { static constexpr long long value = LLONG_MAX; };

__device__ __forceinline__ long long load_now(const long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct SsspCtrl : FrontierCtrl {
    unsigned long long relax;  // improving atomics (diagnostic)
    unsigned long long next_min;  // the next-bucket pass: the smallest tentative distance at or above the bucket's end
};

// one relaxation round as a policy of the engine's kernels.  A parked row's note is the number of its round (long_walk is not told it).
template <class D>
struct SsspRelax {
    static constexpr int kGroupWords = 0;
    static constexpr bool kNotes = true;
    static constexpr bool kReenters = true;
    int64_t n;
    const int64_t *off;
    const int32_t *adj, *wgt;
    D *dist;
    int32_t *stamp;
    SsspCtrl *ctrl;
    long long hi;  // the current bucket ends below hi
    mutable unsigned long long improved = 0;

    __device__ __forceinline__ void relax(int32_t w, long long nd, int32_t mark, const NextQueue &q) const {
        if (nd >= (long long)dist[w]) return;  // (a stale value is too large: the atomic decides)
        const long long old = (long long)__hip_atomic_fetch_min(&dist[w], D(nd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nd >= old) return;
        ++improved;
        if (nd < hi && atomicExch(&stamp[w], mark) != mark) q.push(w);
    }
    __device__ __forceinline__ void short_row(int32_t x, int64_t j0, int64_t j1, int lane, int32_t round, uint32_t *, const NextQueue &q) const {
        const long long dx = (long long)load_now(&dist[x]);
        for (int64_t j = j0 + lane; j < j1; j += kGroup) relax(adj[j], dx + wgt[j], round + 1, q);
    }
    __device__ __forceinline__ void park(int32_t, int32_t round, unsigned long long *notes, int64_t pos, int32_t *) const {
        notes[pos] = (unsigned long long)uint32_t(round);
    }
    __device__ __forceinline__ void long_walk(int32_t x, unsigned long long note, int64_t tid, int64_t threads, const NextQueue &q) const {
        const long long dx = (long long)load_now(&dist[x]);
        const int32_t mark = int32_t(uint32_t(note)) + 1;
        const int64_t j1 = off[x + 1];
        for (int64_t j = off[x] + tid; j < j1; j += threads) relax(adj[j], dx + wgt[j], mark, q);
    }
    __device__ __forceinline__ void settle(int32_t, unsigned long long, int32_t, int, int32_t *) const {}
    // every thread, converged, at the end of a kernel: one add per wave
    __device__ __forceinline__ void finish() const {
        unsigned long long sum = improved;
        sum = wave_sum(sum);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&ctrl->relax, sum);
        improved = 0;
    }
};

template <class D>
__global__ __launch_bounds__(256) void k_sssp_init(int64_t n, int32_t source, D *__restrict__ dist, int32_t *__restrict__ stamp,
                                                   int32_t *__restrict__ frontier) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    dist[v] = v == int64_t(source) ? D(0) : DistInf<D>::value;
    stamp[v] = 0;
    if (v == int64_t(source)) frontier[0] = source;
}

// the smallest tentative distance in [from, infinity)
template <class D>
__global__ __launch_bounds__(256) void k_sssp_next_min(int64_t n, const D *__restrict__ dist, long long from, SsspCtrl *__restrict__ ctrl) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long best = ~0ull;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const D d = dist[v];
        if (d != DistInf<D>::value && (long long)d >= from) best = min(best, (unsigned long long)d);
    }
    best = wave_min(best);
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&ctrl->next_min, best);
}

// k_frontier_collect's predicate: v lies in bucket [lo, hi)
template <class D>
struct SsspInBucket {
    const D *dist;
    long long lo, hi;
    __device__ __forceinline__ bool operator()(int64_t v) const {
        const D d = dist[v];
        return d != DistInf<D>::value && (long long)d >= lo && (long long)d < hi;
    }
};

// the info pass's words (also the pull pass's)
struct SsspAcc {
    int32_t error, far;
    unsigned long long reached, arcs, dist_sum, max_dist;
    unsigned long long violated, untight, wrong_unreached;
};

// dist as the caller sees it (int64, -1 = unreachable) and the sums over the reached vertices
template <class D>
__global__ __launch_bounds__(256) void k_sssp_info(int64_t n, const int64_t *__restrict__ off, const D *__restrict__ dist, long long *__restrict__ out,
                                                   SsspAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;
    unsigned long long reached = 0, arcs = 0, dsum = 0, mx = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        if (v >= n) continue;
        const D d = dist[v];
        if (d == DistInf<D>::value) {
            out[v] = -1;
        } else if (d < 0) {
            acc->error = 1;
            out[v] = -1;
        } else {
            out[v] = (long long)d;
            ++reached;
            arcs += (unsigned long long)(off[v + 1] - off[v]);
            dsum += (unsigned long long)d;
            mx = max(mx, (unsigned long long)d);
        }
    }
    reached = wave_sum(reached);
    arcs = wave_sum(arcs);
    dsum = wave_sum(dsum);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && reached) {
        atomicAdd(&acc->reached, reached);
        atomicAdd(&acc->arcs, arcs);
        atomicAdd(&acc->dist_sum, dsum);
        atomicMax(&acc->max_dist, mx);
    }
}

// THE PULL PASS over dist (int64, below 0 = unreached), an Op of row_classes.hpp's two-width pass: the lanes of a vertex walk its ascending
// row chunk by chunk, a ballot per chunk; the lowest lane of the first chunk with a tight entry holds the smallest-id tight neighbour.
// kCount = false (gmsx_sssp): out at that chunk, parent written by that lane (one writer per vertex), far = the smallest id at max_dist; an
// unreached vertex and the source, with or without a row, are settled before the walk.  kCount = true (gmsx_sssp_verify): the whole row,
// and the three counts.  Arc u→v is met in v's row: the weights are symmetric.
template <bool kCount>
struct SsspPull {
    const int32_t *adj, *wgt;
    const long long *dist;
    int32_t source;
    int32_t *parent;
    SsspAcc *acc;
    unsigned long long max_dist = 0;                          // acc->max_dist, read once before the first row
    unsigned long long violated = 0, untight = 0, wrong = 0;  // this thread's sums: begin() sets them
    __device__ __forceinline__ void begin() { max_dist = kCount ? 0ull : acc->max_dist; violated = untight = wrong = 0; }
    template <int kLanes>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        const RowGroup<kLanes> grp;
        const long long dv = dist[v];
        const bool is_source = v == source;
        if (!kCount) {
            if (dv < 0 || is_source) {
                if (lane == 0) parent[v] = is_source && dv >= 0 ? source : -1;
                if (lane == 0 && is_source && (unsigned long long)dv == max_dist) atomicMin(&acc->far, v);
                return 0;
            }
            if (lane == 0 && (unsigned long long)dv == max_dist) atomicMin(&acc->far, v);
        }
        bool found = false, neighbour_reached = false;
        for (int64_t c = j0; c < j1; c += width) {
            const int64_t j = c + lane;
            bool tight = false;
            int32_t u = -1;
            if (j < j1) {
                u = adj[j];
                const long long du = dist[u];
                if (du >= 0) {
                    const unsigned long long via = (unsigned long long)du + (unsigned long long)uint32_t(wgt[j]);
                    neighbour_reached = true;
                    if (dv >= 0) {
                        tight = (unsigned long long)dv == via;
                        if (kCount && (unsigned long long)dv > via) ++violated;
                    }
                }
            }
            const unsigned long long hits = grp.ballot(tight);
            if (hits) {
                found = true;
                if (!kCount) {
                    if (lane == grp.first(hits)) parent[v] = u;
                    break;
                }
            }
        }
        if (kCount) {
            const bool any_reached = grp.ballot(neighbour_reached) != 0;
            if (lane == 0) {
                if (dv >= 0 && !is_source && !found) ++untight;
                if (dv < 0 && any_reached) ++wrong;
            }
        } else if (!found && lane == 0) {
            ++untight;
        }
        return 0;
    }
    __device__ __forceinline__ void finish() {
        violated = wave_sum(violated);
        untight = wave_sum(untight);
        wrong = wave_sum(wrong);
        if ((threadIdx.x & 63) == 0) {
            if (violated) atomicAdd(&acc->violated, violated);
            if (untight) atomicAdd(&acc->untight, untight);
            if (wrong) atomicAdd(&acc->wrong_unreached, wrong);
        }
    }
};

// ---- attaching weights ---------------------------------------------------------------------------------------------------------------------

struct WeightAcc {
    int32_t bad_range, bad_twin, wmax, pad;
    unsigned long long sum;
};

// a thread per arc j: its row u by a binary search over off (at most 64 steps), its twin by one in v's row (at most 64 steps)
__global__ __launch_bounds__(256) void k_weights_check(int64_t n, int64_t nnz, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                       const int32_t *__restrict__ wgt, int check_twin, WeightAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((nnz + 63) / 64) * 64;
    unsigned long long sum = 0;
    int32_t wmax = 0;
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < end; j += stride) {
        if (j >= nnz) continue;
        const int32_t w = wgt[j];
        if (w < 1) {
            acc->bad_range = 1;
            continue;
        }
        sum += (unsigned long long)w;
        wmax = max(wmax, w);
        if (!check_twin) continue;
        int64_t lo = 0, hi = n;  // the row u with off[u] <= j < off[u + 1]: the last u with off[u] <= j
        for (int step = 0; step < 64 && hi - lo > 1; ++step) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (off[mid] <= j) lo = mid;
            else hi = mid;
        }
        const int64_t u = lo;
        const int32_t v = adj[j];
        if (v < 0 || int64_t(v) >= n || off[u] > j || off[u + 1] <= j) {
            acc->bad_twin = 1;
            continue;
        }
        int64_t a = off[v], b = off[v + 1];  // the first entry of v's row that is >= u
        for (int step = 0; step < 64 && a < b; ++step) {
            const int64_t mid = a + (b - a) / 2;
            if (int64_t(adj[mid]) < u) a = mid + 1;
            else b = mid;
        }
        if (a >= off[v + 1] || int64_t(adj[a]) != u || wgt[a] != w) acc->bad_twin = 1;
    }
    sum = wave_sum(sum);
    wmax = wave_max(wmax);
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&acc->sum, sum);
        atomicMax(&acc->wmax, wmax);
    }
}

// ---- the host ------------------------------------------------------------------------------------------------------------------------------

struct SsspBufs {
    DevBuf dist, stamp, out, parent, ctrl, acc;
    FrontierStore store;
};

struct SsspRun {
    int64_t buckets = 0, rounds = 0, relaxations = 0;
};

// The distances from `source` on the library's stream, n > 0: b.dist holds them (words of D), *run the loop's counts.
template <class D>
int sssp_run(const gmsx_graph *g, int32_t source, long long delta, long long wg_frontier, const SsspBufs &b, SsspRun *run, int *launches) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const unsigned per_vertex = unsigned((n + 255) / 256);
    const unsigned sweep = row_grid(n, 1, cus, 16);
    D *dist = b.dist.as<D>();
    SsspCtrl *ctrl = b.ctrl.as<SsspCtrl>();
    const FrontierBufs bufs = b.store.bufs();
    SsspRelax<D> p{n, g->off, g->adj, g->wgt.as<const int32_t>(), dist, b.stamp.as<int32_t>(), ctrl, 0};

    hipLaunchKernelGGL(k_sssp_init<D>, dim3(per_vertex), dim3(256), 0, s, n, source, dist, b.stamp.as<int32_t>(), bufs.f[0]);
    ++*launches;
    SsspCtrl h;
    std::memset(&h, 0, sizeof h);
    h.count = 1;
    h.next_min = ~0ull;
    // every bucket the loop opens holds a final distance: at most one per vertex, and none beyond the heaviest simple path
    const unsigned __int128 span = (unsigned __int128)(n - 1) * (unsigned __int128)std::max<int32_t>(g->wmax, 1) / (unsigned __int128)delta + 2;
    const int64_t bucket_cap = int64_t(std::min<unsigned __int128>(span, (unsigned __int128)n));
    long long lo = 0;
    for (;;) {
        const long long hi = lo > LLONG_MAX - delta ? LLONG_MAX : lo + delta;
        if (++run->buckets > bucket_cap) return GMSX_ERR_KERNEL;
        p.hi = hi;
        GMSX_HIP(hipMemcpyAsync(ctrl, &h, sizeof h, hipMemcpyHostToDevice, s));
        const int64_t round_cap = int64_t(h.round) + n + 1;  // a bucket is done after at most n rounds (BOUNDS)
        if (int rc = run_frontier_rounds(p, bufs, ctrl, h, wg_frontier, launches, [=](const SsspCtrl &m) { return int64_t(m.round) > round_cap; })) return rc;
        if (h.count > 0) return GMSX_ERR_KERNEL;
        // ---- the next bucket: the one of the smallest tentative distance at or above hi
        if (hi == LLONG_MAX) break;
        hipLaunchKernelGGL(k_sssp_next_min<D>, dim3(sweep), dim3(256), 0, s, n, dist, hi, ctrl);
        ++*launches;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.error || h.count != 0) return GMSX_ERR_KERNEL;
        if (h.next_min == ~0ull) break;
        if (h.next_min > (unsigned long long)LLONG_MAX || (long long)h.next_min < hi) return GMSX_ERR_KERNEL;
        lo = (long long)h.next_min / delta * delta;
        const long long hi2 = lo > LLONG_MAX - delta ? LLONG_MAX : lo + delta;
        h.next = h.nlong = h.bail = h.cur = h.done = 0;
        h.next_min = ~0ull;
        GMSX_HIP(hipMemcpyAsync(ctrl, &h, sizeof h, hipMemcpyHostToDevice, s));
        frontier_collect(n, SsspInBucket<D>{dist, lo, hi2}, bufs.f[0], &ctrl->count, &ctrl->error);
        ++*launches;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.error || h.count < 1 || int64_t(h.count) > n) return GMSX_ERR_KERNEL;
    }
    run->rounds = h.round;
    run->relaxations = int64_t(h.relax);
    return GMSX_OK;
}

int sssp_alloc(const gmsx_graph *g, bool wide, SsspBufs &b) {
    const int64_t n = g->n;
    if (int rc = b.store.alloc(n, g->nnz, true)) return rc;
    if (int rc = wide ? dalloc<long long>(b.dist, n) : dalloc<int32_t>(b.dist, n)) return rc;
    if (int rc = dalloc<int32_t>(b.stamp, n)) return rc;
    if (int rc = dalloc<long long>(b.out, n)) return rc;
    if (int rc = dalloc<int32_t>(b.parent, n)) return rc;
    if (int rc = dalloc<SsspCtrl>(b.ctrl, 1)) return rc;
    if (int rc = dalloc<SsspAcc>(b.acc, 1)) return rc;
    return GMSX_OK;
}

// the pull pass over `dist` (device, int64)
template <bool kCount>
void sssp_pull(const gmsx_graph *g, const long long *dist, int32_t source, int32_t *parent, SsspAcc *acc, int *launches) {
    Ctx &c = ctx();
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    launch_rows_two_width(SsspPull<kCount>{g->adj, g->wgt.as<const int32_t>(), dist, source, parent, acc}, g, nullptr, cus, c.stream, launches);
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_graph_set_weights(gmsx_graph *g, const int32_t *weights) {
    return gmsx::guard([&]() -> int {
        if (!g) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        if (!weights) {  // detach
            g->wgt.reset();
            g->device_bytes -= g->wgt_bytes;
            g->wgt_bytes = g->wsum = 0;
            g->wmax = 0;
            g->wide_dist = false;
            return GMSX_OK;
        }
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        DevBuf fresh, d_acc;
        if (int rc = dalloc<int32_t>(fresh, g->nnz)) return rc;
        if (int rc = dalloc<WeightAcc>(d_acc, 1)) return rc;
        WeightAcc a;
        std::memset(&a, 0, sizeof a);
        if (g->nnz > 0) {
            GMSX_HIP(hipMemcpyAsync(fresh.p, weights, size_t(g->nnz) * sizeof(int32_t), hipMemcpyHostToDevice, s));
            GMSX_HIP(hipMemsetAsync(d_acc.p, 0, sizeof(WeightAcc), s));
            const unsigned grid = unsigned(std::min<int64_t>((g->nnz + 255) / 256, int64_t(cus) * 16));
            hipLaunchKernelGGL(k_weights_check, dim3(grid), dim3(256), 0, s, g->n, g->nnz, g->off, g->adj, fresh.as<const int32_t>(),
                               (g->upload_flags & GMSX_UPLOAD_TRUSTED) ? 0 : 1, d_acc.as<WeightAcc>());
            GMSX_HIP(hipMemcpyAsync(&a, d_acc.p, sizeof a, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            GMSX_HIP(hipGetLastError());
        }
        if (a.bad_range) return GMSX_ERR_INVALID;
        if (a.bad_twin) return GMSX_ERR_NOT_CANONICAL;
        g->device_bytes -= g->wgt_bytes;
        g->wgt = std::move(fresh);
        g->wgt_bytes = int64_t(std::max<int64_t>(g->nnz, 1)) * int64_t(sizeof(int32_t));
        g->device_bytes += g->wgt_bytes;
        g->wsum = int64_t(a.sum);
        g->wmax = a.wmax;
        g->wide_dist = (unsigned __int128)std::max<int64_t>(g->n - 1, 0) * (unsigned __int128)std::max<int32_t>(a.wmax, 0) >= (unsigned __int128)INT_MAX;
        return GMSX_OK;
    });
}

int gmsx_graph_has_weights(const gmsx_graph *g) { return !g ? GMSX_ERR_INVALID : (g->wgt.p ? 1 : 0); }

int gmsx_sssp(const gmsx_graph *g, int32_t source, int64_t delta, int64_t *dist, int32_t *parent, gmsx_sssp_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || delta < 0) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        if (!g->wgt.p || source < 0 || int64_t(source) >= n) return GMSX_ERR_INVALID;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        const bool wide = g->wide_dist || opt_int("SSSP_WIDE", 0) != 0;
        const long long wg_frontier = frontier_wg_option("SSSP_WG_FRONTIER", kWgFrontierDefault);
        long long d = delta;
        if (d == 0) {  // the default rule: a function of the handle's mean weight and mean degree
            const long long cpar = std::max<long long>(1, std::min<long long>(opt_int("SSSP_DELTA_AUTO", kSsspDeltaAutoDefault), 1 << 20));
            const double mean_w = g->nnz > 0 ? double(g->wsum) / double(g->nnz) : 1.0;
            const double mean_deg = std::max(1.0, double(g->nnz) / double(n));
            const double v = double(cpar) * mean_w / mean_deg;
            d = v < 1.0 ? 1 : (v > 9.0e18 ? LLONG_MAX : (long long)(v + 0.5));
        }
        SsspBufs b;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = sssp_alloc(g, wide, b)) return rc;
        SsspAcc *acc = b.acc.as<SsspAcc>();
        GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(SsspAcc), s));
        GMSX_HIP(hipMemsetAsync(&acc->far, 0x7f, sizeof(int32_t), s));
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        SsspRun run;
        int launches = 0;
        if (int rc = wide ? sssp_run<long long>(g, source, d, wg_frontier, b, &run, &launches) : sssp_run<int32_t>(g, source, d, wg_frontier, b, &run, &launches))
            return rc;
        // ---- the info and the pull pass
        const unsigned sweep = row_grid(n, 1, cus, 16);
        if (wide)
            hipLaunchKernelGGL(k_sssp_info<long long>, dim3(sweep), dim3(256), 0, s, n, g->off, b.dist.as<const long long>(), b.out.as<long long>(), acc);
        else
            hipLaunchKernelGGL(k_sssp_info<int32_t>, dim3(sweep), dim3(256), 0, s, n, g->off, b.dist.as<const int32_t>(), b.out.as<long long>(), acc);
        ++launches;
        sssp_pull<false>(g, b.out.as<const long long>(), source, b.parent.as<int32_t>(), acc, &launches);
        SsspAcc a;
        GMSX_HIP(hipMemcpyAsync(&a, acc, sizeof a, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipEventRecord(c.ev[2], s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (a.error || a.untight || a.reached < 1 || a.reached > (unsigned long long)n || a.far < 0 || int64_t(a.far) >= n ||
            a.max_dist > (unsigned long long)LLONG_MAX)
            return GMSX_ERR_KERNEL;
        // the flag words were read as zero: the caller's arrays are written now, through host staging
        std::vector<int64_t> h_dist;
        std::vector<int32_t> h_parent;
        if (dist) {
            h_dist.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_dist.data(), b.out.p, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        }
        if (parent) {
            h_parent.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_parent.data(), b.parent.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        GMSX_HIP(hipStreamSynchronize(s));
        float up_ms = 0.f, ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
        if (dist) std::memcpy(dist, h_dist.data(), size_t(n) * sizeof(int64_t));
        if (parent) std::memcpy(parent, h_parent.data(), size_t(n) * sizeof(int32_t));
        gmsx_sssp_info res;
        std::memset(&res, 0, sizeof res);
        res.reached = int64_t(a.reached);
        res.reached_arcs = int64_t(a.arcs);
        res.dist_sum = int64_t(a.dist_sum);
        res.max_dist = int64_t(a.max_dist);
        res.delta = d;
        res.buckets = run.buckets;
        res.rounds = run.rounds;
        res.relaxations = run.relaxations;
        res.far_vertex = a.far;
        res.wide = wide ? 1 : 0;
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), double(up_ms), uint64_t(res.reached_arcs), 0, uint64_t(res.buckets), launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_sssp_verify(const gmsx_graph *g, int32_t source, const int64_t *dist, gmsx_sssp_check *out, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !out) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        if (!g->wgt.p || source < 0 || int64_t(source) >= n || !dist) return GMSX_ERR_INVALID;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        DevBuf d_dist, d_acc;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = dalloc<long long>(d_dist, n)) return rc;
        if (int rc = dalloc<SsspAcc>(d_acc, 1)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_dist.p, dist, size_t(n) * sizeof(int64_t), hipMemcpyHostToDevice, s));
        GMSX_HIP(hipMemsetAsync(d_acc.p, 0, sizeof(SsspAcc), s));
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        int launches = 0;
        sssp_pull<true>(g, d_dist.as<const long long>(), source, nullptr, d_acc.as<SsspAcc>(), &launches);
        SsspAcc a;
        GMSX_HIP(hipMemcpyAsync(&a, d_acc.p, sizeof a, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipEventRecord(c.ev[2], s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        float up_ms = 0.f, ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
        gmsx_sssp_check res;
        std::memset(&res, 0, sizeof res);
        res.violated_arcs = int64_t(a.violated);
        res.untight = int64_t(a.untight);
        res.wrong_unreached = int64_t(a.wrong_unreached);
        res.source_ok = dist[source] == 0 ? 1 : 0;
        *out = res;
        if (stats) *stats = gmsx_stats{double(ms), double(up_ms), uint64_t(g->nnz), 0, 0, launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
