// Breadth-first search and betweenness centrality on gfx950, over the uploaded CSR.
//   gmsx_bfs          direction-optimising BFS (representations/graphs/log_graph/bfs.cc:120-190, DOBFS): depth[v] and parent[v] = the SMALLEST-id
//                     neighbour of v one level up — what the reference's bottom-up step writes (the first frontier entry of an ascending row,
//                     bfs.cc:51-57), taken here in every direction, so both arrays are facts about (graph, source)
//   gmsx_betweenness  Brandes' algorithm from a list of sources (bc.cc:89-153), one source after the other, in double and without any
//                     floating-point atomic: scores is a fact about (graph, sources, flags)
// The definitions are those of include/gmsx.h.
//
// TOP-DOWN LEVELS are a policy of the frontier-rounds engine (frontier_rounds.hpp: the binning, the parked long rows, the one-workgroup tail under
// BFS_WG_FRONTIER).  A walker of frontier vertex x claims an unvisited entry w by atomicCAS(depth[w], -1, round + 1) and appends it; EVERY walker
// that sees depth[w] == round + 1 lowers parent[w] to x by atomicMin.  The claim adds w's degree to the control block: the reference's scout_count.
// At every round boundary ONE thread (round_stop: the advance kernel's, or thread 0 of the tail) applies the reference's rule — bottom-up when
// scout_count > edges_to_check / alpha (bfs.cc:145), else edges_to_check -= scout_count (:180) — so the decision is the same whether a round
// boundary is a kernel boundary or a barrier of the tail.
//
// BOTTOM-UP LEVELS (k_bfs_bottom_up, k_bfs_bottom_up_rows): two bitmaps of n bits.  Pass 1: a lane per unvisited vertex probes the first
// BFS_BU_PROBE entries of its row and stops at the first set bit (on a degree-relabelled graph those are the hubs); a vertex that found nothing and
// has a longer row is appended to a list.  Pass 2 walks the rest of those rows with a kGroup-lane group (a wave above kLongRow), chunk by chunk, a
// ballot per chunk, out at the first chunk with a hit: the lowest hit lane holds the smallest id.  No lane walks a long row alone, every loop is
// bounded by the row length, nothing waits for another thread.  The step reads `front` and depth of its OWN vertex only, so it has no race.
//
// SWITCHING (the host, at round boundaries; bfs.cc:142-188): bottom-up while the awake count does not fall or exceeds n / beta; then the last level
// is collected into a frontier list and the rounds go on top-down with scout_count = 1.
//
// BETWEENNESS.  Per source: the depths above; a counting sort of the reached vertices by depth (the level histogram of the BFS info pass, one
// workgroup's scan, one scatter — the order inside a level reaches no output); sigma forward and delta backward level by level, both by PULL: the
// row of v is summed by the lanes the binning gives it, each over a fixed stride, the partial sums combined by a fixed shuffle tree; a row above
// kLongRow is cut into chunks of kBcChunk entries, a wave per chunk (handed out by slot: slot_row) writes its partial sum to a slot and one thread
// adds the slots in slot order.
// scores[u] += delta(u) has one writer.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

// first guesses, not tuned values (gmsx.h, OPTIONS)
constexpr long long kBfsAlphaDefault = 15, kBfsBetaDefault = 18, kBfsProbeDefault = 16;
constexpr int kBcChunk = 4096;  // entries of a long row one wave sums (64 per lane)

// control block of one run: the engine's, plus the switching rule's and the bottom-up step's words
struct BfsCtrl : FrontierCtrl {
    int32_t stop;                  // round_stop: the next level belongs to the bottom-up step
    int32_t bu_list;               // vertices pass 1 of the bottom-up step left to pass 2
    unsigned long long scout_acc;  // degrees of what the current round appended so far
    unsigned long long scout;      // … of the last finished round: scout_count
    long long etc;                 // edges_to_check
    unsigned long long awake, awake_deg;  // bottom-up step: vertices found; their degrees (informational: the host's rule reads awake only,
                                          // since after bottom-up levels the reference goes on with scout_count = 1, bfs.cc:175)
};

// the info pass's words
struct BfsAcc {
    int32_t error, maxdepth;
    unsigned long long reached, arcs, depth_sum, best, nonempty, hist_sum;
};

__device__ __forceinline__ bool bit_set(const uint32_t *__restrict__ bits, int32_t w) { return (bits[w >> 5] >> (w & 31)) & 1u; }

// one top-down level as a policy of the engine
struct BfsTopDown {
    static constexpr int kGroupWords = 0;
    static constexpr bool kNotes = false;
    static constexpr bool kStops = true;
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    int32_t *depth, *parent;
    BfsCtrl *ctrl;
    long long alpha;  // 0: never hand over to the bottom-up step

    __device__ __forceinline__ void visit(int32_t x, int32_t w, int32_t nd, const NextQueue &q) const {
        int32_t d = load_now(&depth[w]);
        if (d == -1) {
            d = atomicCAS(&depth[w], -1, nd);
            if (d == -1) {
                q.push(w);
                atomicAdd(&ctrl->scout_acc, (unsigned long long)(off[w + 1] - off[w]));
                d = nd;
            }
        }
        if (d == nd && load_now(&parent[w]) > x) atomicMin(&parent[w], x);
    }
    __device__ __forceinline__ void short_row(int32_t x, int64_t j0, int64_t j1, int lane, int32_t round, uint32_t *, const NextQueue &q) const {
        for (int64_t j = j0 + lane; j < j1; j += kGroup) visit(x, adj[j], round + 1, q);
    }
    __device__ __forceinline__ void park(int32_t, int32_t, unsigned long long *, int64_t, int32_t *) const {}
    __device__ __forceinline__ void long_walk(int32_t x, unsigned long long, int64_t tid, int64_t threads, const NextQueue &q) const {
        const int32_t nd = load_now(&depth[x]) + 1;  // (x is in the frontier: its depth is final, but inside the tail it was claimed by an atomic of this kernel)
        const int64_t j1 = off[x + 1];
        for (int64_t j = off[x] + tid; j < j1; j += threads) visit(x, adj[j], nd, q);
    }
    __device__ __forceinline__ void finish() const {}
    // ONE thread, at a round boundary, behind every append of the round: the reference's rule for the level that comes next
    __device__ __forceinline__ bool round_stop() const {
        const unsigned long long s = atomicExch(&ctrl->scout_acc, 0ull);
        ctrl->scout = s;
        if (alpha > 0 && (long long)s > ctrl->etc / alpha) {
            ctrl->stop = 1;
            return true;
        }
        ctrl->etc -= (long long)s;
        return false;
    }
};

__global__ __launch_bounds__(256) void k_bfs_init(int64_t n, int32_t source, int32_t *__restrict__ depth, int32_t *__restrict__ parent,
                                                  int32_t *__restrict__ hist, int32_t *__restrict__ frontier) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const bool src = v == int64_t(source);
    depth[v] = src ? 0 : -1;
    parent[v] = src ? source : INT_MAX;
    hist[v] = 0;
    if (src) frontier[0] = source;
}

// QueueToBitmap (bfs.cc:90-96)
__global__ __launch_bounds__(256) void k_bfs_list_bits(const int32_t *__restrict__ list, int64_t count, uint32_t *__restrict__ bits) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < count) {
        const int32_t w = list[i];
        atomicOr(&bits[w >> 5], 1u << (w & 31));
    }
}

// v joins level `level` under parent p (one writer per vertex)
__device__ __forceinline__ void bu_take(int32_t v, int32_t p, int32_t level, int32_t *__restrict__ depth, int32_t *__restrict__ parent,
                                        uint32_t *__restrict__ next) {
    depth[v] = level;
    parent[v] = p;
    atomicOr(&next[v >> 5], 1u << (v & 31));
}

// bottom-up, pass 1: a lane per unvisited vertex over the first `probe` entries of its row
__global__ __launch_bounds__(256) void k_bfs_bottom_up(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int32_t level,
                                                       int32_t probe, const uint32_t *__restrict__ front, uint32_t *__restrict__ next,
                                                       int32_t *__restrict__ depth, int32_t *__restrict__ parent, int32_t *__restrict__ list,
                                                       BfsCtrl *__restrict__ ctrl) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;  // whole waves stay converged for the ballot
    unsigned long long awake = 0, deg = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        bool more = false;
        if (v < n && depth[v] == -1) {
            const int64_t j0 = off[v], len = off[v + 1] - j0;
            const int64_t m = min(len, int64_t(probe));
            int32_t p = -1;
            for (int64_t j = j0; j < j0 + m; ++j) {
                const int32_t w = adj[j];
                if (bit_set(front, w)) {
                    p = w;
                    break;
                }
            }
            if (p >= 0) {
                bu_take(int32_t(v), p, level, depth, parent, next);
                ++awake;
                deg += (unsigned long long)len;
            } else {
                more = len > m;
            }
        }
        wave_append(more, int32_t(v), list, &ctrl->bu_list, n, &ctrl->error);
    }
    awake = wave_sum(awake);
    deg = wave_sum(deg);
    if ((threadIdx.x & 63) == 0 && awake) {
        atomicAdd(&ctrl->awake, awake);
        atomicAdd(&ctrl->awake_deg, deg);
    }
}

// bottom-up, pass 2: the rows pass 1 listed, from entry `probe` on, WIDTH lanes per row (kGroup: rows up to kLongRow; 64: the longer ones);
// a ballot per chunk of WIDTH entries, out at the first chunk with a hit
template <int WIDTH>
__global__ __launch_bounds__(256) void k_bfs_bottom_up_rows(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int32_t level,
                                                            int32_t probe, const uint32_t *__restrict__ front, uint32_t *__restrict__ next,
                                                            int32_t *__restrict__ depth, int32_t *__restrict__ parent,
                                                            const int32_t *__restrict__ list, BfsCtrl *__restrict__ ctrl) {
    const RowGroup<WIDTH> grp;
    const int lane = grp.lane;
    const int64_t row0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / WIDTH;
    const int64_t rows_step = (int64_t(gridDim.x) * blockDim.x) / WIDTH;
    const int64_t rows = min(int64_t(ctrl->bu_list), n);
    unsigned long long awake = 0, deg = 0;  // (the lane that holds the hit counts for its group)
    for (int64_t i = row0; i < rows; i += rows_step) {
        const int32_t v = list[i];
        const int64_t j0 = off[v], j1 = off[v + 1];
        const bool is_long = j1 - j0 > kLongRow;
        if (is_long != (WIDTH == 64)) continue;
        for (int64_t c = j0 + probe; c < j1; c += WIDTH) {  // (uniform in the group: its lanes leave together)
            const int64_t j = c + lane;
            const int32_t w = j < j1 ? adj[j] : -1;
            const bool hit = w >= 0 && bit_set(front, w);
            const unsigned long long hits = grp.ballot(hit);
            if (hits) {
                if (lane == grp.first(hits)) {
                    bu_take(v, w, level, depth, parent, next);
                    ++awake;
                    deg += (unsigned long long)(j1 - j0);
                }
                break;
            }
        }
    }
    awake = wave_sum(awake);
    deg = wave_sum(deg);
    if ((threadIdx.x & 63) == 0 && awake) {
        atomicAdd(&ctrl->awake, awake);
        atomicAdd(&ctrl->awake_deg, deg);
    }
}

// BitmapToQueue (bfs.cc:98-110), from the depths: k_frontier_collect's predicate for the vertices of level d
struct BfsAtDepth {
    const int32_t *depth;
    int32_t d;
    __device__ __forceinline__ bool operator()(int64_t v) const { return depth[v] == d; }
};

// the final pass: parent of the unreached = -1, hist[depth] (one add per distinct depth of a wave), the sums
__global__ __launch_bounds__(256) void k_bfs_info(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ depth,
                                                  int32_t *__restrict__ parent, int32_t *__restrict__ hist, BfsAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;
    const int lane = threadIdx.x & 63;
    unsigned long long reached = 0, arcs = 0, dsum = 0;
    int32_t mx = -1;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        int32_t d = -1;
        if (v < n) {
            d = depth[v];
            const int32_t p = parent[v];
            if (d < 0) {
                if (d != -1 || p != INT_MAX) acc->error = 1;
                parent[v] = -1;
                d = -1;
            } else if (int64_t(d) >= n || p < 0 || int64_t(p) >= n) {
                acc->error = 1;
                d = -1;
            } else {
                ++reached;
                arcs += (unsigned long long)(off[v + 1] - off[v]);
                dsum += (unsigned long long)d;
                mx = max(mx, d);
            }
        }
        unsigned long long todo = __ballot(d >= 0);
        while (todo) {  // at most 64 turns: every turn retires the lanes of one depth
            const int first = __ffsll((long long)todo) - 1;
            const int32_t d0 = __shfl(d, first);
            const unsigned long long same = __ballot(d == d0) & todo;
            if (lane == first) atomicAdd(&hist[d0], int32_t(__popcll(same)));
            todo &= ~same;
        }
    }
    reached = wave_sum(reached);
    arcs = wave_sum(arcs);
    dsum = wave_sum(dsum);
    mx = wave_max(mx);
    if (lane == 0 && reached) {
        atomicAdd(&acc->reached, reached);
        atomicAdd(&acc->arcs, arcs);
        atomicAdd(&acc->depth_sum, dsum);
        atomicMax(&acc->maxdepth, mx);
    }
}

// … and over the histogram: the non-empty levels and the widest one as the maximum of size << 32 | ~depth (ties: the smallest depth)
__global__ __launch_bounds__(256) void k_bfs_levels(int64_t n, const int32_t *__restrict__ hist, BfsAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long nonempty = 0, sum = 0, best = 0;
    for (int64_t d = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; d < n; d += stride) {
        const uint32_t s = uint32_t(hist[d]);
        if (!s) continue;
        ++nonempty;
        sum += s;
        best = max(best, ((unsigned long long)s << 32) | (0xffffffffu - uint32_t(d)));
    }
    nonempty = wave_sum(nonempty);
    sum = wave_sum(sum);
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0 && nonempty) {
        atomicAdd(&acc->nonempty, nonempty);
        atomicAdd(&acc->hist_sum, sum);
        atomicMax(&acc->best, best);
    }
}

// ---- betweenness --------------------------------------------------------------------------------------------------------------------------

struct BcCtrl {
    int32_t error, nlong;
    unsigned long long slots;      // slots handed to the parked rows of the level
    unsigned long long max_sigma;  // bits of the largest path count (non-negative doubles order like their bits)
};

struct BcArgs {
    const int64_t *off;
    const int32_t *adj, *depth, *order;
    double *sigma, *delta, *scores;
    int32_t *longs;
    unsigned long long *notes;
    int32_t *slot_row;  // which parked row a slot belongs to
    double *slots;
    int64_t long_cap, slot_cap;
    BcCtrl *ctrl;
    int32_t skip;  // GMSX_BC_EXCLUDE_SOURCE: the source, whose own delta stays out; else -1
};

// loff[d] = vertices of the levels below d, d = 0 .. levels; cursor = the same (the scatter's counters).  ONE workgroup.
__global__ __launch_bounds__(1024) void k_bc_scan(int32_t levels, const int32_t *__restrict__ hist, int32_t *__restrict__ loff,
                                                  int32_t *__restrict__ cursor) {
    __shared__ int32_t s_sum[1024];
    const int t = threadIdx.x;
    const int32_t per = (levels + 1023) / 1024;
    const int32_t lo = min(levels, t * per), hi = min(levels, lo + per);
    int32_t mine = 0;
    for (int32_t d = lo; d < hi; ++d) mine += hist[d];
    s_sum[t] = mine;
    __syncthreads();
    if (t == 0) {
        int32_t run = 0;
        for (int i = 0; i < 1024; ++i) {
            const int32_t x = s_sum[i];
            s_sum[i] = run;
            run += x;
        }
        loff[levels] = run;
    }
    __syncthreads();
    int32_t run = s_sum[t];
    for (int32_t d = lo; d < hi; ++d) {
        loff[d] = run;
        cursor[d] = run;
        run += hist[d];
    }
}

__global__ __launch_bounds__(256) void k_bc_scatter(int64_t n, int32_t levels, const int32_t *__restrict__ depth, const int32_t *__restrict__ loff,
                                                    int32_t *__restrict__ cursor, int32_t *__restrict__ order, BcCtrl *__restrict__ ctrl) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int32_t d = depth[v];
    if (d < 0) return;
    if (d >= levels) {
        ctrl->error = 1;
        return;
    }
    const int32_t pos = atomicAdd(&cursor[d], 1);
    if (pos < loff[d + 1] && int64_t(pos) < n) order[pos] = int32_t(v);
    else ctrl->error = 1;
}

// what entry w of x's row adds: sigma pulls the path counts of the level above, delta the reference's expression (bc.cc:131-132) of the level below
template <bool kDelta>
__device__ __forceinline__ double bc_term(const BcArgs &a, int32_t w, int32_t d, double sx) {
    if (a.depth[w] != (kDelta ? d + 1 : d - 1)) return 0.0;
    if (kDelta) return sx / a.sigma[w] * (1.0 + a.delta[w]);
    return a.sigma[w];
}
// x's single owner stores the finished sum
template <bool kDelta>
__device__ __forceinline__ void bc_store(const BcArgs &a, int32_t x, double sum) {
    if (kDelta) {
        a.delta[x] = sum;
        if (x != a.skip) a.scores[x] += sum;
    } else {
        a.sigma[x] = sum;
        atomicMax(&a.ctrl->max_sigma, (unsigned long long)__double_as_longlong(sum));
    }
}

// level d = order[lo, hi): a kGroup-lane group per vertex, lane l over the entries l, l + kGroup, … of the row, one fixed shuffle tree; a row
// above kLongRow is parked with ceil(len / kBcChunk) slots
template <bool kDelta>
__global__ __launch_bounds__(256) void k_bc_rows(BcArgs a, int32_t lo, int32_t hi, int32_t d) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    for (int64_t i = int64_t(lo) + group0; i < hi; i += groups) {
        const int32_t x = a.order[i];
        const int64_t j0 = a.off[x], j1 = a.off[x + 1];
        if (j1 - j0 > kLongRow) {
            long long park_pos = -1, park_at = -1;  // (lane 0's, handed to the group by shuffles: not through memory)
            if (lane == 0) {
                const int64_t pos = append_checked(a.longs, &a.ctrl->nlong, a.long_cap, x, &a.ctrl->error);
                if (pos >= 0) {
                    const unsigned long long chunks = (unsigned long long)((j1 - j0 + kBcChunk - 1) / kBcChunk);
                    const unsigned long long at = atomicAdd(&a.ctrl->slots, chunks);
                    if (at + chunks <= (unsigned long long)a.slot_cap) {
                        a.notes[pos] = at;
                        park_pos = pos;
                        park_at = (long long)at;
                    } else {
                        a.ctrl->error = 1;
                    }
                }
            }
            // the group fills the slot -> row map of its row (k_bc_long hands a chunk to a wave by its slot)
            park_pos = __shfl(park_pos, 0, kGroup);
            park_at = __shfl(park_at, 0, kGroup);
            if (park_pos >= 0) {
                const int64_t chunks = (j1 - j0 + kBcChunk - 1) / kBcChunk;  // (park_at + chunks <= slot_cap: checked by lane 0)
                for (int64_t c = lane; c < chunks; c += kGroup) a.slot_row[park_at + c] = int32_t(park_pos);
            }
            continue;
        }
        const double sx = kDelta ? a.sigma[x] : 0.0;
        double part = 0.0;
        for (int64_t j = j0 + lane; j < j1; j += kGroup) part += bc_term<kDelta>(a, a.adj[j], d, sx);
        part = wave_sum<kGroup>(part);
        if (lane == 0) bc_store<kDelta>(a, x, part);
    }
}

// … its parked rows: a wave per chunk — slot s belongs to parked row slot_row[s] and is its chunk s - note —, the chunk's partial sum into its slot
template <bool kDelta>
__global__ __launch_bounds__(256) void k_bc_long(BcArgs a, int32_t d) {
    if (a.ctrl->error) return;  // (a parked row without its note)
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, waves = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const int64_t nlong = min(int64_t(a.ctrl->nlong), a.long_cap);
    const int64_t nslots = int64_t(min(a.ctrl->slots, (unsigned long long)a.slot_cap));
    for (int64_t s = wave0; s < nslots; s += waves) {
        const int64_t i = a.slot_row[s];
        if (i < 0 || i >= nlong) {
            a.ctrl->error = 1;
            continue;
        }
        const int32_t x = a.longs[i];
        const int64_t j0 = a.off[x], j1 = a.off[x + 1];
        const int64_t c = s - int64_t(a.notes[i]);
        const int64_t c0 = j0 + c * kBcChunk, c1 = min(j1, c0 + kBcChunk);
        if (c < 0 || c0 >= j1) {
            a.ctrl->error = 1;
            continue;
        }
        const double sx = kDelta ? a.sigma[x] : 0.0;
        double part = 0.0;
        for (int64_t j = c0 + lane; j < c1; j += 64) part += bc_term<kDelta>(a, a.adj[j], d, sx);
        part = wave_sum(part);
        if (lane == 0) a.slots[s] = part;
    }
}

// … added in slot order by the row's one owner
template <bool kDelta>
__global__ __launch_bounds__(256) void k_bc_long_sum(BcArgs a) {
    if (a.ctrl->error) return;
    const int64_t nlong = min(int64_t(a.ctrl->nlong), a.long_cap);
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= nlong) return;
    const int32_t x = a.longs[i];
    const int64_t chunks = (a.off[x + 1] - a.off[x] + kBcChunk - 1) / kBcChunk;
    const double *slot = a.slots + a.notes[i];
    double sum = 0.0;
    for (int64_t c = 0; c < chunks; ++c) sum += slot[c];
    bc_store<kDelta>(a, x, sum);
}

__global__ void k_bc_seed(int32_t source, double *__restrict__ sigma) { sigma[source] = 1.0; }

// ---- the host ------------------------------------------------------------------------------------------------------------------------------

struct BfsOptions {
    long long direction, alpha, beta, probe, wg_frontier;
};

BfsOptions bfs_options() {
    BfsOptions o;
    o.direction = opt_int("BFS_DIRECTION", 0);
    if (o.direction < 0 || o.direction > 2) o.direction = 0;
    o.alpha = std::max<long long>(1, std::min<long long>(opt_int("BFS_ALPHA", kBfsAlphaDefault), INT_MAX));
    o.beta = std::max<long long>(1, std::min<long long>(opt_int("BFS_BETA", kBfsBetaDefault), INT_MAX));
    o.probe = std::max<long long>(0, std::min<long long>(opt_int("BFS_BU_PROBE", kBfsProbeDefault), kLongRow));
    o.wg_frontier = frontier_wg_option("BFS_WG_FRONTIER", kWgFrontierDefault);
    return o;
}

// the device arrays of one BFS; a betweenness call keeps them over its sources
struct BfsBufs {
    DevBuf depth, parent, hist, front, next, bu_list, ctrl, acc;
    FrontierStore store;  // (betweenness parks its own long rows in store.longs between the searches)
    int64_t words = 0;
};

int bfs_alloc(const gmsx_graph *g, BfsBufs &b) {
    const int64_t n = g->n;
    b.words = (n + 31) / 32;
    if (int rc = b.store.alloc(n, g->nnz, false)) return rc;
    if (int rc = dalloc<int32_t>(b.depth, n)) return rc;
    if (int rc = dalloc<int32_t>(b.parent, n)) return rc;
    if (int rc = dalloc<int32_t>(b.hist, n)) return rc;
    if (int rc = dalloc<uint32_t>(b.front, b.words)) return rc;
    if (int rc = dalloc<uint32_t>(b.next, b.words)) return rc;
    if (int rc = dalloc<int32_t>(b.bu_list, n)) return rc;
    if (int rc = dalloc<BfsCtrl>(b.ctrl, 1)) return rc;
    if (int rc = dalloc<BfsAcc>(b.acc, 1)) return rc;
    return GMSX_OK;
}

// One BFS on the library's stream, n > 0 and 0 <= source < n: depth, parent and the level histogram stay on the device, *res is complete.
int bfs_run(const gmsx_graph *g, int32_t source, const BfsOptions &o, const BfsBufs &b, gmsx_bfs_info *res, int *launches) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const unsigned per_vertex = unsigned((n + 255) / 256);
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    const unsigned group_grid = unsigned(cus) * 8;
    int32_t *depth = b.depth.as<int32_t>(), *parent = b.parent.as<int32_t>(), *hist = b.hist.as<int32_t>();
    BfsCtrl *ctrl = b.ctrl.as<BfsCtrl>();
    BfsAcc *acc = b.acc.as<BfsAcc>();
    const FrontierBufs bufs = b.store.bufs();
    const BfsTopDown td{n, g->off, g->adj, depth, parent, ctrl, o.direction == 0 ? o.alpha : 0};
    uint32_t *front = b.front.as<uint32_t>(), *next = b.next.as<uint32_t>();

    int64_t row[2] = {0, 0};
    GMSX_HIP(hipMemcpyAsync(row, g->off + source, sizeof row, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(BfsCtrl), s));
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(BfsAcc), s));
    GMSX_HIP(hipMemsetAsync(&acc->maxdepth, 0xff, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_bfs_init, dim3(per_vertex), dim3(256), 0, s, n, source, depth, parent, hist, bufs.f[0]);
    ++*launches;
    GMSX_HIP(hipStreamSynchronize(s));
    if (row[0] < 0 || row[1] < row[0] || row[1] > g->nnz) return GMSX_ERR_KERNEL;

    BfsCtrl h;
    std::memset(&h, 0, sizeof h);
    h.count = 1;
    h.etc = g->nnz;
    long long scout = row[1] - row[0];
    int64_t level = 0, reached = 1;  // level: the depth of the current frontier
    int32_t bu_levels = 0;
    while (h.count > 0) {
        if (level >= n) return GMSX_ERR_KERNEL;
        if (o.direction == 2 || (o.direction == 0 && scout > h.etc / o.alpha)) {
            // ---- bottom-up levels
            GMSX_HIP(hipMemsetAsync(front, 0, size_t(b.words) * sizeof(uint32_t), s));
            hipLaunchKernelGGL(k_bfs_list_bits, dim3(unsigned((h.count + 255) / 256)), dim3(256), 0, s, bufs.f[h.cur], int64_t(h.count), front);
            ++*launches;
            int64_t awake = h.count, old_awake = 0;
            do {
                old_awake = awake;
                if (++level > n) return GMSX_ERR_KERNEL;
                GMSX_HIP(hipMemsetAsync(next, 0, size_t(b.words) * sizeof(uint32_t), s));
                GMSX_HIP(hipMemsetAsync(&ctrl->bu_list, 0, sizeof(int32_t), s));
                GMSX_HIP(hipMemsetAsync(&ctrl->awake, 0, 2 * sizeof(unsigned long long), s));
                hipLaunchKernelGGL(k_bfs_bottom_up, dim3(sweep), dim3(256), 0, s, n, g->off, g->adj, int32_t(level), int32_t(o.probe), front, next, depth,
                                   parent, b.bu_list.as<int32_t>(), ctrl);
                hipLaunchKernelGGL(k_bfs_bottom_up_rows<kGroup>, dim3(group_grid), dim3(256), 0, s, n, g->off, g->adj, int32_t(level), int32_t(o.probe),
                                   front, next, depth, parent, b.bu_list.as<const int32_t>(), ctrl);
                hipLaunchKernelGGL(k_bfs_bottom_up_rows<64>, dim3(group_grid), dim3(256), 0, s, n, g->off, g->adj, int32_t(level), int32_t(o.probe), front,
                                   next, depth, parent, b.bu_list.as<const int32_t>(), ctrl);
                *launches += 3;
                BfsCtrl hb;
                GMSX_HIP(hipMemcpyAsync(&hb, ctrl, sizeof hb, hipMemcpyDeviceToHost, s));
                GMSX_HIP(hipStreamSynchronize(s));
                if (hb.error || hb.bu_list < 0 || hb.bu_list > n || hb.awake > (unsigned long long)(n - reached)) return GMSX_ERR_KERNEL;
                awake = int64_t(hb.awake);
                reached += awake;
                if (awake > 0) ++bu_levels;
                std::swap(front, next);
            } while (awake > 0 && (o.direction == 2 || awake >= old_awake || awake > n / o.beta));
            if (awake == 0) break;
            // ---- the last level as a frontier list: top-down goes on with scout_count = 1
            h.count = 0;
            h.next = 0;
            h.round = int32_t(level);
            h.done = int32_t(reached - awake);
            h.error = h.nlong = h.bail = h.cur = h.stop = h.bu_list = 0;
            h.scout_acc = 0;
            GMSX_HIP(hipMemcpyAsync(ctrl, &h, sizeof h, hipMemcpyHostToDevice, s));
            frontier_collect(n, BfsAtDepth{depth, int32_t(level)}, bufs.f[0], &ctrl->count, &ctrl->error);
            ++*launches;
            GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            if (h.error || int64_t(h.count) != awake) return GMSX_ERR_KERNEL;
            scout = 1;
        } else {
            // ---- top-down levels: the engine's rounds, until the frontier empties or round_stop hands over
            h.etc -= scout;
            h.stop = 0;
            h.scout_acc = 0;
            h.round = int32_t(level);
            GMSX_HIP(hipMemcpyAsync(ctrl, &h, sizeof h, hipMemcpyHostToDevice, s));
            if (int rc = run_frontier_rounds(td, bufs, ctrl, h, o.wg_frontier, launches, [](const BfsCtrl &m) { return m.stop != 0; })) return rc;
            if (h.round < level) return GMSX_ERR_KERNEL;
            level = h.round;
            reached = int64_t(h.done) + h.count;
            scout = (long long)h.scout;
        }
    }
    // ---- the info
    hipLaunchKernelGGL(k_bfs_info, dim3(sweep), dim3(256), 0, s, n, g->off, depth, parent, hist, acc);
    hipLaunchKernelGGL(k_bfs_levels, dim3(sweep), dim3(256), 0, s, n, hist, acc);
    *launches += 2;
    BfsAcc a;
    GMSX_HIP(hipMemcpyAsync(&a, acc, sizeof a, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (a.error || a.reached != (unsigned long long)reached || a.hist_sum != a.reached || a.maxdepth < 0 || int64_t(a.maxdepth) >= n ||
        a.nonempty != (unsigned long long)(a.maxdepth + 1) || (a.best >> 32) < 1)
        return GMSX_ERR_KERNEL;
    std::memset(res, 0, sizeof *res);
    res->reached = int64_t(a.reached);
    res->reached_arcs = int64_t(a.arcs);
    res->depth_sum = int64_t(a.depth_sum);
    res->widest = int64_t(a.best >> 32);
    res->levels = a.maxdepth + 1;
    res->widest_level = int32_t(0xffffffffu - uint32_t(a.best));
    res->bottom_up_levels = bu_levels;
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_bfs(const gmsx_graph *g, int32_t source, int32_t *depth, int32_t *parent, gmsx_bfs_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        if (source < 0 || int64_t(source) >= n) return GMSX_ERR_INVALID;
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const BfsOptions o = bfs_options();
        BfsBufs b;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = bfs_alloc(g, b)) return rc;
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        gmsx_bfs_info res;
        int launches = 0;
        if (int rc = bfs_run(g, source, o, b, &res, &launches)) return rc;
        GMSX_HIP(hipEventRecord(c.ev[2], s));
        // the flag words were read as zero: the caller's arrays are written now, through host staging
        std::vector<int32_t> h_depth, h_parent;
        if (depth) {
            h_depth.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_depth.data(), b.depth.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (parent) {
            h_parent.resize(size_t(n));
            GMSX_HIP(hipMemcpyAsync(h_parent.data(), b.parent.p, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        GMSX_HIP(hipStreamSynchronize(s));
        float up_ms = 0.f, ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
        if (depth) std::memcpy(depth, h_depth.data(), size_t(n) * sizeof(int32_t));
        if (parent) std::memcpy(parent, h_parent.data(), size_t(n) * sizeof(int32_t));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), double(up_ms), uint64_t(res.reached_arcs), 0, uint64_t(res.levels), launches, 0, 0};
        return GMSX_OK;
    });
}

int gmsx_betweenness(const gmsx_graph *g, int64_t n_sources, const int32_t *sources, uint32_t flags, double *scores, gmsx_bc_info *info,
                     gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || n_sources < 0 || (n_sources > 0 && !sources)) return GMSX_ERR_INVALID;
        if (flags & ~uint32_t(GMSX_BC_EXCLUDE_SOURCE | GMSX_BC_NORMALIZE_MAX)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        const int64_t n = g->n;
        if (n > 0 && !scores) return GMSX_ERR_INVALID;
        for (int64_t i = 0; i < n_sources; ++i)
            if (sources[i] < 0 || int64_t(sources[i]) >= n) return GMSX_ERR_INVALID;
        gmsx_bc_info res;
        std::memset(&res, 0, sizeof res);
        res.sources = n_sources;
        if (n == 0 || n_sources == 0) {
            for (int64_t v = 0; v < n; ++v) scores[v] = 0.0;
            *info = res;
            if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
            return GMSX_OK;
        }
        Ctx &c = ctx();
        hipStream_t s = c.stream;
        const int cus = c.compute_units > 0 ? c.compute_units : 256;
        const BfsOptions o = bfs_options();
        const int64_t slot_cap = g->nnz / kBcChunk + frontier_long_cap(n, g->nnz);
        BfsBufs b;
        DevBuf d_sigma, d_delta, d_scores, d_order, d_loff, d_cursor, d_notes, d_slot_row, d_slots, d_bc;
        GMSX_HIP(hipEventRecord(c.ev[0], s));
        if (int rc = bfs_alloc(g, b)) return rc;
        if (int rc = dalloc<double>(d_sigma, n)) return rc;
        if (int rc = dalloc<double>(d_delta, n)) return rc;
        if (int rc = dalloc<double>(d_scores, n)) return rc;
        if (int rc = dalloc<int32_t>(d_order, n)) return rc;
        if (int rc = dalloc<int32_t>(d_loff, n + 1)) return rc;
        if (int rc = dalloc<int32_t>(d_cursor, n + 1)) return rc;
        if (int rc = dalloc<unsigned long long>(d_notes, b.store.long_cap)) return rc;
        if (int rc = dalloc<int32_t>(d_slot_row, slot_cap)) return rc;
        if (int rc = dalloc<double>(d_slots, slot_cap)) return rc;
        if (int rc = dalloc<BcCtrl>(d_bc, 1)) return rc;
        BcCtrl *bc = d_bc.as<BcCtrl>();
        GMSX_HIP(hipMemsetAsync(d_scores.p, 0, size_t(n) * sizeof(double), s));
        GMSX_HIP(hipMemsetAsync(bc, 0, sizeof(BcCtrl), s));
        GMSX_HIP(hipEventRecord(c.ev[1], s));
        BcArgs a{g->off, g->adj, b.depth.as<const int32_t>(), d_order.as<const int32_t>(), d_sigma.as<double>(), d_delta.as<double>(),
                 d_scores.as<double>(), b.store.longs.as<int32_t>(), d_notes.as<unsigned long long>(), d_slot_row.as<int32_t>(), d_slots.as<double>(), b.store.long_cap, slot_cap, bc, -1};
        const unsigned per_vertex = unsigned((n + 255) / 256);
        const unsigned long_grid = unsigned(cus) * 8;
        const unsigned sum_grid = unsigned((b.store.long_cap + 255) / 256);
        int launches = 0;
        uint64_t arcs = 0, levels_sum = 0;
        std::vector<int32_t> loff;
        // one level of either sweep: the short rows, the parked ones chunk by chunk, their slots
        auto level_pass = [&](bool delta, int32_t d) -> int {
            const int32_t lo = loff[size_t(d)], hi = loff[size_t(d) + 1];
            const unsigned rb = unsigned(std::min<int64_t>((int64_t(hi - lo) * kGroup + 255) / 256, int64_t(cus) * 32));
            GMSX_HIP(hipMemsetAsync(&bc->nlong, 0, sizeof(int32_t) + sizeof(unsigned long long), s));
            if (delta) {
                hipLaunchKernelGGL(k_bc_rows<true>, dim3(rb), dim3(256), 0, s, a, lo, hi, d);
                hipLaunchKernelGGL(k_bc_long<true>, dim3(long_grid), dim3(256), 0, s, a, d);
                hipLaunchKernelGGL(k_bc_long_sum<true>, dim3(sum_grid), dim3(256), 0, s, a);
            } else {
                hipLaunchKernelGGL(k_bc_rows<false>, dim3(rb), dim3(256), 0, s, a, lo, hi, d);
                hipLaunchKernelGGL(k_bc_long<false>, dim3(long_grid), dim3(256), 0, s, a, d);
                hipLaunchKernelGGL(k_bc_long_sum<false>, dim3(sum_grid), dim3(256), 0, s, a);
            }
            launches += 3;
            return GMSX_OK;
        };
        for (int64_t i = 0; i < n_sources; ++i) {
            const int32_t src = sources[i];
            gmsx_bfs_info bi;
            if (int rc = bfs_run(g, src, o, b, &bi, &launches)) return rc;
            res.reached_total += bi.reached;
            res.max_levels = std::max(res.max_levels, bi.levels);
            arcs += uint64_t(bi.reached_arcs);
            levels_sum += uint64_t(bi.levels);
            const int32_t levels = bi.levels;
            // the reached vertices sorted by depth
            hipLaunchKernelGGL(k_bc_scan, dim3(1), dim3(1024), 0, s, levels, b.hist.as<const int32_t>(), d_loff.as<int32_t>(), d_cursor.as<int32_t>());
            hipLaunchKernelGGL(k_bc_scatter, dim3(per_vertex), dim3(256), 0, s, n, levels, b.depth.as<const int32_t>(), d_loff.as<const int32_t>(),
                               d_cursor.as<int32_t>(), d_order.as<int32_t>(), bc);
            launches += 2;
            loff.assign(size_t(levels) + 1, 0);
            GMSX_HIP(hipMemcpyAsync(loff.data(), d_loff.p, loff.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipMemsetAsync(d_sigma.p, 0, size_t(n) * sizeof(double), s));
            GMSX_HIP(hipMemsetAsync(d_delta.p, 0, size_t(n) * sizeof(double), s));
            hipLaunchKernelGGL(k_bc_seed, dim3(1), dim3(1), 0, s, src, d_sigma.as<double>());
            ++launches;
            GMSX_HIP(hipStreamSynchronize(s));
            if (loff[0] != 0 || int64_t(loff[size_t(levels)]) != bi.reached) return GMSX_ERR_KERNEL;
            for (int32_t d = 0; d < levels; ++d)
                if (loff[size_t(d) + 1] <= loff[size_t(d)]) return GMSX_ERR_KERNEL;  // (every level below `levels` holds a vertex)
            a.skip = (flags & GMSX_BC_EXCLUDE_SOURCE) ? src : -1;
            for (int32_t d = 1; d < levels; ++d)
                if (int rc = level_pass(false, d)) return rc;
            for (int32_t d = levels - 2; d >= 0; --d)
                if (int rc = level_pass(true, d)) return rc;
            BcCtrl hb;
            GMSX_HIP(hipMemcpyAsync(&hb, bc, sizeof hb, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
            if (hb.error) return GMSX_ERR_KERNEL;
            double ms_bits;
            std::memcpy(&ms_bits, &hb.max_sigma, sizeof ms_bits);
            res.max_sigma = std::max(std::max(res.max_sigma, ms_bits), 1.0);  // (the source's own count)
        }
        GMSX_HIP(hipEventRecord(c.ev[2], s));
        std::vector<double> h_scores(size_t(n), 0.0);
        GMSX_HIP(hipMemcpyAsync(h_scores.data(), d_scores.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        double mx = 0.0;
        for (double x : h_scores) {
            if (!(x >= 0.0)) return GMSX_ERR_KERNEL;  // (every term is non-negative; a NaN is a fault of the kernels)
            mx = std::max(mx, x);
        }
        res.max_score = mx;
        if ((flags & GMSX_BC_NORMALIZE_MAX) && mx > 0.0)  // bc.cc:144-151; an all-zero result stays zeros
            for (double &x : h_scores) x /= mx;
        float up_ms = 0.f, ms = 0.f;
        GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
        GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
        std::memcpy(scores, h_scores.data(), size_t(n) * sizeof(double));
        *info = res;
        if (stats) *stats = gmsx_stats{double(ms), double(up_ms), arcs, 0, levels_sum, launches, 0, 0};
        return GMSX_OK;
    });
}

}  // extern "C"
