// Minimum (or maximum) spanning forest on gfx950 over the uploaded CSR and its attached weights: Borůvka's rounds on the device union-find.
//   gmsx_min_spanning_forest   the forest's edges ascending by (u, v), its arc mask, label[v] = smallest vertex id of v's tree, and the info
//                              block; no reference counterpart.  The definitions are those of include/gmsx.h.
//
// THE ORDER.  key(e) = (w, lo, hi) for e = {lo, hi}, lo < hi, compared lexicographically; GMSX_MSF_MAXIMUM puts the heavier edge first and
// still breaks ties by the smaller (lo, hi).  On the device the weight travels as k0 = w (minimum) or ~w (maximum), an unsigned word of which
// the smaller one always comes first; ~0 is no edge (weights lie in [1, 2^31 - 1]).  The CSR has no parallel edges and no self loops, so the
// order is strict and the forest is unique: Kruskal's output under the order, and the output of the rounds below.
// INSIDE ONE ROW the order needs two words only: for the arcs v - x of a fixed v, (min(v, x), max(v, x)) ascends with x — (x, v) for x < v, then
// (v, x) for x > v —, so the first crossing arc of v's row in the order is the minimum of k0 << 32 | x, one wave_min (wave_ops.hpp) per group.
//
// A ROUND is four steps with kernel boundaries between them; nothing spins and no workgroup waits for another.  comp = the parent array of
// union_find.hpp, flattened: comp[v] is the root of v's component, read with plain loads (an earlier kernel wrote it).
//   (a) search   MsfSearch, THE HOT PASS: every live vertex v finds the first arc j of its row in the order with comp[adj[j]] != comp[v]
//                (the weight is loaded for crossing arcs only).  It is the Op of row_classes.hpp's live-list row pass: a lane, a 16-lane
//                group, a wave or a workgroup per row by its length (the bounds are MSF_WAVE_ROW and MSF_WG_ROW) — no lane walks a long
//                row alone.  The result goes to best[v] and root[v], one writer each, and the writer folds k0 into the
//                component's word with an integer atomicMin (cw[root]; for the maximum that is the atomicMax of w).  A vertex that finds no
//                crossing arc is dead for good — components only merge.  Under MSF_PRUNE = 1 it is not appended to the next round's live list, so
//                that later rounds touch the shrinking border only; under MSF_PRUNE = 0, THE DEFAULT, the lists stay as classified and every
//                vertex is searched every round — on the four graphs measured the appends cost more than the arcs they save.
//   (b) minimum  k_msf_pair: the live vertices whose k0 equals their component's fold lo << 32 | hi into cpair[root], a 64-bit atomicMin.
//   (c) apply    k_msf_apply: the one vertex of a component whose (k0, lo, hi) is the component's is its WINNER (the chosen edge has one end
//                in the component).  It marks both arc bytes of the edge in the nnz-byte mask — its own arc and the twin found by
//                cc_find_in_row; two components that picked the same edge write the same bytes — calls cc_link(lo, hi) and counts the pick.
//                It compares against root[v], cw and cpair, which no thread of this kernel writes; parent is only walked, never compared.
//   (d) flatten  union_find.hpp's pointer jumping to the roots, so that comp is flat again.
// cw and cpair are one buffer set to ones before every round.  The host loop ends at a round without picks (under the option TIMING every
// round prints its live vertices, the arcs it examined and its winners).  Every component that has a
// crossing edge picks its first one, so the components after round r are a fact about (graph, weights, flags), and so is the number of
// rounds; every round at least doubles the smallest component that still grows: at most 64 rounds, else GMSX_ERR_KERNEL.
// WHY THE PICKS ARE A FOREST.  Under a strict order the first crossing edge of a component belongs to the unique forest (the cut property),
// and a cycle among one round's picks would need an edge that is not the first of the component that picked it.  Only (lo, hi) keeps unit
// weights acyclic.  The union-find does not depend on it: a link inside one component changes nothing.
//
// AFTER THE ROUNDS.  MsfCount: per row the marked `u < v` arcs (and, in the same pass, Σ w, min w, max w over them and the marked `u > v`
// arcs, which must be as many); a scan of the counts; MsfFill: every row compacts its marked arcs chunk by chunk with a ballot, in CSR
// order — the edge list ascends by (u, v) without a sort.  Both are Ops of row_classes.hpp's two-width pass.  k_cc_sizes and k_msf_info give
// trees, isolated and largest_tree.  The host checks edges == n - trees before anything is written.
// STATE: parent, root, sizes, the live lists (2 x their capacities, at most 4 n + 6 entries) as 32-bit words, best, cpair, the row counts and
// their scan as 64-bit words, cw, the nnz-byte mask, and up to 3 (n - 1) words of edges — O(n) words and a byte per arc, DevBufs of the call.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // load_now, wave_append, append_checked, RowGroup
#include "row_classes.hpp"
#include "union_find.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>

namespace gmsx {

namespace {

constexpr int kMsfMaxRounds = 64;
constexpr long long kMsfPruneDefault = 0;  // measured: the live lists cost more than they save on every graph tried
constexpr unsigned long long kNoArc = ~0ull;

// the call's small device block, mirrored to the host after every round
struct MsfCtrl {
    int32_t error;       // the flag word: a cap was exceeded, an append hit its bound, an arc has no twin
    int32_t again;       // flatten: a walk ended below its root (behind error: union_find.hpp's flatten reads the two words together)
    int32_t picks;       // winners of the round (an edge two components picked counts twice)
    int32_t pad;
    int32_t count[2][4];  // vertices in the lane / group / wave / workgroup list of either buffer (row_classes.hpp)
    unsigned long long examined;  // arcs the search pass looked at
};

// the info pass's words
struct MsfAcc {
    int32_t error, pad;
    unsigned long long upper, lower;  // marked arcs u -> v with u < v / with u > v
    unsigned long long weight;        // Σ w over the upper ones
    uint32_t wmin, wmax;
    unsigned long long trees, isolated, largest;
};

__global__ void k_msf_init(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ size) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) {
        parent[v] = int32_t(v);
        size[v] = 0;
    }
}

// (a) THE HOT PASS, the Op of a live-list row pass: WIDTH lanes (1, kGroup, 64, or the 256 threads of the workgroup) per live row.
// flip = 0 (minimum) or ~0 (maximum): k0 = w ^ flip.  next != nullptr: a vertex that found a crossing arc is appended to the next live list
// of its class (next_count, at most next_cap entries).
struct MsfSearch {
    const int64_t *off;
    const int32_t *adj, *wgt, *comp;
    int32_t *next, *next_count;
    int64_t next_cap;
    uint32_t flip;
    unsigned long long *best;
    int32_t *root;
    uint32_t *cw;
    int32_t *error;
    template <int WIDTH>
    __device__ __forceinline__ unsigned long long row(int32_t v, bool active, int lane) const {
        constexpr int kLanes = WIDTH > 64 ? 64 : WIDTH;  // lanes of one wave that share a row
        __shared__ unsigned long long s_min[4];
        unsigned long long examined = 0;
        const int32_t cv = active ? comp[v] : 0;
        const int64_t j1 = active ? off[v + 1] : 0;
        unsigned long long mine = kNoArc;
        for (int64_t j = active ? off[v] + lane : 0; j < j1; j += WIDTH) {
            ++examined;
            const int32_t x = adj[j];
            if (comp[x] != cv) mine = min(mine, ((unsigned long long)(uint32_t(wgt[j]) ^ flip) << 32) | uint32_t(x));
        }
        mine = wave_min<kLanes>(mine);
        if (WIDTH > 64) {
            if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = mine;
            __syncthreads();
            if (threadIdx.x == 0) mine = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
            __syncthreads();
        }
        const bool writer = active && lane == 0;  // the row's one writer
        const bool found = writer && mine != kNoArc;
        if (writer) {
            best[v] = mine;
            root[v] = cv;
        }
        if (found) {
            const uint32_t k0 = uint32_t(mine >> 32);
            if (k0 < load_now(&cw[cv])) atomicMin(&cw[cv], k0);  // (the word only falls: a stale read costs an atomic, never misses one)
        }
        if (next) {
            if (WIDTH > 64) {
                if (found) append_checked(next, next_count, next_cap, v, error);
            } else {
                wave_append(found, v, next, next_count, next_cap, error);
            }
        }
        return examined;
    }
};

// lo << 32 | hi of the arc v - x
__device__ __forceinline__ unsigned long long msf_pair(int32_t v, int32_t x) {
    return ((unsigned long long)uint32_t(min(v, x)) << 32) | uint32_t(max(v, x));
}

// (b) the live vertices whose weight word is their component's fold (lo, hi) into the component's pair
__global__ __launch_bounds__(256) void k_msf_pair(RowLists l, int cur, const unsigned long long *__restrict__ best, const int32_t *__restrict__ root,
                                                  const uint32_t *__restrict__ cw, unsigned long long *__restrict__ cpair,
                                                  const MsfCtrl *__restrict__ ctrl) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    for (int b = 0; b < 4; ++b) {
        const int32_t *list = l.list(cur, b);
        const int64_t rows = l.rows(ctrl->count[cur], b);
        for (int64_t i = tid; i < rows; i += stride) {
            const int32_t v = list[i];
            const unsigned long long mine = best[v];
            if (mine == kNoArc) continue;
            const int32_t r = root[v];
            if (uint32_t(mine >> 32) != cw[r]) continue;
            const unsigned long long pair = msf_pair(v, int32_t(uint32_t(mine)));
            if (pair < load_now(&cpair[r])) atomicMin(&cpair[r], pair);
        }
    }
}

// (c) the winner of every component marks both arcs of its edge, links its ends and counts the pick
__global__ __launch_bounds__(256) void k_msf_apply(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj, RowLists l, int cur,
                                                   const unsigned long long *__restrict__ best, const int32_t *__restrict__ root,
                                                   const uint32_t *__restrict__ cw, const unsigned long long *__restrict__ cpair,
                                                   int32_t *__restrict__ parent, uint8_t *__restrict__ mask, MsfCtrl *__restrict__ ctrl) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    const uint32_t cap = cc_walk_cap(n);
    int32_t picks = 0;
    for (int b = 0; b < 4; ++b) {
        const int32_t *list = l.list(cur, b);
        const int64_t rows = l.rows(ctrl->count[cur], b);
        for (int64_t i = tid; i < rows; i += stride) {
            const int32_t v = list[i];
            const unsigned long long mine = best[v];
            if (mine == kNoArc) continue;
            const int32_t r = root[v], x = int32_t(uint32_t(mine));
            if (uint32_t(mine >> 32) != cw[r] || msf_pair(v, x) != cpair[r]) continue;
            const int64_t own = cc_find_in_row(adj, off[v], off[v + 1], x), twin = cc_find_in_row(adj, off[x], off[x + 1], v);
            if (own < 0 || twin < 0) {
                ctrl->error = 1;
                continue;
            }
            mask[own] = 1;
            mask[twin] = 1;
            cc_link(parent, min(v, x), max(v, x), cap, &ctrl->error);
            ++picks;
        }
    }
    picks = wave_sum(picks);  // (at most n in all)
    if ((threadIdx.x & 63) == 0 && picks) atomicAdd(&ctrl->picks, picks);
}

// per row the marked `u < v` arcs into cnt[u] (one writer); Σ w, min w, max w over them and the marked `u > v` arcs into acc.  An Op of
// row_classes.hpp's two-width pass
struct MsfCount {
    const int32_t *adj, *wgt;
    const uint8_t *mask;
    int64_t *cnt;
    MsfAcc *acc;
    unsigned long long upper = 0, lower = 0, weight = 0;  // this thread's sums: begin() sets them
    uint32_t wmin = 0, wmax = 0;
    __device__ __forceinline__ void begin() { upper = lower = weight = 0; wmin = ~0u; wmax = 0; }
    template <int kLanes>
    __device__ __forceinline__ unsigned long long row(int32_t u, int64_t j0, int64_t j1, int lane, int width) {
        int64_t here = 0;
        unsigned long long low = lower;  // (over the row in a local: counted in the member, the loop keeps a second copy of it, 34 VGPRs for 32)
        for (int64_t j = j0 + lane; j < j1; j += width) {
            if (!mask[j]) continue;
            if (adj[j] > u) {
                const uint32_t w = uint32_t(wgt[j]);
                ++here;
                weight += w;
                wmin = min(wmin, w);
                wmax = max(wmax, w);
            } else {
                ++low;
            }
        }
        lower = low;
        upper += (unsigned long long)here;
        here = wave_sum<kLanes>(here);
        if (lane == 0) cnt[u] = here;
        return 0;
    }
    __device__ __forceinline__ void finish() {
        upper = wave_sum(upper);
        lower = wave_sum(lower);
        weight = wave_sum(weight);
        wmin = wave_min(wmin);
        wmax = wave_max(wmax);
        if ((threadIdx.x & 63) == 0 && (upper || lower)) {
            atomicAdd(&acc->upper, upper);
            atomicAdd(&acc->lower, lower);
            atomicAdd(&acc->weight, weight);
            atomicMin(&acc->wmin, wmin);
            atomicMax(&acc->wmax, wmax);
        }
    }
};

// the marked `u < v` arcs of row u to the positions pos[u], pos[u] + 1, … in CSR order: a ballot per chunk of the row.  An Op of the
// two-width pass (the row's lanes leave together)
struct MsfFill {
    const int32_t *adj, *wgt;
    const uint8_t *mask;
    const int64_t *pos;
    int64_t cap;
    int32_t *eu, *ev, *ew;
    MsfAcc *acc;
    __device__ __forceinline__ void begin() {}
    template <int kLanes>
    __device__ __forceinline__ unsigned long long row(int32_t u, int64_t j0, int64_t j1, int lane, int width) {
        const RowGroup<kLanes> grp;
        int64_t at = pos[u];
        const int64_t stop = pos[u + 1];
        if (at == stop) return 0;
        for (int64_t c = j0; c < j1; c += width) {
            const int64_t j = c + lane;
            const bool take = j < j1 && mask[j] && adj[j] > u;
            const unsigned long long hits = grp.ballot(take);
            if (take) {
                const int64_t p = at + __popcll(hits & ((1ull << lane) - 1ull));
                if (p < stop && p < cap) {
                    eu[p] = u;
                    ev[p] = adj[j];
                    ew[p] = wgt[j];
                } else {
                    acc->error = 1;
                }
            }
            at += __popcll(hits);
        }
        if (at != stop && lane == 0) acc->error = 1;
        return 0;
    }
    __device__ __forceinline__ void finish() {}
};

// per root: trees, isolated vertices (trees of one vertex), the largest tree.  A label that is no root raises the flag.
__global__ __launch_bounds__(256) void k_msf_info(int64_t n, const int32_t *__restrict__ label, const int32_t *__restrict__ size, MsfAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long trees = 0, isolated = 0, largest = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t l = label[v];
        if (l < 0 || l > v || label[l] != l) acc->error = 1;
        if (l != v) continue;
        const uint32_t s = uint32_t(size[v]);
        ++trees;
        isolated += s == 1;
        largest = max(largest, (unsigned long long)s);
    }
    trees = wave_sum(trees);
    isolated = wave_sum(isolated);
    largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0 && trees) {
        atomicAdd(&acc->trees, trees);
        if (isolated) atomicAdd(&acc->isolated, isolated);
        atomicMax(&acc->largest, largest);
    }
}

int msf(const gmsx_graph *g, uint32_t flags, int32_t *edge_u, int32_t *edge_v, int32_t *edge_w, uint8_t *arc_keep, int32_t *label, gmsx_msf_info *info,
        gmsx_stats *stats) {
    gmsx_msf_info res;
    std::memset(&res, 0, sizeof res);
    const int64_t n = g->n, nnz = g->nnz;
    if (n == 0 || nnz == 0) {  // every vertex is a tree of its own
        res.trees = res.isolated = n;
        res.largest_tree = n > 0 ? 1 : 0;
        for (int64_t v = 0; label && v < n; ++v) label[v] = int32_t(v);
        *info = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    // test hooks, first guesses
    const RowBounds bounds = row_bounds("MSF_WAVE_ROW", "MSF_WG_ROW");
    const bool prune = opt_int("MSF_PRUNE", kMsfPruneDefault) != 0;
    const bool timing = opt_on("TIMING");  // one line per round on stderr: its live vertices, the arcs it examined, its winners
    const uint32_t flip = (flags & GMSX_MSF_MAXIMUM) ? ~0u : 0u;
    const bool want_edges = edge_u != nullptr;
    RowListStore lists;
    // ---- setup: the buffers
    DevBuf d_parent, d_root, d_size, d_best, d_comp, d_mask, d_ctrl, d_acc, d_cnt, d_pos, d_eu, d_ev, d_ew;
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_parent, n)) return rc;
    if (int rc = dalloc<int32_t>(d_root, n)) return rc;
    if (int rc = dalloc<int32_t>(d_size, n)) return rc;
    if (int rc = lists.alloc(n, nnz, bounds, true, prune)) return rc;
    if (int rc = dalloc<unsigned long long>(d_best, n)) return rc;
    if (int rc = dalloc<uint32_t>(d_comp, 3 * n)) return rc;  // cpair: n 64-bit words, then cw: n 32-bit words
    if (int rc = dalloc<uint8_t>(d_mask, nnz)) return rc;
    if (int rc = dalloc<MsfCtrl>(d_ctrl, 1)) return rc;
    if (int rc = dalloc<MsfAcc>(d_acc, 1)) return rc;
    if (int rc = dalloc<int64_t>(d_cnt, n + 1)) return rc;
    if (want_edges) {
        if (int rc = dalloc<int64_t>(d_pos, n + 1)) return rc;
        if (int rc = dalloc<int32_t>(d_eu, n - 1)) return rc;
        if (int rc = dalloc<int32_t>(d_ev, n - 1)) return rc;
        if (int rc = dalloc<int32_t>(d_ew, n - 1)) return rc;
    }
    const RowLists &l = lists.l;
    MsfCtrl *ctrl = d_ctrl.as<MsfCtrl>();
    MsfAcc *acc = d_acc.as<MsfAcc>();
    int32_t *parent = d_parent.as<int32_t>();
    unsigned long long *cpair = d_comp.as<unsigned long long>();
    uint32_t *cw = d_comp.as<uint32_t>() + 2 * n;
    unsigned long long *best = d_best.as<unsigned long long>();
    int32_t *root = d_root.as<int32_t>();
    const int32_t *wgt = g->wgt.as<const int32_t>();
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(MsfCtrl), s));
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(MsfAcc), s));
    GMSX_HIP(hipMemsetAsync(&acc->wmin, 0xff, sizeof(uint32_t), s));
    GMSX_HIP(hipMemsetAsync(d_mask.p, 0, size_t(nnz), s));
    GMSX_HIP(hipMemsetAsync(d_cnt.p, 0, size_t(n + 1) * sizeof(int64_t), s));
    // ---- the rounds
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    int launches = 0;
    const unsigned per_vertex = unsigned((n + 255) / 256);
    const unsigned sweep = row_grid(n, 1, cus, 16);
    hipLaunchKernelGGL(k_msf_init, dim3(per_vertex), dim3(256), 0, s, n, parent, d_size.as<int32_t>());
    ++launches;
    classify_rows<true>(g, bounds, l, ctrl->count[0], &ctrl->error, cus, s, &launches);
    MsfCtrl h;
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (h.error) return GMSX_ERR_KERNEL;
    int cur = 0;
    int32_t rounds = 0;
    for (;;) {
        const int64_t live = live_count(h.count[cur], l);
        if (live < 0) return GMSX_ERR_KERNEL;
        if (live == 0) break;  // no vertex has a crossing arc left
        if (rounds >= kMsfMaxRounds) return GMSX_ERR_KERNEL;
        const int nxt = prune ? cur ^ 1 : cur;
        GMSX_HIP(hipMemsetAsync(d_comp.p, 0xff, size_t(n) * 12, s));
        GMSX_HIP(hipMemsetAsync(&ctrl->picks, 0, sizeof(int32_t), s));
        if (prune) GMSX_HIP(hipMemsetAsync(&ctrl->count[nxt][0], 0, 4 * sizeof(int32_t), s));
        // comp is the parent array, flat between the rounds; nxt == cur: no pruning
        auto search = [&](int b) {
            return MsfSearch{g->off, g->adj, wgt, parent, prune ? l.buf[nxt] + l.base[b] : nullptr, &ctrl->count[nxt][b], l.cap[b], flip,
                             best, root, cw, &ctrl->error};
        };
        launch_live_rows(search, l, cur, ctrl->count[cur], h.count[cur], &ctrl->examined, cus, s, &launches);
        const unsigned over_live = unsigned(std::max<int64_t>(1, std::min<int64_t>((live + 255) / 256, int64_t(cus) * 16)));
        hipLaunchKernelGGL(k_msf_pair, dim3(over_live), dim3(256), 0, s, l, cur, best, root, cw, cpair, ctrl);
        hipLaunchKernelGGL(k_msf_apply, dim3(over_live), dim3(256), 0, s, n, g->off, g->adj, l, cur, best, root, cw, cpair, parent,
                           d_mask.as<uint8_t>(), ctrl);
        launches += 2;
        const unsigned long long examined_was = h.examined;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.error || h.picks < 0) return GMSX_ERR_KERNEL;
        if (timing)
            std::fprintf(stderr, "[gmsx msf] round %d: %lld live vertices, %llu arcs examined, %d winners\n", int(rounds) + 1, (long long)live,
                         h.examined - examined_was, int(h.picks));
        if (h.picks == 0) break;
        ++rounds;
        if (int rc = flatten(n, parent, &ctrl->error, cus, s, &launches, nullptr)) return rc;
        cur = nxt;
    }
    // ---- the edge list and the info reduction
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    launch_rows_two_width(MsfCount{g->adj, wgt, d_mask.as<const uint8_t>(), d_cnt.as<int64_t>(), acc}, g, nullptr, cus, s, &launches);
    hipLaunchKernelGGL(k_cc_sizes, dim3(sweep), dim3(256), 0, s, n, parent, d_size.as<int32_t>());
    hipLaunchKernelGGL(k_msf_info, dim3(sweep), dim3(256), 0, s, n, parent, d_size.as<const int32_t>(), acc);
    launches += 2;
    if (want_edges) {
        if (int rc = exclusive_scan_i64(d_cnt.as<const int64_t>(), d_pos.as<int64_t>(), n + 1, s)) return rc;
        ++launches;
        launch_rows_two_width(MsfFill{g->adj, wgt, d_mask.as<const uint8_t>(), d_pos.as<const int64_t>(), n - 1, d_eu.as<int32_t>(), d_ev.as<int32_t>(),
                                      d_ew.as<int32_t>(), acc},
                              g, nullptr, cus, s, &launches);
    }
    MsfAcc a;
    GMSX_HIP(hipMemcpyAsync(&a, acc, sizeof a, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (a.error || a.trees < 1 || a.trees > (unsigned long long)n || a.upper != a.lower || a.upper != (unsigned long long)n - a.trees ||
        a.largest < 1 || (a.upper > 0) != (rounds > 0))
        return GMSX_ERR_KERNEL;
    res.edges = int64_t(a.upper);
    res.total_weight = int64_t(a.weight);
    res.trees = int64_t(a.trees);
    res.isolated = int64_t(a.isolated);
    res.largest_tree = int64_t(a.largest);
    res.min_weight = a.upper ? int32_t(a.wmin) : 0;
    res.max_weight = a.upper ? int32_t(a.wmax) : 0;
    res.rounds = rounds;
    // the flag words were read as zero: the caller's arrays are written now, through host staging
    const size_t ne = size_t(res.edges);
    HostStage out;
    if (int rc = out.fetch(label, parent, size_t(n) * sizeof(int32_t), s)) return rc;
    if (int rc = out.fetch(arc_keep, d_mask.p, size_t(nnz), s)) return rc;
    if (int rc = out.fetch_edges(edge_u, edge_v, edge_w, d_eu, d_ev, d_ew, ne, s)) return rc;
    GMSX_HIP(hipStreamSynchronize(s));
    float up_ms = 0.f, ms = 0.f, info_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&info_ms, c.ev[2], c.ev[3]));
    out.deliver();
    *info = res;
    if (stats) *stats = gmsx_stats{double(ms), double(up_ms) + double(info_ms), uint64_t(res.edges), uint64_t(h.examined), uint64_t(rounds), launches, 0, 0};
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_min_spanning_forest(const gmsx_graph *g, uint32_t flags, int32_t *edge_u, int32_t *edge_v, int32_t *edge_w, uint8_t *arc_keep, int32_t *label,
                             gmsx_msf_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        const int given = (edge_u ? 1 : 0) + (edge_v ? 1 : 0) + (edge_w ? 1 : 0);
        if (!g || !info || (flags & ~uint32_t(GMSX_MSF_MAXIMUM)) || (given != 0 && given != 3)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        if (!g->wgt.p) return GMSX_ERR_INVALID;
        return msf(g, flags, edge_u, edge_v, edge_w, arc_keep, label, info, stats);
    });
}

}  // extern "C"
