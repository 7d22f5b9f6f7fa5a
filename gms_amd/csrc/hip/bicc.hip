// Biconnected components, articulation points and bridges on gfx950: Tarjan–Vishkin on a BFS forest of the uploaded CSR.
//   gmsx_biconnected_components   block[j] = the id of the block of arc j, blocks_at[v] = the blocks that contain v (>= 2: a cut vertex),
//                                 arc_keep[j] = 0 for a bridge, and the info block; no reference counterpart.  The definitions are those of
//                                 include/gmsx.h.
//
// EVERY OUTPUT IS A FACT ABOUT THE GRAPH.  The forest below is whatever the claims of one run made it (a vertex's parent is the neighbour
// whose atomicCAS on its depth came first), and so are the preorder numbers, low, high and the auxiliary sets' representatives — but the
// PARTITION of the edges that the auxiliary sets describe is the blocks for every spanning forest (Tarjan, Vishkin 1985), ids are ranks of each
// block's smallest `u < v` arc, and blocks_at, the bridges and every word of the info block are functions of the partition.  The roots are
// fixed (every component's smallest id) and BFS depth is unique, so `levels` is a fact too.  All state is integers.
//
// THE STEPS (a kernel boundary between any two; nothing spins and no workgroup waits for another):
//   1 roots     label[v] by union_find.hpp over the arcs v -> w, w < v (OpLink in the row pass), flatten; label[v] == v: a root.
//   2 forest    BiccForest on the frontier-rounds engine: the first frontier holds every root at depth 0; a neighbour is claimed by atomicCAS
//               on depth, and the claimer becomes its parent, hands it its rank among its children (an atomicAdd on the child count) and
//               appends it to `order`.  Round d only claims vertices of depth d + 1, so ORDER IS SORTED BY DEPTH as it is appended: no
//               counting sort follows (traversal.hip's k_bc_scan / k_bc_scatter are not needed and stay where they are).  round_stop, ONE
//               thread at every round boundary, notes where the next level starts: loff[d] .. loff[d + 1] is level d of order.
//   3 nd        nd[v] = vertices of v's subtree: bottom-up by level, atomicAdd into the parent.
//   4 preorder  the children counts are scanned (cbase); vertex v takes slot R + cbase[parent] + rank (a root: its place among the R roots) in
//               a layout in which siblings are neighbours; one scan over nd in that layout gives rel[v] = 1 + the nd of v's earlier siblings
//               (a root: the nd of the earlier roots); top-down by level pre[v] = pre[parent] + rel[v].  Every subtree is [pre, pre + nd).
//   5 low, high start at pre[v]; the row pass (OpLowHigh) folds pre[w] over the non-tree neighbours w of v (w != parent[v], parent[w] != v)
//               with the row minimum / maximum of wave_ops.hpp; bottom-up by level atomicMin / atomicMax into the parent.
//   6 unions    a second union-find over the tree edges, each named by its child (OpAux): (i) a non-tree arc v -> w with pre[v] + nd[v] <=
//               pre[w] links v and w; (ii) a tree arc v -> w links v and w iff low[w] < pre[v] or high[w] >= pre[v] + nd[v] (never true for
//               a root v).  Flatten.  The block of arc {v, w} is the set of its end with the larger pre.
//   7 ids       OpFirst: first[set] = the smallest `u < v` arc index of the set (64-bit atomicMin behind a read of the word, which only
//               falls) and edges[set] (a lane adds a run of arcs of one set with one atomic: a giant block costs a few adds per lane).  Per
//               row the arcs that are their set's first are counted (BiccRank<false>), the counts scanned, and BiccRank<true> gives
//               every set the rank of its first arc: ids ascend with each block's smallest edge in CSR order.  k_cc_sizes counts the tree
//               edges of a set; its vertices are that + 1 (the tree edges of a block are a subtree), and a set of one tree edge is a bridge.
//   8 blocks_at a child c is AT THE TOP of its block iff its parent is a root or the parent's own tree edge lies in another set; top[set] =
//               the smallest such child; blocks_at[v] = [v has a parent] + the sets whose top's parent is v.
//   9 info      one reduction over the vertices, then the largest block's id and vertices among the sets with the most edges.
//  10 outputs   only when asked for: OpOut writes block[j] and arc_keep[j] for every arc (4 + 1 bytes per arc, device memory of the call).
// THE ROW PASSES are row_classes.hpp's (a lane, a 16-lane group, a wave or a workgroup per row by its length; the bounds are BCC_WAVE_ROW and
// BCC_WG_ROW); the five Ops below say what an arc means in each.  BiccRank needs a row's CSR order and is an Op of its two-width pass.
// THE SWEEPS BY LEVEL (steps 3, 4, 5; k_bicc_sweep<Op>) do not cost a launch per level on a deep forest: consecutive levels that each hold at
// most BCC_WG_LEVEL vertices are swept by ONE workgroup in one launch with a __syncthreads() between levels; what one level writes and the next
// reads goes through atomics, store_now and load_now (frontier_rounds.hpp; the note at the top of union_find.hpp).  A larger level is a grid-wide
// launch of its own.  The host plans the launches from loff.
// SELF-CHECKS before anything is written: order holds n vertices, Σ nd over the roots = n, Σ edges over the sets = nnz / 2 = the `u > v`
// arcs, Σ blocks_at = n - components + blocks.  Any miss is GMSX_ERR_KERNEL.
// STATE: seventeen 32-bit and four 64-bit words per vertex (the ids' words reuse the preorder's), the row lists and the engine's two
// frontiers: DevBufs of the call; the handle is not touched.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // the engine, load_now, store_now, RowGroup, kGroup
#include "row_classes.hpp"
#include "union_find.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

constexpr int kBiccSweepThreads = 1024;
constexpr long long kBiccWgLevelDefault = 1024;  // a first guess (gmsx.h, OPTIONS)

// control block of the forest's rounds: the engine's, plus the level order's words
struct BiccCtrl : FrontierCtrl {
    int32_t placed;  // vertices appended to order so far
    int32_t seen;    // level starts noted in loff so far
};

// the call's small device block, zeroed per call
struct BiccAcc {
    int32_t error;     // the flag word: a cap was exceeded, an append hit its bound, a self-check of a kernel failed
    int32_t again;     // flatten: a walk ended below its root (behind error: union_find.hpp's flatten reads the two words together)
    int32_t count[4];  // vertices in the group / wave / workgroup list: words 1 .. 3 (row_classes.hpp)
    int32_t max_at;    // largest blocks_at
    int32_t pad;
    unsigned long long examined;      // arcs the arc passes looked at
    unsigned long long upper, lower;  // arcs u -> v with u < v / with u > v
    unsigned long long comps, isolated, nd_roots;
    unsigned long long blocks, bridges, artic, sum_at, sum_edges;
    unsigned long long best_edges;  // edges of the largest block
    unsigned long long best;        // id << 32 | vertices of the block of the smallest id among those
};

// every per-vertex word of the call
struct BiccArrays {
    int32_t *label, *depth, *parent, *rank, *order, *loff, *nd, *slot, *rel, *pre, *low, *high, *aux, *size, *id, *at, *top;
    unsigned long long *kids;  // children per vertex (n + 1 words: scanned as int64)
    int64_t *cbase, *val, *pfx;
    unsigned long long *first, *edges;  // (val's and pfx's words again, behind the preorder)
    int64_t *cnt, *pos;                 // (kids' and cbase's words again, behind the preorder)
};

__global__ __launch_bounds__(256) void k_bicc_init(int64_t n, BiccArrays a) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v > n) return;
    a.kids[v] = 0;
    a.val[v] = 0;
    if (v == n) return;
    a.label[v] = int32_t(v);
    a.aux[v] = int32_t(v);
    a.nd[v] = 1;
    a.size[v] = 0;
    a.at[v] = 0;
    a.id[v] = -1;
    a.top[v] = INT_MAX;
}

// step 1: every edge is linked from its end of the larger id
struct OpLink {
    const int32_t *adj;
    int32_t *parent;
    uint32_t cap;
    int32_t *error;
    template <int>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        unsigned long long seen = 0;
        for (int64_t j = j0 + lane; j < j1; j += width, ++seen) {
            const int32_t w = adj[j];
            if (w < v) cc_link(parent, v, w, cap, error);
        }
        return seen;
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void finish() {}
};

// step 5: pre[w] over the non-tree neighbours of v into low[v] and high[v] (which start at pre[v]); the first lane of every wave's share of
// the row folds its minimum and maximum in
struct OpLowHigh {
    const int32_t *adj, *parent, *pre;
    int32_t *low, *high;
    template <int kLanes>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        const int32_t pv = parent[v];
        int32_t lo = INT_MAX, hi = -1;
        unsigned long long seen = 0;
        for (int64_t j = j0 + lane; j < j1; j += width, ++seen) {
            const int32_t w = adj[j];
            if (w == pv || parent[w] == v) continue;
            const int32_t pw = pre[w];
            lo = min(lo, pw);
            hi = max(hi, pw);
        }
        lo = wave_min<kLanes>(lo);
        hi = wave_max<kLanes>(hi);
        if ((lane & (kLanes - 1)) == 0) {  // (the words only fall / rise: a stale read costs an atomic, never misses one)
            if (lo < load_now(&low[v])) atomicMin(&low[v], lo);
            if (hi > load_now(&high[v])) atomicMax(&high[v], hi);
        }
        return seen;
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void finish() {}
};

// step 6: the two rules of the auxiliary graph
struct OpAux {
    const int32_t *adj, *parent, *pre, *nd, *low, *high;
    int32_t *aux;
    uint32_t cap;
    int32_t *error;
    template <int>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        const int32_t pv = parent[v], first = pre[v], end = first + nd[v];
        unsigned long long seen = 0;
        for (int64_t j = j0 + lane; j < j1; j += width, ++seen) {
            const int32_t w = adj[j];
            if (parent[w] == v) {  // (ii) a tree arc to the child w (a root is its own parent, and no row holds its own vertex)
                if (low[w] < first || high[w] >= end) cc_link(aux, v, w, cap, error);
            } else if (w != pv) {  // (i) a non-tree arc to a later, unrelated subtree
                if (end <= pre[w]) cc_link(aux, v, w, cap, error);
            }
        }
        return seen;
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void finish() {}
};

// the set of arc {v, w}: that of its end with the larger pre
__device__ __forceinline__ int32_t bicc_set(const int32_t *__restrict__ aux, const int32_t *__restrict__ pre, int32_t v, int32_t pre_v, int32_t w) {
    return aux[pre_v > pre[w] ? v : w];
}

// step 7: first[set] and edges[set] over the `u < v` arcs; a lane keeps the run of its current set and adds it when the set changes
struct OpFirst {
    const int32_t *adj, *pre, *aux;
    unsigned long long *first, *edges;
    BiccAcc *acc;
    int32_t run_set;
    unsigned long long run, upper, lower;
    __device__ __forceinline__ void flush() {
        if (run) atomicAdd(&edges[run_set], run);
        run = 0;
    }
    template <int>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        const int32_t pv = pre[v];
        unsigned long long seen = 0;
        for (int64_t j = j0 + lane; j < j1; j += width, ++seen) {
            const int32_t w = adj[j];
            if (w < v) {
                ++lower;
                continue;
            }
            ++upper;
            const int32_t s = bicc_set(aux, pre, v, pv, w);
            if ((unsigned long long)j < load_now(&first[s])) atomicMin(&first[s], (unsigned long long)j);
            if (s != run_set) {
                flush();
                run_set = s;
            }
            ++run;
        }
        return seen;
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void finish() {
        flush();
        upper = wave_sum(upper);
        lower = wave_sum(lower);
        if ((threadIdx.x & 63) == 0 && (upper || lower)) {
            atomicAdd(&acc->upper, upper);
            atomicAdd(&acc->lower, lower);
        }
    }
};

// step 10: the caller's per-arc arrays
struct OpOut {
    const int32_t *adj, *pre, *aux, *id, *size;
    int32_t *block;
    uint8_t *keep;
    template <int>
    __device__ __forceinline__ unsigned long long row(int32_t v, int64_t j0, int64_t j1, int lane, int width) {
        const int32_t pv = pre[v];
        unsigned long long seen = 0;
        for (int64_t j = j0 + lane; j < j1; j += width, ++seen) {
            const int32_t s = bicc_set(aux, pre, v, pv, adj[j]);
            if (block) block[j] = id[s];
            if (keep) keep[j] = size[s] > 1 ? 1 : 0;
        }
        return seen;
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void finish() {}
};

// step 2: one level of the forest as a policy of the engine
struct BiccForest {
    static constexpr int kGroupWords = 0;
    static constexpr bool kNotes = false;
    static constexpr bool kStops = true;
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    int32_t *depth, *parent, *rank, *order, *loff;
    unsigned long long *kids;
    BiccCtrl *ctrl;

    __device__ __forceinline__ void visit(int32_t x, int32_t w, int32_t nd, const NextQueue &q) const {
        if (load_now(&depth[w]) != -1 || atomicCAS(&depth[w], -1, nd) != -1) return;
        parent[w] = x;  // (one writer: the claimer; read behind a kernel boundary)
        rank[w] = int32_t(atomicAdd(&kids[x], 1ull));
        const int64_t pos = int64_t(atomicAdd(&ctrl->placed, 1));
        if (pos < n) order[pos] = w;
        else *q.error = 1;
        q.push(w);
    }
    __device__ __forceinline__ void short_row(int32_t x, int64_t j0, int64_t j1, int lane, int32_t round, uint32_t *, const NextQueue &q) const {
        for (int64_t j = j0 + lane; j < j1; j += kGroup) visit(x, adj[j], round + 1, q);
    }
    __device__ __forceinline__ void park(int32_t, int32_t, unsigned long long *, int64_t, int32_t *) const {}
    __device__ __forceinline__ void long_walk(int32_t x, unsigned long long, int64_t tid, int64_t threads, const NextQueue &q) const {
        const int32_t nd = load_now(&depth[x]) + 1;
        const int64_t j1 = off[x + 1];
        for (int64_t j = off[x] + tid; j < j1; j += threads) visit(x, adj[j], nd, q);
    }
    __device__ __forceinline__ void finish() const {}
    // ONE thread, at a round boundary, behind every append of the round: the next level starts where order stands
    __device__ __forceinline__ bool round_stop() const {
        const int32_t l = ++ctrl->seen;
        if (int64_t(l) <= n + 1) loff[l] = atomicAdd(&ctrl->placed, 0);
        else ctrl->error = 1;
        return false;
    }
};

struct BiccIsRoot {
    const int32_t *label;
    __device__ __forceinline__ bool operator()(int64_t v) const { return label[v] == int32_t(v); }
};

__global__ __launch_bounds__(256) void k_bicc_forest_init(int64_t n, const int32_t *__restrict__ label, int32_t *__restrict__ depth,
                                                          int32_t *__restrict__ parent) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    depth[v] = label[v] == int32_t(v) ? 0 : -1;
    parent[v] = int32_t(v);
}

// A SWEEP BY LEVEL: the levels d0, d0 ± 1, …, d1 of order, op(v) for every vertex of a level, a __syncthreads() between two levels.  More
// than one level: ONE workgroup (the host's plan); one level: any grid.
template <class Op>
__global__ __launch_bounds__(kBiccSweepThreads) void k_bicc_sweep(Op op, int64_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ loff,
                                                                  int32_t d0, int32_t d1) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    const int32_t dir = d1 >= d0 ? 1 : -1;
    for (int32_t d = d0;; d += dir) {  // (at most n levels)
        const int64_t hi = min(int64_t(loff[d + 1]), n);
        for (int64_t i = int64_t(loff[d]) + tid; i < hi; i += stride) op(order[i]);
        if (d == d1) break;
        __syncthreads();
    }
}

// step 3, bottom-up: a finished subtree is added to its parent's
struct SweepNd {
    const int32_t *parent;
    int32_t *nd;
    __device__ __forceinline__ void operator()(int32_t v) const {
        const int32_t p = parent[v];
        if (p != v) atomicAdd(&nd[p], load_now(&nd[v]));
    }
};
// step 4, top-down; low and high start at pre
struct SweepPre {
    const int32_t *parent, *rel;
    int32_t *pre, *low, *high;
    __device__ __forceinline__ void operator()(int32_t v) const {
        const int32_t p = parent[v];
        const int32_t mine = (p != v ? load_now(&pre[p]) : 0) + rel[v];
        store_now(&pre[v], mine);
        low[v] = mine;
        high[v] = mine;
    }
};
// step 5, bottom-up
struct SweepLowHigh {
    const int32_t *parent;
    int32_t *low, *high;
    __device__ __forceinline__ void operator()(int32_t v) const {
        const int32_t p = parent[v];
        if (p == v) return;
        atomicMin(&low[p], load_now(&low[v]));
        atomicMax(&high[p], load_now(&high[v]));
    }
};

// step 4: nd in the layout in which siblings are neighbours (the roots first, in the order of `order`)
__global__ __launch_bounds__(256) void k_bicc_layout(int64_t n, int64_t roots, BiccArrays a, BiccAcc *__restrict__ acc) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = a.order[i];
    const int32_t p = a.parent[v];
    if ((i < roots) != (p == v)) {
        acc->error = 1;
        return;
    }
    const int64_t slot = i < roots ? i : roots + a.cbase[p] + a.rank[v];
    if (slot < 0 || slot >= n) {
        acc->error = 1;
        return;
    }
    a.val[slot] = a.nd[v];
    a.slot[v] = int32_t(slot);
}
// … and rel[v] from its scan: the nd of v's earlier siblings + 1; for a root the nd of the earlier roots
__global__ __launch_bounds__(256) void k_bicc_rel(int64_t n, int64_t roots, BiccArrays a, BiccAcc *__restrict__ acc) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v >= n) return;
    a.rel[v] = 0;
    if (acc->error) return;  // (a vertex without its slot)
    const int32_t p = a.parent[v];
    const int64_t slot = a.slot[v], base = p == int32_t(v) ? 0 : roots + a.cbase[p];  // (where v's siblings start)
    if (slot < 0 || slot >= n || base < 0 || base > slot) {
        acc->error = 1;
        return;
    }
    const int64_t mine = a.pfx[slot];
    a.rel[v] = int32_t(p == int32_t(v) ? mine : 1 + mine - a.pfx[base]);
}

// first, edges, the row counts: all ones / zeros behind the preorder (the words of val, pfx, kids)
__global__ __launch_bounds__(256) void k_bicc_ids_init(int64_t n, BiccArrays a) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v > n) return;
    a.first[v] = ~0ull;
    a.edges[v] = 0;
    a.cnt[v] = 0;
}

// step 7: the `u < v` arcs of row u that are their set's first: counted into cnt[u] (one writer), or ranked from pos[u] on.  An Op of
// row_classes.hpp's two-width pass; a ballot per chunk keeps the CSR order (the row's lanes leave together).
template <bool kAssign>
struct BiccRank {
    const int32_t *adj;
    BiccArrays a;
    int64_t n;
    BiccAcc *acc;
    __device__ __forceinline__ void begin() {}
    template <int kLanes>
    __device__ __forceinline__ unsigned long long row(int32_t u, int64_t j0, int64_t j1, int lane, int width) {
        const RowGroup<kLanes> grp;
        if (j1 == j0) return 0;
        int64_t at = kAssign ? a.pos[u] : 0;
        if (kAssign && at == a.pos[u + 1]) return 0;
        unsigned long long examined = 0;
        const int32_t pu = a.pre[u];
        for (int64_t c = j0; c < j1; c += width) {
            const int64_t j = c + lane;
            bool take = false;
            int32_t s = 0;
            if (j < j1) {
                ++examined;
                const int32_t w = adj[j];
                if (w > u) {
                    s = bicc_set(a.aux, a.pre, u, pu, w);
                    take = a.first[s] == (unsigned long long)j;
                }
            }
            const unsigned long long hits = grp.ballot(take);
            if (kAssign && take) {
                const int64_t r = at + __popcll(hits & ((1ull << lane) - 1ull));
                if (r < n) a.id[s] = int32_t(r);
                else acc->error = 1;
            }
            at += __popcll(hits);
        }
        if (!kAssign && lane == 0) a.cnt[u] = at;
        return examined;
    }
    __device__ __forceinline__ void finish() {}
};

// step 8: top[set] = the smallest child at the top of its block …
__global__ __launch_bounds__(256) void k_bicc_top(int64_t n, BiccArrays a) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t p = a.parent[v];
        if (p == int32_t(v)) continue;
        const int32_t s = a.aux[v];
        if (a.parent[p] == p || a.aux[p] != s) atomicMin(&a.top[s], int32_t(v));
    }
}
// … and blocks_at: a vertex's own tree edge, and one per set whose top hangs under it
__global__ __launch_bounds__(256) void k_bicc_at(int64_t n, BiccArrays a, BiccAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        if (a.parent[v] == int32_t(v)) continue;
        atomicAdd(&a.at[v], 1);
        if (a.aux[v] != int32_t(v)) continue;
        const int32_t t = a.top[v];
        if (t < 0 || int64_t(t) >= n || a.aux[t] != int32_t(v)) {
            acc->error = 1;
            continue;
        }
        atomicAdd(&a.at[a.parent[t]], 1);
    }
}

// step 9: per vertex; a set is named by the non-root vertex v with aux[v] == v
__global__ __launch_bounds__(256) void k_bicc_info(int64_t n, const int64_t *__restrict__ off, BiccArrays a, BiccAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long comps = 0, isolated = 0, nd_roots = 0, blocks = 0, bridges = 0, artic = 0, sum_at = 0, sum_edges = 0, best = 0;
    int32_t max_at = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t at = a.at[v];
        sum_at += (unsigned long long)at;
        artic += at >= 2;
        max_at = max(max_at, at);
        if (a.parent[v] == int32_t(v)) {
            ++comps;
            isolated += off[v + 1] == off[v];
            nd_roots += (unsigned long long)a.nd[v];
            if (a.aux[v] != int32_t(v) || (at > 0) != (a.nd[v] > 1)) acc->error = 1;  // (a root is in no set, and tops a block iff it has a child)
        } else if (a.aux[v] == int32_t(v)) {
            const unsigned long long e = a.edges[v], t = (unsigned long long)a.size[v];
            if (e < t || t < 1 || a.id[v] < 0) acc->error = 1;
            ++blocks;
            bridges += t == 1;
            sum_edges += e;
            best = max(best, e);
        }
    }
    comps = wave_sum(comps);
    isolated = wave_sum(isolated);
    nd_roots = wave_sum(nd_roots);
    blocks = wave_sum(blocks);
    bridges = wave_sum(bridges);
    artic = wave_sum(artic);
    sum_at = wave_sum(sum_at);
    sum_edges = wave_sum(sum_edges);
    best = wave_max(best);
    max_at = wave_max(max_at);
    if ((threadIdx.x & 63) == 0) {
        if (comps) atomicAdd(&acc->comps, comps);
        if (isolated) atomicAdd(&acc->isolated, isolated);
        if (nd_roots) atomicAdd(&acc->nd_roots, nd_roots);
        if (blocks) atomicAdd(&acc->blocks, blocks);
        if (bridges) atomicAdd(&acc->bridges, bridges);
        if (artic) atomicAdd(&acc->artic, artic);
        if (sum_at) atomicAdd(&acc->sum_at, sum_at);
        if (sum_edges) atomicAdd(&acc->sum_edges, sum_edges);
        if (best) atomicMax(&acc->best_edges, best);
        if (max_at) atomicMax(&acc->max_at, max_at);
    }
}
// … and among the sets with the most edges the one of the smallest id, with its vertices (tree edges + 1)
__global__ __launch_bounds__(256) void k_bicc_largest(int64_t n, BiccArrays a, BiccAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const unsigned long long most = acc->best_edges;
    unsigned long long best = ~0ull;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride)
        if (a.parent[v] != int32_t(v) && a.aux[v] == int32_t(v) && a.edges[v] == most)
            best = min(best, ((unsigned long long)uint32_t(a.id[v]) << 32) | uint32_t(a.size[v] + 1));
    best = wave_min(best);
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(&acc->best, best);
}

// one sweep over the levels from .. to (either direction) of the host's copy of loff: runs of levels of at most wg_level vertices each go to
// one workgroup in one launch, every other level to a grid of its own
template <class Op>
void bicc_sweep(const Op &op, int64_t n, const std::vector<int32_t> &loff, int32_t from, int32_t to, int64_t wg_level, const int32_t *order,
                const int32_t *d_loff, hipStream_t s, int *launches) {
    const int32_t dir = to >= from ? 1 : -1;
    auto size = [&](int32_t d) { return int64_t(loff[size_t(d) + 1]) - loff[size_t(d)]; };
    for (int32_t d = from; d != to + dir;) {
        int32_t e = d;
        unsigned grid = 1;
        if (size(d) <= wg_level) {
            while (e != to && size(e + dir) <= wg_level) e += dir;
        } else {
            grid = unsigned((size(d) + kBiccSweepThreads - 1) / kBiccSweepThreads);
        }
        hipLaunchKernelGGL(k_bicc_sweep<Op>, dim3(grid), dim3(kBiccSweepThreads), 0, s, op, n, order, d_loff, d, e);
        ++*launches;
        d = e + dir;
    }
}

int bicc(const gmsx_graph *g, int32_t *block, int32_t *blocks_at, uint8_t *arc_keep, gmsx_bicc_info *info, gmsx_stats *stats) {
    gmsx_bicc_info res;
    std::memset(&res, 0, sizeof res);
    const int64_t n = g->n, nnz = g->nnz;
    if (n == 0 || nnz == 0) {  // every vertex is a component of its own, in no block
        res.components = res.isolated = n;
        for (int64_t v = 0; blocks_at && v < n; ++v) blocks_at[v] = 0;
        *info = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    // test hooks, first guesses
    const RowBounds bounds = row_bounds("BCC_WAVE_ROW", "BCC_WG_ROW");
    const int64_t wg_level = std::max<long long>(0, std::min<long long>(opt_int("BCC_WG_LEVEL", kBiccWgLevelDefault), INT_MAX));
    const long long wg_frontier = frontier_wg_option("BCC_WG_FRONTIER", kWgFrontierDefault);
    const bool timing = opt_on("TIMING");  // one line per call on stderr: the wall time of every phase (each ends in a synchronize then)
    // ---- setup: the buffers
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    DevBuf d32[17], d64[4], d_ctrl, d_acc, d_block, d_keep;
    FrontierStore store;
    BiccArrays a;
    int32_t **w32[17] = {&a.label, &a.depth, &a.parent, &a.rank, &a.order, &a.loff, &a.nd,  &a.slot, &a.rel,
                         &a.pre,   &a.low,   &a.high,   &a.aux,  &a.size,  &a.id,   &a.at, &a.top};
    for (int i = 0; i < 17; ++i) {
        if (int rc = dalloc<int32_t>(d32[i], n + 2)) return rc;
        *w32[i] = d32[i].as<int32_t>();
    }
    for (int i = 0; i < 4; ++i)
        if (int rc = dalloc<int64_t>(d64[i], n + 1)) return rc;
    a.kids = d64[0].as<unsigned long long>();
    a.cbase = d64[1].as<int64_t>();
    a.val = d64[2].as<int64_t>();
    a.pfx = d64[3].as<int64_t>();
    a.cnt = d64[0].as<int64_t>();
    a.pos = d64[1].as<int64_t>();
    a.first = d64[2].as<unsigned long long>();
    a.edges = d64[3].as<unsigned long long>();
    RowListStore lists;
    if (int rc = lists.alloc(n, nnz, bounds, false, false)) return rc;
    if (int rc = store.alloc(n, nnz, false)) return rc;
    if (int rc = dalloc<BiccCtrl>(d_ctrl, 1)) return rc;
    if (int rc = dalloc<BiccAcc>(d_acc, 1)) return rc;
    if (block)
        if (int rc = dalloc<int32_t>(d_block, nnz)) return rc;
    if (arc_keep)
        if (int rc = dalloc<uint8_t>(d_keep, nnz)) return rc;
    BiccCtrl *ctrl = d_ctrl.as<BiccCtrl>();
    BiccAcc *acc = d_acc.as<BiccAcc>();
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(BiccCtrl), s));
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(BiccAcc), s));
    GMSX_HIP(hipMemsetAsync(&acc->best, 0xff, sizeof(unsigned long long), s));
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    int launches = 0;
    const unsigned per_vertex = unsigned((n + 256) / 256);  // n + 1 threads
    const unsigned sweep = row_grid(n, 1, cus, 16);
    const uint32_t cap = cc_walk_cap(n);
    double phase_ms[7] = {0, 0, 0, 0, 0, 0, 0};  // roots, forest, nd, preorder, low / high, arc passes, ids
    auto t0 = std::chrono::steady_clock::now();
    auto phase_end = [&](int which) -> int {  // (TIMING only: the phases of an ordinary call run back to back)
        if (!timing) return GMSX_OK;
        GMSX_HIP(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        phase_ms[which] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return GMSX_OK;
    };
    // ---- 1: the roots
    hipLaunchKernelGGL(k_bicc_init, dim3(per_vertex), dim3(256), 0, s, n, a);
    ++launches;
    classify_rows<false>(g, bounds, lists.l, acc->count, &acc->error, cus, s, &launches);
    auto rows = [&](const auto &op) { launch_rows(op, g, bounds, lists.l, acc->count, &acc->examined, cus, s, &launches); };
    rows(OpLink{g->adj, a.label, cap, &acc->error});
    if (int rc = flatten(n, a.label, &acc->error, cus, s, &launches, nullptr)) return rc;
    hipLaunchKernelGGL(k_bicc_forest_init, dim3(per_vertex), dim3(256), 0, s, n, a.label, a.depth, a.parent);
    frontier_collect(n, BiccIsRoot{a.label}, a.order, &ctrl->placed, &ctrl->error);
    launches += 2;
    BiccCtrl h;
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (h.error || h.placed < 1 || int64_t(h.placed) > n) return GMSX_ERR_KERNEL;
    const int64_t roots = h.placed;
    if (int rc = phase_end(0)) return rc;
    // ---- 2: the forest; order fills level by level
    const FrontierBufs bufs = store.bufs();
    const int32_t loff01[2] = {0, int32_t(roots)};
    h.count = int32_t(roots);
    h.seen = 1;
    GMSX_HIP(hipMemcpyAsync(ctrl, &h, sizeof h, hipMemcpyHostToDevice, s));
    GMSX_HIP(hipMemcpyAsync(a.loff, loff01, sizeof loff01, hipMemcpyHostToDevice, s));
    GMSX_HIP(hipMemcpyAsync(bufs.f[0], a.order, size_t(roots) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    GMSX_HIP(hipStreamSynchronize(s));
    const BiccForest forest{n, g->off, g->adj, a.depth, a.parent, a.rank, a.order, a.loff, a.kids, ctrl};
    if (int rc = run_frontier_rounds(forest, bufs, ctrl, h, wg_frontier, &launches)) return rc;
    const int32_t levels = h.round;
    if (int64_t(h.placed) != n || levels < 1 || int64_t(levels) > n || h.seen != levels + 1) return GMSX_ERR_KERNEL;
    std::vector<int32_t> h_loff(size_t(levels) + 1);
    GMSX_HIP(hipMemcpyAsync(h_loff.data(), a.loff, h_loff.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (h_loff[0] != 0 || int64_t(h_loff[size_t(levels)]) != n) return GMSX_ERR_KERNEL;
    for (int32_t d = 0; d < levels; ++d)
        if (h_loff[size_t(d) + 1] <= h_loff[size_t(d)]) return GMSX_ERR_KERNEL;  // (every level of the forest holds a vertex)
    if (int rc = phase_end(1)) return rc;
    // ---- 3: subtree sizes
    if (levels > 1) bicc_sweep(SweepNd{a.parent, a.nd}, n, h_loff, levels - 1, 1, wg_level, a.order, a.loff, s, &launches);
    if (int rc = phase_end(2)) return rc;
    // ---- 4: the preorder
    if (int rc = exclusive_scan_i64(reinterpret_cast<const int64_t *>(a.kids), a.cbase, n + 1, s)) return rc;
    hipLaunchKernelGGL(k_bicc_layout, dim3(per_vertex), dim3(256), 0, s, n, roots, a, acc);
    if (int rc = exclusive_scan_i64(a.val, a.pfx, n + 1, s)) return rc;
    hipLaunchKernelGGL(k_bicc_rel, dim3(per_vertex), dim3(256), 0, s, n, roots, a, acc);
    launches += 4;
    bicc_sweep(SweepPre{a.parent, a.rel, a.pre, a.low, a.high}, n, h_loff, 0, levels - 1, wg_level, a.order, a.loff, s, &launches);
    if (int rc = phase_end(3)) return rc;
    // ---- 5: low and high
    rows(OpLowHigh{g->adj, a.parent, a.pre, a.low, a.high});
    if (int rc = phase_end(5)) return rc;
    if (levels > 1) bicc_sweep(SweepLowHigh{a.parent, a.low, a.high}, n, h_loff, levels - 1, 1, wg_level, a.order, a.loff, s, &launches);
    if (int rc = phase_end(4)) return rc;
    // ---- 6: the auxiliary unions
    rows(OpAux{g->adj, a.parent, a.pre, a.nd, a.low, a.high, a.aux, cap, &acc->error});
    if (int rc = flatten(n, a.aux, &acc->error, cus, s, &launches, nullptr)) return rc;
    // ---- 7: first arcs, edges, ids
    hipLaunchKernelGGL(k_bicc_ids_init, dim3(per_vertex), dim3(256), 0, s, n, a);
    ++launches;
    rows(OpFirst{g->adj, a.pre, a.aux, a.first, a.edges, acc, -1, 0, 0, 0});
    if (int rc = phase_end(5)) return rc;
    launch_rows_two_width(BiccRank<false>{g->adj, a, n, acc}, g, &acc->examined, cus, s, &launches);
    // (pos is cbase's buffer: the scan reads cnt = kids' buffer)
    if (int rc = exclusive_scan_i64(a.cnt, a.pos, n + 1, s)) return rc;
    ++launches;
    launch_rows_two_width(BiccRank<true>{g->adj, a, n, acc}, g, &acc->examined, cus, s, &launches);
    // ---- 8, 9: sizes, blocks_at, the info reduction
    hipLaunchKernelGGL(k_cc_sizes, dim3(sweep), dim3(256), 0, s, n, a.aux, a.size);
    hipLaunchKernelGGL(k_bicc_top, dim3(sweep), dim3(256), 0, s, n, a);
    hipLaunchKernelGGL(k_bicc_at, dim3(sweep), dim3(256), 0, s, n, a, acc);
    hipLaunchKernelGGL(k_bicc_info, dim3(sweep), dim3(256), 0, s, n, g->off, a, acc);
    hipLaunchKernelGGL(k_bicc_largest, dim3(sweep), dim3(256), 0, s, n, a, acc);
    launches += 5;
    if (int rc = phase_end(6)) return rc;
    // ---- 10: the per-arc outputs
    if (block || arc_keep) {
        rows(OpOut{g->adj, a.pre, a.aux, a.id, a.size, d_block.as<int32_t>(), d_keep.as<uint8_t>()});
        if (int rc = phase_end(5)) return rc;
    }
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    BiccAcc r;
    GMSX_HIP(hipMemcpyAsync(&r, acc, sizeof r, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    const unsigned long long un = (unsigned long long)n;
    if (r.error || r.comps != (unsigned long long)roots || r.nd_roots != un || r.upper != r.lower || r.upper != (unsigned long long)(nnz / 2) ||
        r.sum_edges != r.upper || r.blocks < 1 || r.blocks > un - r.comps || r.sum_at != un - r.comps + r.blocks || r.best == ~0ull ||
        r.best_edges < 1 || (r.best >> 32) >= r.blocks)
        return GMSX_ERR_KERNEL;
    res.blocks = int64_t(r.blocks);
    res.bridges = int64_t(r.bridges);
    res.articulation_points = int64_t(r.artic);
    res.largest_block_edges = int64_t(r.best_edges);
    res.largest_block_vertices = int64_t(uint32_t(r.best));
    res.components = int64_t(r.comps);
    res.isolated = int64_t(r.isolated);
    res.largest_block = int32_t(r.best >> 32);
    res.max_blocks_at = r.max_at;
    res.levels = levels;
    // the flag word was read as zero: the caller's arrays are written now, through host staging
    HostStage out;
    if (int rc = out.fetch(block, d_block.p, size_t(nnz) * sizeof(int32_t), s)) return rc;
    if (int rc = out.fetch(blocks_at, a.at, size_t(n) * sizeof(int32_t), s)) return rc;
    if (int rc = out.fetch(arc_keep, d_keep.p, size_t(nnz), s)) return rc;
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    float up_ms = 0.f, ms = 0.f, out_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&out_ms, c.ev[2], c.ev[3]));
    out.deliver();
    *info = res;
    if (timing)
        std::fprintf(stderr,
                     "[gmsx bicc] roots %.3f forest %.3f nd %.3f preorder %.3f lowhigh %.3f arcs %.3f ids %.3f ms, %d launches, %d levels, %lld roots\n",
                     phase_ms[0], phase_ms[1], phase_ms[2], phase_ms[3], phase_ms[4], phase_ms[5], phase_ms[6], launches, int(levels), (long long)roots);
    if (stats) *stats = gmsx_stats{double(ms), double(up_ms) + double(out_ms), uint64_t(res.blocks), uint64_t(r.examined), uint64_t(levels), launches, 0, 0};
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_biconnected_components(const gmsx_graph *g, uint32_t flags, int32_t *block, int32_t *blocks_at, uint8_t *arc_keep, gmsx_bicc_info *info,
                                gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || flags != 0) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        return bicc(g, block, blocks_at, arc_keep, info, stats);
    });
}

}  // extern "C"
