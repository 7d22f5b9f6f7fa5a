// Label-propagation communities and the exact modularity of a labelling on gfx950 (no reference counterpart; the definitions are those of
// include/gmsx.h).  Everything is an integer; no floating point runs on the device.
//   gmsx_label_propagation   asynchronous label propagation, colour class by colour class: every vertex of the class takes the label of greatest
//                            total weight among its neighbours (ties: it keeps its own if that is a maximum, else the smallest label)
//   gmsx_modularity          W, I, S = Σ D_c² (128 bits), communities, largest and `unstable` of a caller's labelling
//
// THE HOT PASS is the evaluation of one row: gather label[adj[j]] (and w[j]), find (M, the smallest label at M, W_v(own)).  Three row classes,
// four bins — a row's bin is a function of its length alone:
//   short    length <= min(16, LP_WAVE_ROW): a 16-lane group per row; length <= LP_WAVE_ROW (<= 64): a wave per row.  One entry per lane; every
//            lane sums the weights of the entries equal to its own by broadcasting entry after entry, then a pair maximum over the group
//            (wave_ops.hpp).  No atomics, no LDS.
//   medium   length <= LP_LDS_ROW (<= LP_LDS_SLOTS): a workgroup per row and an open-addressing table in LDS of the smallest power of two >= twice
//            the length (at most LP_LDS_SLOTS slots): the key goes in by atomicCAS, the 64-bit weight by an LDS atomic add, then the table is scanned
//            for the pair maximum.  Integer sums and a (max weight, min label) pick do not depend on the order of arrival.
//   long     everything else: the same table, sized from the row's length, in the row's region of a global slab (a region holds the longest
//            row of the graph; as many regions as kLpSlabBytes allows, one at the least, and a class with more long rows than regions takes
//            them in turns).  ALL WORKGROUPS WALK THEM TOGETHER: k_lp_long_fill cuts every row into up to kLpLongParts parts, a workgroup
//            each, which insert with global atomics; k_lp_long_pick, a workgroup per row, scans the table, wipes it for the next row and
//            applies the pick.  The hubs of a power-law graph are adjacent to each other, so a class holds one or two of them: a workgroup
//            per row left the device idle behind one compute unit.  No graph is refused for a hub.
// Linear probing is capped by the table size: a probe loop past it raises the flag word (GMSX_ERR_KERNEL).
//
// CLASSES.  The vertices with at least one arc are counting-sorted by (colour, bin) into cls_vtx, cls_off[4 C + 1] (k_lp_hist, a scan, k_lp_place;
// the order inside one (colour, bin) is the arrival order of an atomic cursor and reaches no output: every row is evaluated on its own).  A
// class is an independent set: within a class the labels are read-only for the readers and written once by each owner.
// SCHEDULING.  A sweep takes the colours 1 … C in order.  A class whose rows hold more than LP_WG_WORK entries gets a launch per non-empty bin;
// consecutive classes that hold at most LP_WG_WORK entries in all are run by ONE workgroup in one launch (k_lp_tiny), class after class with a
// __syncthreads() between them (label and the dirty bytes are written and read by the same workgroup: workgroup-scope visibility is what the
// barrier gives).  No workgroup ever waits for another.
// DIRTY SET (LP_ACTIVE = 1).  dirty[v] = a neighbour of v changed since v was evaluated (sweep 1: every vertex).  A clean vertex holds a label
// that is a maximum, so evaluating it again cannot change it: LP_ACTIVE 0 / 1 give the same bytes.  A vertex that changes sets its neighbours'
// bytes and the word of each neighbour's CLASS — in the array of this sweep if that class is still to come (a larger colour), else in the next
// sweep's.  The host reads both arrays with the control block once per sweep: the classes in front of the first marked one are skipped outright
// (nothing can dirty them before their turn); a later unmarked class may be dirtied by an earlier class of the same sweep, so it is still
// launched, and its workgroups leave at once when its word is still zero on the device.
//
// MODULARITY evaluates every row once in the no-write mode of the same code: W_v(own) sums to I, W_v(own) < M counts `unstable`, and the row's
// total weight goes to D[label[v]] with a 64-bit integer atomic.  k_lp_sumsq squares the D_c in unsigned __int128 per thread, thread 0 of a block
// adds its threads' pairs, and the host adds the per-block (hi, lo) partials.
// STATE: label, the colours, cls_vtx and the sizes as 32-bit words, a dirty byte per vertex, 4 C + 1 offsets, 2 (C + 1) class words, D (modularity
// only) and the slab of the long rows — DevBufs of the call.
#include "coloring_device.hpp"  // the default colouring, and the check of a caller's one, on the device
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // load_now, store_now

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

constexpr int kLpBins = 4;          // 16-lane group, wave, LDS table, global table
constexpr int kLpThreads = 256;
constexpr int kLpSlotsMax = 4096;   // 48 KB of LDS: three workgroups beside each other in the 160 KB of a CU
constexpr int kLpSweepCap = 1000;
constexpr int kLpFoldRounds = 2;     // labels a wave folds before its lanes insert on their own (a first guess: one giant community and a runner-up)
constexpr int kLpLongParts = 256;    // most workgroups that fill the table of one long row together
constexpr int64_t kLpSlabBytes = int64_t(1) << 30;  // the long rows' regions together (one region is allocated whatever its size)
// The three row bounds are UNMEASURED first guesses (gmsx.h, OPTIONS).  LP_WG_WORK and LP_ACTIVE come from tools/communities_probe.py at kronecker 20
// and 22: 0, 1024 and 4096 measured the same, 32768 up to 30 % slower at scale 20; LP_ACTIVE = 1 is 7 – 17 % faster.
constexpr long long kLpWaveRowDefault = 64, kLpLdsRowDefault = 2048, kLpLdsSlotsDefault = kLpSlotsMax, kLpWgWorkDefault = 4096, kLpActiveDefault = 1;

// the call's small device block, mirrored to the host after every sweep
struct LpCtrl {
    int32_t error;    // the flag word: a probe loop passed its cap, a table would not fit its region, a placement hit its bound
    int32_t bad;      // modularity: labels outside [0, n)
    unsigned long long changed;   // label changes of the sweep
    unsigned long long rows, arcs;  // rows evaluated, arcs gathered (gmsx_stats)
    unsigned long long total, intra, unstable;  // no-write mode: W, I, unstable
    unsigned long long max_long;  // longest row of the long bin
    unsigned long long communities, singletons, largest;  // largest = size << 32 | ~label: the maximum is the largest community of the smallest label
};

// what every evaluation kernel gets
struct LpArgs {
    const int64_t *off;
    const int32_t *adj, *wgt;  // wgt == nullptr: every arc weighs 1
    int32_t *label;
    uint8_t *dirty;
    const int32_t *color;      // nullptr in the no-write mode
    int32_t *flags;            // [2][colors + 1]: class c has a dirty vertex, by the parity of the sweep that will evaluate it
    const int32_t *vtx;        // cls_vtx
    int32_t *keys;             // the slab: region r = keys + r * region_slots …
    unsigned long long *wts;   // … and wts + r * region_slots
    unsigned long long *deg;   // no-write mode: D
    LpCtrl *ctrl;
    int64_t region_slots;
    int32_t lds_slots, colors, par;  // par = sweep & 1
    int32_t active, obey;            // the dirty bytes and class words are written (LP_ACTIVE) / read as well (from sweep 2 on)
};

struct LpPick {
    long long m, own, tot;  // M, W_v(own), the row's total weight
    int32_t best;           // the smallest label at M
};

// per-thread tallies of a kernel, folded into the control block at its end
struct LpTally {
    unsigned long long changed = 0, rows = 0, arcs = 0, total = 0, intra = 0, unstable = 0;
    __device__ __forceinline__ void flush(LpCtrl *ctrl) {
        changed = wave_sum(changed), rows = wave_sum(rows), arcs = wave_sum(arcs);
        total = wave_sum(total), intra = wave_sum(intra), unstable = wave_sum(unstable);
        if ((threadIdx.x & 63) != 0) return;
        if (changed) atomicAdd(&ctrl->changed, changed);
        if (rows) atomicAdd(&ctrl->rows, rows);
        if (arcs) atomicAdd(&ctrl->arcs, arcs);
        if (total) atomicAdd(&ctrl->total, total);
        if (intra) atomicAdd(&ctrl->intra, intra);
        if (unstable) atomicAdd(&ctrl->unstable, unstable);
    }
};

// LDS of a workgroup-per-row evaluation: the table of a medium row, and the words the workgroup folds its waves' picks through
struct LpTableLds {
    int32_t keys[kLpSlotsMax];
    unsigned long long wts[kLpSlotsMax];
};
struct LpShared {
    long long m[kLpThreads / 64], own[kLpThreads / 64], tot[kLpThreads / 64];
    int32_t best[kLpThreads / 64];
    int32_t go;
};

__host__ __device__ inline int lp_log2_slots(int64_t len) {  // the smallest power of two >= 2 len, at least 2
    int lg = 1;
    while ((int64_t(1) << lg) < 2 * len) ++lg;
    return lg;
}

// SHORT row: WIDTH lanes, len <= WIDTH entries from j0 on; the pick is valid in every lane of the group
template <int WIDTH>
__device__ __forceinline__ LpPick lp_short(const LpArgs &a, int64_t j0, int len, int lane, int32_t own) {
    int32_t l = -1, w = 0;
    if (lane < len) {
        l = a.label[a.adj[j0 + lane]];
        w = a.wgt ? a.wgt[j0 + lane] : 1;
    }
    long long sum = 0;
    for (int k = 0; k < len; ++k) {  // (len is the group's: its lanes stay together)
        const int32_t lk = __shfl(l, k, WIDTH), wk = __shfl(w, k, WIDTH);
        if (lk == l) sum += wk;
    }
    LpPick p;
    p.tot = wave_sum_all<WIDTH>((long long)w);
    p.own = wave_max_all<WIDTH>(l == own ? sum : 0ll);
    p.m = sum;  // (a lane without an entry holds (0, -1): any entry beats it, its weight is >= 1)
    p.best = l;
    wave_pair_max_all<WIDTH>(p.m, p.best);
    return p;
}

// one entry (label l, weight w) into the table of 2^lg slots: the key by atomicCAS, the weight by an integer atomic add; linear probing, capped
__device__ __forceinline__ void lp_insert(const LpArgs &a, int32_t *keys, unsigned long long *wts, int lg, int32_t l, unsigned long long w) {
    const int64_t slots = int64_t(1) << lg, mask = slots - 1;
    int64_t h = int64_t((uint64_t(uint32_t(l)) * 0x9E3779B97F4A7C15ull) >> (64 - lg));
    for (int64_t probes = 0;; ++probes) {
        if (probes >= slots) {  // (cannot happen: the row holds at most `slots` distinct labels)
            a.ctrl->error = 1;
            return;
        }
        const int32_t old = atomicCAS(&keys[h], -1, l);
        if (old == -1 || old == l) {
            atomicAdd(&wts[h], w);
            return;
        }
        h = (h + 1) & mask;
    }
}

// entries [b, e) of the row that starts at j0 into the table, by all threads of the workgroup.  From the second sweep on most neighbours of a hub
// hold ONE label, and atomics on one address take their turns: measured, a long row cost the same 180 ms per sweep at scale 22 whether its
// table was filled by one workgroup or by 256.  So a wave first folds the entries that equal its first pending lane's label
// into one insert, kLpFoldRounds times, and only what is left goes in entry by entry — sums of integers, whoever adds them.
__device__ __forceinline__ void lp_table_fill(const LpArgs &a, int32_t *keys, unsigned long long *wts, int lg, int64_t j0, int64_t b, int64_t e) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = b; base < e; base += kLpThreads) {  // (uniform in the workgroup: whole waves stay converged for the ballots)
        const int64_t j = base + threadIdx.x;
        bool pending = j < e;
        const int32_t l = pending ? a.label[a.adj[j0 + j]] : -1;
        const unsigned long long w = !pending ? 0ull : a.wgt ? (unsigned long long)uint32_t(a.wgt[j0 + j]) : 1ull;
        for (int r = 0; r < kLpFoldRounds; ++r) {
            const unsigned long long left = __ballot(pending);
            if (!left) break;
            const int leader = __ffsll(left) - 1;
            const int32_t ll = __shfl(l, leader);
            const bool mine = pending && l == ll;
            const unsigned long long sum = wave_sum_all(mine ? w : 0ull);
            if (mine) pending = false;
            if (lane == leader) lp_insert(a, keys, wts, lg, ll, sum);
        }
        if (pending) lp_insert(a, keys, wts, lg, l, w);
    }
}

// the pick of a filled table by all threads of the workgroup (holds barriers; valid in every thread); WIPE: every slot is emptied behind its read,
// which is how a region of the slab stays empty between its rows
template <bool WIPE>
__device__ __forceinline__ LpPick lp_table_pick(int32_t *keys, unsigned long long *wts, int lg, int32_t own, LpShared *sh) {
    const int tid = threadIdx.x;
    const int64_t slots = int64_t(1) << lg;
    long long m = 0, ownw = 0, tot = 0;
    int32_t best = INT_MAX;
    for (int64_t h = tid; h < slots; h += kLpThreads) {
        const int32_t k = load_now(&keys[h]);
        if (k < 0) continue;
        const long long w = (long long)load_now(&wts[h]);
        if (WIPE) {
            keys[h] = -1;
            wts[h] = 0;
        }
        tot += w;
        if (w > m || (w == m && k < best)) m = w, best = k;
        if (k == own) ownw = w;
    }
    wave_pair_max(m, best);
    ownw = wave_max(ownw);
    tot = wave_sum(tot);
    if ((tid & 63) == 0) {
        sh->m[tid >> 6] = m;
        sh->best[tid >> 6] = best;
        sh->own[tid >> 6] = ownw;
        sh->tot[tid >> 6] = tot;
    }
    __syncthreads();
    LpPick p{sh->m[0], sh->own[0], sh->tot[0], sh->best[0]};
    for (int w = 1; w < kLpThreads / 64; ++w) {
        if (sh->m[w] > p.m || (sh->m[w] == p.m && sh->best[w] < p.best)) p.m = sh->m[w], p.best = sh->best[w];
        p.own = max(p.own, sh->own[w]);
        p.tot += sh->tot[w];
    }
    __syncthreads();  // (the next row writes the same words)
    return p;
}

// what follows a pick, by the `width` threads that evaluated row v together (lane = this thread's number among them; `leader` is lane 0).
// WRITE: the new label, and the neighbours' dirty bytes and class words.  Else: the sums of the modularity.
template <bool WRITE>
__device__ __forceinline__ void lp_apply(const LpArgs &a, int32_t v, int32_t cv, int32_t own, int64_t j0, int64_t len, const LpPick &p, int lane,
                                         int width, LpTally &t) {
    const bool moves = len > 0 && p.own < p.m;
    if (lane == 0) {
        ++t.rows;
        t.arcs += (unsigned long long)len;
    }
    if (WRITE) {
        if (!moves) return;
        if (lane == 0) {
            a.label[v] = p.best;
            ++t.changed;
        }
        if (!a.active) return;
        const int64_t stride = int64_t(a.colors) + 1;
        for (int64_t j = lane; j < len; j += width) {
            const int32_t x = a.adj[j0 + j];
            a.dirty[x] = 1;
            const int32_t cx = a.color[x];
            int32_t *word = a.flags + (cx > cv ? a.par : a.par ^ 1) * stride + cx;
            if (!load_now(word)) store_now(word, 1);
        }
    } else if (lane == 0) {
        t.total += (unsigned long long)p.tot;
        t.intra += (unsigned long long)p.own;
        t.unstable += moves ? 1 : 0;
        atomicAdd(&a.deg[own], (unsigned long long)p.tot);
    }
}

// is class c to be evaluated by this launch (its word of this sweep's array; sweep 1 marks every class)
__device__ __forceinline__ bool lp_class_live(const LpArgs &a, int32_t c) {
    return !a.obey || load_now(a.flags + int64_t(a.par) * (int64_t(a.colors) + 1) + c) != 0;
}

// the short rows cls_vtx[first, first + count) of colour cv by groups of WIDTH lanes; `group` of `groups` is this thread's
template <int WIDTH, bool WRITE>
__device__ __forceinline__ void lp_short_rows(const LpArgs &a, int64_t first, int64_t count, int32_t cv, int64_t group, int64_t groups, LpTally &t) {
    const int lane = threadIdx.x & (WIDTH - 1);
    for (int64_t i = group; i < count; i += groups) {
        const int32_t v = a.vtx[first + i];
        if (WRITE && a.active) {
            const uint8_t d = a.dirty[v];
            if (a.obey && !d) continue;
            if (lane == 0 && d) a.dirty[v] = 0;
        }
        const int64_t j0 = a.off[v];
        const int len = int(a.off[v + 1] - j0);
        const int32_t own = a.label[v];
        const LpPick p = lp_short<WIDTH>(a, j0, len, lane, own);
        lp_apply<WRITE>(a, v, cv, own, j0, len, p, lane, WIDTH, t);
    }
}

// is row v to be evaluated (every thread of the workgroup gets the same answer; holds barriers)?  Thread 0 takes the dirty byte away.
template <bool WRITE>
__device__ __forceinline__ bool lp_wg_row_due(const LpArgs &a, int32_t v, LpShared *sh) {
    if (!WRITE || !a.active) return true;
    if (threadIdx.x == 0) {
        sh->go = a.dirty[v];
        a.dirty[v] = 0;
    }
    __syncthreads();
    const int32_t go = sh->go;
    __syncthreads();
    return !a.obey || go;
}

// the medium (tab != nullptr: the table in LDS) or long rows (region 0 of the slab) cls_vtx[first, first + count), every `step`-th from `start`
// on, by the whole workgroup
template <bool WRITE>
__device__ __forceinline__ void lp_wg_rows(const LpArgs &a, int64_t first, int64_t count, int32_t cv, int64_t start, int64_t step, LpTableLds *tab,
                                           LpShared *sh, LpTally &t) {
    for (int64_t i = start; i < count; i += step) {  // (uniform in the workgroup)
        const int32_t v = a.vtx[first + i];
        if (!lp_wg_row_due<WRITE>(a, v, sh)) continue;
        const int64_t j0 = a.off[v], len = a.off[v + 1] - j0;
        const int32_t own = a.label[v];
        int lg = lp_log2_slots(len);
        LpPick p;
        if (tab) {
            while ((1 << lg) > a.lds_slots) --lg;  // (len <= lds_slots: the table is full at the worst)
            for (int h = threadIdx.x; h < (1 << lg); h += kLpThreads) {
                tab->keys[h] = -1;
                tab->wts[h] = 0;
            }
            __syncthreads();
            lp_table_fill(a, tab->keys, tab->wts, lg, j0, 0, len);
            __syncthreads();
            p = lp_table_pick<false>(tab->keys, tab->wts, lg, own, sh);
        } else if ((int64_t(1) << lg) > a.region_slots) {
            if (threadIdx.x == 0) a.ctrl->error = 1;
            continue;
        } else {
            lp_table_fill(a, a.keys, a.wts, lg, j0, 0, len);
            __syncthreads();
            p = lp_table_pick<true>(a.keys, a.wts, lg, own, sh);
        }
        lp_apply<WRITE>(a, v, cv, own, j0, len, p, threadIdx.x, kLpThreads, t);
    }
}

// one of the bins 0 … 2 of one class, a launch of its own
template <int BIN, bool WRITE>
__global__ __launch_bounds__(kLpThreads) void k_lp_bin(LpArgs a, int64_t first, int64_t count, int32_t cv) {
    __shared__ LpTableLds tab;
    __shared__ LpShared sh;
    if (WRITE && !lp_class_live(a, cv)) return;
    LpTally t;
    if (BIN == 0) {
        lp_short_rows<16, WRITE>(a, first, count, cv, (int64_t(blockIdx.x) * kLpThreads + threadIdx.x) / 16, int64_t(gridDim.x) * kLpThreads / 16, t);
    } else if (BIN == 1) {
        lp_short_rows<64, WRITE>(a, first, count, cv, (int64_t(blockIdx.x) * kLpThreads + threadIdx.x) / 64, int64_t(gridDim.x) * kLpThreads / 64, t);
    } else {
        lp_wg_rows<WRITE>(a, first, count, cv, blockIdx.x, gridDim.x, &tab, &sh, t);
    }
    t.flush(a.ctrl);
}

// LONG rows, all workgroups together.  Workgroup (x, y) puts part x of gridDim.x of the row cls_vtx[first + y] into region y of the slab (empty
// before: the pick wipes it) …
template <bool WRITE>
__global__ __launch_bounds__(kLpThreads) void k_lp_long_fill(LpArgs a, int64_t first, int32_t cv) {
    if (WRITE && !lp_class_live(a, cv)) return;
    const int64_t region = blockIdx.y;
    const int32_t v = a.vtx[first + region];
    if (WRITE && a.obey && !a.dirty[v]) return;  // (the byte is taken away by the pick: both kernels see the same one)
    const int64_t j0 = a.off[v], len = a.off[v + 1] - j0;
    const int lg = lp_log2_slots(len);
    if ((int64_t(1) << lg) > a.region_slots) {
        if (threadIdx.x == 0) a.ctrl->error = 1;
        return;
    }
    const int64_t per = (len + gridDim.x - 1) / gridDim.x, b = int64_t(blockIdx.x) * per;
    lp_table_fill(a, a.keys + region * a.region_slots, a.wts + region * a.region_slots, lg, j0, b, min(len, b + per));
}

// … and workgroup y scans the table of its row, wipes it, and applies the pick
template <bool WRITE>
__global__ __launch_bounds__(kLpThreads) void k_lp_long_pick(LpArgs a, int64_t first, int32_t cv) {
    __shared__ LpShared sh;
    if (WRITE && !lp_class_live(a, cv)) return;
    const int64_t region = blockIdx.x;
    const int32_t v = a.vtx[first + region];
    LpTally t;
    if (lp_wg_row_due<WRITE>(a, v, &sh)) {
        const int64_t j0 = a.off[v], len = a.off[v + 1] - j0;
        const int lg = lp_log2_slots(len);
        if ((int64_t(1) << lg) <= a.region_slots) {
            const int32_t own = a.label[v];
            const LpPick p = lp_table_pick<true>(a.keys + region * a.region_slots, a.wts + region * a.region_slots, lg, own, &sh);
            lp_apply<WRITE>(a, v, cv, own, j0, len, p, threadIdx.x, kLpThreads, t);
        }
    }
    t.flush(a.ctrl);
}

// the classes c0 … c1 by ONE workgroup, class after class
__global__ __launch_bounds__(kLpThreads) void k_lp_tiny(LpArgs a, const int64_t *__restrict__ cls_off, int32_t c0, int32_t c1) {
    __shared__ LpTableLds tab;
    __shared__ LpShared sh;
    LpTally t;
    for (int32_t c = c0; c <= c1; ++c) {
        if (lp_class_live(a, c)) {  // (uniform: the word is only written for LATER classes while this launch runs)
            const int64_t *o = cls_off + int64_t(c - 1) * kLpBins;
            lp_short_rows<16, true>(a, o[0], o[1] - o[0], c, threadIdx.x / 16, kLpThreads / 16, t);
            lp_short_rows<64, true>(a, o[1], o[2] - o[1], c, threadIdx.x / 64, kLpThreads / 64, t);
            lp_wg_rows<true>(a, o[2], o[3] - o[2], c, 0, 1, &tab, &sh, t);
            lp_wg_rows<true>(a, o[3], o[4] - o[3], c, 0, 1, nullptr, &sh, t);
        }
        __syncthreads();  // the labels, dirty bytes and class words of this class are visible to the next one
    }
    t.flush(a.ctrl);
}

// ---- setup --------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int lp_bin_of(int64_t len, int64_t group_row, int64_t wave_row, int64_t lds_row) {
    return len <= group_row ? 0 : len <= wave_row ? 1 : len <= lds_row ? 2 : 3;
}

__global__ void k_lp_init(int64_t n, int32_t *__restrict__ label, uint8_t *__restrict__ dirty) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) {
        label[v] = int32_t(v);
        dirty[v] = 1;
    }
}

// cnt[(colour - 1) * 4 + bin] of every vertex with an arc, the entries of every colour and the longest row of the long bin
__global__ __launch_bounds__(256) void k_lp_hist(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ color, int32_t colors,
                                                 int64_t group_row, int64_t wave_row, int64_t lds_row, unsigned long long *__restrict__ cnt,
                                                 unsigned long long *__restrict__ work, LpCtrl *__restrict__ ctrl) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long longest = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int64_t len = off[v + 1] - off[v];
        if (len <= 0) continue;
        const int32_t c = color ? color[v] : 1;
        if (c < 1 || c > colors) {
            ctrl->error = 1;
            continue;
        }
        const int bin = lp_bin_of(len, group_row, wave_row, lds_row);
        atomicAdd(&cnt[int64_t(c - 1) * kLpBins + bin], 1ull);
        atomicAdd(&work[c - 1], (unsigned long long)len);
        if (bin == 3) longest = max(longest, (unsigned long long)len);
    }
    longest = wave_max(longest);
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(&ctrl->max_long, longest);
}

__global__ __launch_bounds__(256) void k_lp_place(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ color, int32_t colors,
                                                  int64_t group_row, int64_t wave_row, int64_t lds_row, const int64_t *__restrict__ cls_off,
                                                  unsigned long long *__restrict__ cursor, int32_t *__restrict__ vtx, int64_t cap,
                                                  LpCtrl *__restrict__ ctrl) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int64_t len = off[v + 1] - off[v];
        if (len <= 0) continue;
        const int32_t c = color ? color[v] : 1;
        if (c < 1 || c > colors) continue;
        const int64_t key = int64_t(c - 1) * kLpBins + lp_bin_of(len, group_row, wave_row, lds_row);
        const int64_t pos = cls_off[key] + int64_t(atomicAdd(&cursor[key], 1ull));
        if (pos < cls_off[key + 1] && pos < cap) vtx[pos] = int32_t(v);
        else ctrl->error = 1;
    }
}

// modularity: a label outside [0, n) is counted before anything reads one as an index
__global__ __launch_bounds__(256) void k_lp_check_labels(int64_t n, const int32_t *__restrict__ label, LpCtrl *__restrict__ ctrl) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n && (label[v] < 0 || int64_t(label[v]) >= n)) ctrl->bad = 1;
}

// ---- the info pass ----------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_lp_sizes(int64_t n, const int32_t *__restrict__ label, int32_t *__restrict__ size) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) atomicAdd(&size[label[v]], 1);
}

__global__ __launch_bounds__(256) void k_lp_info(int64_t n, const int32_t *__restrict__ size, LpCtrl *__restrict__ ctrl) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long communities = 0, singletons = 0, largest = 0;
    for (int64_t l = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; l < n; l += stride) {
        const uint32_t s = uint32_t(size[l]);
        if (!s) continue;
        ++communities;
        singletons += s == 1;
        largest = max(largest, ((unsigned long long)s << 32) | uint32_t(~uint32_t(l)));
    }
    communities = wave_sum(communities);
    singletons = wave_sum(singletons);
    largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0 && communities) {
        atomicAdd(&ctrl->communities, communities);
        if (singletons) atomicAdd(&ctrl->singletons, singletons);
        atomicMax(&ctrl->largest, largest);
    }
}

// Σ D_c² over the labels of a block, exact: out[2 b] = the low, out[2 b + 1] = the high 64 bits of block b's sum
__global__ __launch_bounds__(256) void k_lp_sumsq(int64_t n, const unsigned long long *__restrict__ deg, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long s_lo[256], s_hi[256];
    unsigned __int128 acc = 0;
    for (int64_t l = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; l < n; l += int64_t(gridDim.x) * blockDim.x) {
        const unsigned __int128 d = deg[l];
        acc += d * d;
    }
    s_lo[threadIdx.x] = (unsigned long long)acc;
    s_hi[threadIdx.x] = (unsigned long long)(acc >> 64);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned __int128 sum = 0;
        for (int i = 0; i < 256; ++i) sum += ((unsigned __int128)s_hi[i] << 64) | s_lo[i];
        out[2 * blockIdx.x] = (unsigned long long)sum;
        out[2 * blockIdx.x + 1] = (unsigned long long)(sum >> 64);
    }
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------------------

struct LpOptions {
    int64_t group_row, wave_row, lds_row, wg_work;
    int32_t lds_slots;
    bool active;
};

LpOptions lp_options() {
    LpOptions o;
    o.wave_row = std::max<long long>(0, std::min<long long>(opt_int("LP_WAVE_ROW", kLpWaveRowDefault), 64));
    o.group_row = std::min<int64_t>(16, o.wave_row);
    int lg = 4;  // at least 16 slots, a power of two, at most kLpSlotsMax
    const long long slots = std::max<long long>(16, std::min<long long>(opt_int("LP_LDS_SLOTS", kLpLdsSlotsDefault), kLpSlotsMax));
    while ((2ll << lg) <= slots) ++lg;
    o.lds_slots = 1 << lg;
    o.lds_row = std::max<long long>(o.wave_row, std::min<long long>(opt_int("LP_LDS_ROW", kLpLdsRowDefault), o.lds_slots));
    if (opt_int("LP_LDS_ROW", kLpLdsRowDefault) <= 0) o.lds_row = o.wave_row;  // no medium rows
    o.wg_work = std::max<long long>(0, std::min<long long>(opt_int("LP_WG_WORK", kLpWgWorkDefault), LLONG_MAX / 4));
    o.active = opt_int("LP_ACTIVE", kLpActiveDefault) != 0;
    return o;
}

// the classes of a colouring (or of none: one class), on the device and, the offsets and entries, on the host
struct LpClasses {
    DevBuf vtx, off, slab_keys, slab_wts;
    std::vector<int64_t> h_off;             // [4 C + 1]
    std::vector<unsigned long long> h_work;  // [C] entries of the class
    int64_t region_slots = 2, regions = 1;
};

int lp_build_classes(const gmsx_graph *g, const int32_t *color, int32_t colors, const LpOptions &o, LpCtrl *ctrl, LpClasses &cl, int *launches) {
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int64_t n = g->n, keys = int64_t(colors) * kLpBins;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    DevBuf d_cnt, d_work;
    if (int rc = dalloc<unsigned long long>(d_cnt, 2 * (keys + 1))) return rc;  // the counts, then the cursors
    if (int rc = dalloc<unsigned long long>(d_work, colors)) return rc;
    if (int rc = dalloc<int64_t>(cl.off, keys + 1)) return rc;
    if (int rc = dalloc<int32_t>(cl.vtx, n)) return rc;
    GMSX_HIP(hipMemsetAsync(d_cnt.p, 0, size_t(2 * (keys + 1)) * sizeof(unsigned long long), s));
    GMSX_HIP(hipMemsetAsync(d_work.p, 0, size_t(colors) * sizeof(unsigned long long), s));
    const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16)));
    hipLaunchKernelGGL(k_lp_hist, dim3(grid), dim3(256), 0, s, n, g->off, color, colors, o.group_row, o.wave_row, o.lds_row, d_cnt.as<unsigned long long>(),
                       d_work.as<unsigned long long>(), ctrl);
    if (int rc = exclusive_scan_i64(d_cnt.as<const int64_t>(), cl.off.as<int64_t>(), keys + 1, s)) return rc;
    hipLaunchKernelGGL(k_lp_place, dim3(grid), dim3(256), 0, s, n, g->off, color, colors, o.group_row, o.wave_row, o.lds_row, cl.off.as<const int64_t>(),
                       d_cnt.as<unsigned long long>() + keys + 1, cl.vtx.as<int32_t>(), n, ctrl);
    *launches += 3;
    cl.h_off.assign(size_t(keys + 1), 0);
    cl.h_work.assign(size_t(colors), 0);
    LpCtrl h;
    GMSX_HIP(hipMemcpyAsync(cl.h_off.data(), cl.off.p, size_t(keys + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(cl.h_work.data(), d_work.p, size_t(colors) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (h.error || cl.h_off[0] != 0 || cl.h_off[size_t(keys)] > n || h.max_long > (unsigned long long)g->nnz) return GMSX_ERR_KERNEL;
    for (int64_t k = 0; k < keys; ++k)
        if (cl.h_off[size_t(k)] > cl.h_off[size_t(k + 1)]) return GMSX_ERR_KERNEL;
    // the slab: a region holds the table of the longest row; as many regions as the budget allows, one at the least
    cl.region_slots = int64_t(1) << lp_log2_slots(std::max<int64_t>(1, int64_t(h.max_long)));
    int64_t most_long = 0;
    for (int32_t k = 0; k < colors; ++k) most_long = std::max(most_long, cl.h_off[size_t(k) * kLpBins + 4] - cl.h_off[size_t(k) * kLpBins + 3]);
    cl.regions = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(most_long, int64_t(cus) * 4), kLpSlabBytes / (cl.region_slots * 12)));
    if (most_long > 0) {  // every slot empty: key -1, weight 0 (a pick wipes what it read)
        if (int rc = dalloc<int32_t>(cl.slab_keys, cl.regions * cl.region_slots)) return rc;
        if (int rc = dalloc<unsigned long long>(cl.slab_wts, cl.regions * cl.region_slots)) return rc;
        GMSX_HIP(hipMemsetAsync(cl.slab_keys.p, 0xff, size_t(cl.regions * cl.region_slots) * sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(cl.slab_wts.p, 0, size_t(cl.regions * cl.region_slots) * sizeof(unsigned long long), s));
    }
    return GMSX_OK;
}

// under the option TIMING every launch is waited for and its wall time goes to the words of its kind: [0 … 3] the bins, [4] the one-workgroup launches
struct LpLaunchTimer {
    double *ms;
    int kind;
    std::chrono::steady_clock::time_point t0;
    LpLaunchTimer(double *ms_, int kind_) : ms(ms_), kind(kind_) {
        if (!ms) return;
        (void)hipStreamSynchronize(ctx().stream);
        t0 = std::chrono::steady_clock::now();
    }
    ~LpLaunchTimer() {
        if (!ms) return;
        (void)hipStreamSynchronize(ctx().stream);
        ms[kind] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

// the launches of class c (1-based), bin by bin (a class that turns out clean costs its launches only: every workgroup leaves at the class word)
template <bool WRITE>
void lp_launch_class(const LpArgs &a, const LpClasses &cl, int32_t c, int *launches, double *ms = nullptr) {
    Ctx &x = ctx();
    const int cus = x.compute_units > 0 ? x.compute_units : 256;
    const int64_t *o = cl.h_off.data() + size_t(c - 1) * kLpBins;
    const int64_t cap = int64_t(cus) * 8;
    const int64_t cnt[4] = {o[1] - o[0], o[2] - o[1], o[3] - o[2], o[4] - o[3]};
    const int64_t want[4] = {(cnt[0] * 16 + kLpThreads - 1) / kLpThreads, (cnt[1] * 64 + kLpThreads - 1) / kLpThreads, cnt[2], cnt[3]};
    for (int b = 0; b < 3; ++b) {
        if (cnt[b] <= 0) continue;
        const unsigned grid = unsigned(std::max<int64_t>(1, std::min<int64_t>(want[b], cap)));
        const LpLaunchTimer timer(ms, b);
        if (b == 0) hipLaunchKernelGGL((k_lp_bin<0, WRITE>), dim3(grid), dim3(kLpThreads), 0, x.stream, a, o[0], cnt[0], c);
        if (b == 1) hipLaunchKernelGGL((k_lp_bin<1, WRITE>), dim3(grid), dim3(kLpThreads), 0, x.stream, a, o[1], cnt[1], c);
        if (b == 2) hipLaunchKernelGGL((k_lp_bin<2, WRITE>), dim3(grid), dim3(kLpThreads), 0, x.stream, a, o[2], cnt[2], c);
        ++*launches;
    }
    // the long rows, as many at a time as the slab has regions; the parts of a row: so that the launch fills the device a few times over
    for (int64_t r0 = 0; r0 < cnt[3]; r0 += cl.regions) {
        const int64_t rows = std::min<int64_t>(cl.regions, cnt[3] - r0);
        const unsigned parts = unsigned(std::max<int64_t>(1, std::min<int64_t>(kLpLongParts, (int64_t(cus) * 4) / rows)));
        const LpLaunchTimer timer(ms, 3);
        hipLaunchKernelGGL((k_lp_long_fill<WRITE>), dim3(parts, unsigned(rows)), dim3(kLpThreads), 0, x.stream, a, o[3] + r0, c);
        hipLaunchKernelGGL((k_lp_long_pick<WRITE>), dim3(unsigned(rows)), dim3(kLpThreads), 0, x.stream, a, o[3] + r0, c);
        *launches += 2;
    }
}

// communities, singletons, the largest community and its smallest label from the labels on the device (size: n zeroed words)
int lp_info_pass(int64_t n, const int32_t *label, int32_t *size, LpCtrl *ctrl, int *launches) {
    Ctx &c = ctx();
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const unsigned per_vertex = unsigned((n + 255) / 256);
    const unsigned sweep = unsigned(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16)));
    GMSX_HIP(hipMemsetAsync(size, 0, size_t(n) * sizeof(int32_t), c.stream));
    hipLaunchKernelGGL(k_lp_sizes, dim3(per_vertex), dim3(256), 0, c.stream, n, label, size);
    hipLaunchKernelGGL(k_lp_info, dim3(sweep), dim3(256), 0, c.stream, n, size, ctrl);
    *launches += 2;
    return GMSX_OK;
}

int label_propagation(const gmsx_graph *g, uint32_t flags, const int32_t *coloring, int32_t max_sweeps, int32_t *label, gmsx_lp_info *info,
                      gmsx_stats *stats) {
    gmsx_lp_info res;
    std::memset(&res, 0, sizeof res);
    const int64_t n = g->n;
    if (n == 0) {
        *info = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const LpOptions o = lp_options();
    const bool timing = opt_on("TIMING");  // one line per sweep on stderr: its changes, rows, arcs and launches, and the wall time of every kind of launch
    const int32_t cap = max_sweeps == 0 ? kLpSweepCap : max_sweeps;
    int launches = 0, color_launches = 0;
    // ---- the colouring: the caller's, checked on the device, or Jones–Plassmann's under the id order, left on the device
    DevBuf d_color, d_round, d_label, d_dirty, d_flags, d_ctrl, d_size;
    int32_t colors = 0;
    if (coloring) {
        if (int rc = dalloc<int32_t>(d_color, n)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_color.p, coloring, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        unsigned long long acc[8];
        int32_t ctl[4];
        float ms = 0.f;
        if (int rc = coloring_verify_device(g, d_color.as<const int32_t>(), acc, ctl, &ms)) return rc;
        if (ctl[1]) return GMSX_ERR_KERNEL;
        // (the verifier's words: [0] arcs between equal colours, [1] colours below 1, [2] the largest colour + 2^31)
        const int64_t top = int64_t(acc[2]) - (1ll << 31);
        if (acc[0] || acc[1] || top < 1 || top > n) return GMSX_ERR_INVALID;  // (a colour above n names more classes than vertices)
        colors = int32_t(top);
        color_launches = 3;
    } else {
        gmsx_coloring_info ci;
        std::memset(&ci, 0, sizeof ci);
        if (int rc = coloring_jp_device(g, nullptr, 0, d_color, d_round, ci, &color_launches)) return rc;
        d_round.reset();
        colors = ci.colors;
    }
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_label, n)) return rc;
    if (int rc = dalloc<uint8_t>(d_dirty, n)) return rc;
    if (int rc = dalloc<int32_t>(d_flags, 2 * (int64_t(colors) + 1))) return rc;
    if (int rc = dalloc<LpCtrl>(d_ctrl, 1)) return rc;
    if (int rc = dalloc<int32_t>(d_size, n)) return rc;
    LpCtrl *ctrl = d_ctrl.as<LpCtrl>();
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(LpCtrl), s));
    LpClasses cl;
    if (int rc = lp_build_classes(g, d_color.as<const int32_t>(), colors, o, ctrl, cl, &launches)) return rc;
    const size_t flag_words = size_t(colors) + 1;
    std::vector<int32_t> h_flags(2 * flag_words, 1);  // sweep 1 evaluates every class
    GMSX_HIP(hipMemsetAsync(d_flags.p, 0, 2 * flag_words * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_lp_init, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, n, d_label.as<int32_t>(), d_dirty.as<uint8_t>());
    ++launches;
    LpArgs a;
    a.off = g->off, a.adj = g->adj, a.wgt = (flags & GMSX_LP_WEIGHTED) ? g->wgt.as<const int32_t>() : nullptr;
    a.label = d_label.as<int32_t>(), a.dirty = d_dirty.as<uint8_t>(), a.color = d_color.as<const int32_t>(), a.flags = d_flags.as<int32_t>();
    a.vtx = cl.vtx.as<const int32_t>(), a.keys = cl.slab_keys.as<int32_t>(), a.wts = cl.slab_wts.as<unsigned long long>(), a.deg = nullptr, a.ctrl = ctrl;
    a.region_slots = cl.region_slots, a.lds_slots = o.lds_slots, a.colors = colors, a.par = 1, a.active = o.active ? 1 : 0, a.obey = 0;
    // ---- the sweeps
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    LpCtrl h;
    std::memset(&h, 0, sizeof h);
    unsigned long long rows_all = 0, arcs_all = 0;
    for (int32_t sweep = 1; sweep <= cap; ++sweep) {
        const int par = sweep & 1;
        const bool obey = o.active && sweep > 1;  // sweep 1 evaluates every vertex: no byte is read
        a.par = par;
        a.obey = obey ? 1 : 0;
        const int32_t *mark = h_flags.data() + size_t(par) * flag_words;
        const int before = launches;
        double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        const auto sweep_t0 = std::chrono::steady_clock::now();
        bool ran = false;
        for (int32_t k = 1; k <= colors;) {
            const int64_t *ko = cl.h_off.data() + size_t(k - 1) * kLpBins;
            if (ko[4] == ko[0] || (obey && !ran && !mark[k])) {  // no vertex, or clean with nothing in front of it that could dirty it
                ++k;
                continue;
            }
            // what the class weighs: its entries and its vertices, whether it is marked or not (an unmarked class may be dirtied before its turn)
            auto weight = [&](int32_t q) -> unsigned long long {
                return cl.h_work[size_t(q - 1)] + (unsigned long long)(cl.h_off[size_t(q) * kLpBins] - cl.h_off[size_t(q - 1) * kLpBins]);
            };
            unsigned long long sum = weight(k);
            if (o.wg_work > 0 && sum <= (unsigned long long)o.wg_work) {
                int32_t last = k;
                while (last < colors && sum + weight(last + 1) <= (unsigned long long)o.wg_work) sum += weight(++last);
                {
                    const LpLaunchTimer timer(timing ? ms : nullptr, 4);
                    hipLaunchKernelGGL(k_lp_tiny, dim3(1), dim3(kLpThreads), 0, s, a, cl.off.as<const int64_t>(), k, last);
                }
                ++launches;
                k = last + 1;
            } else {
                lp_launch_class<true>(a, cl, k, &launches, timing ? ms : nullptr);
                ++k;
            }
            ran = true;
        }
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(h_flags.data(), d_flags.p, 2 * flag_words * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemsetAsync(a.flags + size_t(par) * flag_words, 0, flag_words * sizeof(int32_t), s));  // this sweep's words are used up
        GMSX_HIP(hipMemsetAsync(&ctrl->changed, 0, 3 * sizeof(unsigned long long), s));                     // changed, rows, arcs
        GMSX_HIP(hipStreamSynchronize(s));
        GMSX_HIP(hipGetLastError());
        if (h.error || h.changed > (unsigned long long)n) return GMSX_ERR_KERNEL;
        if (timing)
            std::fprintf(stderr, "[gmsx communities] sweep %d: %llu changes, %llu rows, %llu arcs, %d launches, %.3f ms (every launch waited for: bins %.3f %.3f %.3f %.3f, one workgroup %.3f)\n",
                         int(sweep), h.changed, h.rows, h.arcs, launches - before,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - sweep_t0).count(), ms[0], ms[1], ms[2], ms[3], ms[4]);
        rows_all += h.rows;
        arcs_all += h.arcs;
        res.sweeps = sweep;
        res.changes += int64_t(h.changed);
        if (sweep == 1) res.first_sweep_changes = int64_t(h.changed);
        if (h.changed == 0) {
            res.converged = 1;
            break;
        }
    }
    // ---- the info reduction
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    if (int rc = lp_info_pass(n, a.label, d_size.as<int32_t>(), ctrl, &launches)) return rc;
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    const unsigned long long big = h.largest >> 32;
    if (h.error || h.communities < 1 || h.communities > (unsigned long long)n || big < 1 || big > (unsigned long long)n) return GMSX_ERR_KERNEL;
    res.communities = int64_t(h.communities);
    res.singletons = int64_t(h.singletons);
    res.largest = int64_t(big);
    res.largest_label = int32_t(~uint32_t(h.largest));
    res.colors = colors;
    // the flag word was read as zero: the caller's array is written now, through host staging
    std::vector<int32_t> h_label;
    if (label) {
        h_label.resize(size_t(n));
        GMSX_HIP(hipMemcpy(h_label.data(), a.label, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    float up_ms = 0.f, ms = 0.f, info_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&info_ms, c.ev[2], c.ev[3]));
    if (label) std::memcpy(label, h_label.data(), size_t(n) * sizeof(int32_t));
    *info = res;
    if (stats) *stats = gmsx_stats{double(ms), double(up_ms) + double(info_ms), rows_all, arcs_all, uint64_t(res.sweeps), launches + color_launches, 0, 0};
    return GMSX_OK;
}

int modularity(const gmsx_graph *g, uint32_t flags, const int32_t *label, gmsx_modularity_info *info, gmsx_stats *stats) {
    gmsx_modularity_info res;
    std::memset(&res, 0, sizeof res);
    const int64_t n = g->n;
    if (n == 0) {
        *info = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    const LpOptions o = lp_options();
    int launches = 0;
    const unsigned blocks = unsigned(std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, int64_t(cus) * 4)));
    DevBuf d_label, d_ctrl, d_size, d_deg, d_part;
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_label, n)) return rc;
    if (int rc = dalloc<LpCtrl>(d_ctrl, 1)) return rc;
    if (int rc = dalloc<int32_t>(d_size, n)) return rc;
    if (int rc = dalloc<unsigned long long>(d_deg, n)) return rc;
    if (int rc = dalloc<unsigned long long>(d_part, 2 * int64_t(blocks))) return rc;
    LpCtrl *ctrl = d_ctrl.as<LpCtrl>();
    GMSX_HIP(hipMemcpyAsync(d_label.p, label, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(LpCtrl), s));
    GMSX_HIP(hipMemsetAsync(d_deg.p, 0, size_t(n) * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_lp_check_labels, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, n, d_label.as<const int32_t>(), ctrl);
    ++launches;
    LpCtrl h;
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (h.bad) return GMSX_ERR_INVALID;
    LpClasses cl;
    if (int rc = lp_build_classes(g, nullptr, 1, o, ctrl, cl, &launches)) return rc;
    LpArgs a;
    a.off = g->off, a.adj = g->adj, a.wgt = (flags & GMSX_LP_WEIGHTED) ? g->wgt.as<const int32_t>() : nullptr;
    a.label = d_label.as<int32_t>(), a.dirty = nullptr, a.color = nullptr, a.flags = nullptr;
    a.vtx = cl.vtx.as<const int32_t>(), a.keys = cl.slab_keys.as<int32_t>(), a.wts = cl.slab_wts.as<unsigned long long>();
    a.deg = d_deg.as<unsigned long long>(), a.ctrl = ctrl;
    a.region_slots = cl.region_slots, a.lds_slots = o.lds_slots, a.colors = 1, a.par = 0, a.active = 0, a.obey = 0;
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    lp_launch_class<false>(a, cl, 1, &launches);
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    if (int rc = lp_info_pass(n, a.label, d_size.as<int32_t>(), ctrl, &launches)) return rc;
    hipLaunchKernelGGL(k_lp_sumsq, dim3(blocks), dim3(256), 0, s, n, d_deg.as<const unsigned long long>(), d_part.as<unsigned long long>());
    ++launches;
    std::vector<unsigned long long> part(2 * size_t(blocks));
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(part.data(), d_part.p, part.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    const unsigned long long big = h.largest >> 32;
    if (h.error || h.communities < 1 || h.communities > (unsigned long long)n || big < 1 || big > (unsigned long long)n || h.intra > h.total ||
        h.total > (unsigned long long)LLONG_MAX)
        return GMSX_ERR_KERNEL;
    unsigned __int128 sumsq = 0;
    for (size_t b = 0; b < size_t(blocks); ++b) sumsq += ((unsigned __int128)part[2 * b + 1] << 64) | part[2 * b];
    if (sumsq > (unsigned __int128)h.total * h.total) return GMSX_ERR_KERNEL;  // (Σ D_c² <= (Σ D_c)²)
    res.total_weight = int64_t(h.total);
    res.intra_weight = int64_t(h.intra);
    res.sumsq_hi = uint64_t(sumsq >> 64);
    res.sumsq_lo = uint64_t(sumsq);
    res.communities = int64_t(h.communities);
    res.largest = int64_t(big);
    res.unstable = int64_t(h.unstable);
    if (h.total > 0) {  // THE fixed expression (gmsx.h): three long doubles, one subtraction, rounded to double once
        const long double w = (long double)res.total_weight;
        const long double sq = (long double)res.sumsq_hi * 18446744073709551616.0L + (long double)res.sumsq_lo;
        res.modularity = double((long double)res.intra_weight / w - sq / (w * w));
    }
    float up_ms = 0.f, ms = 0.f, info_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&info_ms, c.ev[2], c.ev[3]));
    *info = res;
    if (stats) *stats = gmsx_stats{double(ms), double(up_ms) + double(info_ms), uint64_t(h.rows), uint64_t(h.arcs), 0, launches, 0, 0};
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_label_propagation(const gmsx_graph *g, uint32_t flags, const int32_t *coloring, int32_t max_sweeps, int32_t *label, gmsx_lp_info *info,
                           gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || (flags & ~uint32_t(GMSX_LP_WEIGHTED)) || max_sweeps < 0) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        if ((flags & GMSX_LP_WEIGHTED) && !g->wgt.p) return GMSX_ERR_INVALID;
        return label_propagation(g, flags, coloring, max_sweeps, label, info, stats);
    });
}

int gmsx_modularity(const gmsx_graph *g, uint32_t flags, const int32_t *label, gmsx_modularity_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || (flags & ~uint32_t(GMSX_LP_WEIGHTED))) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        if (((flags & GMSX_LP_WEIGHTED) && !g->wgt.p) || (g->n > 0 && !label)) return GMSX_ERR_INVALID;
        return modularity(g, flags, label, info, stats);
    });
}

}  // extern "C"
