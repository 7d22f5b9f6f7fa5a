// Greedy (weighted) matching and its verifier on gfx950 over the uploaded CSR: the locally dominant rounds (Preis; Manne, Bisseling).
//   gmsx_greedy_matching   mate[v], the pairs ascending by u with their weights, and the info block; no reference counterpart.
//   gmsx_matching_verify   the six integers of gmsx_matching_check for any mate array: invalid == 0 && undominated == 0 iff it is THE matching.
// The definitions are those of include/gmsx.h.
//
// THE ORDER.  key(e) = (heavier w first, h(lo, hi), lo, hi) for e = {lo, hi}, lo < hi; h = match_mix, a fixed 32-bit mixer; without
// GMSX_MATCH_WEIGHTED every w is 1.  On the device the weight travels as k0 = ~w (0 when unweighted), an unsigned word of which the smaller
// one comes first, and k0 << 32 | h is one 64-bit word; ~0 is no arc (weights lie in [1, 2^31 - 1]).  The order is strict, so the greedy
// matching — take the edges in the order, keep an edge iff both ends are free — is unique, and the rounds below give it.
// INSIDE ONE ROW (lo, hi) ascends with x for the arcs v - x of a fixed v, as in msf.hip, so the first free arc of v's row is the minimum of
// (k0 << 32 | h, x).  Two arcs of one row can share h (one to a smaller, one to a larger neighbour), so x does decide: the row minimum is a
// wave_min_all of the 64-bit word and a wave_min of x over the lanes that hold it (wave_ops.hpp).
//
// A ROUND is two steps with a kernel boundary between them; nothing spins and no workgroup waits for another.  The live lists hold every free
// vertex that may still have a free neighbour.
//   (a) search   MatchSearch, THE HOT PASS: every listed v finds cand[v] = the other end of the first arc of its row in the order whose other
//                end is free (mate[x] < 0, plain loads: the pair pass of the round before wrote it; the weight is loaded for free ends
//                only), or -1.  It is the Op of row_classes.hpp's live-list row pass: a lane, a 16-lane group, a wave or a workgroup per
//                row by its length (the bounds are MATCH_WAVE_ROW and MATCH_WG_ROW) — no lane walks a long row alone.  cand[v] and
//                candw[v] (the arc's weight) have one writer.  Under MATCH_KEEP = 1 a vertex whose candidate of the last
//                round is still free keeps it without walking its row: mates only appear, so its first free arc cannot have changed.
//   (b) pair     k_match_pair: mate[v] = cand[v] where cand[cand[v]] == v — every vertex writes its own word only, and the kernel reads
//                cand, which it does not write.  A vertex without a candidate is dead for good (matched vertices stay matched) and a paired
//                one is done: neither is appended to the next live lists; the others are (wave_append: bounds-checked).
// The first live edge in the order is mutual, so a round with a live edge pairs at least one: the host loop ends at empty lists, a round
// without pairs that leaves a vertex listed is GMSX_ERR_KERNEL, and so are more than n / 2 + 1 rounds.  The set paired in round r is the
// set of locally dominant edges among the live ones — a fact about (graph, weights, flags), and `rounds` with it.  Under the option TIMING
// every round prints its listed vertices, the arcs it examined and its pairs.
//
// AFTER THE ROUNDS.  k_match_info: per vertex the mark mate[v] > v, Σ w, min w, max w over the marked, the matched and the exposed vertices,
// and mate[mate[v]] == v; a scan of the marks; k_match_fill: pair i of the scan goes to slot i, so the list ascends by u without a sort.
// The host checks 2 * pairs == matched before anything is written.
// STATE: mate, cand, candw, the live lists (2 x their capacities, at most 4 n + 6 entries) as 32-bit words, the marks and their scan as 64-bit
// words, up to 3 (n / 2) words of pairs — O(n) words, DevBufs of the call.  The verifier: mate, the valid mate and a key word per vertex.
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // wave_append
#include "row_classes.hpp"
#include "union_find.hpp"       // cc_find_in_row

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>

namespace gmsx {

namespace {

constexpr long long kMatchKeepDefault = 1;
constexpr unsigned long long kNoKey = ~0ull;

// the call's small device block, mirrored to the host after every round
struct MatchCtrl {
    int32_t error;        // the flag word: an append hit its bound
    int32_t took;         // vertices that took a mate this round: two per pair
    int32_t count[2][4];  // vertices in the lane / group / wave / workgroup list of either buffer (row_classes.hpp)
    unsigned long long examined;  // arcs the search pass looked at
};

// the info pass's words
struct MatchAcc {
    int32_t error, pad;
    unsigned long long matched, upper;  // vertices with a mate / with a mate of a larger id
    unsigned long long weight;          // Σ w over the upper ones
    unsigned long long exposed;         // free vertices with an arc
    uint32_t wmin, wmax;
};

// the verifier's words
struct MatchCheckAcc {
    unsigned long long invalid, pairs, weight, augmentable, undominated;
};

// h(lo, hi) of gmsx.h
__host__ __device__ __forceinline__ uint32_t match_mix(uint32_t lo, uint32_t hi) {
    uint32_t h = lo * 0x9E3779B1u + hi;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// k0 << 32 | h of the arc v - x; k0 = ~w, or 0 when unweighted
__device__ __forceinline__ unsigned long long match_key(int32_t v, int32_t x, uint32_t k0) {
    return ((unsigned long long)k0 << 32) | match_mix(uint32_t(min(v, x)), uint32_t(max(v, x)));
}

__global__ void k_match_init(int64_t n, int32_t *__restrict__ mate, int32_t *__restrict__ cand) {
    const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (v < n) {
        mate[v] = -1;
        cand[v] = -1;
    }
}

// (a) THE HOT PASS, the Op of a live-list row pass: WIDTH lanes (1, kGroup, 64, or the 256 threads of the workgroup) per listed row.
// wgt == nullptr: unit weights (k0 = 0).  keep: a candidate that is still free stands.
struct MatchSearch {
    const int64_t *off;
    const int32_t *adj, *wgt, *mate;
    int keep;
    int32_t *cand, *candw;
    template <int WIDTH>
    __device__ __forceinline__ unsigned long long row(int32_t v, bool active, int lane) const {
        constexpr int kLanes = WIDTH > 64 ? 64 : WIDTH;  // lanes of one wave that share a row
        __shared__ unsigned long long s_key[4];
        __shared__ uint32_t s_x[4];
        unsigned long long examined = 0;
        bool walk = active;
        if (active && keep) {  // (the lanes of a row read the same two words)
            const int32_t c = cand[v];
            if (c >= 0 && mate[c] < 0) walk = false;
        }
        const int64_t j1 = walk ? off[v + 1] : 0;
        unsigned long long mine = kNoKey;
        uint32_t mine_x = ~0u;
        for (int64_t j = walk ? off[v] + lane : 0; j < j1; j += WIDTH) {
            ++examined;
            const int32_t x = adj[j];
            if (x == v || mate[x] >= 0) continue;
            const unsigned long long k = match_key(v, x, wgt ? ~uint32_t(wgt[j]) : 0u);
            if (k < mine || (k == mine && uint32_t(x) < mine_x)) {
                mine = k;
                mine_x = uint32_t(x);
            }
        }
        unsigned long long best = wave_min_all<kLanes>(mine);
        uint32_t best_x = wave_min<kLanes>(mine == best ? mine_x : ~0u);
        if (WIDTH > 64) {
            if ((threadIdx.x & 63) == 0) {
                s_key[threadIdx.x >> 6] = best;
                s_x[threadIdx.x >> 6] = best_x;
            }
            __syncthreads();
            if (threadIdx.x == 0)
                for (int w = 1; w < 4; ++w)
                    if (s_key[w] < best || (s_key[w] == best && s_x[w] < best_x)) {
                        best = s_key[w];
                        best_x = s_x[w];
                    }
            __syncthreads();
        }
        if (walk && lane == 0) {  // the row's one writer
            cand[v] = best != kNoKey ? int32_t(best_x) : -1;
            candw[v] = wgt ? int32_t(~uint32_t(best >> 32)) : 1;
        }
        return examined;
    }
};

// (b) mutual candidates become mates; whoever still has a candidate goes to the next list of its class
__global__ __launch_bounds__(256) void k_match_pair(RowLists l, int cur, const int32_t *__restrict__ cand, int32_t *__restrict__ mate,
                                                    MatchCtrl *__restrict__ ctrl) {
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    int32_t took = 0;
    for (int b = 0; b < 4; ++b) {
        const int32_t *list = l.list(cur, b);
        const int64_t rows = l.rows(ctrl->count[cur], b);
        const int64_t end = ((rows + 63) / 64) * 64;  // whole waves stay converged for the ballot
        for (int64_t i = tid; i < end; i += stride) {
            bool stay = false;
            int32_t v = 0;
            if (i < rows) {
                v = list[i];
                const int32_t c = cand[v];
                if (c >= 0) {
                    if (cand[c] == v) {
                        mate[v] = c;
                        ++took;
                    } else {
                        stay = true;
                    }
                }
            }
            wave_append(stay, v, l.list(cur ^ 1, b), &ctrl->count[cur ^ 1][b], l.cap[b], &ctrl->error);
        }
    }
    took = wave_sum(took);  // (at most n in all)
    if ((threadIdx.x & 63) == 0 && took) atomicAdd(&ctrl->took, took);
}

// per vertex the mark mate[v] > v into cnt[v]; the matched, the exposed, Σ w, min w, max w; a mate whose mate is someone else raises the flag
__global__ __launch_bounds__(256) void k_match_info(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ mate,
                                                    const int32_t *__restrict__ candw, int64_t *__restrict__ cnt, MatchAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long matched = 0, upper = 0, weight = 0, exposed = 0;
    uint32_t wmin = ~0u, wmax = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t m = mate[v];
        cnt[v] = m > v ? 1 : 0;
        if (m < 0) {
            exposed += off[v + 1] > off[v];
            continue;
        }
        ++matched;
        if (m >= n || m == v || mate[m] != int32_t(v) || candw[m] != candw[v]) {
            acc->error = 1;
            continue;
        }
        if (m > v) {
            const uint32_t w = uint32_t(candw[v]);
            ++upper;
            weight += w;
            wmin = min(wmin, w);
            wmax = max(wmax, w);
        }
    }
    matched = wave_sum(matched);
    upper = wave_sum(upper);
    weight = wave_sum(weight);
    exposed = wave_sum(exposed);
    wmin = wave_min(wmin);
    wmax = wave_max(wmax);
    if ((threadIdx.x & 63) == 0) {
        if (matched) atomicAdd(&acc->matched, matched);
        if (exposed) atomicAdd(&acc->exposed, exposed);
        if (upper) {
            atomicAdd(&acc->upper, upper);
            atomicAdd(&acc->weight, weight);
            atomicMin(&acc->wmin, wmin);
            atomicMax(&acc->wmax, wmax);
        }
    }
}

// the pair of every marked vertex to the slot its scan gives: ascending by u
__global__ __launch_bounds__(256) void k_match_fill(int64_t n, const int32_t *__restrict__ mate, const int32_t *__restrict__ candw,
                                                    const int64_t *__restrict__ pos, int64_t cap, int32_t *__restrict__ eu, int32_t *__restrict__ ev,
                                                    int32_t *__restrict__ ew, MatchAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t m = mate[v];
        if (m <= v) continue;
        const int64_t p = pos[v];
        if (p >= 0 && p < cap) {
            eu[p] = int32_t(v);
            ev[p] = m;
            ew[p] = candw[v];
        } else {
            acc->error = 1;
        }
    }
}

// the verifier, per vertex: eff[v] = mate[v] if it is valid (in range, a neighbour, mutual), else -1; vkey[v] = k0 << 32 | h of that edge
__global__ __launch_bounds__(256) void k_match_valid(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                     const int32_t *__restrict__ wgt, const int32_t *__restrict__ mate, int32_t *__restrict__ eff,
                                                     unsigned long long *__restrict__ vkey, MatchCheckAcc *__restrict__ acc) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    unsigned long long invalid = 0, pairs = 0, weight = 0;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t m = mate[v];
        int32_t e = -1;
        unsigned long long key = kNoKey;
        if (m != -1) {
            int64_t j = -1;
            if (m >= 0 && m < n && m != v && mate[m] == int32_t(v)) j = cc_find_in_row(adj, off[v], off[v + 1], m);
            if (j >= 0) {
                const uint32_t w = wgt ? uint32_t(wgt[j]) : 1u;
                e = m;
                key = match_key(int32_t(v), m, wgt ? ~w : 0u);
                if (m > v) {
                    ++pairs;
                    weight += w;
                }
            } else {
                ++invalid;
            }
        }
        eff[v] = e;
        vkey[v] = key;
    }
    invalid = wave_sum(invalid);
    pairs = wave_sum(pairs);
    weight = wave_sum(weight);
    if ((threadIdx.x & 63) == 0) {
        if (invalid) atomicAdd(&acc->invalid, invalid);
        if (pairs) {
            atomicAdd(&acc->pairs, pairs);
            atomicAdd(&acc->weight, weight);
        }
    }
}

// is the matching edge of a (its key word ka, its other end ma) earlier in the order than the edge {u, x}, u < x, of key word k?
__device__ __forceinline__ bool match_earlier(unsigned long long ka, int32_t a, int32_t ma, unsigned long long k, int32_t u, int32_t x) {
    if (ka != k) return ka < k;
    const int32_t lo = min(a, ma), hi = max(a, ma);
    return lo != u ? lo < u : hi < x;
}

// the verifier, per edge u < x that is not in the (valid) matching: both ends free = augmentable; no adjacent matching edge earlier in the
// order = undominated.  An Op of row_classes.hpp's two-width pass
struct MatchCheck {
    const int32_t *adj, *wgt, *eff;
    const unsigned long long *vkey;
    MatchCheckAcc *acc;
    unsigned long long augmentable = 0, undominated = 0;  // this thread's sums: begin() sets them
    __device__ __forceinline__ void begin() { augmentable = undominated = 0; }
    template <int>
    __device__ __forceinline__ unsigned long long row(int32_t u, int64_t j0, int64_t j1, int lane, int width) {
        const int32_t mu = eff[u];
        const unsigned long long ku = vkey[u];
        for (int64_t j = j0 + lane; j < j1; j += width) {
            const int32_t x = adj[j];
            if (x <= u || x == mu) continue;
            const int32_t mx = eff[x];
            if (mu < 0 && mx < 0) {
                ++augmentable;
                ++undominated;
                continue;
            }
            const unsigned long long k = match_key(u, x, wgt ? ~uint32_t(wgt[j]) : 0u);
            const bool dominated = (mu >= 0 && match_earlier(ku, u, mu, k, u, x)) || (mx >= 0 && match_earlier(vkey[x], x, mx, k, u, x));
            undominated += !dominated;
        }
        return 0;
    }
    __device__ __forceinline__ void finish() {
        augmentable = wave_sum(augmentable);
        undominated = wave_sum(undominated);
        if ((threadIdx.x & 63) == 0 && undominated) {
            atomicAdd(&acc->augmentable, augmentable);
            atomicAdd(&acc->undominated, undominated);
        }
    }
};

int matching(const gmsx_graph *g, uint32_t flags, int32_t *mate_out, int32_t *edge_u, int32_t *edge_v, int32_t *edge_w, gmsx_matching_info *info,
             gmsx_stats *stats) {
    gmsx_matching_info res;
    std::memset(&res, 0, sizeof res);
    const int64_t n = g->n, nnz = g->nnz;
    if (n == 0 || nnz == 0) {  // every vertex is free
        res.free_vertices = n;
        for (int64_t v = 0; mate_out && v < n; ++v) mate_out[v] = -1;
        *info = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    // test hooks, first guesses
    const RowBounds bounds = row_bounds("MATCH_WAVE_ROW", "MATCH_WG_ROW");
    const int keep = opt_int("MATCH_KEEP", kMatchKeepDefault) != 0 ? 1 : 0;
    const bool timing = opt_on("TIMING");  // one line per round on stderr: its listed vertices, the arcs it examined, its pairs
    const bool want_edges = edge_u != nullptr;
    const int64_t room = std::max<int64_t>(n / 2, 1);
    RowListStore lists;
    // ---- setup: the buffers
    DevBuf d_mate, d_cand, d_candw, d_ctrl, d_acc, d_cnt, d_pos, d_eu, d_ev, d_ew;
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_mate, n)) return rc;
    if (int rc = dalloc<int32_t>(d_cand, n)) return rc;
    if (int rc = dalloc<int32_t>(d_candw, n)) return rc;
    if (int rc = lists.alloc(n, nnz, bounds, true, true)) return rc;
    if (int rc = dalloc<MatchCtrl>(d_ctrl, 1)) return rc;
    if (int rc = dalloc<MatchAcc>(d_acc, 1)) return rc;
    if (int rc = dalloc<int64_t>(d_cnt, n + 1)) return rc;
    if (want_edges) {
        if (int rc = dalloc<int64_t>(d_pos, n + 1)) return rc;
        if (int rc = dalloc<int32_t>(d_eu, room)) return rc;
        if (int rc = dalloc<int32_t>(d_ev, room)) return rc;
        if (int rc = dalloc<int32_t>(d_ew, room)) return rc;
    }
    const RowLists &l = lists.l;
    MatchCtrl *ctrl = d_ctrl.as<MatchCtrl>();
    MatchAcc *acc = d_acc.as<MatchAcc>();
    int32_t *mate = d_mate.as<int32_t>(), *cand = d_cand.as<int32_t>(), *candw = d_candw.as<int32_t>();
    const int32_t *wgt = (flags & GMSX_MATCH_WEIGHTED) ? g->wgt.as<const int32_t>() : nullptr;
    GMSX_HIP(hipMemsetAsync(ctrl, 0, sizeof(MatchCtrl), s));
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(MatchAcc), s));
    GMSX_HIP(hipMemsetAsync(&acc->wmin, 0xff, sizeof(uint32_t), s));
    GMSX_HIP(hipMemsetAsync(d_candw.p, 0, size_t(n) * sizeof(int32_t), s));
    GMSX_HIP(hipMemsetAsync(d_cnt.p, 0, size_t(n + 1) * sizeof(int64_t), s));
    // ---- the rounds
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    int launches = 0;
    const unsigned per_vertex = unsigned((n + 255) / 256);
    const unsigned sweep = row_grid(n, 1, cus, 16);
    hipLaunchKernelGGL(k_match_init, dim3(per_vertex), dim3(256), 0, s, n, mate, cand);
    ++launches;
    classify_rows<true>(g, bounds, l, ctrl->count[0], &ctrl->error, cus, s, &launches);
    MatchCtrl h;
    GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (h.error) return GMSX_ERR_KERNEL;
    int cur = 0;
    int64_t rounds = 0;
    for (;;) {
        const int64_t live = live_count(h.count[cur], l);
        if (live < 0) return GMSX_ERR_KERNEL;
        if (live == 0) break;  // no vertex has a candidate left
        if (rounds > n / 2 + 1) return GMSX_ERR_KERNEL;
        GMSX_HIP(hipMemsetAsync(&ctrl->took, 0, sizeof(int32_t), s));
        GMSX_HIP(hipMemsetAsync(&ctrl->count[cur ^ 1][0], 0, 4 * sizeof(int32_t), s));
        auto search = [&](int) { return MatchSearch{g->off, g->adj, wgt, mate, keep, cand, candw}; };
        launch_live_rows(search, l, cur, ctrl->count[cur], h.count[cur], &ctrl->examined, cus, s, &launches);
        const unsigned over_live = unsigned(std::max<int64_t>(1, std::min<int64_t>((live + 255) / 256, int64_t(cus) * 16)));
        hipLaunchKernelGGL(k_match_pair, dim3(over_live), dim3(256), 0, s, l, cur, cand, mate, ctrl);
        ++launches;
        const unsigned long long examined_was = h.examined;
        GMSX_HIP(hipMemcpyAsync(&h, ctrl, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h.error || h.took < 0 || (h.took & 1)) return GMSX_ERR_KERNEL;
        if (timing)
            std::fprintf(stderr, "[gmsx matching] round %lld: %lld live vertices, %llu arcs examined, %d pairs\n", (long long)rounds + 1, (long long)live,
                         h.examined - examined_was, int(h.took / 2));
        cur ^= 1;
        if (h.took > 0) {
            ++rounds;
        } else {  // a round without a pair ends the rounds: a vertex that still has a candidate then is a live one left
            for (int b = 0; b < 4; ++b)
                if (h.count[cur][b] != 0) return GMSX_ERR_KERNEL;
        }
    }
    // ---- the pair list and the info reduction
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    hipLaunchKernelGGL(k_match_info, dim3(sweep), dim3(256), 0, s, n, g->off, mate, candw, d_cnt.as<int64_t>(), acc);
    ++launches;
    if (want_edges) {
        if (int rc = exclusive_scan_i64(d_cnt.as<const int64_t>(), d_pos.as<int64_t>(), n + 1, s)) return rc;
        hipLaunchKernelGGL(k_match_fill, dim3(sweep), dim3(256), 0, s, n, mate, candw, d_pos.as<const int64_t>(), room, d_eu.as<int32_t>(),
                           d_ev.as<int32_t>(), d_ew.as<int32_t>(), acc);
        launches += 2;
    }
    MatchAcc a;
    GMSX_HIP(hipMemcpyAsync(&a, acc, sizeof a, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipEventRecord(c.ev[3], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (a.error || a.matched > (unsigned long long)n || 2 * a.upper != a.matched || (a.upper > 0) != (rounds > 0) || a.upper < (unsigned long long)rounds)
        return GMSX_ERR_KERNEL;
    res.pairs = int64_t(a.upper);
    res.total_weight = int64_t(a.weight);
    res.free_vertices = n - int64_t(a.matched);
    res.exposed = int64_t(a.exposed);
    res.min_weight = a.upper ? int32_t(a.wmin) : 0;
    res.max_weight = a.upper ? int32_t(a.wmax) : 0;
    res.rounds = int32_t(rounds);
    // the flag words were read as zero: the caller's arrays are written now, through host staging
    const size_t ne = size_t(res.pairs);
    HostStage out;
    if (int rc = out.fetch(mate_out, mate, size_t(n) * sizeof(int32_t), s)) return rc;
    if (int rc = out.fetch_edges(edge_u, edge_v, edge_w, d_eu, d_ev, d_ew, ne, s)) return rc;
    GMSX_HIP(hipStreamSynchronize(s));
    float up_ms = 0.f, ms = 0.f, info_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    GMSX_HIP(hipEventElapsedTime(&info_ms, c.ev[2], c.ev[3]));
    out.deliver();
    *info = res;
    if (stats) *stats = gmsx_stats{double(ms), double(up_ms) + double(info_ms), uint64_t(res.pairs), uint64_t(h.examined), uint64_t(rounds), launches, 0, 0};
    return GMSX_OK;
}

int matching_verify(const gmsx_graph *g, uint32_t flags, const int32_t *mate_in, gmsx_matching_check *out, gmsx_stats *stats) {
    gmsx_matching_check res;
    std::memset(&res, 0, sizeof res);
    const int64_t n = g->n, nnz = g->nnz;
    if (n == 0 || nnz == 0) {  // no edge: every entry but -1 is invalid
        for (int64_t v = 0; v < n; ++v) res.invalid += mate_in[v] != -1;
        res.free_vertices = n;
        *out = res;
        if (stats) *stats = gmsx_stats{0.0, 0.0, 0, 0, 0, 0, 0, 0};
        return GMSX_OK;
    }
    Ctx &c = ctx();
    hipStream_t s = c.stream;
    const int cus = c.compute_units > 0 ? c.compute_units : 256;
    DevBuf d_mate, d_eff, d_key, d_acc;
    GMSX_HIP(hipEventRecord(c.ev[0], s));
    if (int rc = dalloc<int32_t>(d_mate, n)) return rc;
    if (int rc = dalloc<int32_t>(d_eff, n)) return rc;
    if (int rc = dalloc<unsigned long long>(d_key, n)) return rc;
    if (int rc = dalloc<MatchCheckAcc>(d_acc, 1)) return rc;
    MatchCheckAcc *acc = d_acc.as<MatchCheckAcc>();
    const int32_t *wgt = (flags & GMSX_MATCH_WEIGHTED) ? g->wgt.as<const int32_t>() : nullptr;
    GMSX_HIP(hipMemcpyAsync(d_mate.p, mate_in, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    GMSX_HIP(hipMemsetAsync(acc, 0, sizeof(MatchCheckAcc), s));
    GMSX_HIP(hipEventRecord(c.ev[1], s));
    int launches = 1;
    hipLaunchKernelGGL(k_match_valid, dim3(row_grid(n, 1, cus, 16)), dim3(256), 0, s, n, g->off, g->adj, wgt, d_mate.as<const int32_t>(), d_eff.as<int32_t>(),
                       d_key.as<unsigned long long>(), acc);
    launch_rows_two_width(MatchCheck{g->adj, wgt, d_eff.as<const int32_t>(), d_key.as<const unsigned long long>(), acc}, g, nullptr, cus, s, &launches);
    MatchCheckAcc a;
    GMSX_HIP(hipMemcpyAsync(&a, acc, sizeof a, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipEventRecord(c.ev[2], s));
    GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipGetLastError());
    if (2 * a.pairs > (unsigned long long)n || a.invalid > (unsigned long long)n || a.augmentable > a.undominated) return GMSX_ERR_KERNEL;
    float up_ms = 0.f, ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&up_ms, c.ev[0], c.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&ms, c.ev[1], c.ev[2]));
    res.invalid = int64_t(a.invalid);
    res.pairs = int64_t(a.pairs);
    res.total_weight = int64_t(a.weight);
    res.free_vertices = n - 2 * int64_t(a.pairs);
    res.augmentable = int64_t(a.augmentable);
    res.undominated = int64_t(a.undominated);
    *out = res;
    if (stats) *stats = gmsx_stats{double(ms), double(up_ms), uint64_t(res.pairs), uint64_t(nnz), 0, launches, 0, 0};
    return GMSX_OK;
}

}  // namespace
}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_greedy_matching(const gmsx_graph *g, uint32_t flags, int32_t *mate, int32_t *edge_u, int32_t *edge_v, int32_t *edge_w, gmsx_matching_info *info,
                         gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        const int given = (edge_u ? 1 : 0) + (edge_v ? 1 : 0) + (edge_w ? 1 : 0);
        if (!g || !info || (flags & ~uint32_t(GMSX_MATCH_WEIGHTED)) || (given != 0 && given != 3)) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;  // (before the handle is read: without a device there is no valid one)
        if ((flags & GMSX_MATCH_WEIGHTED) && !g->wgt.p) return GMSX_ERR_INVALID;
        return matching(g, flags, mate, edge_u, edge_v, edge_w, info, stats);
    });
}

int gmsx_matching_verify(const gmsx_graph *g, uint32_t flags, const int32_t *mate, gmsx_matching_check *out, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !out || (flags & ~uint32_t(GMSX_MATCH_WEIGHTED))) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        if (((flags & GMSX_MATCH_WEIGHTED) && !g->wgt.p) || (!mate && g->n > 0)) return GMSX_ERR_INVALID;
        return matching_verify(g, flags, mate, out, stats);
    });
}

}  // extern "C"
