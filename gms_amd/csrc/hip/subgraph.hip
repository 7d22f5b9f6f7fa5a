// SUBGRAPH MATCHING on gfx950: the device counterpart of the reference's VF2
//   GMS::SubGraphIso::VF2::solve          gms/algorithms/non_set_based/subgraphiso/vf2/sequential/vf2.hpp:53-81
//   generateCandidatePairSet              vf2/util/candidateGeneration.hpp:12-56
//   checkSynRules                         vf2/util/feasibilityRules.hpp:48-92 (the look-ahead rules :96-125 only cut subtrees without an embedding)
// Every embedding f of a small connected pattern P (k <= 32 vertices) into the uploaded graph G, induced (VF2's question) or not (MONO).
//
// Formulation.  The reference files VF2 under "non set based"; on the device it is set algebra over the full rows of the CSR.  The matching order
// is static: pi_0 = 0, pi_(i+1) = the smallest pattern vertex adjacent to {pi_0 .. pi_i} — the order the reference's candidate rule walks a
// connected pattern in.  The candidates of level i, given the images of the levels before it, are
//     ∩ { N(f(pi_j)) : j < i, pi_j adjacent to pi_i }  \  ∪ { N(f(pi_j)) : j < i, pi_j not adjacent to pi_i }      (the difference: INDUCED only)
// minus the images themselves, minus the vertices of a degree below deg_P(pi_i).  Level i has at least one earlier neighbour, so its candidates
// are a subset of one row: the BASE, the shortest row among its earlier neighbours' images.  The base is streamed 64 ids at a time, each lane
// tests its id against the other rows by binary search (kcs_in_row of kcstar_list.hip), and the ballot of the kept lanes is the level's
// candidate mask: no candidate list is ever materialised, so a task has no slab and no request is refused for the width of a neighbourhood.
// (kcstar_list.hip carries filtered lists from a level to its children, its T_j chain; a general pattern would need one list per (level, later
// vertex).  That is not built here.)
// A task is an arc (u, v) = (f(pi_0), f(pi_1)) of G that passes the two degree filters (k = 1: a vertex), in ascending (u, v); one wave searches
// one task depth-first, candidates ascending, so the embeddings of the whole call come out in ascending lexicographic order of
// (f(pi_0), .., f(pi_(k-1))) — and in INDUCED mode the first of them is the embedding the reference's sequential VF2 returns.  The search state
// is spread over the lanes: lane j holds level j (k <= 32): its image and that image's row, its base row, the position of the 64-id chunk under
// work and that chunk's candidate mask; lane j also holds pi_j, the mask of the earlier levels adjacent to level j and deg_P(pi_j), loaded once
// from the kernel arguments.  The last level is not walked: its mask is pop-counted (count pass) or its rows are stored at once (fill pass).
// Count / scan / fill, the launches and the pass-1 cache are the scaffold of two_pass_list.hpp (all slabs are empty).
// GMSX_SGM_FIRST: a task that meets its first embedding does an atomicMin of its task index into one word and ends; every task reads that word
// (relaxed, agent scope) when it starts and at every step down and quits when a lower task has found one; the host launches ascending ranges
// of tasks and stops after the first launch that found one; the row itself is written by a fill launch over the winning task alone.  The
// lowest task that holds an embedding never quits, so timing decides only how much abandoned work is done.
#include "two_pass_list.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

namespace gmsx {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kSgmMaxK = 32;
constexpr int kAccFlags = 0, kAccStop = 1, kAccWords = 2;
constexpr unsigned long long kFlagOut = 2, kFlagMismatch = 4;
constexpr unsigned long long kNoTask = ~0ull;

// the pattern as the kernel sees it: by value in the kernel arguments, the device never reads pattern memory
struct SgmPattern {
    int32_t k, induced;
    int32_t pi[kSgmMaxK];      // the matching order: pattern vertex of level i
    uint32_t back[kSgmMaxK];   // bit j (j < i): pi_j is adjacent to pi_i
    int32_t mindeg[kSgmMaxK];  // deg_P(pi_i)
};

__device__ __forceinline__ unsigned long long sgm_shfl64(unsigned long long v, int j) {
    const unsigned lo = unsigned(__shfl(int(unsigned(v)), j));
    const unsigned hi = unsigned(__shfl(int(unsigned(v >> 32)), j));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// w in the ascending row [row, row + len)?
__device__ __forceinline__ bool sgm_in_row(const int32_t *__restrict__ row, int len, int32_t w) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && row[lo] == w;
}

// One wave per task.  FILL = false: cnt[t] = the embeddings of task t; with `first` nothing but acc[kAccStop] (atomicMin of t) is written.
// FILL = true: task t's rows from row cbase[t] on (cbase = the exclusive scan of cnt); with `first` (cbase == nullptr) the one task's first
// embedding into row 0.
template <bool FILL>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_sgm(const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                             const int32_t *__restrict__ task_a, const int32_t *__restrict__ task_b, int64_t t0,
                                                             int64_t t1, const SgmPattern pat, int first, int64_t *__restrict__ cnt,
                                                             const int64_t *__restrict__ cbase, int32_t *__restrict__ out, int64_t cap,
                                                             unsigned long long *__restrict__ acc) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t t = t0 + int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (t >= t1) return;  // the waves of a workgroup never meet at a barrier
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int k = pat.k;
    const bool induced = pat.induced != 0;
    const bool racing = !FILL && first;
    // has a lower task found an embedding already?  A stale value only delays the quit.
    auto beaten = [&]() -> bool {
        return racing && uni64(__hip_atomic_load(&acc[kAccStop], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < (unsigned long long)t;
    };
    if (beaten()) return;

    // the pattern, lane j = level j
    const int32_t my_pi = pat.pi[lane & (kSgmMaxK - 1)];
    const uint32_t my_back = pat.back[lane & (kSgmMaxK - 1)];
    const int32_t my_mind = pat.mindeg[lane & (kSgmMaxK - 1)];
    // search state, lane j = level j: the image chosen at level j and its row; the base row level j takes its candidates from and which level's
    // image it belongs to, the first position of the 64-id chunk under work and the candidates of that chunk not yet taken
    int32_t img = -1;
    long long ioff = 0, boff = 0;
    int ilen = 0, blen = 0, bsel = 0, cpos = 0;
    unsigned long long mask = 0;

    long long kc = 0, cb = 0, my_cnt = 0;
    if (FILL) {
        cb = cbase ? cbase[t] : 0;
        my_cnt = cbase ? cbase[t + 1] - cb : 1;
    }
    bool failed = false, done = false;

    auto set_image = [&](int d, int32_t x) {
        const long long xo = uni64(off[x]);
        const int xl = int(uni64(off[x + 1]) - xo);
        if (lane == d) {
            img = x;
            ioff = xo;
            ilen = xl;
        }
    };
    // level d starts: its base is the shortest row among the images of its earlier neighbours (the lowest such level on a tie)
    auto open_level = [&](int d) {
        const uint32_t bk = uni32(uint32_t(__shfl(int(my_back), d)));
        int best = 0, best_len = 0x7fffffff;
        for (int j = 0; j < d; ++j) {
            const int len = uni32(__shfl(ilen, j));
            if (((bk >> j) & 1u) && len < best_len) {
                best = j;
                best_len = len;
            }
        }
        const long long bo = (long long)uni64(sgm_shfl64((unsigned long long)ioff, best));
        if (lane == d) {
            boff = bo;
            blen = best_len;
            bsel = best;
            cpos = -64;
            mask = 0ull;
        }
    };
    // the rows of one embedding each for the candidates `m` of the chunk held in w, which close the pattern at level d (d = k - 1)
    auto emit_chunk = [&](int d, int32_t w, unsigned long long m) {
        if (first) m &= ~m + 1ull;  // the lowest candidate only
        const long long nc = __popcll(m);
        if (FILL) {
            if (kc + nc > my_cnt) {
                failed = true;
            } else if (cb + kc + nc > cap) {
                if (lane == 0) atomicOr(&acc[kAccFlags], kFlagOut);
            } else {
                const bool mine = (m >> lane) & 1ull;
                int32_t *row = out + (cb + kc + __popcll(m & lt)) * (long long)k;
                for (int j = 0; j < d; ++j) {
                    const int32_t xj = __shfl(img, j);
                    const int pj = __shfl(my_pi, j);
                    if (mine) row[pj] = xj;
                }
                const int pd = __shfl(my_pi, d);
                if (mine) row[pd] = w;
            }
        }
        kc += nc;
        if (first && nc) done = true;
    };

    const int32_t a = uni32(task_a[t]);
    set_image(0, a);
    if (k == 1) {
        emit_chunk(0, a, 1ull);  // lane 0 holds a
    } else {
        const int32_t b = uni32(task_b[t]);
        if (k == 2) {
            emit_chunk(1, b, 1ull);
        } else {
            set_image(1, b);
            int d = 2;
            open_level(2);
            while (!failed && !done) {
                const int len = uni32(__shfl(blen, d));
                int cbeg = uni32(__shfl(cpos, d));
                unsigned long long m = uni64(sgm_shfl64(mask, d));
                const long long bo = (long long)uni64(sgm_shfl64((unsigned long long)boff, d));
                if (m == 0ull) {
                    cbeg += 64;
                    if (cbeg >= len) {
                        if (d == 2) break;
                        --d;
                        continue;
                    }
                    const uint32_t bk = uni32(uint32_t(__shfl(int(my_back), d)));
                    const int bs = uni32(__shfl(bsel, d));
                    const int mind = uni32(__shfl(my_mind, d));
                    const int i = cbeg + lane;
                    int32_t w = -1;
                    bool keep = false;
                    if (i < len) {
                        w = adj[bo + i];
                        keep = true;
                        if (mind > 1) keep = off[w + 1] - off[w] >= mind;  // a member of a row has a neighbour
                    }
                    for (int j = 0; j < d; ++j) {
                        const int32_t xj = uni32(__shfl(img, j));
                        const long long xo = (long long)uni64(sgm_shfl64((unsigned long long)ioff, j));
                        const int xl = uni32(__shfl(ilen, j));
                        const bool nb = (bk >> j) & 1u;
                        if (keep) {
                            if (w == xj) keep = false;
                            else if (nb) keep = j == bs || sgm_in_row(adj + xo, xl, w);
                            else if (induced) keep = !sgm_in_row(adj + xo, xl, w);
                        }
                    }
                    m = __ballot(keep);
                    if (d + 1 == k) {  // the last level: the whole chunk at once
                        if (racing) {
                            if (m != 0ull) {
                                if (lane == 0) atomicMin(&acc[kAccStop], (unsigned long long)t);
                                return;
                            }
                        } else {
                            emit_chunk(d, w, m);
                        }
                        m = 0ull;
                    }
                    if (lane == d) {
                        cpos = cbeg;
                        mask = m;
                    }
                    continue;
                }
                const int bit = __builtin_ctzll(m);
                m &= m - 1ull;
                if (lane == d) mask = m;
                set_image(d, uni32(adj[bo + cbeg + bit]));
                if (beaten()) return;
                ++d;
                open_level(d);
            }
        }
    }
    if (racing) {
        if (kc > 0 && lane == 0) atomicMin(&acc[kAccStop], (unsigned long long)t);  // k <= 2: the task is its own embedding
        return;
    }
    if (FILL) {
        if ((failed || kc != my_cnt) && lane == 0) atomicOr(&acc[kAccFlags], kFlagMismatch);
    } else if (lane == 0) {
        cnt[t] = kc;
    }
}

// ---- host ----

// The pattern checked and ordered.  adjm[a] = the neighbours of pattern vertex a as a bit mask.
struct HostPattern {
    int k = 0;
    uint32_t adjm[kSgmMaxK] = {};
    int32_t order[kSgmMaxK];
};

int pattern_check(int32_t k, const int64_t *p_off, const int32_t *p_neigh, HostPattern &hp) {
    if (k < 1 || !p_off || !p_neigh) return GMSX_ERR_INVALID;
    if (k > kSgmMaxK) return GMSX_ERR_UNSUPPORTED;
    hp.k = k;
    if (p_off[0] != 0) return GMSX_ERR_NOT_CANONICAL;
    for (int a = 0; a < k; ++a) {
        const int64_t b0 = p_off[a], b1 = p_off[a + 1];
        if (b1 < b0 || b1 - b0 >= k) return GMSX_ERR_NOT_CANONICAL;  // a strictly ascending loop-free row has at most k - 1 ids
        for (int64_t e = b0; e < b1; ++e) {
            const int32_t b = p_neigh[e];
            if (b < 0 || b >= k || b == a || (e > b0 && p_neigh[e - 1] >= b)) return GMSX_ERR_NOT_CANONICAL;
            hp.adjm[a] |= 1u << b;
        }
    }
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b)
            if (((hp.adjm[a] >> b) & 1u) != ((hp.adjm[b] >> a) & 1u)) return GMSX_ERR_NOT_CANONICAL;
    // pi_0 = 0, pi_(i+1) = the smallest vertex adjacent to {pi_0 .. pi_i}: none left before all k are placed = disconnected
    uint32_t placed = 1u, frontier = hp.adjm[0];
    hp.order[0] = 0;
    for (int i = 1; i < k; ++i) {
        const uint32_t f = frontier & ~placed;
        if (!f) return GMSX_ERR_UNSUPPORTED;
        const int v = __builtin_ctz(f);
        hp.order[i] = v;
        placed |= 1u << v;
        frontier |= hp.adjm[v];
    }
    return GMSX_OK;
}

SgmPattern kernel_pattern(const HostPattern &hp, bool induced) {
    SgmPattern p{};
    p.k = hp.k;
    p.induced = induced ? 1 : 0;
    for (int i = 0; i < hp.k; ++i) {
        const int v = hp.order[i];
        p.pi[i] = v;
        p.mindeg[i] = __builtin_popcount(hp.adjm[v]);
        for (int j = 0; j < i; ++j)
            if ((hp.adjm[v] >> hp.order[j]) & 1u) p.back[i] |= 1u << j;
    }
    return p;
}

struct SgmPass1 : ListPass1 {  // task[0]: images of pi_0, task[1]: images of pi_1 (caller ids; -1 for k = 1)
    gmsx_subgraph_info info{};
    std::vector<int64_t> p_off;  // the pattern the pass belongs to, compared in full
    std::vector<int32_t> p_neigh;
};
SgmPass1 &pass1_cache() {
    static SgmPass1 c;
    return c;
}

// tasks per launch (test hook SGM_LAUNCH_TASKS: a small value splits a small graph into many launches).  Both defaults are first guesses.
int64_t launch_tasks(bool first) {
    const long long v = opt_int("SGM_LAUNCH_TASKS", 0);
    return v >= 1 ? int64_t(v) : (first ? int64_t(1) << 16 : int64_t(1) << 24);
}

void launch(bool fill, const gmsx_graph *g, const ListPass1 &p1, int64_t t0, int64_t t1, const SgmPattern &pat, int first, int64_t *cnt,
            const int64_t *cbase, int32_t *out, int64_t cap, unsigned long long *acc) {
    const unsigned blocks = unsigned((t1 - t0 + kWavesPerBlock - 1) / kWavesPerBlock);
    if (fill)
        hipLaunchKernelGGL((k_sgm<true>), dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx().stream, g->off, g->adj, p1.task[0].as<const int32_t>(),
                           p1.task[1].as<const int32_t>(), t0, t1, pat, first, cnt, cbase, out, cap, acc);
    else
        hipLaunchKernelGGL((k_sgm<false>), dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx().stream, g->off, g->adj, p1.task[0].as<const int32_t>(),
                           p1.task[1].as<const int32_t>(), t0, t1, pat, first, cnt, cbase, out, cap, acc);
}

// the task list of (g, pattern, part, nparts) into the cleared p1: the arcs (u, v) in ascending (u, v) with u in the shard, d(u) >= deg_P(pi_0)
// and d(v) >= deg_P(pi_1); k = 1: the shard's vertices
int build_tasks(const gmsx_graph *g, const SgmPattern &pat, int part, int nparts, ListPass1 &p1, double *setup_ms) {
    hipStream_t s = ctx().stream;
    const int64_t n = g->n, nnz = g->nnz;
    const auto h0 = std::chrono::steady_clock::now();
    std::vector<int64_t> off(size_t(n + 1), 0);
    std::vector<int32_t> adj(size_t(pat.k > 1 ? nnz : 0));
    if (n > 0) {
        GMSX_HIP(hipMemcpyAsync(off.data(), g->off, size_t(n + 1) * 8, hipMemcpyDeviceToHost, s));
        if (!adj.empty()) GMSX_HIP(hipMemcpyAsync(adj.data(), g->adj, adj.size() * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
    }
    std::vector<int32_t> task_a, task_b;
    if (pat.k <= n) {
        for (int64_t u = 0; u < n; ++u) {
            if (shard_of(u, nparts) != part) continue;
            const int64_t b0 = off[size_t(u)], b1 = off[size_t(u) + 1];
            if (b1 - b0 < pat.mindeg[0]) continue;
            if (pat.k == 1) {
                task_a.push_back(int32_t(u));
                task_b.push_back(-1);
                continue;
            }
            for (int64_t e = b0; e < b1; ++e) {
                const int32_t v = adj[size_t(e)];
                if (off[size_t(v) + 1] - off[size_t(v)] < pat.mindeg[1]) continue;
                task_a.push_back(int32_t(u));
                task_b.push_back(v);
            }
        }
    }
    p1.soff.assign(task_a.size() + 1, 0);  // no task has a slab
    const std::vector<int32_t> *tasks[] = {&task_a, &task_b};
    if (int rc = upload_tasks(p1, tasks, 2, s)) return rc;
    GMSX_HIP(hipStreamSynchronize(s));
    *setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    return GMSX_OK;
}

gmsx_subgraph_info make_info(const HostPattern &hp, int64_t embeddings, int64_t tasks) {
    gmsx_subgraph_info info{};
    info.embeddings = embeddings;
    info.tasks = tasks;
    info.k = hp.k;
    for (int i = 0; i < kSgmMaxK; ++i) info.order[i] = i < hp.k ? hp.order[i] : -1;
    return info;
}

// the count pass of the listing into the cleared p1
int sgm_pass1(const gmsx_graph *g, const HostPattern &hp, const SgmPattern &pat, int part, int nparts, SgmPass1 &p1, double *ms, double *setup_ms,
              int *launches) {
    hipStream_t s = ctx().stream;
    if (int rc = build_tasks(g, pat, part, nparts, p1, setup_ms)) return rc;
    const int64_t nt = p1.n_tasks;
    DevBuf cnt, mem, acc;
    if (int rc = alloc_zeroed(cnt, size_t(nt + 1) * 8, s)) return rc;
    if (int rc = alloc_zeroed(mem, size_t(nt + 1) * 8, s)) return rc;
    if (int rc = alloc_zeroed(acc, size_t(kAccWords) * 8, s)) return rc;
    const ListArena arena{4ull << 20, nullptr, launch_tasks(false)};
    if (int rc = run_list_pass(p1, arena, 0, launches, [&](const Launch &l, void *, unsigned long long) {
            launch(false, g, p1, l.t0, l.t1, pat, 0, cnt.as<int64_t>(), nullptr, nullptr, 0, acc.as<unsigned long long>());
        }))
        return rc;
    unsigned long long host[kAccWords];
    int64_t tot[2] = {0, 0};
    if (int rc = finish_count_pass(p1, cnt, mem, acc, host, kAccWords, tot, 0, ms)) return rc;
    if (host[kAccFlags]) return GMSX_ERR_KERNEL;
    p1.info = make_info(hp, tot[0], nt);
    return GMSX_OK;
}

int sgm_list(const gmsx_graph *g, const HostPattern &hp, const int64_t *p_off, const int32_t *p_neigh, uint32_t flags, int part, int nparts,
             int32_t *maps, int64_t capacity, gmsx_subgraph_info *info, gmsx_stats *st) {
    hipStream_t s = ctx().stream;
    const int k = hp.k;
    const SgmPattern pat = kernel_pattern(hp, !(flags & GMSX_SGM_MONO));
    SgmPass1 &p1 = pass1_cache();
    const bool sizing = maps == nullptr;
    const size_t arcs = size_t(p_off[k]);
    if (p1.valid && !(p1.p_off.size() == size_t(k) + 1 && std::equal(p1.p_off.begin(), p1.p_off.end(), p_off) && p1.p_neigh.size() == arcs &&
                      std::equal(p1.p_neigh.begin(), p1.p_neigh.end(), p_neigh)))
        p1.clear();  // pass 1 of another pattern
    double ms1 = 0.0, ms2 = 0.0, setup = 0.0;
    int launches = 0;
    if (int rc = ensure_pass1(p1, ListKey(g->serial, g, g->off, g->adj, g->n, g->nnz, part, nparts, k, flags), sizing,
                              [&] { return sgm_pass1(g, hp, pat, part, nparts, p1, &ms1, &setup, &launches); }))
        return rc;
    p1.p_off.assign(p_off, p_off + k + 1);
    p1.p_neigh.assign(p_neigh, p_neigh + arcs);
    *info = p1.info;
    if (!sizing) {
        const int64_t ne = p1.info.embeddings;
        if (capacity < ne) return GMSX_ERR_INVALID;
        DevBuf d_maps, acc;
        GMSX_HIP(hipMalloc(&d_maps.p, size_t(ne > 0 ? ne : 1) * size_t(k) * 4));
        if (int rc = alloc_zeroed(acc, size_t(kAccWords) * 8, s)) return rc;
        const ListArena arena{4ull << 20, nullptr, launch_tasks(false)};
        if (int rc = run_list_pass(p1, arena, 2, &launches, [&](const Launch &l, void *, unsigned long long) {
                launch(true, g, p1, l.t0, l.t1, pat, 0, nullptr, p1.cbase.as<const int64_t>(), d_maps.as<int32_t>(), ne, acc.as<unsigned long long>());
            }))
            return rc;
        unsigned long long host[kAccWords];
        if (int rc = finish_fill_pass(acc, host, kAccWords, 2, &ms2)) return rc;
        if (host[kAccFlags]) return GMSX_ERR_KERNEL;
        // the caller's array is written only now, on success
        if (ne > 0) {
            GMSX_HIP(hipMemcpyAsync(maps, d_maps.p, size_t(ne) * size_t(k) * 4, hipMemcpyDeviceToHost, s));
            GMSX_HIP(hipStreamSynchronize(s));
        }
    }
    if (st) *st = gmsx_stats{ms1 + ms2, setup, uint64_t(p1.n_tasks), 0, 0, launches, 0, 0};
    return GMSX_OK;
}

// GMSX_SGM_FIRST: one call, nothing cached
int sgm_first(const gmsx_graph *g, const HostPattern &hp, uint32_t flags, int part, int nparts, int32_t *maps, gmsx_subgraph_info *info,
              gmsx_stats *st) {
    Ctx &cx = ctx();
    hipStream_t s = cx.stream;
    const int k = hp.k;
    const SgmPattern pat = kernel_pattern(hp, !(flags & GMSX_SGM_MONO));
    ListPass1 p1;
    double setup = 0.0;
    if (int rc = build_tasks(g, pat, part, nparts, p1, &setup)) return rc;
    const int64_t nt = p1.n_tasks, per = launch_tasks(true);
    DevBuf acc, d_row;
    if (int rc = alloc_zeroed(acc, size_t(kAccWords) * 8, s)) return rc;
    GMSX_HIP(hipMalloc(&d_row.p, size_t(k) * 4));
    unsigned long long host[kAccWords] = {0, kNoTask};
    GMSX_HIP(hipMemcpyAsync(acc.as<unsigned long long>() + kAccStop, &host[kAccStop], 8, hipMemcpyHostToDevice, s));
    int launches = 0;
    GMSX_HIP(hipEventRecord(cx.ev[0], s));
    for (int64_t t0 = 0; t0 < nt && host[kAccStop] == kNoTask; t0 += per) {  // ascending ranges; the first launch that found one is the last
        launch(false, g, p1, t0, std::min(nt, t0 + per), pat, 1, nullptr, nullptr, nullptr, 0, acc.as<unsigned long long>());
        GMSX_HIP(hipGetLastError());
        ++launches;
        GMSX_HIP(hipMemcpyAsync(host, acc.p, size_t(kAccWords) * 8, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
    }
    GMSX_HIP(hipEventRecord(cx.ev[1], s));
    const bool found = host[kAccStop] != kNoTask;
    if (found && int64_t(host[kAccStop]) >= nt) return GMSX_ERR_KERNEL;
    GMSX_HIP(hipEventRecord(cx.ev[2], s));
    if (found && maps) {  // the winning row: a fill over that one task, which stops at its first embedding
        const int64_t w = int64_t(host[kAccStop]);
        launch(true, g, p1, w, w + 1, pat, 1, nullptr, nullptr, d_row.as<int32_t>(), 1, acc.as<unsigned long long>());
        GMSX_HIP(hipGetLastError());
        ++launches;
    }
    GMSX_HIP(hipEventRecord(cx.ev[3], s));
    GMSX_HIP(hipMemcpyAsync(host, acc.p, size_t(kAccWords) * 8, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    if (host[kAccFlags]) return GMSX_ERR_KERNEL;
    float f1 = 0.f, f2 = 0.f;
    GMSX_HIP(hipEventElapsedTime(&f1, cx.ev[0], cx.ev[1]));
    GMSX_HIP(hipEventElapsedTime(&f2, cx.ev[2], cx.ev[3]));
    *info = make_info(hp, found ? 1 : 0, nt);
    if (found && maps) {
        GMSX_HIP(hipMemcpyAsync(maps, d_row.p, size_t(k) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
    }
    if (st) *st = gmsx_stats{double(f1) + double(f2), setup, uint64_t(nt), 0, 0, launches, 0, 0};
    return GMSX_OK;
}

}  // namespace

}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_subgraph_order(int32_t k, const int64_t *p_offsets, const int32_t *p_neigh, int32_t *order) {
    return gmsx::guard([&]() -> int {
        if (!order) return GMSX_ERR_INVALID;
        HostPattern hp;
        if (int rc = pattern_check(k, p_offsets, p_neigh, hp)) return rc;
        std::copy(hp.order, hp.order + k, order);
        return GMSX_OK;
    });
}

int gmsx_subgraph_match(const gmsx_graph *g, int32_t k, const int64_t *p_offsets, const int32_t *p_neigh, uint32_t flags, int part, int nparts,
                        int32_t *maps, int64_t capacity, gmsx_subgraph_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || capacity < 0 || nparts < 1 || part < 0 || part >= nparts) return GMSX_ERR_INVALID;
        if (flags & ~uint32_t(GMSX_SGM_MONO | GMSX_SGM_FIRST)) return GMSX_ERR_INVALID;
        HostPattern hp;
        if (int rc = pattern_check(k, p_offsets, p_neigh, hp)) return rc;
        if ((flags & GMSX_SGM_FIRST) && maps && capacity < 1) return GMSX_ERR_INVALID;
        if (int rc = ensure_init()) return rc;
        if (flags & GMSX_SGM_FIRST) return sgm_first(g, hp, flags, part, nparts, maps, info, stats);
        return sgm_list(g, hp, p_offsets, p_neigh, flags, part, nparts, maps, capacity, info, stats);
    });
}

}  // extern "C"
