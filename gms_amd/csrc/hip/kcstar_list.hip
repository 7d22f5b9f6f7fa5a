// k-clique-star LISTING on gfx950: the device replacement for
//   KCliqueStar::Par::CliqueStarList   gms/algorithms/set_based/k_clique_star_list/parallel/recursive.h:19-43
//   Seq::RecursiveStepCliqueStar       gms/algorithms/set_based/k_clique_star_list/sequential/recursive.h:31-71
// One (clique, star) pair per k-clique: the k members, and every vertex outside the clique adjacent to all of them.  With
// GMSX_KCSTAR_CLIQUES_ONLY the stars are left out: k-clique listing (k = 3: triangle listing).
//
// Formulation.  The PIVOT of a clique is its member of the highest rank id (lowest degree: the shortest full row of the clique).  A task is
// (pivot u, first member v in N+(u)); for k = 1 a task is a vertex.  One wave searches one task, four independent waves per workgroup.
// All sets are sorted lists of CALLER ids over the FULL rows of the CSR:
//   T_1     = N(u) ∩ N(v)                      u's row streamed 64 ids at a time, v's row binary-searched (as pairs.hip does)
//   T_(j+1) = { w in T_j : w in N(x) }         for the chosen member x, ballot / popcount compaction
// The next member is a w in T_j with newid[w] below the rank id of the member chosen last, so the chain of rank ids strictly decreases and
// every clique is met exactly once.  Members are never in their own rows, so T_(k-1) is exactly the star, ascending: pass 1 counts it,
// pass 2 stores it where it belongs.  With CLIQUES_ONLY nothing but candidates is carried (the rank filter is applied when a list is
// built) and the last level is not built: every element of T_(k-2) closes a clique.  A branch stops when fewer candidates remain than
// members are still needed.  T_1 … T_(k-2) live in the task's slab of a global arena (k - 2 lists of d(u) ids).  The per-level search state
// (position, candidate mask, list size, chosen member) is spread over the lanes: lane j holds level j (k <= 63).
// The task list is the shard's pivots in rank-id order, each pivot's first members in ascending caller id; the two passes over it (count:
// cliques and star ids per task, the largest star per call by integer atomicMax; scan; fill), the launches that fit the slab budget (test
// hook KCSTAR_SLAB_MB) and the pass-1 cache are the scaffold of two_pass_list.hpp.  Nothing that shapes the search depends on timing.
#include "two_pass_list.hpp"

#include <algorithm>
#include <chrono>
#include <vector>

namespace gmsx {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kAccMax = 0, kAccFlags = 1, kAccWords = 2;
constexpr unsigned long long kFlagSlab = 1, kFlagOut = 2, kFlagMismatch = 4;

__device__ __forceinline__ void kcs_flag(unsigned long long *acc, unsigned long long f) { atomicOr(&acc[kAccFlags], f); }

__device__ __forceinline__ unsigned long long kcs_shfl64(unsigned long long v, int j) {
    const unsigned lo = unsigned(__shfl(int(unsigned(v)), j));
    const unsigned hi = unsigned(__shfl(int(unsigned(v >> 32)), j));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// w in the ascending row [row, row + len)?
__device__ __forceinline__ bool kcs_in_row(const int32_t *__restrict__ row, long long len, int32_t w) {
    long long lo = 0, hi = len;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (row[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && row[lo] == w;
}

// words of one task's slab: max(k - 2, 0) lists of d(u) ids, a 16-byte multiple
__host__ __device__ inline long long kcs_need(long long k, long long deg) {
    const long long lists = k > 2 ? k - 2 : 0;
    return (lists * deg + 3) & ~3ll;
}

// One wave per task.  FILL = false: cnt[t], mem[t] and the largest star.  FILL = true: the pairs, task t's clique rows from row cbase[t]
// on and its stars from out_star[mbase[t]] on; cbase / mbase are the exclusive scans of pass 1's cnt / mem (n_tasks + 1 entries).
template <bool FILL>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_kcstar_list(
    const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const int32_t *__restrict__ newid, const int32_t *__restrict__ task_a,
    const int32_t *__restrict__ task_b, const int64_t *__restrict__ slab_off, int64_t t0, int64_t t1, int32_t *arena, unsigned long long arena_words,
    int k, int only, int64_t *__restrict__ cnt, int64_t *__restrict__ mem, const int64_t *__restrict__ cbase, const int64_t *__restrict__ mbase,
    int32_t *__restrict__ out_cl, int64_t *__restrict__ out_soff, int32_t *__restrict__ out_star, int64_t cl_cap, int64_t star_cap,
    unsigned long long *__restrict__ acc) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t t = t0 + int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (t >= t1) return;  // the waves of a workgroup never meet at a barrier
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int32_t a = uni32(task_a[t]);
    const int32_t b = uni32(task_b[t]);
    const int64_t ab = uni64(off[a]);
    const long long da = uni64(off[a + 1]) - ab;
    const unsigned long long base = (unsigned long long)(slab_off[t] - slab_off[t0]);
    const unsigned long long have = (unsigned long long)(slab_off[t + 1] - slab_off[t]);
    if (have < (unsigned long long)kcs_need(k, da) || base + have > arena_words) {
        if (lane == 0) kcs_flag(acc, kFlagSlab);
        return;
    }
    int32_t *const slab = arena + base;
    const long long cap = da;  // ids per list: every T_j is a subset of N(a)

    // task bookkeeping (uniform)
    long long kc = 0, run = 0, maxs = 0, my_cnt = 0, my_mem = 0, cb = 0, mb = 0;
    if (FILL) {
        cb = cbase[t];
        mb = mbase[t];
        my_cnt = cbase[t + 1] - cb;
        my_mem = mbase[t + 1] - mb;
    }
    bool failed = false;

    // search state, lane j = level j: the member chosen at level j and its rank id; of the list level j chooses from: its size, the first
    // position of the 64-id chunk under work and the candidates of that chunk not yet taken
    int32_t memb = 0, mrank = 0;
    long long lsize = 0, lbase = 0;
    unsigned long long lmask = 0;

    // dst[0 ..) = { w in src[0 .. ns) : w in N(x), and with `only` newid[w] < rx }, at most dcap ids (more: *over).  dst == nullptr counts.
    // *ncand = the kept ids whose rank id is below rx (with want_cand).
    auto filter = [&](const int32_t *src, long long ns, int32_t x, int32_t rx, bool want_cand, int32_t *dst, long long dcap, long long *ncand,
                      bool *over) -> long long {
        const int64_t xb = uni64(off[x]);
        const long long xl = uni64(off[x + 1]) - xb;
        const int32_t *xrow = adj + xb;
        long long kept = 0, cand = 0;
        for (long long i0 = 0; i0 < ns; i0 += 64) {
            const long long i = i0 + lane;
            int32_t w = -1;
            bool keep = false;
            if (i < ns) {
                w = src[i];
                keep = kcs_in_row(xrow, xl, w);
            }
            bool is_cand = false;
            if (keep && (only || want_cand)) is_cand = newid[w] < rx;
            if (only) keep = is_cand;
            const unsigned long long bm = __ballot(keep);
            const long long at = kept + __popcll(bm & lt);
            if (keep && dst && at < dcap) dst[at] = w;
            kept += __popcll(bm);
            cand += __popcll(__ballot(is_cand));
        }
        *ncand = cand;
        *over = dst && kept > dcap;
        return kept;
    };
    // where star `star` of the next pair goes in pass 2 (nullptr: pass 1, or the span / the array is used up: counted only, then reported)
    auto star_dst = [&](long long *dcap) -> int32_t * {
        if (!FILL) return nullptr;
        const long long room = std::min<long long>(my_mem - run, star_cap - (mb + run));
        *dcap = room > 0 ? room : 0;
        return out_star + mb + run;
    };
    // one pair: the clique memb[0 .. d) + x, its star of `star` ids already stored by star_dst's filter
    auto emit = [&](int d, int32_t x, long long star, bool over) {
        if (FILL) {
            const long long ci = cb + kc;
            if (kc >= my_cnt || over || (!only && run + star > my_mem)) {
                failed = true;
            } else if (ci >= cl_cap) {
                if (lane == 0) kcs_flag(acc, kFlagOut);
            } else {
                const int32_t id = lane < d ? memb : x;
                int rk = 0;
                for (int j = 0; j <= d; ++j) rk += __shfl(id, j) < id ? 1 : 0;
                if (lane <= d) out_cl[ci * (long long)k + rk] = id;
                if (!only && lane == 0) out_soff[ci] = mb + run;
            }
        }
        ++kc;
        run += star;
        maxs = star > maxs ? star : maxs;
    };
    // CLIQUES_ONLY, last level: every candidate of the chunk held in w (mask `m`) closes a clique with memb[0 .. d)
    auto emit_chunk = [&](int d, int32_t w, unsigned long long m) {
        const long long nc = __popcll(m);
        if (FILL) {
            if (kc + nc > my_cnt) {
                failed = true;
            } else if (cb + kc + nc > cl_cap) {
                if (lane == 0) kcs_flag(acc, kFlagOut);
            } else {
                int mpos = 0;  // lane j < d: how many members are below member j
                for (int j = 0; j < d; ++j) mpos += __shfl(memb, j) < memb ? 1 : 0;
                const bool mine = (m >> lane) & 1ull;
                int32_t *row = out_cl + (cb + kc + __popcll(m & lt)) * (long long)k;
                int wpos = 0;
                for (int j = 0; j < d; ++j) {
                    const int32_t mj = __shfl(memb, j);
                    const int pj = __shfl(mpos, j);
                    if (mine) row[pj + (w < mj ? 1 : 0)] = mj;
                    wpos += mj < w ? 1 : 0;
                }
                if (mine) row[wpos] = w;
            }
        }
        kc += nc;
    };
    // the list level j chooses from: level 1 the pivot's row itself, level j >= 2 list j - 2 of the slab
    auto list_of = [&](int j) -> const int32_t * { return j <= 1 ? adj + ab : slab + (long long)(j - 2) * cap; };
    // member x (rank id rx) joins memb[0 .. d), chosen from list_of(d) of ns ids.  Returns true when the search goes one level down.
    auto step = [&](int d, long long ns, int32_t x, int32_t rx) -> bool {
        if (d + 1 == k) {  // x completes the clique
            long long star = 0, nc = 0, dcap = 0;
            bool over = false;
            if (!only) {
                int32_t *dst = star_dst(&dcap);
                star = filter(list_of(d), ns, x, rx, false, dst, dcap, &nc, &over);
                if (!dst) over = false;
            }
            emit(d, x, star, over);
            return false;
        }
        long long nc = 0;
        bool over = false;
        int32_t *dst = slab + (long long)(d - 1) * cap;  // list_of(d + 1)
        const long long kept = filter(list_of(d), ns, x, rx, true, dst, cap, &nc, &over);
        if (over) {  // cannot happen (a subset of N(a)): never step past the slab
            if (lane == 0) kcs_flag(acc, kFlagSlab);
            failed = true;
            return false;
        }
        wave_slab_sync();
        if (nc < (long long)(k - (d + 1))) return false;  // fewer candidates than members still needed
        if (lane == d) {
            memb = x;
            mrank = rx;
        }
        if (lane == d + 1) {
            lsize = kept;
            lbase = -64;
            lmask = 0;
        }
        return true;
    };

    if (lane == 0) {
        memb = a;
        mrank = newid[a];
    }
    if (k == 1) {  // (v, N(v)) for every vertex
        if (only) {
            emit(0, a, 0, false);
        } else {
            long long dcap = 0;
            int32_t *dst = star_dst(&dcap);
            if (dst)
                for (long long i = lane; i < da && i < dcap; i += 64) dst[i] = adj[ab + i];
            emit(0, a, da, dst && da > dcap);
        }
    } else if (step(1, da, b, uni32(newid[b]))) {
        int d = 2;
        while (!failed) {
            const long long size = __shfl(int(lsize), d);  // a list is shorter than 2^31 ids
            long long cbeg = (long long)__shfl(int(lbase), d);
            unsigned long long m = kcs_shfl64(lmask, d);
            const int32_t *T = list_of(d);
            if (m == 0ull) {
                cbeg += 64;
                if (cbeg >= size) {
                    if (d == 2) break;
                    --d;
                    continue;
                }
                const long long i = cbeg + lane;
                const int32_t last = __shfl(mrank, d - 1);
                int32_t w = -1;
                bool c = false;
                if (i < size) {
                    w = T[i];
                    c = only ? true : newid[w] < last;
                }
                m = __ballot(c);
                if (only && d + 1 == k) {  // the last level of CLIQUES_ONLY: the whole chunk at once
                    emit_chunk(d, w, m);
                    m = 0ull;
                }
                if (lane == d) {
                    lbase = cbeg;
                    lmask = m;
                }
                continue;
            }
            const int bit = __builtin_ctzll(m);
            m &= m - 1ull;
            if (lane == d) lmask = m;
            const int32_t x = uni32(T[cbeg + bit]);
            if (step(d, size, x, uni32(newid[x]))) ++d;
        }
    }

    if (FILL) {
        if (failed || kc != my_cnt || run != my_mem) {
            if (lane == 0) kcs_flag(acc, kFlagMismatch);
        }
    } else if (lane == 0) {
        cnt[t] = kc;
        mem[t] = run;
        if (maxs > 0) atomicMax(&acc[kAccMax], (unsigned long long)maxs);
    }
}

struct StarPass1 : ListPass1 {  // task[0]: pivots, task[1]: first members (caller ids; -1 for k = 1)
    gmsx_kclique_star_list_info info{};
};
StarPass1 &pass1_cache() {
    static StarPass1 c;
    return c;
}
constexpr ListArena kArena{4ull << 30, "KCSTAR_SLAB_MB", int64_t(1) << 24};  // the option is a test hook: a small budget splits a small graph into many launches

template <bool FILL>
int run_pass(const gmsx_graph *g, const ListPass1 &p1, int k, uint32_t flags, int64_t *cnt, int64_t *mem, int32_t *out_cl, int64_t *out_soff,
             int32_t *out_star, int64_t cl_cap, int64_t star_cap, unsigned long long *acc, int *launches) {
    const int only = (flags & GMSX_KCSTAR_CLIQUES_ONLY) ? 1 : 0;
    return run_list_pass(p1, kArena, FILL ? 2 : 0, launches, [&](const Launch &l, void *arena, unsigned long long arena_words) {
        const unsigned blocks = unsigned((l.t1 - l.t0 + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL((k_kcstar_list<FILL>), dim3(blocks), dim3(64 * kWavesPerBlock), 0, ctx().stream, g->off, g->adj, g->newid,
                           p1.task[0].as<const int32_t>(), p1.task[1].as<const int32_t>(), p1.slab_off.as<const int64_t>(), l.t0, l.t1,
                           static_cast<int32_t *>(arena), arena_words, k, only, cnt, mem, p1.cbase.as<const int64_t>(), p1.mbase.as<const int64_t>(),
                           out_cl, out_soff, out_star, cl_cap, star_cap, acc);
    });
}

// pass 1 of (g, k, flags, part, nparts) into the cleared p1
int kcstar_pass1(const gmsx_graph *g, int k, uint32_t flags, int part, int nparts, StarPass1 &p1, double *ms, double *setup_ms, int *launches) {
    hipStream_t s = ctx().stream;
    const int64_t n = g->n, nnz = g->nnz;
    const auto h0 = std::chrono::steady_clock::now();
    // ---- task list: the shard's pivots by rank id (decreasing degree), each pivot's first members — its neighbours of a lower rank id — in
    // the order of its row (ascending caller id).  A pivot with fewer than k - 1 neighbours closes no clique.
    std::vector<int32_t> newid(static_cast<size_t>(n)), oldid(static_cast<size_t>(n)), adj(static_cast<size_t>(nnz));
    std::vector<int64_t> off(static_cast<size_t>(n + 1), 0);
    if (n > 0) {
        GMSX_HIP(hipMemcpyAsync(newid.data(), g->newid, size_t(n) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(oldid.data(), g->oldid, size_t(n) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(off.data(), g->off, size_t(n + 1) * 8, hipMemcpyDeviceToHost, s));
        if (nnz > 0 && k > 1) GMSX_HIP(hipMemcpyAsync(adj.data(), g->adj, size_t(nnz) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
    }
    std::vector<int32_t> task_a, task_b;
    p1.soff.assign(1, 0);
    for (int64_t r = 0; r < n; ++r) {
        if (shard_of(r, nparts) != part) continue;
        const int32_t a = oldid[size_t(r)];
        const int64_t b0 = off[size_t(a)], b1 = off[size_t(a) + 1];
        if (b1 - b0 < k - 1) continue;
        const int64_t need = kcs_need(k, b1 - b0);
        if (k == 1) {
            task_a.push_back(a);
            task_b.push_back(-1);
            p1.soff.push_back(p1.soff.back() + need);
            continue;
        }
        for (int64_t e = b0; e < b1; ++e) {
            const int32_t w = adj[size_t(e)];
            if (newid[size_t(w)] >= r) continue;
            task_a.push_back(a);
            task_b.push_back(w);
            p1.soff.push_back(p1.soff.back() + need);
        }
    }
    const std::vector<int32_t> *tasks[] = {&task_a, &task_b};
    if (int rc = upload_tasks(p1, tasks, 2, s)) return rc;
    const int64_t nt = p1.n_tasks;
    DevBuf cnt, mem, acc;
    if (int rc = alloc_zeroed(cnt, size_t(nt + 1) * 8, s)) return rc;
    if (int rc = alloc_zeroed(mem, size_t(nt + 1) * 8, s)) return rc;
    if (int rc = alloc_zeroed(acc, size_t(kAccWords) * 8, s)) return rc;
    GMSX_HIP(hipStreamSynchronize(s));
    *setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    if (int rc = run_pass<false>(g, p1, k, flags, cnt.as<int64_t>(), mem.as<int64_t>(), nullptr, nullptr, nullptr, 0, 0, acc.as<unsigned long long>(),
                                 launches))
        return rc;
    unsigned long long host[kAccWords];
    int64_t tot[2] = {0, 0};
    if (int rc = finish_count_pass(p1, cnt, mem, acc, host, kAccWords, tot, 0, ms)) return rc;
    if (host[kAccFlags]) return GMSX_ERR_KERNEL;
    gmsx_kclique_star_list_info info{};
    info.cliques = tot[0];
    info.star_members = tot[1];
    info.k = k;
    info.max_star = int32_t(host[kAccMax]);
    p1.info = info;
    return GMSX_OK;
}

int kcstar_list(const gmsx_graph *g, int k, uint32_t flags, int part, int nparts, int32_t *cliques, int64_t *star_offsets, int32_t *star_members,
                int64_t cliques_capacity, int64_t star_capacity, gmsx_kclique_star_list_info *info, gmsx_stats *st) {
    hipStream_t s = ctx().stream;
    StarPass1 &p1 = pass1_cache();
    const bool only = (flags & GMSX_KCSTAR_CLIQUES_ONLY) != 0;
    const bool sizing = cliques == nullptr && star_offsets == nullptr && star_members == nullptr;
    double ms1 = 0.0, ms2 = 0.0, setup = 0.0;
    int launches = 0;
    if (int rc = ensure_pass1(p1, ListKey(g->serial, g, g->off, g->adj, g->n, g->nnz, part, nparts, k, flags), sizing,
                              [&] { return kcstar_pass1(g, k, flags, part, nparts, p1, &ms1, &setup, &launches); }))
        return rc;
    *info = p1.info;
    if (!sizing) {
        const int64_t nc = p1.info.cliques, nm = p1.info.star_members;
        if (!cliques || cliques_capacity < nc) return GMSX_ERR_INVALID;
        if (!only && (!star_offsets || star_capacity < nm || (nm > 0 && !star_members))) return GMSX_ERR_INVALID;
        DevBuf d_cl, d_soff, d_star, acc;
        GMSX_HIP(hipMalloc(&d_cl.p, size_t(nc > 0 ? nc : 1) * size_t(k) * 4));
        GMSX_HIP(hipMalloc(&d_soff.p, size_t(nc + 1) * 8));
        GMSX_HIP(hipMalloc(&d_star.p, size_t(nm > 0 ? nm : 1) * 4));
        if (int rc = alloc_zeroed(acc, size_t(kAccWords) * 8, s)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_soff.as<int64_t>() + nc, &nm, 8, hipMemcpyHostToDevice, s));
        if (int rc = run_pass<true>(g, p1, k, flags, nullptr, nullptr, d_cl.as<int32_t>(), d_soff.as<int64_t>(), d_star.as<int32_t>(), nc, nm,
                                    acc.as<unsigned long long>(), &launches))
            return rc;
        unsigned long long host[kAccWords];
        if (int rc = finish_fill_pass(acc, host, kAccWords, 2, &ms2)) return rc;
        if (host[kAccFlags]) return GMSX_ERR_KERNEL;
        // the caller's buffers are written only now, on success
        if (nc > 0) GMSX_HIP(hipMemcpyAsync(cliques, d_cl.p, size_t(nc) * size_t(k) * 4, hipMemcpyDeviceToHost, s));
        if (!only) {
            GMSX_HIP(hipMemcpyAsync(star_offsets, d_soff.p, size_t(nc + 1) * 8, hipMemcpyDeviceToHost, s));
            if (nm > 0) GMSX_HIP(hipMemcpyAsync(star_members, d_star.p, size_t(nm) * 4, hipMemcpyDeviceToHost, s));
        }
        GMSX_HIP(hipStreamSynchronize(s));
    }
    if (st) *st = gmsx_stats{ms1 + ms2, setup, uint64_t(p1.n_tasks), 0, 0, launches, 0, 0};
    return GMSX_OK;
}

}  // namespace

}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_kclique_star_list(const gmsx_graph *g, int k, uint32_t flags, int part, int nparts, int32_t *cliques, int64_t *star_offsets,
                           int32_t *star_members, int64_t cliques_capacity, int64_t star_capacity, gmsx_kclique_star_list_info *info,
                           gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || k < 1 || nparts < 1 || part < 0 || part >= nparts || cliques_capacity < 0 || star_capacity < 0) return GMSX_ERR_INVALID;
        if (flags & ~uint32_t(GMSX_KCSTAR_CLIQUES_ONLY)) return GMSX_ERR_INVALID;
        if ((flags & GMSX_KCSTAR_CLIQUES_ONLY) && (star_offsets || star_members)) return GMSX_ERR_INVALID;
        if (k > 63) return GMSX_ERR_UNSUPPORTED;
        if (int rc = ensure_init()) return rc;
        return kcstar_list(g, k, flags, part, nparts, cliques, star_offsets, star_members, cliques_capacity, star_capacity, info, stats);
    });
}

}  // extern "C"
