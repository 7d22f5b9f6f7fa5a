// Bron–Kerbosch maximal-clique LISTING on gfx950: the device replacement for
//   BkEppsteinPar::mceBench   gms/algorithms/set_based/maximal_clique_enum/parallel/eppsteinPAR.h:18-53
//   BkTomita::expand          gms/algorithms/set_based/maximal_clique_enum/sequential/tomita.h:12-86
// compiled WITHOUT -DBK_COUNT (the listing build: every maximal clique is put into `sol`, tomita.h:79-84).
//
// The formulation is the count's (bk.hip): start vertex v (rank id r) searches with cand = the oriented row N+(r) and fini = the
// in-neighbours N-(r); inside a search all sets are bitmaps over that local universe — Cadj (c x c bits), XT (c rows of x bits), and per
// level P, Xc (finished candidates), Xf (finished in-neighbours) and ext = P \ Cadj[pivot].  The pivot is argmax popc(P & Cadj[u]) over
// u in P ∪ Xc, ties to the lowest local index.  In addition the chosen local indices R are kept, one word per level; at a leaf
// (P, Xc, Xf all empty) the wave maps {v} ∪ R through N+(r) and oldid to the caller's ids, ranks them by count and stores them ascending.
//
// One wave per start vertex; every structure of a search lives in its own slab of a global arena (Cadj | XT | levels | R).  The task list is
// the shard's start vertices in rank-id order, i.e. by decreasing degree; the two passes over it (count: cliques and member total per task,
// size histogram and largest clique per call; scan; fill), the launches that fit the arena budget (test hook BK_LIST_ARENA_MB) and the
// pass-1 cache are the scaffold of two_pass_list.hpp.  Nothing that shapes the search depends on timing (pivot ties by index, DFS order by
// index), which is what that scheme asks of a kernel.
#include "rank_check.hpp"
#include "two_pass_list.hpp"

#include <algorithm>
#include <vector>

namespace gmsx {

namespace {

constexpr int kListBins = 65;                   // size histogram: [s] for s < 64, [64] = 64 or more
constexpr int kListMax = kListBins;             // acc[kListMax]: largest clique
constexpr int kListFlags = kListBins + 1;       // acc[kListFlags]: error bits below
constexpr int kListAcc = kListBins + 2;
constexpr unsigned long long kFlagSlab = 1, kFlagOut = 2, kFlagMismatch = 4, kFlagShape = 8;

// words of one start vertex's slab: cand ids (c) | fini ids (x) | Cadj (c*cw) | XT (c*xw) | c+1 levels of P, Xc, ext (cw each), Xf (xw)
// | R (c+1) | member scratch (c+1); 16-byte multiple
__host__ __device__ inline unsigned long long bkl_need(long long c, long long x) {
    const long long cw = (c + 31) / 32, xw = (x + 31) / 32;
    const long long w = c + x + c * cw + c * xw + (c + 1) * (3 * cw + xw) + 2 * (c + 1);
    return (unsigned long long)((w + 3) & ~3ll);
}

__device__ __forceinline__ void bkl_flag(unsigned long long *acc, unsigned long long f) { atomicOr(&acc[kListFlags], f); }

// local index of rank id t in the ascending candidate list, or -1
__device__ __forceinline__ int bkl_find(const uint32_t *cand, int c, uint32_t t) {
    int lo = 0, hi = c;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cand[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo < c && cand[lo] == t ? lo : -1;
}

// lowest set bit of E (cw words) above bit `cur` (cur < 0: from bit 0), or -1.  Lane l reads the words congruent to l mod 64 — the
// words it wrote itself — so no fence is needed between writing E and scanning it.
__device__ __forceinline__ long long bkl_next(const uint32_t *E, long long cw, long long cur, int lane) {
    const long long first = cur < 0 ? 0 : (cur >> 5);
    for (long long base = first & ~63ll; base < cw; base += 64) {
        const long long i = base + lane;
        uint32_t w = 0;
        if (i < cw && i >= first) {
            w = E[i];
            if (i == first && cur >= 0) w &= (cur & 31) == 31 ? 0u : (~0u << ((cur & 31) + 1));
        }
        const unsigned long long b = __ballot(w != 0);
        if (b) {
            const int l = __builtin_ctzll(b);
            const uint32_t ww = uint32_t(__builtin_amdgcn_readlane(int(w), l));
            return (base + l) * 32 + __builtin_ctz(ww);
        }
    }
    return -1;
}

// Tomita pivot of level (P, Xc) — argmax over u in P ∪ Xc of popc(P & Cadj[u]), lowest u on ties — and ext = P \ Cadj[pivot] into E
__device__ __forceinline__ void bkl_pivot(const uint32_t *P, const uint32_t *Xc, uint32_t *E, const uint32_t *Cadj, long long c, long long cw,
                                          int lane) {
    unsigned long long key = 0;
    for (long long u = lane; u < c; u += 64) {
        const uint32_t bit = 1u << (u & 31);
        if (!((P[u >> 5] | Xc[u >> 5]) & bit)) continue;
        const uint32_t *row = Cadj + u * cw;
        unsigned s = 0;
        for (long long w = 0; w < cw; ++w) s += __popc(P[w] & row[w]);
        const unsigned long long k = (static_cast<unsigned long long>(s + 1) << 32) | (0xFFFFFFFFu - uint32_t(u));
        key = k > key ? k : key;
    }
    key = wave_max_all_halves(key);
    const long long piv = (long long)(0xFFFFFFFFu - uint32_t(key));
    const uint32_t *prow = Cadj + piv * cw;
    for (long long i = lane; i < cw; i += 64) E[i] = P[i] & ~prow[i];
}

// One wave per task.  FILL = false: cnt[t], mem[t] and the per-call histogram / maximum.  FILL = true: the cliques, task t's at
// out_off[cbase[t] ...] and out_mem[mbase[t] ...]; cbase / mbase are the exclusive scans of pass 1's cnt / mem (n_tasks + 1 entries).
template <bool FILL>
__global__ __launch_bounds__(64) void k_bk_list(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const int32_t *__restrict__ newid,
                                                const int32_t *__restrict__ oldid, const int64_t *__restrict__ hoff, const uint16_t *__restrict__ hadj,
                                                const int64_t *__restrict__ toff, const int32_t *__restrict__ tadj, const int32_t *__restrict__ dplus,
                                                const int32_t *__restrict__ task_r, const int64_t *__restrict__ slab_off, int64_t t0, int64_t t1,
                                                uint32_t *arena, unsigned long long arena_words, int64_t *__restrict__ cnt,
                                                int64_t *__restrict__ mem, const int64_t *__restrict__ cbase, const int64_t *__restrict__ mbase,
                                                int64_t *__restrict__ out_off, int32_t *__restrict__ out_mem, int64_t off_cap, int64_t mem_cap,
                                                unsigned long long *__restrict__ acc) {
    const int64_t t = t0 + int64_t(blockIdx.x);
    if (t >= t1) return;
    const int lane = int(threadIdx.x);
    const int32_t r = task_r[t];
    const long long c = dplus[r];
    const int32_t o = oldid[r];
    const long long deg = off[o + 1] - off[o];
    const long long x = deg - c;
    const unsigned long long base = (unsigned long long)(slab_off[t] - slab_off[t0]);
    const unsigned long long need = (unsigned long long)(slab_off[t + 1] - slab_off[t]);
    if (x < 0 || need < bkl_need(c, x) || base + need > arena_words) {
        if (lane == 0) bkl_flag(acc, kFlagSlab);
        return;
    }
    const long long cw = (c + 31) / 32, xw = (x + 31) / 32;
    const long long lvl = 3 * cw + xw;
    uint32_t *const cand = arena + base;
    uint32_t *const fini = cand + c;
    uint32_t *const Cadj = fini + x;
    uint32_t *const XT = Cadj + c * cw;
    uint32_t *const L = XT + c * xw;
    uint32_t *const Rst = L + (c + 1) * lvl;
    uint32_t *const ids = Rst + (c + 1);

    // task bookkeeping (uniform)
    long long k = 0, run = 0, maxs = 0;
    unsigned long long hcount = 0;  // lane l: cliques of size l (l >= 1), lane 0: of size 64 or more
    long long my_cnt = 0, my_mem = 0, cb = 0, mb = 0;
    if (FILL) {
        cb = cbase[t];
        mb = mbase[t];
        my_cnt = cbase[t + 1] - cb;
        my_mem = mbase[t + 1] - mb;
    }
    bool failed = false;

    // a maximal clique {v} ∪ cand[R[0 .. s-2]] of s members
    auto emit = [&](long long s) {
        if (FILL) {
            if (k >= my_cnt || run + s > my_mem) {
                failed = true;
            } else {
                const long long pos = mb + run, ci = cb + k;
                if (ci >= off_cap || pos + s > mem_cap) {
                    if (lane == 0) bkl_flag(acc, kFlagOut);
                } else {
                    if (lane == 0) out_off[ci] = pos;
                    if (s <= 64) {
                        int32_t id = 0;
                        if (lane < s) id = lane == 0 ? o : oldid[cand[Rst[lane - 1]]];
                        int rk = 0;
                        for (int j = 0; j < int(s); ++j) rk += __shfl(id, j) < id ? 1 : 0;
                        if (lane < s) out_mem[pos + rk] = id;
                    } else {
                        for (long long i = lane; i < s; i += 64) ids[i] = uint32_t(i == 0 ? o : oldid[cand[Rst[i - 1]]]);
                        wave_slab_sync();
                        for (long long i = lane; i < s; i += 64) {
                            const int32_t me = int32_t(ids[i]);
                            long long rk = 0;
                            for (long long j = 0; j < s; ++j) rk += int32_t(ids[j]) < me ? 1 : 0;
                            out_mem[pos + rk] = me;
                        }
                        wave_slab_sync();
                    }
                }
            }
        } else {
            const int bin = s < 64 ? int(s) : 0;
            if (lane == bin) ++hcount;
            maxs = s > maxs ? s : maxs;
        }
        ++k;
        run += s;
    };

    if (c == 0) {
        if (x == 0) emit(1);  // an isolated vertex is a maximal clique (eppsteinPAR.h:32-47, tomita.h:73-78)
    } else {
        // ---- local universe: cand = N+(r) ascending (hub part, then tail part), fini = N-(r) in CSR order
        long long nc = 0;
        {
            const int64_t hb = hoff[r], he = hoff[r + 1];
            for (int64_t j0 = hb; j0 < he; j0 += 64) {
                const int64_t j = j0 + lane;
                const uint32_t w = j < he ? uint32_t(hadj[j]) : 0xFFFFu;
                const bool keep = w != 0xFFFFu;
                const unsigned long long b = __ballot(keep);
                const long long at = nc + __popcll(b & ((1ull << lane) - 1ull));
                if (keep && at < c) cand[at] = w;
                nc += __popcll(b);
            }
            const int64_t tb = toff[r], te = toff[r + 1];
            for (int64_t j = tb + lane; j < te; j += 64) {
                const long long at = nc + (j - tb);
                if (at < c) cand[at] = uint32_t(tadj[j]);
            }
            nc += te - tb;
        }
        long long nx = 0;
        {
            const int64_t b0 = off[o];
            for (int64_t j0 = 0; j0 < deg; j0 += 64) {
                const int64_t j = j0 + lane;
                const int32_t w = j < deg ? newid[adj[b0 + j]] : -1;
                const bool keep = w > r;
                const unsigned long long b = __ballot(keep);
                const long long at = nx + __popcll(b & ((1ull << lane) - 1ull));
                if (keep && at < x) fini[at] = uint32_t(w);
                nx += __popcll(b);
            }
        }
        if (nc != c || nx != x) {
            if (lane == 0) bkl_flag(acc, kFlagShape);
            return;
        }
        for (long long i = lane; i < c * (cw + xw); i += 64) Cadj[i] = 0u;  // Cadj and XT are contiguous
        wave_slab_sync();
        // ---- Cadj | XT: every neighbour's oriented row, up to rank id r (nothing at or above r is a candidate); a lane per row
        for (long long jj = lane; jj < c + x; jj += 64) {
            const bool is_c = jj < c;
            const long long idx = is_c ? jj : jj - c;
            const uint32_t w = is_c ? cand[idx] : fini[idx];
            auto hit = [&](uint32_t tgt) {
                const int j = bkl_find(cand, int(c), tgt);
                if (j < 0) return;
                if (is_c) {
                    atomicOr(&Cadj[idx * cw + (j >> 5)], 1u << (j & 31));
                    atomicOr(&Cadj[(long long)j * cw + (idx >> 5)], 1u << (idx & 31));
                } else {
                    atomicOr(&XT[(long long)j * xw + (idx >> 5)], 1u << (idx & 31));
                }
            };
            bool done = false;
            for (int64_t e = hoff[w], ee = hoff[w + 1]; e < ee; ++e) {
                const uint32_t tgt = hadj[e];
                if (tgt == 0xFFFFu) continue;
                if (tgt >= uint32_t(r)) { done = true; break; }
                hit(tgt);
            }
            if (!done) {
                for (int64_t e = toff[w], ee = toff[w + 1]; e < ee; ++e) {
                    const uint32_t tgt = uint32_t(tadj[e]);
                    if (tgt >= uint32_t(r)) break;
                    hit(tgt);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // the atomics were performed in L2: drop L1 lines of the slab
        __builtin_amdgcn_wave_barrier();

        // ---- level 0: P = cand, Xc = {}, Xf = fini
        {
            uint32_t *P = L, *Xc = L + cw, *Xf = L + 3 * cw;
            for (long long i = lane; i < cw; i += 64) {
                P[i] = (i < cw - 1 || (c & 31) == 0) ? ~0u : ((1u << (c & 31)) - 1u);
                Xc[i] = 0u;
            }
            for (long long i = lane; i < xw; i += 64) Xf[i] = (i < xw - 1 || (x & 31) == 0) ? ~0u : ((1u << (x & 31)) - 1u);
            if (lane == 0) Rst[0] = 0xFFFFFFFFu;
            wave_slab_sync();
            bkl_pivot(P, Xc, L + 2 * cw, Cadj, c, cw, lane);
        }
        long long d = 0;
        while (!failed) {
            uint32_t *P = L + d * lvl, *Xc = P + cw, *E = P + 2 * cw, *Xf = P + 3 * cw;
            const uint32_t cur_raw = Rst[d];
            const long long cur = cur_raw == 0xFFFFFFFFu ? -1 : (long long)cur_raw;
            const long long q = bkl_next(E, cw, cur, lane);
            if (q < 0) {
                if (d == 0) break;
                --d;
                continue;
            }
            const long long qw = q >> 5;
            const uint32_t qb = 1u << (q & 31);
            if (lane == int(qw & 63)) {  // the owner lane of that word
                P[qw] &= ~qb;
                Xc[qw] |= qb;
            }
            if (lane == 0) Rst[d] = uint32_t(q);
            if (d + 1 > c) {  // cannot happen (every level adds a candidate to R): never step past the slab
                if (lane == 0) bkl_flag(acc, kFlagSlab);
                failed = true;
                break;
            }
            uint32_t *Pn = P + lvl, *Xcn = Pn + cw, *Xfn = Pn + 3 * cw;
            const uint32_t *row = Cadj + q * cw;
            const uint32_t *xrow = XT + q * xw;
            bool anyP = false, anyX = false;
            for (long long i = lane; i < cw; i += 64) {
                const uint32_t p = P[i] & row[i], xc = Xc[i] & row[i];
                Pn[i] = p;
                Xcn[i] = xc;
                anyP |= p != 0u;
                anyX |= xc != 0u;
            }
            for (long long i = lane; i < xw; i += 64) {
                const uint32_t xf = Xf[i] & xrow[i];
                Xfn[i] = xf;
                anyX |= xf != 0u;
            }
            const bool wP = __ballot(anyP) != 0ull, wX = __ballot(anyX) != 0ull;
            wave_slab_sync();
            if (!wP) {
                if (!wX) emit(d + 2);
                continue;
            }
            ++d;
            if (lane == 0) Rst[d] = 0xFFFFFFFFu;
            bkl_pivot(Pn, Xcn, Pn + 2 * cw, Cadj, c, cw, lane);
            wave_slab_sync();
        }
    }

    if (FILL) {
        if (failed || k != my_cnt || run != my_mem) {
            if (lane == 0) bkl_flag(acc, kFlagMismatch);
        }
    } else {
        if (lane == 0) {
            cnt[t] = k;
            mem[t] = run;
            if (maxs > 0) atomicMax(&acc[kListMax], (unsigned long long)maxs);
        }
        if (hcount) atomicAdd(&acc[lane == 0 ? 64 : lane], hcount);
    }
}

struct BkListPass1 : ListPass1 {  // task[0]: the start vertices' rank ids
    gmsx_bk_list_info info{};
};
BkListPass1 &pass1_cache() {
    static BkListPass1 c;
    return c;
}
constexpr ListArena kArena{8ull << 30, "BK_LIST_ARENA_MB", kNoTaskCap};  // the option is a test hook: a small arena splits a small graph into many launches

template <bool FILL>
int run_pass(const gmsx_graph *g, const ListPass1 &p1, int64_t *cnt, int64_t *mem, int64_t *out_off, int32_t *out_mem, int64_t off_cap,
             int64_t mem_cap, unsigned long long *acc, int *launches) {
    return run_list_pass(p1, kArena, FILL ? 2 : 0, launches, [&](const Launch &l, void *arena, unsigned long long arena_words) {
        hipLaunchKernelGGL((k_bk_list<FILL>), dim3(unsigned(l.t1 - l.t0)), dim3(64), 0, ctx().stream, g->off, g->adj, g->newid, g->oldid, g->hoff,
                           g->hadj, g->toff, g->tadj, g->dplus, p1.task[0].as<const int32_t>(), p1.slab_off.as<const int64_t>(), l.t0, l.t1,
                           static_cast<uint32_t *>(arena), arena_words, cnt, mem, p1.cbase.as<const int64_t>(), p1.mbase.as<const int64_t>(), out_off,
                           out_mem, off_cap, mem_cap, acc);
    });
}

// pass 1 of (g, part, nparts) into the cleared p1
int bk_list_pass1(const gmsx_graph *g, int part, int nparts, BkListPass1 &p1, double *ms, int *launches) {
    hipStream_t s = ctx().stream;
    const int64_t n = g->n;
    // ---- task list: the shard's start vertices that yield a clique or a search, by rank id (decreasing degree: heavy first)
    std::vector<int32_t> dplus(static_cast<size_t>(n)), oldid(static_cast<size_t>(n));
    std::vector<int64_t> off(static_cast<size_t>(n + 1));
    if (n > 0) {
        GMSX_HIP(hipMemcpyAsync(dplus.data(), g->dplus, size_t(n) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(oldid.data(), g->oldid, size_t(n) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipMemcpyAsync(off.data(), g->off, size_t(n + 1) * 8, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
    }
    std::vector<int32_t> task_r;
    p1.soff.assign(1, 0);
    for (int64_t r = 0; r < n; ++r) {
        if (shard_of(r, nparts) != part) continue;
        const long long c = dplus[size_t(r)];
        const int32_t o = oldid[size_t(r)];
        const long long x = off[size_t(o) + 1] - off[size_t(o)] - c;
        if (c == 0 && x > 0) continue;  // every clique through v has a member of higher rank: another start vertex lists it
        task_r.push_back(int32_t(r));
        p1.soff.push_back(p1.soff.back() + int64_t(bkl_need(c, x)));
    }
    const std::vector<int32_t> *tasks[] = {&task_r};
    if (int rc = upload_tasks(p1, tasks, 1, s)) return rc;
    const int64_t nt = p1.n_tasks;
    DevBuf cnt, mem, acc;
    if (int rc = alloc_zeroed(cnt, size_t(nt + 1) * 8, s)) return rc;
    if (int rc = alloc_zeroed(mem, size_t(nt + 1) * 8, s)) return rc;
    if (int rc = alloc_zeroed(acc, size_t(kListAcc) * 8, s)) return rc;
    if (int rc = run_pass<false>(g, p1, cnt.as<int64_t>(), mem.as<int64_t>(), nullptr, nullptr, 0, 0, acc.as<unsigned long long>(), launches)) return rc;
    unsigned long long host[kListAcc];
    int64_t tot[2] = {0, 0};
    if (int rc = finish_count_pass(p1, cnt, mem, acc, host, kListAcc, tot, 0, ms)) return rc;
    if (host[kListFlags]) return GMSX_ERR_KERNEL;
    gmsx_bk_list_info info{};
    info.cliques = tot[0];
    info.members = tot[1];
    info.max_size = int32_t(host[kListMax]);
    for (int b = 0; b < kListBins; ++b) info.size_hist[b] = int64_t(host[b]);
    info.size_hist[0] = 0;
    p1.info = info;
    return GMSX_OK;
}

int bk_list(const gmsx_graph *g, int part, int nparts, int64_t *offsets, int32_t *members, int64_t offsets_capacity, int64_t members_capacity,
            gmsx_bk_list_info *info, gmsx_stats *st) {
    hipStream_t s = ctx().stream;
    BkListPass1 &p1 = pass1_cache();
    const bool sizing = offsets == nullptr && members == nullptr;
    double ms1 = 0.0, ms2 = 0.0;
    int launches = 0;
    if (int rc = ensure_pass1(p1, ListKey(g->serial, g, g->off, g->adj, g->n, g->nnz, part, nparts), sizing, [&] { return bk_list_pass1(g, part, nparts, p1, &ms1, &launches); })) return rc;
    *info = p1.info;
    if (!sizing) {
        const int64_t nc = p1.info.cliques, nm = p1.info.members;
        if (!offsets || offsets_capacity < nc + 1 || members_capacity < nm || (nm > 0 && !members)) return GMSX_ERR_INVALID;
        DevBuf d_off, d_mem, acc;
        GMSX_HIP(hipMalloc(&d_off.p, size_t(nc + 1) * 8));
        GMSX_HIP(hipMalloc(&d_mem.p, size_t(nm > 0 ? nm : 1) * 4));
        if (int rc = alloc_zeroed(acc, size_t(kListAcc) * 8, s)) return rc;
        GMSX_HIP(hipMemcpyAsync(d_off.as<int64_t>() + nc, &nm, 8, hipMemcpyHostToDevice, s));
        if (int rc = run_pass<true>(g, p1, nullptr, nullptr, d_off.as<int64_t>(), d_mem.as<int32_t>(), nc, nm, acc.as<unsigned long long>(), &launches))
            return rc;
        unsigned long long host[kListAcc];
        if (int rc = finish_fill_pass(acc, host, kListAcc, 2, &ms2)) return rc;
        if (host[kListFlags]) return GMSX_ERR_KERNEL;
        // the caller's buffers are written only now, on success
        GMSX_HIP(hipMemcpyAsync(offsets, d_off.p, size_t(nc + 1) * 8, hipMemcpyDeviceToHost, s));
        if (nm > 0) GMSX_HIP(hipMemcpyAsync(members, d_mem.p, size_t(nm) * 4, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
    }
    if (st) *st = gmsx_stats{ms1 + ms2, 0.0, uint64_t(p1.n_tasks), 0, 0, launches, 0, 0};
    return GMSX_OK;
}

}  // namespace

}  // namespace gmsx

using namespace gmsx;

extern "C" {

int gmsx_bk_list(const gmsx_graph *g, const int32_t *rank, int part, int nparts, int64_t *offsets, int32_t *members, int64_t offsets_capacity,
                 int64_t members_capacity, gmsx_bk_list_info *info, gmsx_stats *stats) {
    return gmsx::guard([&]() -> int {
        if (!g || !info || nparts < 1 || part < 0 || part >= nparts || offsets_capacity < 0 || members_capacity < 0) return GMSX_ERR_INVALID;
        if (rank)  // validated as gmsx_bk_partial does; the set of maximal cliques does not depend on it
            if (int rc = check_rank_permutation(rank, g->n)) return rc;
        if (int rc = ensure_init()) return rc;
        return bk_list(g, part, nparts, offsets, members, offsets_capacity, members_capacity, info, stats);
    });
}

}  // extern "C"
