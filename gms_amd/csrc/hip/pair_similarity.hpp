// The per-pair operators over full CSR rows that more than one translation unit needs (pairs.hip, linkpred.hip): one wave per pair.
//   wave_intersect_count   |N(u) ∩ N(v)|, the 64 lanes stream the SHORTER row and binary-search each id in the longer one
//   wave_pair_similarity   GMS::VertexSim::vertex_similarity<Metric> (vertex_similarity/vertex_similarity.h:30-222) of one pair
// A score is a function of the pair and the graph alone — lane order and shuffle tree of the Adamic-Adar / resource sums included — so every
// caller of wave_pair_similarity gets the bits gmsx_vertex_similarity_batch returns.
#pragma once
#include "device_graph.hpp"

namespace gmsx {

// |A ∩ B| for two ascending rows; wave-uniform arguments; returns the wave-uniform count
__device__ __forceinline__ uint32_t wave_intersect_count(const int32_t *__restrict__ a, int64_t la, const int32_t *__restrict__ b,
                                                         int64_t lb, int lane) {
    if (la > lb) {  // stream the shorter, search the longer
        const int32_t *t = a; a = b; b = t;
        const int64_t tl = la; la = lb; lb = tl;
    }
    uint32_t cnt = 0;
    for (int64_t base = 0; base < la; base += 64) {
        const int64_t i = base + lane;
        bool hit = false;
        if (i < la) {
            const int32_t x = a[i];
            int64_t lo = 0, hi = lb;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (b[mid] < x) lo = mid + 1; else hi = mid;
            }
            hit = lo < lb && b[lo] == x;
        }
        cnt += uint32_t(__popcll(__ballot(hit)));
    }
    return cnt;
}

// metric(N(u), N(v)) for in-range u, v; wave-uniform arguments, the whole wave calls it; returns the wave-uniform score.  Count-based
// metrics reuse wave_intersect_count; Adamic-Adar / resource allocation add a per-common-neighbour term while intersecting.
__device__ __forceinline__ double wave_pair_similarity(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, int metric, int32_t u,
                                                       int32_t v, int lane) {
    const int32_t *a = adj + off[u], *b = adj + off[v];
    int64_t la = off[u + 1] - off[u], lb = off[v + 1] - off[v];
    const double ca = double(la), cb = double(lb);
    double r;
    if (metric == GMSX_SIM_ADAMIC_ADAR || metric == GMSX_SIM_RESOURCE) {
        if (la > lb) {
            const int32_t *t = a; a = b; b = t;
            const int64_t tl = la; la = lb; lb = tl;
        }
        double sum = 0.0;
        for (int64_t base = 0; base < la; base += 64) {
            const int64_t i = base + lane;
            if (i < la) {
                const int32_t x = a[i];
                int64_t lo = 0, hi = lb;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (b[mid] < x) lo = mid + 1; else hi = mid;
                }
                if (lo < lb && b[lo] == x) {
                    const double deg = double(off[x + 1] - off[x]);
                    sum += metric == GMSX_SIM_ADAMIC_ADAR ? 1.0 / log(deg) : 1.0 / deg;
                }
            }
        }
        sum = wave_sum_all(sum);
        r = sum;
    } else {
        const double cnt = double(wave_intersect_count(a, la, b, lb, lane));
        switch (metric) {
            case GMSX_SIM_JACCARD: r = (la == 0 && lb == 0) ? 1.0 : cnt / (ca + cb + cnt); break;   // sic, vertex_similarity.h:31-36
            case GMSX_SIM_OVERLAP: r = cnt / (ca < cb ? ca : cb); break;                              // :66-68
            case GMSX_SIM_COMMON_NEIGHBORS: r = cnt; break;                                           // :139-143
            case GMSX_SIM_TOTAL_NEIGHBORS: r = ca + cb - cnt; break;                                  // union_count, :155-159
            default: r = ca * cb; break;                                                              // :171-174
        }
    }
    return r;
}

}  // namespace gmsx
