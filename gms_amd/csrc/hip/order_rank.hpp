// An order as the kernels consume it — rank[] on the device, validated — and later[v] = |{ w in N(v) : rank[w] > rank[v] }|: shared by
// gmsx_order_quality (core.hip: the count IS the grade) and gmsx_coloring_jp (coloring.hip: the count is the predecessor counter of
// Jones–Plassmann).  later[] is counted over ALL vertices with the row binning of frontier_rounds.hpp: a kGroup-lane group per row up to
// kLongRow entries, longer rows parked and walked by all workgroups together.
#pragma once
#include "frontier_rounds.hpp"

namespace gmsx {
namespace {

// ordering -> rank[] (device) + validation: every entry in [0, n) and hit once
__global__ void k_oq_rank(int64_t n, const int32_t *__restrict__ ordering, int rank_format, int32_t *__restrict__ rank, int32_t *__restrict__ seen,
                          int32_t *__restrict__ bad) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t x = ordering[i];
    if (x < 0 || int64_t(x) >= n) {
        *bad = 1;
        return;
    }
    if (atomicAdd(&seen[x], 1) != 0) *bad = 1;
    if (!rank_format) rank[x] = int32_t(i);  // ordering[i] = i-th vertex
}

// later[v] = |{ w in N(v) : rank[w] > rank[v] }|: a 16-lane group per vertex, rows above kLongRow parked for k_oq_later_long
__global__ __launch_bounds__(256) void k_oq_later(int64_t n, const int64_t *__restrict__ off, const int32_t *__restrict__ adj,
                                                  const int32_t *__restrict__ rank, int32_t *__restrict__ later, int32_t *__restrict__ longs,
                                                  int64_t long_cap, int32_t *__restrict__ ctl /* [0] long rows, [1] error */) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t group0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) / kGroup;
    const int64_t groups = (int64_t(gridDim.x) * blockDim.x) / kGroup;
    const int64_t end = ((n + 3) / 4) * 4;  // the four groups of a wave stay together for the shuffles
    for (int64_t v = group0; v < end; v += groups) {
        int32_t cnt = 0;
        if (v < n) {
            const int64_t j0 = off[v], j1 = off[v + 1];
            if (j1 - j0 > kLongRow) {
                if (lane == 0) {
                    later[v] = 0;
                    append_checked(longs, &ctl[0], long_cap, int32_t(v), &ctl[1]);
                }
                cnt = -1;
            } else {
                const int32_t rv = rank[v];
                for (int64_t j = j0 + lane; j < j1; j += kGroup) cnt += rank[adj[j]] > rv ? 1 : 0;
            }
        }
        const bool parked = cnt < 0;
        if (parked) cnt = 0;
        cnt = wave_sum<kGroup>(cnt);
        if (v < n && lane == 0 && !parked) later[v] = cnt;
    }
}
__global__ __launch_bounds__(256) void k_oq_later_long(const int64_t *__restrict__ off, const int32_t *__restrict__ adj, const int32_t *__restrict__ rank,
                                                       int32_t *__restrict__ later, const int32_t *__restrict__ longs, int64_t long_cap,
                                                       const int32_t *__restrict__ ctl) {
    const int64_t nlong = min(int64_t(ctl[0]), long_cap);
    const int64_t tid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, threads = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = 0; i < nlong; ++i) {
        const int32_t v = longs[i];
        const int32_t rv = rank[v];
        const int64_t j0 = off[v], j1 = off[v + 1];
        int32_t cnt = 0;
        for (int64_t j = j0 + tid; j < j1; j += threads) cnt += rank[adj[j]] > rv ? 1 : 0;
        cnt = wave_sum(cnt);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&later[v], cnt);
    }
}

}  // namespace
}  // namespace gmsx
