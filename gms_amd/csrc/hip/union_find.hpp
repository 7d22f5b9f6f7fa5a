// The device union-find of the library, stated once: connected components and Jarvis–Patrick clustering (components.hip) and the Borůvka
// rounds of the minimum spanning forest (msf.hip) link through it.
//
// THE UNION-FIND.  parent[n] (int32, a DevBuf of the call; the handle is not touched), parent[v] = v at the start.  THE ONE RULE: a root is
// only ever hooked under a SMALLER vertex id — link(u, v) walks to both roots and, where they differ, does atomicCAS(&parent[larger], larger,
// smaller) at device scope; when the CAS fails (the larger root was hooked meanwhile) it walks again from the two roots it held.  So
//   - parents only decrease, and every value parent[x] ever holds is an ancestor-or-self of x in every later state (a stale read is still an
//     ancestor: correctness never depends on freshness);
//   - the root of a finished tree is the smallest id of its component;
//   - after a full flatten label[v] is the smallest vertex id of v's component: a fact about the edge set, independent of the arrival order of
//     the atomics.
// MEMORY MODEL.  The L2s of the eight XCDs are not coherent for plain loads inside one kernel, and a plain load may be served from a CU's L1 for
// good.  Every read of parent inside a walk or a retry loop is a relaxed agent-scope atomic load (load_now), every compression write an
// atomicMin (linking kernels, where other threads hook and compress the same word) or a relaxed agent-scope store (flatten kernels, where a
// word has one writer).  No loop spins on a cached value, and NO LOOP IS UNBOUNDED: a walk strictly descends, so it takes fewer than n steps; a
// retry follows a failed CAS, i.e. a root that stopped being one, which happens fewer than n times to the roots one link holds.  Both loops
// carry the cap n + 64, and exceeding it (memory that is not a parent array any more) raises the call's flag word: GMSX_ERR_KERNEL.
//
// FLATTEN (k_cc_flatten): every vertex walks up to kCcJump steps and stores where it got; a round in which every walk reached a root changes
// nothing afterwards.  The host reads the flag between launches (a path of 2^20 vertices hooked into one chain needs four rounds).
// SIZES (k_cc_sizes): size[label[v]] by atomicAdd, one add per distinct label of a wave (in the giant component that is one add per wave).
#pragma once
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "frontier_rounds.hpp"  // load_now, store_now

#include <algorithm>
#include <climits>

namespace gmsx {
namespace {

constexpr int kCcJump = 64;        // steps of one flatten walk
constexpr int kCcFlattenMax = 64;  // flatten rounds before the call gives up (every round divides the depth by kCcJump)

// the cap of both loops for a parent array of n words: what cc_find and cc_link are given
__host__ __device__ __forceinline__ uint32_t cc_walk_cap(int64_t n) { return uint32_t(n + 64 < int64_t(INT_MAX) ? n + 64 : int64_t(INT_MAX)); }

// root of x; compresses by halving on the way (atomicMin: other threads hook and compress the same words, and parents only decrease)
__device__ __forceinline__ int32_t cc_find(int32_t *__restrict__ parent, int32_t x, uint32_t cap, int32_t *error) {
    int32_t p = load_now(&parent[x]);
    for (uint32_t it = 0; p != x; ++it) {
        if (it > cap) {
            *error = 1;
            return x;
        }
        const int32_t gp = load_now(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

// the one rule: the larger root goes under the smaller one, or the walk starts again from the two roots just read
__device__ __forceinline__ void cc_link(int32_t *__restrict__ parent, int32_t u, int32_t v, uint32_t cap, int32_t *error) {
    int32_t ru = cc_find(parent, u, cap, error), rv = cc_find(parent, v, cap, error);
    for (uint32_t it = 0; ru != rv; ++it) {
        if (it > cap) {
            *error = 1;
            return;
        }
        const int32_t hi = max(ru, rv), lo = min(ru, rv);
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
        ru = cc_find(parent, hi, cap, error);
        rv = cc_find(parent, lo, cap, error);
    }
}

// position of x in the ascending row [lo, hi) of adj, or -1
__device__ __forceinline__ int64_t cc_find_in_row(const int32_t *__restrict__ adj, int64_t lo, int64_t hi, int32_t x) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (adj[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && adj[lo] == x) ? lo : -1;
}

// one flatten round: parent[v] = where a walk of at most kCcJump steps got; *again when one ended below its root.  Nothing hooks while
// this runs and parent[v] has one writer, so the roots are fixed and a relaxed agent-scope store is enough.
[[maybe_unused]] __global__ __launch_bounds__(256) void k_cc_flatten(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ again_flag) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    bool again = false;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += stride) {
        const int32_t p0 = load_now(&parent[v]);
        int32_t x = p0, p = load_now(&parent[x]);
        for (int it = 0; p != x && it < kCcJump; ++it) {
            x = p;
            p = load_now(&parent[x]);
        }
        if (p != x) again = true;
        if (x != p0) store_now(&parent[v], x);
    }
    if (__ballot(again) && (threadIdx.x & 63) == 0) store_now(again_flag, 1);
}

// size[label[v]] += 1, one add per distinct label of a wave
[[maybe_unused]] __global__ __launch_bounds__(256) void k_cc_sizes(int64_t n, const int32_t *__restrict__ label, int32_t *__restrict__ size) {
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    const int64_t end = ((n + 63) / 64) * 64;
    const int lane = threadIdx.x & 63;
    for (int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; v < end; v += stride) {
        const int32_t l = v < n ? label[v] : -1;
        unsigned long long todo = __ballot(l >= 0);
        while (todo) {  // at most 64 turns: every turn retires the lanes of one label
            const int first = __ffsll((long long)todo) - 1;
            const int32_t l0 = __shfl(l, first);
            const unsigned long long same = __ballot(l == l0) & todo;
            if (lane == first) atomicAdd(&size[l0], int32_t(__popcll(same)));
            todo &= ~same;
        }
    }
}

// pointer jumping until a round changes nothing; flags = the call's two adjacent device words {error, again}, read between launches
[[maybe_unused]] int flatten(int64_t n, int32_t *parent, int32_t *flags, int cus, hipStream_t s, int *launches, int32_t *rounds) {
    const unsigned sweep = unsigned(std::min<int64_t>((n + 255) / 256, int64_t(cus) * 16));
    for (int r = 1; r <= kCcFlattenMax; ++r) {
        GMSX_HIP(hipMemsetAsync(flags + 1, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(k_cc_flatten, dim3(sweep), dim3(256), 0, s, n, parent, flags + 1);
        ++*launches;
        int32_t h[2] = {0, 0};  // error, again
        GMSX_HIP(hipMemcpyAsync(h, flags, sizeof h, hipMemcpyDeviceToHost, s));
        GMSX_HIP(hipStreamSynchronize(s));
        if (h[0]) return GMSX_ERR_KERNEL;
        if (!h[1]) {
            if (rounds) *rounds = r;
            return GMSX_OK;
        }
    }
    return GMSX_ERR_KERNEL;
}

}  // namespace
}  // namespace gmsx
