// The wave shuffle trees of the library, stated once.  This is the only file that shuffles by an offset (__shfl_down, __shfl_xor,
// __shfl_up); broadcasts (__shfl(x, lane)), ballots, readlane and readfirstlane stay where they are used.
//
// Every function is called by ALL lanes of the wave (of the WIDTH-lane group: WIDTH a power of two <= 64, groups aligned to WIDTH lanes).
//   wave_sum / wave_max / wave_min / wave_or           the DOWN tree: offsets WIDTH/2, …, 1 with __shfl_down(x, o, WIDTH).  The result is valid in
//                                                      LANE 0 OF EACH GROUP ONLY; the other lanes hold partial values.
//   wave_sum_all / wave_max_all / wave_min_all / wave_or_all
//                                                      the same offsets as a BUTTERFLY (__shfl_xor): the result is valid in EVERY lane.
//   wave_incl_scan<WIDTH>(x, lane_in_group)            inclusive prefix sum over the group (__shfl_up, offsets 1, 2, …, WIDTH/2).
//   wave_fold2 / wave_fold2_all(a, b, f)               the down tree / the butterfly over a PAIR: f(a, b, a_of_other_lane, b_of_other_lane) updates a, b.
//   wave_pair_max / wave_pair_max_all<WIDTH>(w, l)     the down tree / the butterfly over a (weight, label) pair: the larger weight wins, of equal weights
//                                                      the SMALLER label (label propagation's pick: integers, so the order of the lanes cannot matter).
//   block_sum<kWaves>(x, s_w)                          the down tree per wave, then s_w[0] + s_w[1] + … on thread 0; two barriers.
// THE ORDER OF THE ADDITIONS IS PART OF THE CONTRACT: lane l adds x[l + o] to x[l] for o = WIDTH/2, …, 1 in this order.  Floating-point callers
// (PageRank's scores, betweenness' dependencies, the pair similarities) are bit-identical to their goldens only because of it, so a change of
// the tree (another order, DPP row reductions, a swizzle) is a change of their results.
#pragma once
#include <hip/hip_runtime.h>

namespace gmsx {

// the width a WIDTH-lane tree hands to the shuffle: a full wave names the runtime's own default, warpSize, so that the compiler selects exactly the
// instructions of a bare __shfl_down(x, o) (a literal 64 folds earlier and selects other address arithmetic)
template <int WIDTH>
__device__ __forceinline__ int shfl_width() { return WIDTH == 64 ? warpSize : WIDTH; }

template <int WIDTH, class T, class F>
__device__ __forceinline__ T wave_fold(T x, F f) {
    for (int o = WIDTH / 2; o > 0; o >>= 1) x = f(x, __shfl_down(x, o, shfl_width<WIDTH>()));
    return x;
}
template <int WIDTH, class T, class F>
__device__ __forceinline__ T wave_fold_all(T x, F f) {
    for (int o = WIDTH / 2; o > 0; o >>= 1) x = f(x, __shfl_xor(x, o, shfl_width<WIDTH>()));
    return x;
}
struct FoldSum { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct FoldMax { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); } };
struct FoldMin { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return min(a, b); } };
struct FoldOr { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; } };
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_sum(T x) { return wave_fold<WIDTH>(x, FoldSum()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_max(T x) { return wave_fold<WIDTH>(x, FoldMax()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_min(T x) { return wave_fold<WIDTH>(x, FoldMin()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_or(T x) { return wave_fold<WIDTH>(x, FoldOr()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_sum_all(T x) { return wave_fold_all<WIDTH>(x, FoldSum()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_max_all(T x) { return wave_fold_all<WIDTH>(x, FoldMax()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_min_all(T x) { return wave_fold_all<WIDTH>(x, FoldMin()); }
template <int WIDTH = 64, class T> __device__ __forceinline__ T wave_or_all(T x) { return wave_fold_all<WIDTH>(x, FoldOr()); }

// the down-tree sum over groups whose width (a power of two <= 64) is known at run time only
template <class T>
__device__ __forceinline__ T wave_sum(T x, int width) {
    for (int o = width >> 1; o > 0; o >>= 1) x += __shfl_down(x, o, width);
    return x;
}

template <int WIDTH = 64, class T>
__device__ __forceinline__ T wave_incl_scan(T x, int lane_in_group) {
#pragma unroll
    for (int d = 1; d < WIDTH; d <<= 1) {
        const T y = __shfl_up(x, d, shfl_width<WIDTH>());
        if (lane_in_group >= d) x += y;
    }
    return x;
}

template <class A, class B, class F>
__device__ __forceinline__ void wave_fold2(A &a, B &b, F f) {
    for (int o = 32; o > 0; o >>= 1) {
        const A a2 = __shfl_down(a, o);
        const B b2 = __shfl_down(b, o);
        f(a, b, a2, b2);
    }
}
template <class A, class B, class F>
__device__ __forceinline__ void wave_fold2_all(A &a, B &b, F f) {
    for (int o = 32; o > 0; o >>= 1) {
        const A a2 = __shfl_xor(a, o);
        const B b2 = __shfl_xor(b, o);
        f(a, b, a2, b2);
    }
}

// the maximum of a (weight, label) pair over WIDTH-lane groups: (w, l) beats (w2, l2) iff w > w2, or w == w2 and l < l2
template <int WIDTH = 64, class W, class L>
__device__ __forceinline__ void wave_pair_max(W &w, L &l) {
    for (int o = WIDTH / 2; o > 0; o >>= 1) {
        const W w2 = __shfl_down(w, o, shfl_width<WIDTH>());
        const L l2 = __shfl_down(l, o, shfl_width<WIDTH>());
        if (w2 > w || (w2 == w && l2 < l)) w = w2, l = l2;
    }
}
template <int WIDTH = 64, class W, class L>
__device__ __forceinline__ void wave_pair_max_all(W &w, L &l) {
    for (int o = WIDTH / 2; o > 0; o >>= 1) {
        const W w2 = __shfl_xor(w, o, shfl_width<WIDTH>());
        const L l2 = __shfl_xor(l, o, shfl_width<WIDTH>());
        if (w2 > w || (w2 == w && l2 < l)) w = w2, l = l2;
    }
}

// the butterfly maximum of a 64-bit key, shuffled as two 32-bit halves (bk_list.hip's order keys)
__device__ __forceinline__ unsigned long long wave_max_all_halves(unsigned long long k) {
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = unsigned(__shfl_xor(int(unsigned(k)), m));
        const unsigned hi = unsigned(__shfl_xor(int(unsigned(k >> 32)), m));
        const unsigned long long o = (static_cast<unsigned long long>(hi) << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

// the fixed tree of a workgroup of 64 kWaves threads; EVERY thread calls it; the total is returned to thread 0 (0 elsewhere)
template <int kWaves, class T>
__device__ __forceinline__ T block_sum(T x, T *s_w) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    T r = T(0);
    if (threadIdx.x == 0) {
        r = s_w[0];
        for (int w = 1; w < kWaves; ++w) r += s_w[w];
    }
    __syncthreads();
    return r;
}

}  // namespace gmsx
