// The dense core of the triangle count (hip/tc.hip, k_tc_core): how many of the top rank ids leave the streamed path for the matrix cores, and how
// the core's 64 x 64 blocks are ordered and accounted.  Plain C++: tests/cpp/test_tc_core_plan.cpp checks it on the host.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gmsx {

constexpr int kTcCoreBucket = 1024;  // K is a multiple of this when the rule picks it
constexpr int kTcCoreCap = 32768;    // a lane's f32 sum in the mask epilogue stays <= 64 K = 2^21: exact
// Rates the rule weighs against each other (profiles/tc_core/README.md): the hub-item kernel's beyond-L2 bytes over its time,
// k_tc_core's K^3 / 6 bit-MACs over its time, and what one more kernel on the launch stream costs whatever it does.
constexpr double kTcCoreStreamBytesPerSec = 7.35e12;
constexpr double kTcCoreBitMacsPerSec = 1.7e15;  // RMAT scale 26: K = 18 432 in 0.606 ms, 16 384 in 0.415 ms, 24 576 in 1.56 ms (1.72, 1.77, 1.59 P/s)
constexpr double kTcCoreLaunchSec = 20e-6;
// What an unset GMSX_TC_CORE means: -1 = the rule below, 0 = no core.
constexpr int kTcCoreDefault = -1;

// a forced or chosen K against what the graph allows: every id of a core row must be a hub id, and the cap above
inline int tc_core_clamp(long long want, long long hub_limit, long long n) {
    return int(std::max<long long>(0, std::min<long long>(std::min<long long>(want, kTcCoreCap), std::min<long long>(hub_limit, n))));
}

// bucket_units[b] = 16-byte units the streamed path reads for the edges of the pivots [1024 b, 1024 (b + 1)).  Returns the multiple of 1024, at most
// cap, that maximises  units(K) * 16 / b_stream - (K^3 / 6) / r_core - launch  — the time the streamed path saves minus what the core costs — and 0
// when no K gains.  Ties go to the smaller K, which makes the result monotone in r_core.
inline int choose_tc_core(const std::vector<uint64_t> &bucket_units, int cap, double b_stream = kTcCoreStreamBytesPerSec,
                          double r_core = kTcCoreBitMacsPerSec, double launch_sec = kTcCoreLaunchSec) {
    int best_k = 0;
    double best = 0.0;
    unsigned long long units = 0;
    for (size_t b = 0; b < bucket_units.size(); ++b) {
        const long long k = (long long)(b + 1) * kTcCoreBucket;
        if (k > cap) break;
        units += bucket_units[b];
        const double gain = double(units) * 16.0 / b_stream - (double(k) * double(k) * double(k) / 6.0) / r_core - launch_sec;
        if (gain > best) {
            best = gain;
            best_k = int(k);
        }
    }
    return best_k;
}

// ---- the block sequence: 64 x 64 blocks (bi >= bj) of the K x K matrix, nb = ceil(K / 64) per side, by DESCENDING cost — a block multiplies the
// columns below 64 (bj + 1), so the blocks of the highest bj come first.  Block t of the sequence: c = nb - 1 - bj is the largest c with
// c (c + 1) / 2 <= t, and bi = bj + (t - c (c + 1) / 2).  Shard `part` of `nparts` takes the blocks t = part, part + nparts, …
inline long long tc_core_blocks(int k) {
    const long long nb = (k + 63) / 64;
    return nb * (nb + 1) / 2;
}
// algorithmic bytes of one block, no reuse assumed: the fragments of 2 x 64 rows, 8 (bj + 1) bytes each, and two mask words per lane and tile row
inline unsigned long long tc_core_block_bytes(int bj) { return 1024ull * (unsigned long long)(bj + 1) + 1024ull; }
inline unsigned long long tc_core_bytes(int k, int part, int nparts) {
    const long long nb = (k + 63) / 64;
    unsigned long long bytes = 0;
    long long t = 0;
    for (long long c = 0; c < nb; ++c)  // the c + 1 blocks of bj = nb - 1 - c
        for (long long r = 0; r <= c; ++r, ++t)
            if (nparts <= 1 || t % nparts == part) bytes += tc_core_block_bytes(int(nb - 1 - c));
    return bytes;
}

}  // namespace gmsx
