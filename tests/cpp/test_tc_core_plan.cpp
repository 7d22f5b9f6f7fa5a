// choose_tc_core and the block bookkeeping (gms_amd/csrc/host/tc_core_plan.hpp): hand-derived cases, then the chooser's properties over seeded random buckets.
#include "tc_core_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace gmsx;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

int main() {
    // all-zero buckets (and no buckets, and no room for one bucket): no core
    CHECK(choose_tc_core(std::vector<uint64_t>(32, 0), kTcCoreCap) == 0);
    CHECK(choose_tc_core({}, kTcCoreCap) == 0);
    CHECK(choose_tc_core(std::vector<uint64_t>(32, ~0ull >> 8), 1023) == 0);
    // buckets large enough: the cap — K^3 / 6 / r_core at the cap is 4.5 ms, every bucket here saves 2.2 ms of streaming
    CHECK(choose_tc_core(std::vector<uint64_t>(32, 1000000000ull), kTcCoreCap, kTcCoreStreamBytesPerSec, 1.3e15) == kTcCoreCap);
    CHECK(choose_tc_core(std::vector<uint64_t>(32, 1000000000ull), 5000) == 4096);  // the largest multiple of 1024 below a cap that is none
    CHECK(choose_tc_core(std::vector<uint64_t>(3, 1000000000ull), kTcCoreCap) == 3072);  // no more buckets than it was given
    // by hand, b_stream = 16 bytes/s and r_core = 1024^3 / 6 bit-MACs/s: gain(K = 1024 k) = units(K) - k^3 seconds
    {
        const double b = 16.0, r = 1024.0 * 1024.0 * 1024.0 / 6.0;
        CHECK(choose_tc_core({2, 9, 0, 0}, 4096, b, r, 0.0) == 2048);   // gains 1, 3, -16, -53
        CHECK(choose_tc_core({2, 6, 0, 0}, 4096, b, r, 0.0) == 1024);   // gains 1, 0
        CHECK(choose_tc_core({1, 8, 0, 0}, 4096, b, r, 0.0) == 2048);   // gains 0, 1: a zero gain is no gain, the later positive one is
        CHECK(choose_tc_core({1, 7, 0, 0}, 4096, b, r, 0.0) == 0);      // gains 0, 0
        CHECK(choose_tc_core({2, 9, 0, 0}, 4096, b, r, 3.0) == 0);      // the launch takes what the best K gains
        CHECK(choose_tc_core({2, 9, 0, 90}, 4096, b, r, 3.0) == 4096);  // gains -2, 0, -19, 34
    }
    CHECK(tc_core_clamp(5000, 65535, 1 << 20) == 5000);
    CHECK(tc_core_clamp(5000, 300, 1 << 20) == 300);
    CHECK(tc_core_clamp(5000, 65535, 200) == 200);
    CHECK(tc_core_clamp(1 << 20, 65535, 1 << 20) == kTcCoreCap);
    CHECK(tc_core_clamp(-1, 65535, 100) == 0);
    // blocks: nb (nb + 1) / 2, bytes 1024 (bj + 2) each; the shards' shares add up to the whole
    CHECK(tc_core_blocks(1) == 1 && tc_core_blocks(64) == 1 && tc_core_blocks(65) == 3 && tc_core_blocks(16384) == 32896);
    CHECK(tc_core_bytes(64, 0, 1) == 2048);
    CHECK(tc_core_bytes(129, 0, 1) == 1024ull * (1 * 4 + 2 * 3 + 3 * 2));  // bj = 2: one block, bj = 1: two, bj = 0: three
    for (int k : {1, 63, 64, 65, 100, 129, 1000, 5000, 16384})
        for (int nparts : {2, 3, 5, 8}) {
            unsigned long long sum = 0;
            for (int p = 0; p < nparts; ++p) sum += tc_core_bytes(k, p, nparts);
            CHECK(sum == tc_core_bytes(k, 0, 1));
        }

    std::mt19937_64 rng(20240611u);
    for (int iter = 0; iter < 400; ++iter) {
        const int cap = int(rng() % 40000);
        std::vector<uint64_t> bucket(size_t(rng() % 40));
        const int shift = int(rng() % 40);
        for (uint64_t &u : bucket) u = (rng() >> 24) >> shift;
        int prev = -1;
        for (double r_core : {1e12, 1e13, 1e14, 3e14, 1.3e15, 1e16, 1e18}) {
            const int k = choose_tc_core(bucket, cap, kTcCoreStreamBytesPerSec, r_core);
            CHECK(k >= 0 && k % kTcCoreBucket == 0 && k <= cap && k <= int(bucket.size()) * kTcCoreBucket);
            CHECK(k >= prev);  // a faster core never shrinks
            prev = k;
        }
    }
    if (failures) return 1;
    std::printf("tc core plan ok\n");
    return 0;
}
