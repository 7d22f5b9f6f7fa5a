// The bins of a k-clique count (hip/kclique.hip): the pivots are cut by out-degree d+ into bins (from, dmax], each with a kernel kind, a workgroup size,
// row widths and a dynamic-LDS size.  This is the ONE place where a bin is defined; the driver resolves each bin's positions in the d+ order once and
// derives from that list the shard rule of the receivers' pass (KcBins::lo), the size of the matrix-core pool, the launches, and the `slab_from` of the
// traffic statistic.  Plain C++: tests/cpp/test_kc_bin_plan.cpp checks it on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gmsx {

constexpr int kKcMaxBins = 16;           // what KcBins (the receivers' shard rule) holds
constexpr int kKcBitmapWords = 2048;     // the pivot's 65 536-bit hub bitmap (device_graph.hpp's kBitmapWords)
constexpr int kKcRowList = 256;          // entries of a wave's neighbour list in the k = 4 slab count (2 bytes each)
// dynamic LDS the LDS-matrix variants may ask for: the CU's 160 KB minus their 16.2 KB of static LDS (bitmap + prefix counts + tail filter + reduction slots)
constexpr int kKcLdsDynMax = 143 * 1024;
constexpr int kKcSlabLdsMax = 155 * 1024;  // … and the slab variants, whose bitmap is part of the dynamic LDS
// widths of the two triangular LDS bins (k = 4): the matrix of d+ <= 1472 and its forward list fill one CU's LDS (153.6 of the 155 KB a launch may ask
// for, static part included); two matrices of d+ <= 960 fit it together (2 x 78.0 KB with the static 4.3 KB each).  Multiples of 32: W = dmax / 32 words.
constexpr int kKcTriTop = 1472, kKcTriTwo = 960;
constexpr int kKcLdsTop = 1024;   // the widest rectangular LDS matrix
constexpr int kKcWaveTop = 32;    // one wave per pivot up to here

// words of a triangular LDS matrix in front of row i: row t is stored with (t >> 5) + 1 words (kclique.hip's kc_tri_off)
constexpr uint32_t kc_tri_words(int i) {
    const int q = i >> 5, r = i & 31;
    return uint32_t((q + 1) * (16 * q + r));
}
// the 2-byte list of the members streamed forward, behind the matrix
constexpr size_t kc_fwd_list_bytes(int dmax) { return (size_t(dmax) * 2 + 15) & ~size_t(15); }
// bitmap + prefix counts + the row stage of a slab variant (four rows of W words per wave)
constexpr size_t kc_slab_stage_bytes(int threads, int W) { return size_t(kKcBitmapWords) * 4 + size_t(kKcBitmapWords) * 2 + size_t(threads / 64) * 4 * W * 4; }

enum class KcKind { Wave, Lds, LdsTri, Slab };  // wave kernel; bit-matrix in LDS, rectangular / triangular; bit-matrix in a global slab

struct KcShape {      // what a launch of the bin passes
    int threads;
    int WS, WT;       // row stride in words; rows of the k = 4 band (slab count)
    size_t lds;       // dynamic LDS bytes
};
struct KcBin {
    int from, dmax;   // pivots of from < d+ <= dmax (the first bin of a plan is cut at max_d)
    KcKind kind;
    int wpl;          // words per lane of a slab row (1, 2, 4); 0 otherwise
    int W;            // words per bit row
    KcShape count;    // BUILD + count in one kernel
    bool can_export;  // a k = 4 count may BUILD this bin into the matrix-core pool instead …
    KcShape build;    // … with this shape (can_export only)
};

// The bins of a count of k-cliques (3 <= k <= 10; vtx: the per-vertex triangle counts, k = 3) over the pivots of d+ <= max_d, widest first.  `tri`: the
// triangular layout is on — it serves the k = 4 count only, where it replaces the rectangular bins above 512 and most of the first slab bin.
inline std::vector<KcBin> kc_bin_plan(int k, bool vtx, bool tri, int max_d) {
    const bool k4 = k == 4 && !vtx;
    tri = tri && k4;
    std::vector<KcBin> out;
    auto add = [&](KcBin b) {
        if (b.from < max_d) out.push_back(b);
    };
    // slab bins: one / two / four words per lane; k >= 5 stops at 4096
    const int slab_bottom = tri ? kKcTriTop : kKcLdsTop;
    const int slab_threads = k == 4 ? 1024 : 512;
    for (int wpl = k <= 4 ? 4 : 2; wpl >= 1; wpl >>= 1) {
        const int dmax = 2048 * wpl, W = dmax / 32;
        const int WT = wpl == 4 ? 128 : wpl == 2 ? 288 : 576;  // k = 4 row band: WT rows x (W + 1) words of LDS (multiple of 32)
        size_t lds = kc_slab_stage_bytes(slab_threads, W);
        if (k == 4) {  // the band and the waves' neighbour lists reuse the dead bitmap / stage
            const size_t band = size_t(WT) * (W + 1) * 4 + size_t(slab_threads / 64) * kKcRowList * 2;
            if (band > lds) lds = band;
        }
        if (vtx) lds += size_t(dmax) * 4;  // column counters
        // (EXPORT: 128 registers x 1024 threads, rows of W words through the stage, no count)
        add({wpl == 1 ? slab_bottom : dmax / 2, dmax, KcKind::Slab, wpl, W, {slab_threads, W + 1, WT, lds}, k4,
             {1024, W, 0, kc_slab_stage_bytes(1024, W) + kc_fwd_list_bytes(dmax)}});
    }
    // LDS bins: (next entry, entry] — cut where another workgroup fits a CU
    static const int m_rect[] = {1024, 704, 640, 512, 384, 256, 192, 128, 96, 64, 32}, m_tri[] = {kKcTriTop, kKcTriTwo, 512, 384, 256, 192, 128, 96, 64, 32};
    const int *m = tri ? m_tri : m_rect;
    const int n_m = tri ? int(sizeof(m_tri) / sizeof(int)) : int(sizeof(m_rect) / sizeof(int));
    for (int b = 0; b + 1 < n_m; ++b) {
        const int dmax = m[b], W = dmax / 32, WS = W | 1;  // odd stride: rows of one column spread over the LDS banks
        const bool tri_bin = tri && dmax > 512;
        // (d+ <= 640: TWO 1024-thread workgroups fit a CU — 53.8 KB of matrix each; the bitmap, the prefix counts and the tail filter are static LDS)
        const int threads = dmax >= 640 ? 1024 : dmax >= 384 ? 512 : 256;
        const size_t lds = (tri_bin ? size_t(kc_tri_words(dmax)) : size_t(dmax) * WS) * 4 + (vtx ? size_t(dmax) * 4 : 0) + kc_fwd_list_bytes(dmax);
        const KcShape shape{threads, WS, 0, lds};
        add({m[b + 1], dmax, tri_bin ? KcKind::LdsTri : KcKind::Lds, 0, W, shape, tri_bin, shape});
    }
    add({0, kKcWaveTop, KcKind::Wave, 0, 1, {256, 1, 0, 0}, false, {256, 1, 0, 0}});
    return out;
}

}  // namespace gmsx
