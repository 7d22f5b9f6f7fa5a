// kc_bin_plan (gms_amd/csrc/host/kc_bin_plan.hpp): the bins of every k-clique call against tables written out by hand, then the properties every plan has.
#include "kc_bin_plan.hpp"

#include <cstdio>

using namespace gmsx;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

constexpr KcKind S = KcKind::Slab, M = KcKind::Lds, T = KcKind::LdsTri, V = KcKind::Wave;
struct Row {
    int from, dmax;
    KcKind kind;
    int wpl, threads, W, WS, WT;
    size_t lds;
    bool exp;
    int e_threads, e_WS, e_WT;  // the export shape (exp only)
    size_t e_lds;
};
// rectangular LDS bins below 512 and the wave bin: the same in every table (no per-vertex counters)
#define NARROW                                                                                                                     \
    {384, 512, M, 0, 512, 16, 17, 0, 35840, false, 0, 0, 0, 0}, {256, 384, M, 0, 512, 12, 13, 0, 20736, false, 0, 0, 0, 0},        \
        {192, 256, M, 0, 256, 8, 9, 0, 9728, false, 0, 0, 0, 0}, {128, 192, M, 0, 256, 6, 7, 0, 5760, false, 0, 0, 0, 0},          \
        {96, 128, M, 0, 256, 4, 5, 0, 2816, false, 0, 0, 0, 0}, {64, 96, M, 0, 256, 3, 3, 0, 1344, false, 0, 0, 0, 0},             \
        {32, 64, M, 0, 256, 2, 3, 0, 896, false, 0, 0, 0, 0}, {0, 32, V, 0, 256, 1, 1, 0, 0, false, 0, 0, 0, 0}
#define RECT_TOP                                                                                                                   \
    {704, 1024, M, 0, 1024, 32, 33, 0, 137216, false, 0, 0, 0, 0}, {640, 704, M, 0, 1024, 22, 23, 0, 66176, false, 0, 0, 0, 0},    \
        {512, 640, M, 0, 1024, 20, 21, 0, 55040, false, 0, 0, 0, 0}
// k = 3: 512-thread slab workgroups, bitmap + prefix + stage
static const Row k3[] = {{4096, 8192, S, 4, 512, 256, 257, 128, 45056, false, 0, 0, 0, 0}, {2048, 4096, S, 2, 512, 128, 129, 288, 28672, false, 0, 0, 0, 0},
                         {1024, 2048, S, 1, 512, 64, 65, 576, 20480, false, 0, 0, 0, 0}, RECT_TOP, NARROW};
// k >= 5: the same without the four-words-per-lane bin
static const Row k5[] = {{2048, 4096, S, 2, 512, 128, 129, 288, 28672, false, 0, 0, 0, 0}, {1024, 2048, S, 1, 512, 64, 65, 576, 20480, false, 0, 0, 0, 0}, RECT_TOP, NARROW};
// per-vertex counts: dmax column counters of 4 bytes more in every workgroup bin
static const Row vtx[] = {{4096, 8192, S, 4, 512, 256, 257, 128, 77824, false, 0, 0, 0, 0},
                          {2048, 4096, S, 2, 512, 128, 129, 288, 45056, false, 0, 0, 0, 0},
                          {1024, 2048, S, 1, 512, 64, 65, 576, 28672, false, 0, 0, 0, 0},
                          {704, 1024, M, 0, 1024, 32, 33, 0, 141312, false, 0, 0, 0, 0},
                          {640, 704, M, 0, 1024, 22, 23, 0, 68992, false, 0, 0, 0, 0},
                          {512, 640, M, 0, 1024, 20, 21, 0, 57600, false, 0, 0, 0, 0},
                          {384, 512, M, 0, 512, 16, 17, 0, 37888, false, 0, 0, 0, 0},
                          {256, 384, M, 0, 512, 12, 13, 0, 22272, false, 0, 0, 0, 0},
                          {192, 256, M, 0, 256, 8, 9, 0, 10752, false, 0, 0, 0, 0},
                          {128, 192, M, 0, 256, 6, 7, 0, 6528, false, 0, 0, 0, 0},
                          {96, 128, M, 0, 256, 4, 5, 0, 3328, false, 0, 0, 0, 0},
                          {64, 96, M, 0, 256, 3, 3, 0, 1728, false, 0, 0, 0, 0},
                          {32, 64, M, 0, 256, 2, 3, 0, 1152, false, 0, 0, 0, 0},
                          {0, 32, V, 0, 256, 1, 1, 0, 0, false, 0, 0, 0, 0}};
// k = 4: 1024-thread slab workgroups whose LDS is the row band + the waves' neighbour lists; every slab bin can export (1024 threads, stride W, stage + forward list)
#define K4_SLAB(from1)                                                                                      \
    {4096, 8192, S, 4, 1024, 256, 257, 128, 139776, true, 1024, 256, 0, 94208},                            \
        {2048, 4096, S, 2, 1024, 128, 129, 288, 156800, true, 1024, 128, 0, 53248}, {                      \
        from1, 2048, S, 1, 1024, 64, 65, 576, 157952, true, 1024, 64, 0, 32768                             \
    }
static const Row k4_rect[] = {K4_SLAB(1024), RECT_TOP, NARROW};
// … with the triangular layout: two triangular bins instead of the rectangular ones above 512, exported with the shape they count with
static const Row k4_tri[] = {K4_SLAB(1472), {960, 1472, T, 0, 1024, 46, 47, 0, 141312, true, 1024, 47, 0, 141312}, {512, 960, T, 0, 1024, 30, 31, 0, 61440, true, 1024, 31, 0, 61440},
                             NARROW};

template <size_t N>
static void check_table(const Row (&want)[N], int k, bool vtx_, bool tri, int max_d) {
    const std::vector<KcBin> got = kc_bin_plan(k, vtx_, tri, max_d);
    size_t at = 0;
    for (const Row &w : want) {
        if (w.from >= max_d) continue;  // bins wholly above the limit are not planned
        if (at >= got.size()) break;
        const KcBin &b = got[at++];
        const bool same = b.from == w.from && b.dmax == w.dmax && b.kind == w.kind && b.wpl == w.wpl && b.W == w.W && b.count.threads == w.threads && b.count.WS == w.WS &&
                          b.count.WT == w.WT && b.count.lds == w.lds && b.can_export == w.exp &&
                          (!w.exp || (b.build.threads == w.e_threads && b.build.WS == w.e_WS && b.build.WT == w.e_WT && b.build.lds == w.e_lds));
        if (!same) std::printf("k %d vtx %d tri %d max_d %d: bin (%d, %d] differs from the table\n", k, int(vtx_), int(tri), max_d, w.from, w.dmax);
        CHECK(same);
    }
    size_t n_want = 0;
    for (const Row &w : want) n_want += w.from < max_d;
    CHECK(at == n_want && got.size() == n_want);
}

int main() {
    const int max_ds[] = {1, 8, 32, 33, 40, 300, 512, 513, 960, 1000, 1024, 1472, 1473, 2048, 4096, 4097, 8192};
    for (int k = 3; k <= 10; ++k)
        for (int v = 0; v < 2; ++v)
            for (int t = 0; t < 2; ++t)
                for (int max_d : max_ds) {
                    const bool vtx_ = v != 0, tri = t != 0;
                    if (vtx_ && k != 3) continue;  // the per-vertex counts are triangle counts
                    if (max_d > (k <= 4 ? 8192 : 4096)) continue;
                    if (vtx_) check_table(vtx, k, vtx_, tri, max_d);
                    else if (k == 3) check_table(k3, k, vtx_, tri, max_d);
                    else if (k == 4 && tri) check_table(k4_tri, k, vtx_, tri, max_d);
                    else if (k == 4) check_table(k4_rect, k, vtx_, tri, max_d);
                    else check_table(k5, k, vtx_, tri, max_d);
                    // the properties
                    const std::vector<KcBin> plan = kc_bin_plan(k, vtx_, tri, max_d);
                    CHECK(!plan.empty() && plan.size() <= size_t(kKcMaxBins));
                    if (plan.empty()) continue;
                    // the bins tile (0, max_d], widest first, no gap and no overlap: the first one holds max_d, each starts where the next one ends
                    CHECK(plan.front().from < max_d && max_d <= plan.front().dmax && plan.back().from == 0);
                    for (size_t i = 0; i + 1 < plan.size(); ++i) CHECK(plan[i].from == plan[i + 1].dmax);
                    for (const KcBin &b : plan) {
                        CHECK(b.from < b.dmax);
                        if (b.kind == KcKind::Wave) continue;
                        CHECK(b.W * 32 == b.dmax && b.count.threads % 64 == 0 && b.count.threads <= 1024);
                        const size_t limit = b.kind == KcKind::Slab ? size_t(kKcSlabLdsMax) : size_t(kKcLdsDynMax);
                        CHECK(b.count.lds <= limit);
                        if (b.can_export) CHECK(b.build.lds <= limit && b.build.threads == 1024);
                        // the k = 4 count builds for the matrix cores what it keeps as a slab or a triangular matrix (the kernels have no rectangular
                        // LDS export) — with the triangular layout on, exactly the bins above 512
                        CHECK(b.can_export == (k == 4 && !vtx_ && (b.kind == KcKind::Slab || b.kind == KcKind::LdsTri)));
                        if (k == 4 && !vtx_ && tri) CHECK(b.can_export == (b.from >= 512));
                        CHECK((b.kind == KcKind::LdsTri) == (k == 4 && !vtx_ && tri && b.from >= 512 && b.dmax <= kKcTriTop));
                    }
                }
    CHECK(kc_tri_words(0) == 0 && kc_tri_words(32) == 32 && kc_tri_words(33) == 34 && kc_tri_words(64) == 96 && kc_tri_words(1472) == 34592);
    if (failures) return 1;
    std::printf("kc bin plan ok\n");
    return 0;
}
