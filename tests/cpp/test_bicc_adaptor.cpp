// GPU test of gmsx::biconnected_components / gmsx::articulation_points / gmsx::bridges (include/gmsx_set_graph.hpp), compiled against
// libgmsx.so only: loads the file argv[2] ("file") or generates the kronecker graph of scale argv[2] at degree argv[3] ("kron"), never
// relabelled, runs the adaptor functions over both set flavours (which must agree) and prints
// "bicc blocks bridges articulation_points levels fnv_block fnv_blocks_at" — fnv = FNV-1a over the bytes of the int32 array
// (tests/test_bicc_adaptor_gpu.py compares the line with the goldens).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<int32_t> block, blocks_at, cut;
    std::vector<std::pair<int32_t, int32_t>> bridges;
    gmsx_bicc_info info{};
};

template <class G>
static Result run(const G &g) {
    Result r;
    gmsx_bicc_info cut_info{}, bridge_info{};
    if (gmsx::biconnected_components(g, r.block, r.blocks_at, &r.info) != r.info.blocks) {
        std::fprintf(stderr, "the return value is not info.blocks\n");
        std::exit(3);
    }
    r.cut = gmsx::articulation_points(g, &cut_info);
    r.bridges = gmsx::bridges(g, &bridge_info);
    if (std::memcmp(&cut_info, &r.info, sizeof cut_info) != 0 || std::memcmp(&bridge_info, &r.info, sizeof bridge_info) != 0 ||
        int64_t(r.cut.size()) != r.info.articulation_points || int64_t(r.bridges.size()) != r.info.bridges) {
        std::fprintf(stderr, "the three calls disagree\n");
        std::exit(4);
    }
    // the cut vertices ascend and are the vertices of two blocks or more; the bridges ascend, u < v, and are the blocks of one edge
    for (size_t i = 0; i < r.cut.size(); ++i)
        if (r.blocks_at[size_t(r.cut[i])] < 2 || (i > 0 && r.cut[i] <= r.cut[i - 1])) {
            std::fprintf(stderr, "cut vertex %d\n", int(r.cut[i]));
            std::exit(5);
        }
    std::vector<int64_t> edges_of(size_t(r.info.blocks), 0);
    for (int64_t u = 0; u < g.num_nodes(); ++u)
        for (int64_t j = g.offsets()[u]; j < g.offsets()[u + 1]; ++j)
            if (int64_t(g.neighbors()[j]) > u) ++edges_of[size_t(r.block[size_t(j)])];
    for (size_t i = 0; i < r.bridges.size(); ++i) {
        const auto &e = r.bridges[i];
        const int32_t *lo = g.neighbors() + g.offsets()[e.first], *hi = g.neighbors() + g.offsets()[e.first + 1];
        const int32_t *at = std::lower_bound(lo, hi, e.second);
        if (e.first >= e.second || at == hi || *at != e.second || edges_of[size_t(r.block[size_t(at - g.neighbors())])] != 1 ||
            (i > 0 && !(r.bridges[i - 1] < e))) {
            std::fprintf(stderr, "bridge %d %d\n", int(e.first), int(e.second));
            std::exit(5);
        }
    }
    return r;
}

static unsigned long long fnv(const std::vector<int32_t> &a) {
    unsigned long long x = 1469598103934665603ull;
    for (int32_t value : a) {
        unsigned char bytes[4];
        std::memcpy(bytes, &value, 4);
        for (unsigned char b : bytes) {
            x ^= b;
            x *= 1099511628211ull;
        }
    }
    return x;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    gmsx_csr *csr = nullptr;
    if (std::strcmp(argv[1], "file") == 0)
        gmsx::detail::check(gmsx_csr_load(argv[2], 1, GMSX_RELABEL_NEVER, &csr), "gmsx_csr_load");
    else
        gmsx::detail::check(gmsx_csr_generate(GMSX_GEN_KRONECKER, std::atoi(argv[2]), argc > 3 ? std::atoi(argv[3]) : 16, GMSX_RELABEL_NEVER, 0, &csr),
                            "gmsx_csr_generate");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted), b = run(roaring);
    if (a.block != b.block || a.blocks_at != b.blocks_at || a.cut != b.cut || a.bridges != b.bridges) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    std::printf("bicc %lld %lld %lld %d %llu %llu\n", (long long)a.info.blocks, (long long)a.info.bridges, (long long)a.info.articulation_points,
                int(a.info.levels), fnv(a.block), fnv(a.blocks_at));
    gmsx_csr_free(csr);
    return 0;
}
