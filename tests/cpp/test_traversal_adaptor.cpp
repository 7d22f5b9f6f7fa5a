// GPU test of gmsx::bfs / betweenness / pick_sources (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the graph file argv[1]
// with the library's loader, runs the adaptor functions over both set flavours (which must agree byte for byte) and prints "picks p0 … p15", per
// source argv[2 …] "parent s reached v0 …" and "depth s levels v0 …", and per source list (the first 1, 4 and 8 picks) and flag set
// "bc k flags max_score s0 …" with 17 significant digits (tests/test_traversal_adaptor_gpu.py compares them with the goldens).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<std::vector<int32_t>> parent, depth;
    std::vector<gmsx_bfs_info> info;
    std::vector<std::vector<double>> scores;
    std::vector<double> max_score;
};

static const int kLists[3] = {1, 4, 8};
static const uint32_t kFlags[2] = {GMSX_BC_DEFAULT, GMSX_BC_EXCLUDE_SOURCE | GMSX_BC_NORMALIZE_MAX};

template <class G>
static Result run(const G &g, const std::vector<int32_t> &sources, const std::vector<int32_t> &picks) {
    Result r;
    for (int32_t s : sources) {
        r.parent.emplace_back();
        r.depth.emplace_back();
        r.info.emplace_back();
        if (gmsx::bfs(g, s, r.parent.back(), &r.depth.back(), &r.info.back()) != r.info.back().reached) {
            std::fprintf(stderr, "the return value is not info.reached\n");
            std::exit(3);
        }
    }
    for (int k : kLists)
        for (uint32_t flags : kFlags) {
            r.scores.emplace_back();
            gmsx_bc_info bi{};
            const std::vector<int32_t> list(picks.begin(), picks.begin() + k);
            r.max_score.push_back(gmsx::betweenness(g, list, r.scores.back(), flags, &bi));
            if (bi.max_score != r.max_score.back() || bi.sources != k) {
                std::fprintf(stderr, "the return value is not info.max_score\n");
                std::exit(3);
            }
        }
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    std::vector<int32_t> sources;
    for (int i = 2; i < argc; ++i) sources.push_back(int32_t(std::atoi(argv[i])));
    const std::vector<int32_t> picks = gmsx::pick_sources(csr, 16);
    if (gmsx::pick_sources(csr, 3, sources[0]) != std::vector<int32_t>(3, sources[0])) return 4;
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted, sources, picks), b = run(roaring, sources, picks);
    if (a.parent != b.parent || a.depth != b.depth || a.scores != b.scores) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    std::printf("picks");
    for (int32_t p : picks) std::printf(" %d", int(p));
    std::printf("\n");
    for (size_t i = 0; i < sources.size(); ++i) {
        std::printf("parent %d %lld", int(sources[i]), (long long)a.info[i].reached);
        for (int32_t x : a.parent[i]) std::printf(" %d", int(x));
        std::printf("\ndepth %d %d", int(sources[i]), int(a.info[i].levels));
        for (int32_t x : a.depth[i]) std::printf(" %d", int(x));
        std::printf("\n");
    }
    size_t at = 0;
    for (int k : kLists)
        for (uint32_t flags : kFlags) {
            std::printf("bc %d %u %.17g", k, unsigned(flags), a.max_score[at]);
            for (double x : a.scores[at]) std::printf(" %.17g", x);
            std::printf("\n");
            ++at;
        }
    gmsx_csr_free(csr);
    return 0;
}
