// GPU test of gmsx::coloring / coloring_order / coloring_check (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: generates
// kronecker <scale> at degree 16 (argv[1]) with the library's generator, reads the rank vectors named on the command line (argv[2..]: files of
// n int32) and prints, over both set flavours (which must agree), "color <tag> c0 c1 …" and "info <tag> colors rounds max_pred first_round" for
// the id order, every file and the five heuristics, and "check <tag> conflicts invalid max_color distinct max_degree" for each
// (tests/test_coloring_adaptor_gpu.py compares them with the goldens).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Run {
    std::string tag;
    std::vector<int32_t> coloring;
    gmsx_coloring_info info{};
    gmsx_coloring_check check{};
};

template <class G>
static std::vector<Run> run(const G &g, const std::vector<std::vector<int32_t>> &ranks) {
    std::vector<Run> out;
    for (size_t i = 0; i < ranks.size(); ++i) {
        Run r;
        r.tag = "file" + std::to_string(i);
        r.coloring = gmsx::coloring(g, ranks[i], true, &r.info);
        // the same priority in order format
        std::vector<int32_t> order(ranks[i].size());
        for (size_t v = 0; v < ranks[i].size(); ++v) order[size_t(ranks[i][v])] = int32_t(v);
        gmsx_coloring_info again{};
        if (gmsx::coloring(g, order, false, &again) != r.coloring || again.colors != r.info.colors || again.rounds != r.info.rounds) {
            std::fprintf(stderr, "order format and rank format disagree\n");
            std::exit(3);
        }
        r.check = gmsx::coloring_check(g, r.coloring);
        out.push_back(r);
    }
    for (const char *h : {"id", "ff", "lf", "sl", "adg"}) {
        Run r;
        r.tag = h;
        r.coloring = gmsx::coloring(g, h, 0.001, &r.info);
        r.check = gmsx::coloring_check(g, r.coloring);
        out.push_back(r);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_generate(GMSX_GEN_KRONECKER, std::atoi(argv[1]), 16, GMSX_RELABEL_AUTO, 0, &csr), "gmsx_csr_generate");
    const size_t n = size_t(gmsx_csr_num_nodes(csr));
    std::vector<std::vector<int32_t>> ranks;
    for (int i = 2; i < argc; ++i) {
        std::vector<int32_t> r(n);
        std::FILE *f = std::fopen(argv[i], "rb");
        if (!f || std::fread(r.data(), 4, n, f) != n) return 4;
        std::fclose(f);
        ranks.push_back(r);
    }
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const std::vector<Run> a = run(sorted, ranks), b = run(roaring, ranks);
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].coloring != b[i].coloring || a[i].info.colors != b[i].info.colors) {
            std::fprintf(stderr, "the two flavours disagree\n");
            return 6;
        }
        std::printf("color %s", a[i].tag.c_str());
        for (int32_t c : a[i].coloring) std::printf(" %d", int(c));
        std::printf("\ninfo %s %d %d %d %lld\n", a[i].tag.c_str(), int(a[i].info.colors), int(a[i].info.rounds), int(a[i].info.max_pred),
                    (long long)a[i].info.first_round);
        std::printf("check %s %lld %lld %d %d %d\n", a[i].tag.c_str(), (long long)a[i].check.conflicts, (long long)a[i].check.invalid,
                    int(a[i].check.max_color), int(a[i].check.distinct), int(a[i].check.max_degree));
    }
    gmsx_csr_free(csr);
    return 0;
}
