// Test of gmsx::pagerank / pagerank_residual / top_scores (include/gmsx_set_graph.hpp), compiled against libgmsx.so only.
//   test_pagerank_adaptor --host         top_scores alone (no device): exits 0 when its checks hold
//   test_pagerank_adaptor FILE | kronecker SCALE
// loads the graph with the library's loader (or generates it), runs the adaptor over both set flavours (which must agree byte for byte) at the
// reference's arguments, with GMSX_PR_DANGLING and with GMSX_PR_FLOAT32, and prints per run "run FLAGS iterations converged argmax error sum
// residual", "top FLAGS id:score …" and "scores FLAGS s0 s1 …" — the doubles as hex floats (tests/test_pagerank_adaptor_gpu.py compares them
// with the goldens).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gmsx_set_graph.hpp"

static int host_checks() {
    const std::vector<double> s = {0.25, 0.5, 0.125, 0.5, 0.0, 0.5, 0.25};
    const auto top = gmsx::top_scores(s, 5);
    const std::vector<std::pair<int32_t, double>> want = {{1, 0.5}, {3, 0.5}, {5, 0.5}, {0, 0.25}, {6, 0.25}};  // ties: the smaller id
    if (top != want) return 1;
    if (gmsx::top_scores(s, 0).size() != 0 || gmsx::top_scores(s, 100).size() != s.size()) return 2;
    if (gmsx::top_scores(s, 100).back() != std::pair<int32_t, double>{4, 0.0}) return 3;
    if (!gmsx::top_scores({}, 5).empty()) return 4;
    return 0;
}

struct Result {
    std::vector<double> scores;
    gmsx_pagerank_info info{};
    double residual = 0.0;
};

template <class G>
static Result run(const G &g, uint32_t flags) {
    Result r;
    if (gmsx::pagerank(g, r.scores, 0.85, 20, 1e-4, nullptr, flags, &r.info) != r.info.iterations) {
        std::fprintf(stderr, "the return value is not info.iterations\n");
        std::exit(3);
    }
    r.residual = gmsx::pagerank_residual(g, r.scores, 0.85, nullptr, flags);
    const auto top = gmsx::top_scores(r.scores, 1);
    if (!top.empty() && (top[0].first != r.info.argmax || top[0].second != r.info.max_score)) {
        std::fprintf(stderr, "top_scores disagrees with info.argmax\n");
        std::exit(3);
    }
    return r;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (std::string(argv[1]) == "--host") {
        const int rc = host_checks();
        std::printf(rc ? "top_scores: check %d failed\n" : "top_scores ok\n", rc);
        return rc;
    }
    gmsx_csr *csr = nullptr;
    if (std::string(argv[1]) == "kronecker" && argc >= 3)
        gmsx::detail::check(gmsx_csr_generate(GMSX_GEN_KRONECKER, std::atoi(argv[2]), 16, GMSX_RELABEL_AUTO, 0, &csr), "gmsx_csr_generate");
    else
        gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    for (uint32_t flags : {uint32_t(GMSX_PR_DEFAULT), uint32_t(GMSX_PR_DANGLING), uint32_t(GMSX_PR_FLOAT32)}) {
        const Result a = run(sorted, flags), b = run(roaring, flags);
        if (a.scores != b.scores || std::memcmp(&a.info, &b.info, sizeof a.info) != 0 || a.residual != b.residual) {
            std::fprintf(stderr, "the two flavours disagree\n");
            return 6;
        }
        std::printf("run %u %d %d %d %a %a %a\n", flags, int(a.info.iterations), int(a.info.converged), int(a.info.argmax), a.info.error, a.info.sum,
                    a.residual);
        std::printf("top %u", flags);
        for (const auto &kv : gmsx::top_scores(a.scores, 5)) std::printf(" %d:%a", int(kv.first), kv.second);
        std::printf("\nscores %u", flags);
        for (double x : a.scores) std::printf(" %a", x);
        std::printf("\n");
    }
    gmsx_csr_free(csr);
    return 0;
}
