// GPU test of gmsx::connected_components / jarvis_patrick / ktruss_components (include/gmsx_set_graph.hpp), compiled against libgmsx.so only:
// loads the graph file argv[1] with the library's loader, runs the adaptor functions over both set flavours (which must agree) and prints
// "cc components label …", "jp components kept_edges label …" (metric argv[2], threshold argv[3]) and per k = 2 … argv[4]
// "ktruss k components kept_edges label …" (tests/test_components_adaptor_gpu.py compares them with the goldens and the restatement).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<int32_t> cc, jp;
    std::vector<std::vector<int32_t>> truss;
    gmsx_components_info cc_info{}, jp_info{};
    std::vector<gmsx_components_info> truss_info;
};

template <class G>
static Result run(const G &g, int metric, double threshold, int32_t max_k) {
    Result r;
    if (gmsx::connected_components(g, r.cc, &r.cc_info) != r.cc_info.components || gmsx::jarvis_patrick(g, metric, threshold, r.jp, &r.jp_info) != r.jp_info.components) {
        std::fprintf(stderr, "the return value is not info.components\n");
        std::exit(3);
    }
    for (int32_t k = 2; k <= max_k; ++k) {
        r.truss.emplace_back();
        r.truss_info.emplace_back();
        gmsx::ktruss_components(g, k, r.truss.back(), &r.truss_info.back());
    }
    return r;
}

static void print_vec(const std::vector<int32_t> &v) {
    for (int32_t x : v) std::printf(" %d", int(x));
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int metric = std::atoi(argv[2]);
    const double threshold = std::atof(argv[3]);
    const int32_t max_k = std::atoi(argv[4]);
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted, metric, threshold, max_k), b = run(roaring, metric, threshold, max_k);
    if (a.cc != b.cc || a.jp != b.jp || a.truss != b.truss) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    std::printf("cc %lld", (long long)a.cc_info.components);
    print_vec(a.cc);
    std::printf("jp %lld %lld", (long long)a.jp_info.components, (long long)a.jp_info.kept_edges);
    print_vec(a.jp);
    for (int32_t k = 2; k <= max_k; ++k) {
        std::printf("ktruss %d %lld %lld", int(k), (long long)a.truss_info[size_t(k - 2)].components, (long long)a.truss_info[size_t(k - 2)].kept_edges);
        print_vec(a.truss[size_t(k - 2)]);
    }
    gmsx_csr_free(csr);
    return 0;
}
