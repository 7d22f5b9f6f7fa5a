// GPU test of gmsx::edge_support / truss_numbers / ktruss_edges (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the
// graph file argv[1] with the library's loader, runs the adaptor functions over both set flavours (which must agree) and prints
// "info max_truss levels rounds max_support top_edges triangles", "support …" and "truss …" (per arc) and per k = 2 … max_truss "ktruss k u v u v …"
// (tests/test_truss_adaptor_gpu.py compares them with the goldens).
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    int32_t max_truss = 0;
    uint64_t triangles = 0;
    gmsx_truss_info info{};
    std::vector<int32_t> support, truss;
};

template <class G>
static Result run(const G &g) {
    Result r;
    r.triangles = gmsx::edge_support(g, r.support);
    r.max_truss = gmsx::truss_numbers(g, r.truss, &r.info);
    if (r.info.max_truss != r.max_truss || uint64_t(r.info.triangles) != r.triangles || r.triangles != uint64_t(gmsx::count_total(g))) {
        std::fprintf(stderr, "truss_numbers, edge_support and count_total disagree\n");
        std::exit(3);
    }
    return r;
}

static void print_vec(const char *tag, const std::vector<int32_t> &v) {
    std::printf("%s", tag);
    for (int32_t x : v) std::printf(" %d", int(x));
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted), b = run(roaring);
    if (a.support != b.support || a.truss != b.truss || a.max_truss != b.max_truss) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    std::printf("info %d %d %d %d %lld %lld\n", int(a.info.max_truss), int(a.info.levels), int(a.info.rounds), int(a.info.max_support),
                (long long)a.info.top_edges, (long long)a.info.triangles);
    print_vec("support", a.support);
    print_vec("truss", a.truss);
    for (int32_t k = 2; k <= a.max_truss; ++k) {
        std::printf("ktruss %d", int(k));
        for (const std::pair<int32_t, int32_t> &e : gmsx::ktruss_edges(sorted, k)) std::printf(" %d %d", int(e.first), int(e.second));
        std::printf("\n");
    }
    gmsx_csr_free(csr);
    return 0;
}
