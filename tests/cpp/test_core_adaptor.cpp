// GPU test of gmsx::core_numbers / degeneracy_order / degree_order / order_quality (include/gmsx_set_graph.hpp), compiled against libgmsx.so
// only: loads the graph file argv[1] with the library's loader, runs the four adaptor functions over both set flavours (which must agree)
// and prints "degeneracy d", "core …", "order …" (order format), "degrank …" (rank format) and "quality <tag> max_later core_number faulty
// excess" for the exact order, the degree order and the ADG order (tests/test_core_adaptor_gpu.py compares them with the goldens).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    int32_t degeneracy = 0;
    gmsx_core_info info{};
    std::vector<int32_t> core, rank, order, degrank, adg;
    gmsx_order_quality_info q_exact{}, q_degree{}, q_adg{};
};

template <class G>
static Result run(const G &g) {
    Result r;
    r.degeneracy = gmsx::core_numbers(g, r.core, &r.info);
    if (gmsx::degeneracy_order(g, r.rank, true) != r.degeneracy || gmsx::degeneracy_order(g, r.order, false) != r.degeneracy) {
        std::fprintf(stderr, "degeneracy_order and core_numbers disagree on the degeneracy\n");
        std::exit(3);
    }
    for (size_t i = 0; i < r.order.size(); ++i) {
        if (r.rank[size_t(r.order[i])] != int32_t(i)) {
            std::fprintf(stderr, "order format is not the inverse of rank format\n");
            std::exit(4);
        }
    }
    gmsx::degree_order(g, r.degrank, true);
    gmsx::adg_rank(g, 0.001, r.adg, true);
    r.q_exact = gmsx::order_quality(g, r.order, false);                 // graded against the degeneracy computed on the device
    r.q_degree = gmsx::order_quality(g, r.degrank, true, r.degeneracy);
    r.q_adg = gmsx::order_quality(g, r.adg, true, r.degeneracy);
    if (r.q_exact.core_number != r.degeneracy || r.q_exact.max_later != r.degeneracy || r.q_exact.faulty != 0 || r.q_exact.excess != 0 ||
        r.q_exact.relative_error != 0.0 || r.q_adg.max_later > r.q_degree.max_later) {
        std::fprintf(stderr, "the exact order is not graded as exact (or ADG is worse than the degree order)\n");
        std::exit(5);
    }
    return r;
}

static void print_vec(const char *tag, const std::vector<int32_t> &v) {
    std::printf("%s", tag);
    for (int32_t x : v) std::printf(" %d", int(x));
    std::printf("\n");
}
static void print_q(const char *tag, const gmsx_order_quality_info &q) {
    std::printf("quality %s %d %d %lld %lld\n", tag, int(q.max_later), int(q.core_number), (long long)q.faulty, (long long)q.excess);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted), b = run(roaring);
    if (a.core != b.core || a.rank != b.rank || a.order != b.order || a.degrank != b.degrank || a.degeneracy != b.degeneracy) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    std::printf("degeneracy %d levels %d rounds %d top_core %lld\n", int(a.degeneracy), int(a.info.levels), int(a.info.rounds), (long long)a.info.top_core);
    print_vec("core", a.core);
    print_vec("order", a.order);
    print_vec("degrank", a.degrank);
    print_q("exact", a.q_exact);
    print_q("degree", a.q_degree);
    print_q("adg", a.q_adg);
    gmsx_csr_free(csr);
    return 0;
}
