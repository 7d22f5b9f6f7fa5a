// GPU test of gmsx::clique_stars / gmsx::cliques (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the graph file argv[1]
// with the library's loader, lists its (clique, star) pairs for k = argv[2] on the device over both set flavours and prints them, one per
// line, "c1 … ck | s1 …" (tests/test_kcstar_list_gpu.py compares them with the goldens).  The two flavours must give the same pairs, and
// gmsx::cliques the same cliques.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "gmsx_set_graph.hpp"

using Pair = std::pair<std::vector<int>, std::vector<int>>;

template <class S>
static std::vector<int> ids_of(const S &s) {
    std::vector<int> m;
    for (auto v : s) m.push_back(int(v));
    if (!std::is_sorted(m.begin(), m.end())) {
        std::fprintf(stderr, "a set is not ascending\n");
        std::exit(3);
    }
    return m;
}

template <class G>
static std::vector<Pair> as_pairs(const G &g, int k) {
    std::vector<Pair> out;
    std::vector<std::vector<int>> only;
    for (const auto &p : gmsx::clique_stars(g, k)) out.emplace_back(ids_of(p[0]), ids_of(p[1]));
    for (const auto &c : gmsx::cliques(g, k)) only.push_back(ids_of(c));
    std::sort(out.begin(), out.end());
    std::sort(only.begin(), only.end());
    if (only.size() != out.size()) {
        std::fprintf(stderr, "cliques() and clique_stars() disagree in size\n");
        std::exit(6);
    }
    for (size_t i = 0; i < out.size(); ++i) {
        if (only[i] != out[i].first || int(only[i].size()) != k) {
            std::fprintf(stderr, "cliques() and clique_stars() disagree\n");
            std::exit(6);
        }
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int k = std::atoi(argv[2]);
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const auto a = as_pairs(sorted, k), b = as_pairs(roaring, k);
    if (a != b) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 4;
    }
    uint64_t stars = 0;
    gmsx::detail::check(gmsx_kclique_star_count(sorted.device(), k, &stars, nullptr, nullptr), "gmsx_kclique_star_count");
    if (uint64_t(a.size()) != stars) {
        std::fprintf(stderr, "list size != gmsx_kclique_star_count\n");
        return 5;
    }
    for (const auto &p : a) {
        for (int v : p.first) std::printf("%d ", v);
        std::printf("|");
        for (int v : p.second) std::printf(" %d", v);
        std::printf("\n");
    }
    gmsx_csr_free(csr);
    return 0;
}
