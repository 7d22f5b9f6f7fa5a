// GPU test of gmsx::maximal_cliques (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the graph file argv[1] with the
// library's loader, lists its maximal cliques on the device over both set flavours and prints them, one per line, members ascending and
// space-separated (tests/test_bk_list_gpu.py compares them with the goldens).  The two flavours and a rank vector must give the same set.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "gmsx_set_graph.hpp"

template <class G>
static std::vector<std::vector<int>> as_lists(const G &g, bool with_rank) {
    std::vector<std::vector<int>> out;
    std::vector<int32_t> rank(size_t(g.num_nodes()));
    for (size_t i = 0; i < rank.size(); ++i) rank[i] = int32_t(rank.size() - 1 - i);
    const auto cliques = with_rank ? gmsx::maximal_cliques(g, rank) : gmsx::maximal_cliques(g);
    for (const auto &c : cliques) {
        std::vector<int> m;
        for (auto v : c) m.push_back(int(v));
        if (!std::is_sorted(m.begin(), m.end())) {
            std::fprintf(stderr, "a clique is not ascending\n");
            std::exit(3);
        }
        out.push_back(m);
    }
    std::sort(out.begin(), out.end());
    return out;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const auto a = as_lists(sorted, false), b = as_lists(roaring, true);
    if (a != b) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 4;
    }
    if (a.size() != gmsx::maximal_clique_count(sorted)) {
        std::fprintf(stderr, "list size != maximal_clique_count\n");
        return 5;
    }
    for (const auto &c : a) {
        for (size_t i = 0; i < c.size(); ++i) std::printf(i ? " %d" : "%d", c[i]);
        std::printf("\n");
    }
    gmsx_csr_free(csr);
    return 0;
}
