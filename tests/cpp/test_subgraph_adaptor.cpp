// GPU test of gmsx::subgraph_isomorphism / subgraph_isomorphisms (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the
// target argv[1] and the patterns argv[2 ..] with the library's loader (never relabelled) and prints per pattern i
//   "iso i t:p ..."        the std::map of subgraph_isomorphism in key order (target vertex : pattern vertex; nothing after the index if empty)
//   "induced i k ids ..."  the rows of subgraph_isomorphisms, flattened, and "mono i k ids ..." those of GMSX_SGM_MONO
// (tests/test_subgraph_adaptor_gpu.py compares them with the goldens).  The pattern is handed over once as a graph object and once as raw arrays.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "gmsx_set_graph.hpp"

static void print_rows(const char *tag, int i, int k, const std::vector<int32_t> &rows) {
    std::printf("%s %d %d", tag, i, k);
    for (int32_t x : rows) std::printf(" %d", int(x));
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_NEVER, &csr), "gmsx_csr_load");
    auto g = gmsx::HipSetGraph::FromCsr(csr);
    auto g_roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    for (int i = 2; i < argc; ++i) {
        gmsx_csr *pc = nullptr;
        gmsx::detail::check(gmsx_csr_load(argv[i], 1, GMSX_RELABEL_NEVER, &pc), "gmsx_csr_load (pattern)");
        auto pattern = gmsx::HipSetGraph::FromCsr(pc);
        const int k = int(pattern.num_nodes());
        const std::map<int, int> iso = gmsx::subgraph_isomorphism(g, pattern);
        std::printf("iso %d", i - 2);
        for (const auto &pr : iso) std::printf(" %d:%d", pr.first, pr.second);
        std::printf("\n");
        gmsx_subgraph_info info{};
        const std::vector<int32_t> induced = gmsx::subgraph_isomorphisms(g, pattern, GMSX_SGM_INDUCED, 0, 1, &info);
        const std::vector<int32_t> mono = gmsx::subgraph_isomorphisms(g_roaring, k, gmsx_csr_offsets(pc), gmsx_csr_neighbors(pc), GMSX_SGM_MONO);
        if (info.k != k || info.embeddings * k != int64_t(induced.size()) || iso.empty() != induced.empty() ||
            gmsx::subgraph_isomorphism(g_roaring, pattern, GMSX_SGM_MONO).empty() != mono.empty()) {
            std::fprintf(stderr, "info, the list and the single mapping disagree\n");
            return 3;
        }
        print_rows("induced", i - 2, k, induced);
        print_rows("mono", i - 2, k, mono);
        gmsx_csr_free(pc);
    }
    gmsx_csr_free(csr);
    return 0;
}
