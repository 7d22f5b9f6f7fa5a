// GPU test of gmsx::cycle4_count / gmsx::motif_census4 (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the graph file
// argv[1] with the library's loader, runs the adaptor functions over both set flavours (which must agree) and prints "cycle4 cycles",
// "at_vertex …", "subgraphs …", "induced …" and "walked wedges max_codegree" (tests/test_motifs_adaptor_gpu.py compares them with the restatement).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    uint64_t cycles = 0;
    std::vector<int64_t> at;
    gmsx_motif_info info{};
};

template <class G>
static Result run(const G &g) {
    Result r;
    r.cycles = gmsx::cycle4_count(g, r.at);
    if (gmsx::cycle4_count(g) != r.cycles) {
        std::fprintf(stderr, "the count depends on at_vertex\n");
        std::exit(3);
    }
    r.info = gmsx::motif_census4(g);
    return r;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted), b = run(roaring);
    if (a.cycles != b.cycles || a.at != b.at || std::memcmp(&a.info, &b.info, sizeof a.info) != 0) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    std::printf("cycle4 %llu\nat_vertex", (unsigned long long)a.cycles);
    for (int64_t x : a.at) std::printf(" %lld", (long long)x);
    std::printf("\nsubgraphs");
    for (int k = 0; k < GMSX_MOTIF_KINDS; ++k) std::printf(" %llu", (unsigned long long)a.info.subgraphs[k]);
    std::printf("\ninduced");
    for (int k = 0; k < GMSX_MOTIF_KINDS; ++k) std::printf(" %llu", (unsigned long long)a.info.induced[k]);
    std::printf("\nwalked %llu %d\n", (unsigned long long)a.info.wedges_walked, int(a.info.max_codegree));
    gmsx_csr_free(csr);
    return 0;
}
