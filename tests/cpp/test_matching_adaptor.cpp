// GPU test of gmsx::greedy_matching / gmsx::matching_verify (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the weighted
// file argv[2] ("file") or generates the weighted kronecker graph of scale argv[2] ("kron"), attaches the weights, runs the adaptor functions
// over both set flavours (which must agree) and prints, for unit weights and for the attached ones,
// "matching unit|weighted pairs total_weight free_vertices rounds fnv certified" — fnv = FNV-1a over the bytes of the mate int32 array,
// certified = what gmsx::matching_verify returns for it (tests/test_matching_adaptor_gpu.py compares the lines with the goldens).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<int32_t> mate;
    std::vector<gmsx::WeightedEdge> edges;
    gmsx_matching_info info{};
    bool certified = false;
};

template <class G>
static Result run(const G &g, const gmsx_csr *csr, uint32_t flags) {
    const int64_t nnz = g.num_nodes() > 0 ? g.offsets()[g.num_nodes()] : 0;
    gmsx::set_weights(g, std::vector<int32_t>(gmsx_csr_weights(csr), gmsx_csr_weights(csr) + nnz));
    Result r;
    gmsx_matching_info plain{};
    std::vector<int32_t> again;
    if (gmsx::greedy_matching(g, r.mate, flags, &r.edges, &r.info) != r.info.pairs || int64_t(r.edges.size()) != r.info.pairs) {
        std::fprintf(stderr, "the return value is not info.pairs\n");
        std::exit(3);
    }
    gmsx::greedy_matching(g, again, flags, nullptr, &plain);
    if (std::memcmp(&plain, &r.info, sizeof plain) != 0 || again != r.mate) {
        std::fprintf(stderr, "the two calls disagree\n");
        std::exit(4);
    }
    // the pair list is the mate array: ascending by u, u < v, both ends point at each other, and nobody else is matched
    int64_t matched = 0;
    for (int32_t m : r.mate) matched += m >= 0;
    for (size_t i = 0; i < r.edges.size(); ++i) {
        const gmsx::WeightedEdge &e = r.edges[i];
        if (e.u >= e.v || r.mate[size_t(e.u)] != e.v || r.mate[size_t(e.v)] != e.u || (i > 0 && r.edges[i - 1].u >= e.u)) {
            std::fprintf(stderr, "pair %d %d does not fit the mate array\n", int(e.u), int(e.v));
            std::exit(5);
        }
    }
    if (matched != 2 * r.info.pairs || matched + r.info.free_vertices != g.num_nodes()) {
        std::fprintf(stderr, "%lld vertices are matched for %lld pairs\n", (long long)matched, (long long)r.info.pairs);
        std::exit(5);
    }
    gmsx_matching_check check{};
    r.certified = gmsx::matching_verify(g, r.mate, flags, &check) && check.pairs == r.info.pairs && check.total_weight == r.info.total_weight &&
                  check.augmentable == 0;
    // a dropped pair must show
    if (!r.edges.empty()) {
        std::vector<int32_t> fewer = r.mate;
        fewer[size_t(r.edges[0].u)] = fewer[size_t(r.edges[0].v)] = -1;
        if (gmsx::matching_verify(g, fewer, flags, &check) || check.augmentable < 1 || check.invalid != 0) r.certified = false;
    }
    return r;
}

static unsigned long long fnv(const std::vector<int32_t> &mate) {
    unsigned long long x = 1469598103934665603ull;
    for (int32_t value : mate) {
        unsigned char bytes[4];
        std::memcpy(bytes, &value, 4);
        for (unsigned char b : bytes) {
            x ^= b;
            x *= 1099511628211ull;
        }
    }
    return x;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    gmsx_csr *csr = nullptr;
    if (std::strcmp(argv[1], "file") == 0)
        gmsx::detail::check(gmsx_csr_load_weighted(argv[2], 1, GMSX_RELABEL_NEVER, &csr), "gmsx_csr_load_weighted");
    else
        gmsx::detail::check(gmsx_csr_generate_weighted(GMSX_GEN_KRONECKER, std::atoi(argv[2]), 16, GMSX_RELABEL_NEVER, 0, &csr), "gmsx_csr_generate_weighted");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    for (uint32_t flags : {0u, uint32_t(GMSX_MATCH_WEIGHTED)}) {
        const Result a = run(sorted, csr, flags), b = run(roaring, csr, flags);
        if (a.mate != b.mate || a.edges != b.edges) {
            std::fprintf(stderr, "the two flavours disagree\n");
            return 6;
        }
        std::printf("matching %s %lld %lld %lld %d %llu %d\n", flags ? "weighted" : "unit", (long long)a.info.pairs, (long long)a.info.total_weight,
                    (long long)a.info.free_vertices, int(a.info.rounds), fnv(a.mate), int(a.certified && b.certified));
    }
    gmsx_csr_free(csr);
    return 0;
}
