// GPU test of gmsx::min_spanning_forest / gmsx::msf_arc_mask (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the weighted
// file argv[2] ("file") or generates the weighted kronecker graph of scale argv[2] ("kron"), attaches the weights, runs the adaptor functions
// over both set flavours (which must agree) and prints, for the minimum and the maximum forest,
// "msf min|max edges total_weight trees rounds fnv mask_ones" — fnv = FNV-1a over the bytes of the u, v and w int32 arrays
// (tests/test_msf_adaptor_gpu.py compares the lines with the goldens).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<gmsx::WeightedEdge> edges;
    std::vector<uint8_t> mask;
    gmsx_msf_info info{};
};

template <class G>
static Result run(const G &g, const gmsx_csr *csr, uint32_t flags) {
    const int64_t nnz = g.num_nodes() > 0 ? g.offsets()[g.num_nodes()] : 0;
    gmsx::set_weights(g, std::vector<int32_t>(gmsx_csr_weights(csr), gmsx_csr_weights(csr) + nnz));
    Result r;
    gmsx_msf_info mask_info{};
    if (gmsx::min_spanning_forest(g, r.edges, flags, &r.info) != r.info.total_weight) {
        std::fprintf(stderr, "the return value is not info.total_weight\n");
        std::exit(3);
    }
    r.mask = gmsx::msf_arc_mask(g, flags, &mask_info);
    if (std::memcmp(&mask_info, &r.info, sizeof mask_info) != 0 || int64_t(r.mask.size()) != nnz || int64_t(r.edges.size()) != r.info.edges) {
        std::fprintf(stderr, "the two calls disagree\n");
        std::exit(4);
    }
    // every listed edge is marked on both of its arcs, and nothing else is
    int64_t ones = 0;
    for (uint8_t b : r.mask) ones += b;
    for (const gmsx::WeightedEdge &e : r.edges) {
        bool both = e.u < e.v;
        for (int k = 0; k < 2 && both; ++k) {
            const int32_t a = k ? e.v : e.u, b = k ? e.u : e.v;
            const int32_t *lo = g.neighbors() + g.offsets()[a], *hi = g.neighbors() + g.offsets()[a + 1];
            const int32_t *at = std::lower_bound(lo, hi, b);
            both = at != hi && *at == b && r.mask[size_t(at - g.neighbors())] == 1;
        }
        if (!both) {
            std::fprintf(stderr, "edge %d %d is not marked on both arcs\n", int(e.u), int(e.v));
            std::exit(5);
        }
    }
    if (ones != 2 * r.info.edges) {
        std::fprintf(stderr, "%lld bytes are set for %lld edges\n", (long long)ones, (long long)r.info.edges);
        std::exit(5);
    }
    return r;
}

static unsigned long long fnv(const std::vector<gmsx::WeightedEdge> &edges) {
    unsigned long long x = 1469598103934665603ull;
    for (int field = 0; field < 3; ++field)
        for (const gmsx::WeightedEdge &e : edges) {
            const int32_t value = field == 0 ? e.u : field == 1 ? e.v : e.w;
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
    for (uint32_t flags : {0u, uint32_t(GMSX_MSF_MAXIMUM)}) {
        const Result a = run(sorted, csr, flags), b = run(roaring, csr, flags);
        if (a.edges != b.edges || a.mask != b.mask) {
            std::fprintf(stderr, "the two flavours disagree\n");
            return 6;
        }
        std::printf("msf %s %lld %lld %lld %d %llu %lld\n", flags ? "max" : "min", (long long)a.info.edges, (long long)a.info.total_weight,
                    (long long)a.info.trees, int(a.info.rounds), fnv(a.edges), (long long)(2 * a.info.edges));
    }
    gmsx_csr_free(csr);
    return 0;
}
