// GPU test of gmsx::label_propagation / gmsx::modularity (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the weighted file
// argv[2] ("file") or generates the weighted kronecker graph of scale argv[2] ("kron"), attaches the weights, runs the adaptor functions over both
// set flavours (which must agree) and prints, unweighted ("u") and weighted ("w"),
// "lp u|w communities largest singletons changes sweeps colors converged fnv W I S_hi S_lo unstable" — fnv = FNV-1a over the bytes of the int32
// labels (tests/test_communities_adaptor_gpu.py compares the lines with the goldens).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<int32_t> label;
    gmsx_lp_info info{};
    gmsx_modularity_info mod{};
};

template <class G>
static Result run(const G &g, const gmsx_csr *csr, uint32_t flags) {
    const int64_t nnz = g.num_nodes() > 0 ? g.offsets()[g.num_nodes()] : 0;
    gmsx::set_weights(g, std::vector<int32_t>(gmsx_csr_weights(csr), gmsx_csr_weights(csr) + nnz));
    Result r;
    if (gmsx::label_propagation(g, r.label, flags, nullptr, 0, &r.info) != r.info.communities) {
        std::fprintf(stderr, "the return value is not info.communities\n");
        std::exit(3);
    }
    // the default colouring passed by the caller gives the same bytes
    const std::vector<int32_t> colors = gmsx::coloring(g, "id");
    std::vector<int32_t> again;
    gmsx_lp_info info2{};
    gmsx::label_propagation(g, again, flags, &colors, 0, &info2);
    if (again != r.label || std::memcmp(&info2, &r.info, sizeof info2) != 0) {
        std::fprintf(stderr, "the caller's copy of the default colouring gives another result\n");
        std::exit(4);
    }
    r.mod = gmsx::modularity(g, r.label, flags);
    if (r.mod.communities != r.info.communities || r.mod.largest != r.info.largest || (r.info.converged && r.mod.unstable != 0)) {
        std::fprintf(stderr, "the two calls disagree\n");
        std::exit(5);
    }
    return r;
}

static unsigned long long fnv(const std::vector<int32_t> &label) {
    unsigned long long x = 1469598103934665603ull;
    for (const int32_t value : label) {
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
    for (uint32_t flags : {0u, uint32_t(GMSX_LP_WEIGHTED)}) {
        const Result a = run(sorted, csr, flags), b = run(roaring, csr, flags);
        if (a.label != b.label || std::memcmp(&a.info, &b.info, sizeof a.info) != 0 || std::memcmp(&a.mod, &b.mod, sizeof a.mod) != 0) {
            std::fprintf(stderr, "the two flavours disagree\n");
            return 6;
        }
        std::printf("lp %s %lld %lld %lld %lld %d %d %d %llu %lld %lld %llu %llu %lld\n", flags ? "w" : "u", (long long)a.info.communities,
                    (long long)a.info.largest, (long long)a.info.singletons, (long long)a.info.changes, int(a.info.sweeps), int(a.info.colors),
                    int(a.info.converged), fnv(a.label), (long long)a.mod.total_weight, (long long)a.mod.intra_weight,
                    (unsigned long long)a.mod.sumsq_hi, (unsigned long long)a.mod.sumsq_lo, (long long)a.mod.unstable);
    }
    gmsx_csr_free(csr);
    return 0;
}
