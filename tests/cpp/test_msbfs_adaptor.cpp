// GPU test of gmsx::bfs_multi / closeness (include/gmsx_set_graph.hpp), compiled against libgmsx.so only: loads the graph file argv[1] with the
// library's loader (or generates "kronecker SCALE" with its generator), runs the adaptor functions over both set flavours from every vertex as
// a source (which must agree byte for byte) and prints per source "source i reached reached_arcs depth_sum levels closeness harmonic" — the
// doubles as hex floats —, "dist_sum v0 …", "reach v0 …", "far v0 …" and "top closeness harmonic"
// (tests/test_msbfs_adaptor_gpu.py compares them with the goldens).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gmsx_set_graph.hpp"

struct Result {
    std::vector<gmsx_bfs_source> per;
    std::vector<int32_t> depth, reach, far;
    std::vector<int64_t> dist_sum;
    std::vector<double> close, harm;
    double top_close = 0.0, top_harm = 0.0;
    gmsx_bfs_multi_info info{};
};

template <class G>
static Result run(const G &g, const std::vector<int32_t> &sources) {
    Result r;
    if (gmsx::bfs_multi(g, sources, r.per, &r.depth, &r.dist_sum, &r.reach, &r.far, &r.info) != r.info.reached_total) {
        std::fprintf(stderr, "the return value is not info.reached_total\n");
        std::exit(3);
    }
    r.top_close = gmsx::closeness(g, sources, r.close);
    r.top_harm = gmsx::closeness(g, sources, r.harm, true);
    for (size_t i = 0; i < sources.size(); ++i)
        if (r.close[i] != r.per[i].closeness || r.harm[i] != r.per[i].harmonic || r.depth[i * size_t(g.num_nodes()) + size_t(sources[i])] != 0) {
            std::fprintf(stderr, "closeness() disagrees with bfs_multi()\n");
            std::exit(3);
        }
    return r;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    if (std::string(argv[1]) == "kronecker" && argc >= 3)
        gmsx::detail::check(gmsx_csr_generate(GMSX_GEN_KRONECKER, std::atoi(argv[2]), 16, GMSX_RELABEL_AUTO, 0, &csr), "gmsx_csr_generate");
    else
        gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    std::vector<int32_t> sources(size_t(gmsx_csr_num_nodes(csr)));
    for (size_t i = 0; i < sources.size(); ++i) sources[i] = int32_t(i);
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    const Result a = run(sorted, sources), b = run(roaring, sources);
    if (a.per.size() != b.per.size() || std::memcmp(a.per.data(), b.per.data(), a.per.size() * sizeof(gmsx_bfs_source)) != 0 || a.depth != b.depth ||
        a.dist_sum != b.dist_sum || a.reach != b.reach || a.far != b.far) {
        std::fprintf(stderr, "the two flavours disagree\n");
        return 6;
    }
    for (size_t i = 0; i < a.per.size(); ++i)
        std::printf("source %zu %lld %lld %lld %d %a %a\n", i, (long long)a.per[i].reached, (long long)a.per[i].reached_arcs, (long long)a.per[i].depth_sum,
                    int(a.per[i].levels), a.per[i].closeness, a.per[i].harmonic);
    std::printf("dist_sum");
    for (int64_t x : a.dist_sum) std::printf(" %lld", (long long)x);
    std::printf("\nreach");
    for (int32_t x : a.reach) std::printf(" %d", int(x));
    std::printf("\nfar");
    for (int32_t x : a.far) std::printf(" %d", int(x));
    std::printf("\ntop %a %a\n", a.top_close, a.top_harm);
    gmsx_csr_free(csr);
    return 0;
}
