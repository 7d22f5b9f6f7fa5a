// GPU test of gmsx::link_prediction / link_prediction_shard / merge_link_predictions / link_prediction_precision (include/gmsx_set_graph.hpp),
// compiled against libgmsx.so only: loads the graph file argv[1] with the library's loader and, for every further argument "metric:q", prints
// "R metric q size" and the padded result verbatim, one "E u v score" line per entry (score as a hex float), over both set flavours (which must
// agree); three shards merged must equal the whole.  Then K5 (nothing qualifies: one padded entry) and the precision of a list against the
// graph itself.  tests/test_link_prediction_adaptor_gpu.py compares the lines with the goldens.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gmsx_set_graph.hpp"

template <class G>
static gmsx::ScoredEdges run(const G &g, int metric, int64_t q) {
    const gmsx::ScoredEdges whole = gmsx::link_prediction(g, metric, q);
    std::vector<gmsx::ScoredEdges> parts;
    for (int p = 0; p < 3; ++p) parts.push_back(gmsx::link_prediction_shard(g, metric, q, p, 3));
    const gmsx::ScoredEdges merged = gmsx::merge_link_predictions(parts, q);
    if (merged.edges != whole.edges || merged.found != whole.found || merged.scores.size() != whole.scores.size() ||
        std::memcmp(merged.scores.data(), whole.scores.data(), whole.scores.size() * sizeof(double)) != 0) {
        std::fprintf(stderr, "three shards merged differ from the whole (metric %d, q %lld)\n", metric, (long long)q);
        std::exit(7);
    }
    return whole;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    gmsx_csr *csr = nullptr;
    gmsx::detail::check(gmsx_csr_load(argv[1], 1, GMSX_RELABEL_AUTO, &csr), "gmsx_csr_load");
    auto sorted = gmsx::HipSetGraph::FromCsr(csr);
    auto roaring = gmsx::HipRoaringGraph::FromCsr(csr);
    for (int i = 2; i < argc; ++i) {
        int metric = 0;
        long long q = 0;
        if (std::sscanf(argv[i], "%d:%lld", &metric, &q) != 2) return 2;
        const gmsx::ScoredEdges a = run(sorted, metric, q), b = run(roaring, metric, q);
        if (a.edges != b.edges || a.scores.size() != b.scores.size() || std::memcmp(a.scores.data(), b.scores.data(), a.scores.size() * sizeof(double)) != 0) {
            std::fprintf(stderr, "the two flavours disagree\n");
            return 6;
        }
        std::printf("R %d %lld %zu\n", metric, q, a.edges.size());
        for (size_t e = 0; e < a.edges.size(); ++e) std::printf("E %d %d %a\n", int(a.edges[e].first), int(a.edges[e].second), a.scores[e]);
    }
    // nothing qualifies: K5 has no non-edge — the reference returns exactly one (-1.0, (0,0)) entry
    {
        std::vector<int32_t> src, dst;
        for (int32_t x = 0; x < 5; ++x)
            for (int32_t y = 0; y < x; ++y) { src.push_back(x); dst.push_back(y); }
        gmsx_csr *k5 = nullptr;
        gmsx::detail::check(gmsx_csr_from_edges(5, int64_t(src.size()), src.data(), dst.data(), 1, GMSX_RELABEL_NEVER, &k5), "gmsx_csr_from_edges");
        auto g5 = gmsx::HipSetGraph::FromCsr(k5);
        for (int metric = 0; metric < 7; ++metric) {
            const gmsx::ScoredEdges r = run(g5, metric, 4);
            std::printf("K5 %d %zu %d %d %a %lld\n", metric, r.edges.size(), int(r.edges[0].first), int(r.edges[0].second), r.scores[0], (long long)r.found);
        }
        // every edge of K5 predicted once plus one of them again, swapped: all 10 edges hit, 11 predictions
        std::vector<std::pair<int32_t, int32_t>> pred;
        for (size_t e = 0; e < src.size(); ++e) pred.emplace_back(src[e], dst[e]);
        pred.emplace_back(dst[0], src[0]);
        const gmsx::LinkPredictionScore sc = gmsx::link_prediction_precision(g5, pred);
        std::printf("P %lld %lld %a %a\n", (long long)sc.true_positives, (long long)sc.true_count, sc.precision, sc.recall);
        gmsx_csr_free(k5);
    }
    gmsx_csr_free(csr);
    return 0;
}
