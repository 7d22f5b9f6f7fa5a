// TEST: the opt-in listing route of include/gmsx_gms_glue.hpp.  Compiled by tests/test_bk_list_glue.py against the reference tree where it lies:
//   -DMINEBENCH_TEST -DGMSX_GLUE_BK_LIST [-DBK_COUNT] -DEXPECT_ROUTED=1   mceBench<HipSetGraph> / <HipRoaringGraph> list on the device (gmsx_bk_list)
//   -DMINEBENCH_TEST [-DBK_COUNT] -DEXPECT_ROUTED=0                       no opt-in: the reference's generic template, as before
// Run, a routed build lists the maximal cliques of a small Kronecker graph on the device and compares them with the reference's own list over
// RoaringGraph; without a device it must fail loudly ("no HIP device") — never return an empty list.
#include "gms/third_party/gapbs/benchmark.h"
#include <gms/common/cli/cli.h>
#include <gms/common/types.h>
#include <gms/representations/graphs/set_graph.h>
#include <gms/algorithms/set_based/maximal_clique_enum/bron_kerbosch.h>
#include <gmsx_gms_glue.hpp>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

static_assert(GMSX_GLUE_BK_LIST_ROUTED == EXPECT_ROUTED, "mceBench listing route does not follow GMSX_GLUE_BK_LIST / MINEBENCH_TEST");

template <class SGraph>
static std::vector<std::vector<int>> listed(const CSRGraph &g) {
    SGraph sg = SGraph::FromCGraph(g);
    pvector<NodeId> rank(sg.num_nodes());
    PpParallel::getDegreeOrdering<SGraph, true, pvector<NodeId>>(sg, rank);
    std::vector<std::vector<int>> out;
    for (const auto &s : BkEppsteinPar::mceBench<SGraph>(sg, rank)) {
        std::vector<int> m;
        for (auto v : s) m.push_back(int(v));
        std::sort(m.begin(), m.end());
        out.push_back(m);
    }
    std::sort(out.begin(), out.end());
#ifdef BK_COUNT
    if (BK_CLIQUE_COUNTER != out.size()) {
        std::printf("BK_CLIQUE_COUNTER %zu != %zu listed\n", size_t(BK_CLIQUE_COUNTER), out.size());
        std::exit(7);
    }
#endif
    return out;
}

int main() {
    std::vector<std::string> argv_s = {"glue", "-g", "kronecker", "8", "--deg", "16"};
    std::vector<char *> argv;
    for (auto &s : argv_s) argv.push_back(const_cast<char *>(s.c_str()));
    GMS::CLI::Parser parser;
    GMS::CLI::Args args = parser.parse((int)argv.size(), argv.data());
    CSRGraph g = args.load_graph();
    const auto want = listed<RoaringGraph>(g);  // the reference over its own sets
    const auto got = listed<HipSetGraph>(g);    // routed: the device; not routed: the generic template over the gmsx host sets
    const auto got_r = listed<HipRoaringGraph>(g);
    std::printf("routed %d listed %zu %zu %zu\n", GMSX_GLUE_BK_LIST_ROUTED, want.size(), got.size(), got_r.size());
    return !want.empty() && got == want && got_r == want ? 0 : 1;
}
