// gmsx_driver — command-line driver with the reference drivers' flags and output lines, running the device path
// through include/gmsx_set_graph.hpp (C++ adaptor) -> include/gmsx.h (C-ABI).
//
// Mirrors (paths relative to the spcl/gms tree):
//   flags        gms/common/cli/cli.h:75-155   -g kronecker|uniform <scale> [--deg d] | -f file ; -v ; -n trials ; -t threads ; -p name=value
//   loading      gms/common/cli/cli.h:157-184  (generate/load, reject directed, relabel when WorthRelabelling)
//   trial loop   gms/common/benchmark.h:96-196 ("GraphExec buildTime", "Preprocess Time", "Trial Time", "Verification", "@@@ …", "Average Time")
//   kernels      triangle_count.cc:22-48, k_clique_count_set_based.cc:27-47, maximal_clique_enum_bron_kerbosch.cc:32-57 (ADG rank + mceBench)
//   verifiers    triangle_count/verifier.h:13-85 (serial host recount), maximal_clique_enum/verifier.h:41-49 (sequential Tomita
//                recount): `-v` recounts ON THE HOST with this file's own plain loops (not the device, not oracle/) for graphs up
//                to a stated size; beyond it the check is a differently decomposed device run and the output says so.
// Added:  --gpus N   one process per GPU (this binary FORKS its N ranks before it touches HIP and stays behind as their supervisor), every rank counts its
//                    shard (gmsx_*_partial) and ONE u64 all-reduce over RCCL (gmsx_comm_allreduce_u64) replaces the OpenMP
//                    reduction(+:total) of parallel/total.h:12.  --gpus 1 runs the same path with a 1-rank communicator.
// Added:  bk --list FILE   the maximal cliques of the last trial (gmsx_bk_list, outside the timed trial), one per line, members ascending.
// Added:  bk --order adg|deg|dgr   which preprocessor the timed "Preprocess Time" runs and hands its rank to the search: gmsx_adg_rank (default; BK-GMS-ADG),
//                    gmsx_degree_rank (BK-GMS-DEG) or the exact degeneracy order of gmsx_core_decomposition (BK-GMS-DGR).  The count does not depend on it.
// Added:  lp --metric jaccard|overlap|adamic_adar|resource|common|total|prefatt -q N [--list FILE]   GMS::LinkPrediction::link_prediction_similarity<Metric>
//                    (set_based/link_prediction/link_prediction.h:42-101) on the device (gmsx_link_prediction): the N best-scoring non-edges; N defaults to m / 4, the
//                    choice of the reference's bench_ranking (link_prediction.cc:36).  --list writes the result of the last trial in the reference's shape, padding
//                    included, one "u v score" line per entry, worst first, the score as a hex float.  Not sharded (--gpus > 1 is refused).
// Added:  kcstar -p clique-size=k [--list FILE]   KCliqueStar::Par::CliqueStarList (k_clique_star_list/parallel/recursive.h:19-43) on the device: prints the
//                    reference's "total k-cliques: N" line (:34, N = the number of pairs); --list writes the pairs of the last trial (gmsx_kclique_star_list, outside
//                    the timed trial), one per line: "c1 … ck | s1 …", clique and star ascending.  Not sharded (--gpus > 1 is refused).
// Added:  color [--order id|ff|lf|sl|adg] [--eps e]   GMS::Coloring::JonesV3::graph_coloring_jones (non_set_based/coloring/coloring_jones_v3.h:38-68) on the device
//                    (gmsx_coloring_jp) with the trial loop and the labels of benchmarkGraphColoringWithReordering (coloring.cc:82-129): per trial "Preprocess Time"
//                    (the order: id = getSimpleIdOrdering, the reference's; ff = n-1-v; lf = gmsx_degree_rank; sl = gmsx_core_decomposition; adg = gmsx_adg_rank(eps)),
//                    "Trial Time", "Colors" and with -v "Verification" (gmsx_coloring_verify read as GCVerifierMaxColor), then the three averages.  A colouring is
//                    global: not sharded (--gpus > 1 is refused).
// Added:  truss      the k-truss decomposition on the device (gmsx_truss_decomposition; no reference driver) with the usual trial loop: per trial "Trial Time",
//                    "Max Truss", "Levels", "Rounds", "Triangles" and with -v "Verification" (the triangles against gmsx_tc_total), after the last trial the
//                    trussness histogram ("truss k: edges"), then "Average Time".  Single GPU: not sharded (--gpus > 1 is refused).
// Added:  sgi -p pattern-file=FILE [--mono] [--list FILE]   the reference's subgraph-isomorphism drivers (non_set_based/subgraphiso/vf2/sequential/
//                    subgraphiso_vf2_sequential.cpp, its -p pattern-file of util/command_line.hpp:42) on the device (gmsx_subgraph_match): per trial the FIRST
//                    embedding ("isomorphism: t:p ..." — target vertex : pattern vertex, by ascending target vertex, the pairs of Result::isomorphism — or the
//                    reference's "No isomorphisms were found"), with -v "Verification" the way subgraphisomorphismVerification checks it
//                    (util/subgraphiso_verification.hpp:11-78), then the "@@@" line.  Target and pattern are loaded WITHOUT relabelling: the reference's driver
//                    builds both with Builder::MakeGraph and never relabels (subgraphiso_vf2_parallel.cpp:25-32), so its ids are the file's.  --mono: the
//                    non-induced mode; --list writes every embedding (outside the timed trials), one row per line, column p = the image of pattern vertex p.
//                    Not sharded (--gpus > 1 is refused).
// Added:  cc         the reference's connected-components driver (representations/graphs/log_graph/cc.cc:141-149: ShiloachVishkin, PrintCompStats, CCVerifier) on the
//                    device (gmsx_connected_components) with the usual trial loop: per trial "Trial Time", "Components" and with -v "Verification" — this driver's
//                    own BFS per label over the host CSR, the way CCVerifier checks (cc.cc:98-138), which also holds every label to the smallest id of its
//                    component —, then the "@@@" line; after the last trial PrintCompStats' facts (cc.cc:75-91): the five largest components as label:size
//                    and the number of components.  A component is global: not sharded (--gpus > 1 is refused).
// Added:  jp --metric NAME --threshold X   Jarvis–Patrick clustering on the device (gmsx_jarvis_patrick; no reference driver; NAME as for lp): the same
//                    loop and output plus "Kept Edges"; -v runs the BFS over the kept arcs the call returns and checks that they are symmetric.
// Added:  motifs     the 3- / 4-vertex motif census on the device (gmsx_motif_census4; no reference driver) with the usual trial loop: per trial
//                    "Trial Time", the eight motifs as "name: non-induced induced N", "Wedges Walked", "Max Codegree" and with -v "Verification" — the
//                    counting rule of the 4-cycle kernels as this driver's own serial loop over the host CSR, the degree sums, the triangle count and
//                    the induced / non-induced identities —, then the "@@@" line.  Not sharded (--gpus > 1 is refused).
// Added:  bfs [-r SOURCE]   the reference's BFS driver (representations/graphs/log_graph/bfs.cc:261-275: DOBFS from SourcePicker's sources, PrintBFSStats,
//                    BFSVerifier) on the device (gmsx_bfs): trial t starts from the t-th picked source (-r: always SOURCE); per trial "Trial Time", "Source",
//                    "Levels", "Bottom-up Levels" and with -v "Verification" — BFSVerifier's checks (bfs.cc:212-258) as this driver's own serial BFS —,
//                    then the "@@@" line; after the last trial PrintBFSStats' line (bfs.cc:193-204).  Not sharded (--gpus > 1 is refused).
// Added:  bc [-r SOURCE] [-i ITERS]   the reference's betweenness driver (log_graph/bc.cc:235-253: Brandes from ITERS picked sources per trial — the
//                    picker runs on across the trials —, PrintTopScores, BCVerifier) on the device (gmsx_betweenness, normalised): per trial "Trial
//                    Time", "Max Score" and with -v "Verification" — BCVerifier's serial Brandes (bc.cc:172-232) in double, held to the derived bound
//                    2 eps (L (d + 2) + S + 1) of include/gmsx.h's definition plus 2 eps for the normalisation —, then the "@@@" line; after the
//                    last trial PrintTopScores' five id:score lines (bc.cc:156-164; ties: the smaller id).  Not sharded.
// Added:  closeness [-r SOURCE] [-i SOURCES]   closeness centrality of SOURCES picked sources per trial (the picker runs on across the trials, as for
//                    bc) by batched multi-source BFS on the device (gmsx_bfs_multi; no reference driver): per trial "Trial Time", "Max Score" and with
//                    -v "Verification" — this driver's own serial BFS per source must give the same reached, depth_sum and levels —, then the "@@@"
//                    line; after the last trial the top five sources by closeness in PrintTopScores' shape (ties: the earlier source).  Not sharded.
// Added:  pr [-i ITERS] [-t TOL]   the reference's PageRank driver (log_graph/pr.cc:100-114: PageRankPull with at most ITERS sweeps — default 20 — until the
//                    L1 change of a sweep is below TOL — default 1e-4; for this subcommand -t is the tolerance, as in the reference's CLPageRank —,
//                    PrintTopScores, PRVerifier) on the device (gmsx_pagerank, damping 0.85, in double): per trial "Trial Time", "Iterations", "Error"
//                    and with -v "Verification" — PRVerifier's rule, residual < TOL, with the residual from gmsx_pagerank_residual and, beside it,
//                    from this driver's own serial push sweep over the host CSR (pr.cc:79-97), which must agree —, then the "@@@" line; after the
//                    last trial PrintTopScores' five id:score lines (pr.cc:64-74; ties: the smaller id).  Not sharded.
// Added:  sssp [-r SOURCE] [-d DELTA]   the reference's shortest-path driver (log_graph/sssp.cc:178-199: DeltaStep from SourcePicker's sources,
//                    PrintSSSPStats, SSSPVerifier) on the device (gmsx_sssp): a -g graph gets the generator's weights (InsertWeights), a -f file
//                    .wel / .gr / .wsg keeps its own and an .el gets the generator's; the graph is not relabelled (sssp.cc does not).  Per trial
//                    "Trial Time", "Source", "Delta", "Buckets" and with -v "Verification" (gmsx_sssp_verify's verdict), then the "@@@" line; after
//                    the last trial PrintSSSPStats' line.  -d 0 (the default) = the library's choice.  Not sharded (--gpus > 1 is refused).
// Added:  msf [--max]   the minimum (--max: maximum) spanning forest over the weights on the device (gmsx_min_spanning_forest; no reference driver):
//                    the graph is generated or loaded with its weights as for sssp.  Per trial "Trial Time", "Trees", "Edges", "Total Weight",
//                    "Rounds" and with -v "Verification" — this driver's own serial Kruskal under the order of gmsx.h (weight, then the smaller
//                    (min id, max id)) must give the same edge list and total weight —, then the "@@@" line.  Not sharded (--gpus > 1 is refused).
// Added:  communities [-i MAX_SWEEPS] [--weighted]   communities by label propagation on the device (gmsx_label_propagation under the default colouring,
//                    then gmsx_modularity of the result; no reference driver — `lp` is the link-prediction driver): --weighted generates or loads
//                    the graph with its weights as for sssp and sums them.  Per trial "Trial Time", "Communities", "Sweeps", "Modularity" and with
//                    -v "Verification" — this driver's own sequential propagation over the host CSR, the vertices ascending by (colour, id), must
//                    give the same label for every vertex —, then the "@@@" line.  Not sharded (--gpus > 1 is refused).
// Added:  matching [--weighted]   the greedy matching on the device (gmsx_greedy_matching; no reference driver): unit weights, or with --weighted the
//                    weights, heavier first; the graph is generated or loaded with its weights as for sssp either way (never relabelled).  Per trial "Trial Time", "Pairs", "Total Weight",
//                    "Free", "Rounds" and with -v "Verification" — this driver's own sequential greedy over the edges sorted by the order of gmsx.h
//                    must give the same mate for every vertex, and gmsx_matching_verify must certify it —, then the "@@@" line.  Not sharded
//                    (--gpus > 1 is refused).
// Usage:  gmsx_driver <tc|vertex|kclique|kcstar|bk|lp|color|truss|sgi|cc|jp|motifs|bfs|bc|closeness|pr|sssp|msf|communities|matching> [reference flags] [--gpus N]     e.g.  gmsx_driver tc -g kronecker 20 --deg 16 -n 3 -v
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <csignal>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "gmsx_set_graph.hpp"

namespace {

struct Args {  // gms/common/cli/args.h:17-107 defaults
    std::string kernel;
    bool verify = false;
    int64_t trials = 3, threads = 0;
    std::string file, gen;
    int scale = -1, deg = 16;
    int clique_size = 4;
    int gpus = 0;  // 0 = single process without a communicator
    std::string list;  // bk --list FILE: the maximal cliques of the last trial, one per line (gmsx_bk_list)
    std::string metric = "jaccard";  // lp --metric
    int64_t q = 0;     // lp -q N (0: m / 4)
    std::string order; // bk --order adg|deg|dgr: the preprocessing step in front of the search (default adg); color --order id|ff|lf|sl|adg (default id)
    double eps = 0.001; // color --eps: epsilon of --order adg
    std::string pattern_file;  // sgi -p pattern-file=FILE
    bool mono = false;         // sgi --mono
    double threshold = std::nan("");  // jp --threshold X
    bool metric_given = false;
    int64_t start = -1;  // bfs, bc -r SOURCE (gapbs/command_line.h: start_vertex)
    int64_t iters = 1;   // bc -i ITERS
    bool iters_given = false;
    double tol = 1e-4;   // pr -t TOL
    int64_t delta = 0;   // sssp -d DELTA (0: the library's choice)
    bool maximum = false;  // msf --max
    bool weighted = false; // communities --weighted, matching --weighted
    int error = 0;
};

struct Timer {  // gapbs/timer.h:18-47
    std::chrono::high_resolution_clock::time_point t0, t1;
    void Start() { t0 = std::chrono::high_resolution_clock::now(); }
    void Stop() { t1 = std::chrono::high_resolution_clock::now(); }
    double Seconds() const { return std::chrono::duration<double>(t1 - t0).count(); }
};
void PrintTime(const std::string &s, double sec) { std::printf("%-21s%3.5lf\n", (s + ":").c_str(), sec); }          // gapbs/util.h:31-33
void PrintLabel(const std::string &l, const std::string &v) { std::printf("%-21s%7s\n", (l + ":").c_str(), v.c_str()); }  // util.h:27-29

int lp_metric(const std::string &name) {
    static const char *names[] = {"jaccard", "overlap", "adamic_adar", "resource", "common", "total", "prefatt"};  // the GMSX_SIM_* order
    for (int i = 0; i < 7; ++i)
        if (name == names[i]) return i;
    return -1;
}

Args parse(int argc, char **argv) {
    Args a;
    if (argc < 2) { a.error = 101; return a; }
    a.kernel = argv[1];
    for (int i = 2; i < argc; ++i) {
        const std::string f = argv[i];
        auto need = [&](int k) { if (i + k >= argc) { a.error = 100; return false; } return true; };
        if (f == "-v" || f == "--verify") a.verify = true;
        else if (f == "-n" || f == "--num-trials") { if (!need(1)) break; a.trials = std::atoll(argv[++i]); }
        else if (f == "-t" && a.kernel == "pr") { if (!need(1)) break; a.tol = std::atof(argv[++i]); if (!(a.tol >= 0.0)) a.error = 100; }
        else if (f == "-t" || f == "--threads") { if (!need(1)) break; a.threads = std::atoll(argv[++i]); }
        else if (f == "-f" || f == "--file") { if (!need(1)) break; a.file = argv[++i]; }
        else if (f == "-g" || f == "--gen") { if (!need(2)) break; a.gen = argv[++i]; a.scale = std::atoi(argv[++i]); }
        else if (f == "--deg") { if (!need(1)) break; a.deg = std::atoi(argv[++i]); }
        else if (f == "--list") { if (!need(1)) break; a.list = argv[++i]; }
        else if (f == "--metric") { if (!need(1)) break; a.metric = argv[++i]; a.metric_given = true; }
        else if (f == "-r") { if (!need(1)) break; a.start = std::atoll(argv[++i]); if (a.start < 0 || a.start > INT32_MAX) a.error = 100; }
        else if (f == "-d" && a.kernel == "sssp") { if (!need(1)) break; a.delta = std::atoll(argv[++i]); if (a.delta < 0) a.error = 100; }
        else if (f == "-i") { if (!need(1)) break; a.iters = std::atoll(argv[++i]); a.iters_given = true; if (a.iters < 1) a.error = 100; }
        else if (f == "-q") { if (!need(1)) break; a.q = std::atoll(argv[++i]); if (a.q < 1) a.error = 100; }
        else if (f == "--order") { if (!need(1)) break; a.order = argv[++i]; }
        else if (f == "--mono") a.mono = true;
        else if (f == "--max") a.maximum = true;
        else if (f == "--weighted") a.weighted = true;
        else if (f == "--threshold") { if (!need(1)) break; a.threshold = std::atof(argv[++i]); }
        else if (f == "--eps") { if (!need(1)) break; a.eps = std::atof(argv[++i]); }
        else if (f == "--gpus") { if (!need(1)) break; a.gpus = std::atoi(argv[++i]); if (a.gpus < 1 || a.gpus > 64) a.error = 100; }
        else if (f == "--opt") {  // --opt NAME=VALUE -> gmsx_set_option (limits, kernel variants, diagnostics: include/gmsx.h); unknown names are refused
            if (!need(1)) break;
            const std::string kv = argv[++i];
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || gmsx_set_option(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str()) != GMSX_OK) {
                std::fprintf(stderr, "gmsx_driver: --opt %s: not an option of this library (names: include/gmsx.h)\n", kv.c_str());
                a.error = 100;
            }
        } else if (f == "-p" || f == "--param") {
            if (!need(1)) break;
            const std::string kv = argv[++i];
            if (kv.rfind("clique-size=", 0) == 0) a.clique_size = std::atoi(kv.c_str() + 12);
            else if (kv.rfind("cs=", 0) == 0) a.clique_size = std::atoi(kv.c_str() + 3);
            else if (kv.rfind("pattern-file=", 0) == 0) a.pattern_file = kv.substr(13);
            else a.error = 100;
        } else a.error = 100;
    }
    if (!a.error && a.file.empty() && a.gen.empty()) a.error = 101;  // cli/cli.h:131-133
    if (!a.error && !a.gen.empty() && a.gen != "kronecker" && a.gen != "uniform") a.error = 100;
    if (!a.error && !a.list.empty() && ((a.kernel != "bk" && a.kernel != "kcstar" && a.kernel != "lp" && a.kernel != "sgi") || a.gpus > 1)) a.error = 100;  // one process writes the whole list
    if (!a.error && (a.kernel == "kcstar" || a.kernel == "lp" || a.kernel == "truss" || a.kernel == "sgi" || a.kernel == "cc" || a.kernel == "jp" || a.kernel == "motifs" || a.kernel == "pr") && a.gpus > 1) a.error = 100;
    if (!a.error && ((a.kernel == "jp") != !std::isnan(a.threshold))) a.error = 100;  // the threshold is required, and only there
    const bool traversal = a.kernel == "bfs" || a.kernel == "bc" || a.kernel == "closeness" || a.kernel == "sssp";
    if (!a.error && traversal && (a.gpus > 1 || a.metric_given)) a.error = 100;  // a traversal is global; it has no metric
    if (!a.error && a.kernel == "pr" && a.metric_given) a.error = 100;              // … nor has PageRank
    if (!a.error && ((a.kernel == "msf" && (a.gpus > 1 || a.metric_given)) || (a.maximum && a.kernel != "msf"))) a.error = 100;  // a forest is global
    if (!a.error && ((a.kernel == "communities" && (a.gpus > 1 || a.metric_given)) || (a.weighted && a.kernel != "communities" && a.kernel != "matching"))) a.error = 100;  // communities are global
    if (!a.error && a.kernel == "matching" && (a.gpus > 1 || a.metric_given)) a.error = 100;  // … and so is a matching
    if (!a.error && a.kernel == "bicc" && (a.gpus > 1 || a.metric_given)) a.error = 100;  // … and so are the blocks
    if (!a.error && a.kernel == "communities" && a.iters > INT32_MAX) a.error = 100;
    if (!a.error && ((a.start >= 0 && !traversal) || (a.iters != 1 && a.kernel != "bc" && a.kernel != "closeness" && a.kernel != "pr" && a.kernel != "communities"))) a.error = 100;
    if (!a.error && ((a.kernel == "sgi") != !a.pattern_file.empty() || (a.mono && a.kernel != "sgi"))) a.error = 100;  // util/command_line.hpp:22: the pattern is required
    if (!a.error && (a.kernel == "lp" || a.kernel == "jp") && lp_metric(a.metric) < 0) a.error = 100;
    if (!a.error && !a.order.empty() && a.kernel != "bk" && a.kernel != "color") a.error = 100;  // only Bron–Kerbosch and the colouring have a preprocessing step
    if (!a.error && !a.order.empty() && a.kernel == "bk" && a.order != "adg" && a.order != "deg" && a.order != "dgr") a.error = 100;
    if (!a.error && a.kernel == "color") {
        const std::string &o = a.order;
        if ((!o.empty() && o != "id" && o != "ff" && o != "lf" && o != "sl" && o != "adg") || a.gpus > 1) a.error = 100;
    }
    return a;
}

void usage(const char *argv0) {
    std::printf("usage: %s <tc|vertex|kclique|kcstar|bk|lp|color|truss|sgi|cc|jp|motifs|bfs|bc|closeness|pr|sssp|msf|communities|matching|bicc> (-g kronecker|uniform <scale> [--deg d] | -f file.{el,sg}) [-v] [-n trials] [-t threads] "
                "[-p clique-size=k] [--gpus N] [--opt NAME=VALUE ...] [bk, kcstar: --list FILE] [bk: --order adg|deg|dgr] "
                "[lp: --metric jaccard|overlap|adamic_adar|resource|common|total|prefatt -q N --list FILE] [color: --order id|ff|lf|sl|adg --eps e] [sgi: -p pattern-file=FILE --mono --list FILE] "
                "[jp: --metric NAME --threshold X] [bfs, bc, closeness, sssp: -r SOURCE] [bc: -i ITERS] [closeness: -i SOURCES] [pr: -i ITERS -t TOL] [sssp: -d DELTA] [msf: --max] [communities: -i MAX_SWEEPS --weighted] [matching: --weighted]\n", argv0);
}

// ---- host-side verifiers: this driver's own plain loops over the host CSR (independent of the device kernels) ----------
struct HostGraph {
    int64_t n;
    const int64_t *off;
    const int32_t *adj;
    int64_t deg(int32_t v) const { return off[v + 1] - off[v]; }
    const int32_t *row(int32_t v) const { return adj + off[v]; }
};
size_t merge_count(const int32_t *a, size_t na, const int32_t *b, size_t nb) {
    size_t i = 0, j = 0, c = 0;
    while (i < na && j < nb) {
        if (a[i] < b[j]) ++i;
        else if (b[j] < a[i]) ++j;
        else { ++c; ++i; ++j; }
    }
    return c;
}
// Verify::compute_total_count + Verify::vertex_count (triangle_count/verifier.h:13-31,44-85): every directed pair (u,v), full
// rows; per_vertex[u] = Σ_v |N(u)∩N(v)| (= 2·triangles at u), total = Σ / 6
uint64_t host_triangles(const HostGraph &g, std::vector<int64_t> *per_vertex) {
    if (per_vertex) per_vertex->assign(size_t(g.n), 0);
    uint64_t total = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : total)
    for (int64_t u = 0; u < g.n; ++u) {
        uint64_t c = 0;
        for (int64_t j = g.off[u]; j < g.off[u + 1]; ++j) {
            const int32_t v = g.adj[j];
            c += merge_count(g.row(int32_t(u)), size_t(g.deg(int32_t(u))), g.row(v), size_t(g.deg(v)));
        }
        if (per_vertex) (*per_vertex)[size_t(u)] = int64_t(c);
        total += c;
    }
    return total / 6;
}
// CliqueCount (k_clique_count_set_based.h:5-31) recounted on a degree-oriented DAG: the recursion of :5-17 over
// N+(v) = { w in N(v) : (deg w, w) > (deg v, v) } meets every k-clique once, so the reference's value is k! times the sum
struct Dag {
    std::vector<int64_t> off;
    std::vector<int32_t> adj;
    const int32_t *row(int32_t v) const { return adj.data() + off[size_t(v)]; }
    size_t deg(int32_t v) const { return size_t(off[size_t(v) + 1] - off[size_t(v)]); }
};
uint64_t host_kclique_step(const Dag &d, size_t k, const std::vector<int32_t> &isect) {
    if (k == 1) return isect.size();
    uint64_t cur = 0;
    std::vector<int32_t> next;
    for (int32_t v : isect) {
        next.clear();
        std::set_intersection(isect.begin(), isect.end(), d.row(v), d.row(v) + d.deg(v), std::back_inserter(next));
        if (next.size() + 1 >= k - 1) cur += host_kclique_step(d, k - 1, next);
    }
    return cur;
}
uint64_t host_kclique(const HostGraph &g, size_t k) {
    Dag d;
    d.off.assign(size_t(g.n) + 1, 0);
    auto above = [&](int32_t w, int32_t v) { return g.deg(w) != g.deg(v) ? g.deg(w) > g.deg(v) : w > v; };
    for (int64_t v = 0; v < g.n; ++v) {
        int64_t c = 0;
        for (int64_t j = g.off[v]; j < g.off[v + 1]; ++j) c += above(g.adj[j], int32_t(v));
        d.off[size_t(v) + 1] = d.off[size_t(v)] + c;
    }
    d.adj.resize(size_t(d.off[size_t(g.n)]));
    for (int64_t v = 0; v < g.n; ++v) {
        int64_t p = d.off[size_t(v)];
        for (int64_t j = g.off[v]; j < g.off[v + 1]; ++j)
            if (above(g.adj[j], int32_t(v))) d.adj[size_t(p++)] = g.adj[j];  // stays ascending
    }
    uint64_t total = 0;
    if (k == 1) total = uint64_t(g.n);
    else {
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : total)
        for (int64_t u = 0; u < g.n; ++u) {
            const std::vector<int32_t> nu(d.row(int32_t(u)), d.row(int32_t(u)) + d.deg(int32_t(u)));
            total += host_kclique_step(d, k - 1, nu);
        }
    }
    for (size_t i = 2; i <= k; ++i) total *= uint64_t(i);  // mod 2^64 like size_t
    return total;
}
// BkTomita::expand with findPivot (sequential/tomita.h:12-86) under the Eppstein outer loop (eppsteinPAR.h:31-48), count only
void host_bk_expand(const HostGraph &g, std::vector<int32_t> cand, std::vector<int32_t> fini, uint64_t &count) {
    if (cand.empty()) {
        if (fini.empty()) ++count;
        return;
    }
    int32_t pivot = -1;
    size_t best = 0;
    bool first = true;
    for (const std::vector<int32_t> *s : {&cand, &fini})
        for (int32_t x : *s) {
            const size_t c = merge_count(cand.data(), cand.size(), g.row(x), size_t(g.deg(x)));
            if (first || c > best) { best = c; pivot = x; first = false; }
        }
    std::vector<int32_t> ext;
    std::set_difference(cand.begin(), cand.end(), g.row(pivot), g.row(pivot) + g.deg(pivot), std::back_inserter(ext));
    for (int32_t q : ext) {
        std::vector<int32_t> c2, f2;
        std::set_intersection(cand.begin(), cand.end(), g.row(q), g.row(q) + g.deg(q), std::back_inserter(c2));
        std::set_intersection(fini.begin(), fini.end(), g.row(q), g.row(q) + g.deg(q), std::back_inserter(f2));
        host_bk_expand(g, std::move(c2), std::move(f2), count);
        cand.erase(std::lower_bound(cand.begin(), cand.end(), q));
        fini.insert(std::lower_bound(fini.begin(), fini.end(), q), q);
    }
}
uint64_t host_bk(const HostGraph &g, const std::vector<int32_t> &rank) {
    uint64_t total = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : total)
    for (int64_t v = 0; v < g.n; ++v) {
        std::vector<int32_t> cand, fini;
        for (int64_t j = g.off[v]; j < g.off[v + 1]; ++j) (rank[size_t(g.adj[j])] > rank[size_t(v)] ? cand : fini).push_back(g.adj[j]);
        uint64_t c = 0;
        host_bk_expand(g, std::move(cand), std::move(fini), c);
        total += c;
    }
    return total;
}
// sizes up to which `-v` recounts on the host (seconds on a few cores); larger graphs get a re-decomposed device run
constexpr uint64_t kHostTcElements = 20000000000ull;  // Σ(d_u+d_v) merged ids
constexpr int64_t kHostKcEdges = 1000000, kHostBkEdges = 60000;

// `--gpus N`: one process per GPU.  The launcher forks N children BEFORE it touches HIP and stays behind as their supervisor; a child
// simply returns from here (-1) and continues into main's body as rank r — no exec, no second start-up.  The supervisor reaps with
// waitpid(-1): the first child that fails (non-zero exit or a signal — e.g. gmsx_init(rank) with fewer devices than ranks, a load error)
// takes the others down (SIGTERM, SIGKILL after a grace period): ranks blocked in ncclCommInitRank / ncclAllReduce have no timeout of
// their own and would otherwise wait for the dead one forever.  A failed rank is never restarted.
// Under a profiler preload (rocprofv3 …) the tool library has initialised the GPU in THIS process already, and a forked child of a
// process with a live HIP runtime cannot use the GPU: refused with a message.  Profile one rank at a time instead, no launcher hop:
//   GMSX_DRIVER_RANK=r GMSX_DRIVER_NRANKS=N GMSX_DRIVER_ID_FILE=/tmp/id rocprofv3 … -- gmsx_driver <args without --gpus>
// (Only what actually puts a tool library into THIS process counts: an LD_PRELOAD entry, or the tool list rocprofv3 exports for the
// rocprofiler-register hook — a user's own ROCPROF_* / ROCP_* configuration variables alone do not.)
bool profiler_preloaded() {
    const char *pre = std::getenv("LD_PRELOAD");
    if (pre && (std::strstr(pre, "rocprof") || std::strstr(pre, "roctracer") || std::strstr(pre, "rocprofiler"))) return true;
    const char *tools = std::getenv("ROCP_TOOL_LIBRARIES");
    return tools && *tools;
}
// the supervisor's SIGTERM / SIGINT (a `timeout`, a scheduler cancel, Ctrl-C): taken note of here, acted on in the reaping loop
volatile std::sig_atomic_t g_stop_signal = 0;
extern "C" void on_stop_signal(int sig) { g_stop_signal = sig; }

int launch_ranks(int gpus) {
    if (profiler_preloaded()) {
        std::fprintf(stderr, "gmsx_driver --gpus: a profiler library is preloaded (it has initialised the GPU in this process); ranks cannot be\n"
                             "forked from it.  Start the ranks directly under the profiler with GMSX_DRIVER_RANK / GMSX_DRIVER_NRANKS /\n"
                             "GMSX_DRIVER_ID_FILE set and without --gpus.\n");
        return 6;
    }
    char idfile[] = "/tmp/gmsx_driver_id_XXXXXX";
    const int fd = mkstemp(idfile);
    if (fd < 0) { std::perror("mkstemp"); return 4; }
    close(fd);
    unlink(idfile);  // rank 0 re-creates it atomically once the id is written
    std::fflush(stdout);
    std::fflush(stderr);
    std::vector<pid_t> kids;
    auto kill_rest = [&](int sig) {
        for (pid_t k : kids)
            if (k > 0) kill(k, sig);
    };
    for (int r = 0; r < gpus; ++r) {
        const pid_t pid = fork();
        if (pid < 0) {
            std::perror("fork");
            kill_rest(SIGKILL);
            while (waitpid(-1, nullptr, 0) > 0) {}
            return 4;
        }
        if (pid == 0) {  // rank r: carry on in main()
            prctl(PR_SET_PDEATHSIG, SIGTERM);  // … and never outlive the supervisor (SIGKILLed, say): a rank blocked in RCCL holds its GPU for good
            if (getppid() == 1) _exit(4);      // (it died between fork and prctl)
            setenv("GMSX_DRIVER_RANK", std::to_string(r).c_str(), 1);
            setenv("GMSX_DRIVER_NRANKS", std::to_string(gpus).c_str(), 1);
            setenv("GMSX_DRIVER_ID_FILE", idfile, 1);
            // one node by construction: keep RCCL's bootstrap off the (possibly absent) external network unless the user chose otherwise
            setenv("NCCL_SOCKET_IFNAME", "lo", 0);
            setenv("NCCL_IB_DISABLE", "1", 0);
            if (std::getenv("GMSX_DRIVER_TEST_HANG")) pause();  // test hook: a rank that never finishes (as one blocked in a collective would)
            return -1;
        }
        kids.push_back(pid);
    }
    // a stop signal to the supervisor goes on to the ranks (no SA_RESTART: the blocking waitpid returns EINTR and the loop sees the flag)
    struct sigaction sa {};
    sa.sa_handler = on_stop_signal;
    sigemptyset(&sa.sa_mask);
    sigaction(SIGTERM, &sa, nullptr);
    sigaction(SIGINT, &sa, nullptr);
    int worst = 0, alive = gpus;
    bool killing = false;
    auto t_kill = std::chrono::steady_clock::now();
    while (alive > 0) {
        if (g_stop_signal && !killing) {
            std::fprintf(stderr, "gmsx_driver --gpus: signal %d; stopping the %d rank(s)\n", int(g_stop_signal), alive);
            worst = 128 + int(g_stop_signal);
            killing = true;
            t_kill = std::chrono::steady_clock::now();
            kill_rest(SIGTERM);
        }
        int st = 0;
        const pid_t k = waitpid(-1, &st, killing ? WNOHANG : 0);
        if (k < 0) {
            if (errno == EINTR) continue;  // a stop signal arrived while waiting
            break;                         // no children left
        }
        if (k == 0) {      // tearing down: give SIGTERM two seconds, then SIGKILL
            if (std::chrono::steady_clock::now() - t_kill > std::chrono::seconds(2)) kill_rest(SIGKILL);
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
            continue;
        }
        for (pid_t &x : kids)
            if (x == k) x = -1;
        --alive;
        const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
        if (code != 0 && !killing) {
            worst = code;
            std::fprintf(stderr, "gmsx_driver --gpus: a rank ended with status %d; stopping the other %d\n", code, alive);
            killing = true;
            t_kill = std::chrono::steady_clock::now();
            kill_rest(SIGTERM);
        }
    }
    unlink(idfile);
    unlink((std::string(idfile) + ".tmp").c_str());
    return worst;
}

// benchmarkGraphColoringWithReordering (coloring.cc:82-129) around gmsx::coloring: its labels, its three averages
int run_color(const Args &args, const gmsx::HipSetGraph &g) {
    const std::string heuristic = args.order.empty() ? "id" : args.order;
    double total_seconds = 0, pp_total_seconds = 0;
    int64_t total_colors = 0;
    Timer t;
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        std::vector<int32_t> order;
        const bool has_order = gmsx::coloring_order(g, heuristic.c_str(), args.eps, order);
        t.Stop();
        PrintTime("Preprocess Time", t.Seconds());
        pp_total_seconds += t.Seconds();
        t.Start();
        gmsx_coloring_info info{};
        const std::vector<int32_t> coloring = has_order ? gmsx::coloring(g, order, true, &info) : gmsx::coloring(g, heuristic.c_str(), args.eps, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        const gmsx_coloring_check chk = gmsx::coloring_check(g, coloring);
        const int n_col = int(chk.distinct);  // uniqueColorsCount (coloring_common.h:205-209)
        total_colors += n_col;
        PrintLabel("Colors", std::to_string(n_col));
        if (args.verify) {  // GCVerifierMaxColor(g, coloring, nCol) (coloring_common.h:102-122)
            const bool ok = chk.invalid == 0 && chk.conflicts == 0 && chk.max_color <= n_col && info.colors == n_col;
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ coloring jones_v3 pp:" << heuristic << std::endl;
    }
    const double trials = double(args.trials > 0 ? args.trials : 1);
    PrintTime("Average Time", total_seconds / trials);
    PrintTime("Average pp Time", pp_total_seconds / trials);
    PrintTime("Average colors", double(total_colors) / trials);
    return 0;
}

// the k-truss decomposition (gmsx::truss_numbers) under the usual trial loop
int run_truss(const Args &args, const gmsx::HipSetGraph &g) {
    double total_seconds = 0;
    Timer t;
    std::vector<int32_t> truss;
    gmsx_truss_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        gmsx::truss_numbers(g, truss, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Max Truss", std::to_string(info.max_truss));
        PrintLabel("Levels", std::to_string(info.levels));
        PrintLabel("Rounds", std::to_string(info.rounds));
        PrintLabel("Triangles", std::to_string(info.triangles));
        if (args.verify) PrintLabel("Verification", uint64_t(info.triangles) == uint64_t(gmsx::count_total(g)) ? "PASS" : "FAIL");
        std::cout << "@@@ truss decomposition" << std::endl;
    }
    std::vector<int64_t> hist(size_t(info.max_truss) + 1, 0);
    for (int64_t u = 0; u < g.num_nodes() && !truss.empty(); ++u)  // (-n 0: no trial has filled truss)
        for (int64_t j = g.offsets()[u]; j < g.offsets()[u + 1]; ++j)
            if (u < g.neighbors()[j]) ++hist[size_t(truss[size_t(j)])];
    for (size_t k = 0; k < hist.size(); ++k)
        if (hist[k]) std::printf("truss %zu: %lld\n", k, (long long)hist[k]);
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// CCVerifier's check (cc.cc:98-138) as this driver's own loop: a BFS over the kept arcs (keep == nullptr: all) from the first unvisited vertex,
// which must carry its own id as label; everything it reaches must carry that label too.  Holds the labels to the smallest id of every component.
bool verify_components(const HostGraph &hg, const std::vector<int32_t> &comp, const uint8_t *keep) {
    if (int64_t(comp.size()) != hg.n) return false;
    std::vector<char> visited(size_t(hg.n), 0);
    std::vector<int32_t> frontier;
    frontier.reserve(size_t(hg.n));
    if (keep)  // an edge is kept if either arc is: the output of gmsx_jarvis_patrick marks both
        for (int64_t u = 0; u < hg.n; ++u)
            for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
                const int32_t v = hg.adj[j];
                const int32_t *b = hg.adj + hg.off[v], *e = hg.adj + hg.off[v + 1], *p = std::lower_bound(b, e, int32_t(u));
                if (p == e || *p != u || (keep[j] != 0) != (keep[p - hg.adj] != 0)) return false;
            }
    for (int64_t s = 0; s < hg.n; ++s) {
        if (visited[size_t(s)]) continue;
        if (comp[size_t(s)] != s) return false;
        frontier.clear();
        frontier.push_back(int32_t(s));
        visited[size_t(s)] = 1;
        for (size_t at = 0; at < frontier.size(); ++at) {
            const int32_t u = frontier[at];
            for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
                if (keep && !keep[j]) continue;
                const int32_t v = hg.adj[j];
                if (comp[size_t(v)] != s) return false;
                if (!visited[size_t(v)]) {
                    visited[size_t(v)] = 1;
                    frontier.push_back(v);
                }
            }
        }
    }
    return true;
}

// The counting rule of gmsx_cycle4_count as a serial loop (no reference counterpart): ranks by decreasing (degree, id); for every source u with at
// least two later neighbours, every wedge u - v - w with rank(v) > rank(u) < rank(w) adds to cnt[w]; the cycles of u are Σ_w C(cnt[w], 2); a
// second walk returns the counters to zero.  Returns the cycles and the wedges walked.
void host_cycle4(const HostGraph &hg, uint64_t *cycles, uint64_t *wedges) {
    std::vector<int32_t> order(size_t(hg.n)), rank(size_t(hg.n));
    for (int64_t v = 0; v < hg.n; ++v) order[size_t(v)] = int32_t(v);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const int64_t da = hg.off[a + 1] - hg.off[a], db = hg.off[b + 1] - hg.off[b];
        return da != db ? da > db : a > b;
    });
    for (int64_t i = 0; i < hg.n; ++i) rank[size_t(order[size_t(i)])] = int32_t(i);
    std::vector<uint32_t> cnt(size_t(hg.n), 0);
    uint64_t c = 0, w_all = 0;
    for (int64_t u = 0; u < hg.n; ++u) {
        const int32_t ru = rank[size_t(u)];
        int64_t later = 0;
        for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) later += rank[size_t(hg.adj[j])] > ru;
        if (later < 2) continue;
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
                const int32_t v = hg.adj[j];
                if (rank[size_t(v)] <= ru) continue;
                for (int64_t k = hg.off[v]; k < hg.off[v + 1]; ++k) {
                    const int32_t w = hg.adj[k];
                    if (rank[size_t(w)] <= ru) continue;
                    if (pass == 0) {
                        ++cnt[size_t(w)];
                        ++w_all;
                    } else {
                        const uint64_t x = cnt[size_t(w)];
                        c += x * (x - 1) / 2;
                        cnt[size_t(w)] = 0;
                    }
                }
            }
    }
    *cycles = c;
    *wedges = w_all;
}

// the motif census (gmsx::motif_census4) under the usual trial loop: the sixteen counts, one "@@@" line per trial
int run_motifs(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg) {
    static const char *const names[GMSX_MOTIF_KINDS] = {"wedge", "triangle", "star3", "path4", "paw", "cycle4", "diamond", "clique4"};
    double total_seconds = 0;
    Timer t;
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        const gmsx_motif_info info = gmsx::motif_census4(g);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        for (int k = 0; k < GMSX_MOTIF_KINDS; ++k) PrintLabel(names[k], std::to_string(info.subgraphs[k]) + " induced " + std::to_string(info.induced[k]));
        PrintLabel("Wedges Walked", std::to_string(info.wedges_walked));
        PrintLabel("Max Codegree", std::to_string(info.max_codegree));
        if (args.verify) {
            uint64_t cycles = 0, wedges = 0;
            host_cycle4(hg, &cycles, &wedges);
            unsigned __int128 w2 = 0, w3 = 0;
            for (int64_t v = 0; v < hg.n; ++v) {
                const unsigned __int128 d = (unsigned __int128)(hg.off[v + 1] - hg.off[v]);
                if (d >= 2) w2 += d * (d - 1) / 2;
                if (d >= 3) w3 += d * (d - 1) * (d - 2) / 6;
            }
            const uint64_t *s = info.subgraphs, *i = info.induced;
            bool ok = cycles == s[GMSX_MOTIF_CYCLE4] && wedges == info.wedges_walked && w2 == s[GMSX_MOTIF_WEDGE] && w3 == s[GMSX_MOTIF_STAR3];
            ok = ok && s[GMSX_MOTIF_TRIANGLE] == uint64_t(gmsx::count_total(g)) && gmsx::cycle4_count(g) == cycles;
            ok = ok && i[GMSX_MOTIF_CLIQUE4] == s[GMSX_MOTIF_CLIQUE4] && i[GMSX_MOTIF_DIAMOND] + 6 * s[GMSX_MOTIF_CLIQUE4] == s[GMSX_MOTIF_DIAMOND];
            ok = ok && i[GMSX_MOTIF_CYCLE4] + i[GMSX_MOTIF_DIAMOND] + 3 * s[GMSX_MOTIF_CLIQUE4] == s[GMSX_MOTIF_CYCLE4];
            ok = ok && i[GMSX_MOTIF_PAW] + 4 * i[GMSX_MOTIF_DIAMOND] + 12 * s[GMSX_MOTIF_CLIQUE4] == s[GMSX_MOTIF_PAW];
            ok = ok && i[GMSX_MOTIF_STAR3] + i[GMSX_MOTIF_PAW] + 2 * i[GMSX_MOTIF_DIAMOND] + 4 * s[GMSX_MOTIF_CLIQUE4] == s[GMSX_MOTIF_STAR3];
            ok = ok && i[GMSX_MOTIF_PATH4] + 2 * i[GMSX_MOTIF_PAW] + 4 * i[GMSX_MOTIF_CYCLE4] + 6 * i[GMSX_MOTIF_DIAMOND] + 12 * s[GMSX_MOTIF_CLIQUE4] == s[GMSX_MOTIF_PATH4];
            ok = ok && i[GMSX_MOTIF_TRIANGLE] == s[GMSX_MOTIF_TRIANGLE] && i[GMSX_MOTIF_WEDGE] + 3 * s[GMSX_MOTIF_TRIANGLE] == s[GMSX_MOTIF_WEDGE];
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ motif census" << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// connected components (cc) and Jarvis–Patrick clustering (jp) under the usual trial loop, with PrintCompStats' facts (cc.cc:75-91) at the end
int run_components(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg) {
    const bool jp = args.kernel == "jp";
    double total_seconds = 0;
    Timer t;
    std::vector<int32_t> comp(size_t(hg.n) + 1);
    std::vector<uint8_t> keep;
    if (jp && args.verify) keep.resize(size_t(hg.off[hg.n]) + 1);
    gmsx_components_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        if (jp)
            gmsx::detail::check(gmsx_jarvis_patrick(g.device(), lp_metric(args.metric), args.threshold, comp.data(), keep.empty() ? nullptr : keep.data(), &info, nullptr),
                                "gmsx_jarvis_patrick");
        else gmsx::detail::check(gmsx_connected_components(g.device(), nullptr, comp.data(), &info, nullptr), "gmsx_connected_components");
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Components", std::to_string(info.components));
        if (jp) PrintLabel("Kept Edges", std::to_string(info.kept_edges));
        if (args.verify) {
            std::vector<int32_t> labels(comp.begin(), comp.begin() + hg.n);
            PrintLabel("Verification", verify_components(hg, labels, keep.empty() ? nullptr : keep.data()) ? "PASS" : "FAIL");
        }
        if (jp) std::cout << "@@@ jarvis-patrick " << args.metric << " " << args.threshold << std::endl;
        else std::cout << "@@@ connected components" << std::endl;
    }
    if (args.trials > 0) {
        std::vector<int64_t> size(size_t(hg.n) + 1, 0);
        for (int64_t v = 0; v < hg.n; ++v) ++size[size_t(comp[size_t(v)])];
        std::vector<std::pair<int64_t, int32_t>> top;  // (-size, label): ascending = largest first, ties by the smaller label
        for (int64_t v = 0; v < hg.n; ++v)
            if (size[size_t(v)]) top.emplace_back(-size[size_t(v)], int32_t(v));
        const size_t k = std::min<size_t>(5, top.size());
        std::partial_sort(top.begin(), top.begin() + k, top.end());
        std::cout << std::endl << k << " biggest clusters" << std::endl;
        for (size_t i = 0; i < k; ++i) std::cout << top[i].second << ":" << -top[i].first << std::endl;
        std::cout << "There are " << top.size() << " components" << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// Hopcroft–Tarjan on the host, iterative (a depth-first search with an edge stack), its blocks renumbered by their smallest `u < v` arc in CSR
// order: block per arc, blocks_at per vertex, arc_keep per arc as include/gmsx.h defines them.  The driver's own loop, independent of the device.
void host_bicc(const HostGraph &hg, std::vector<int32_t> &block, std::vector<int32_t> &blocks_at, std::vector<uint8_t> &keep) {
    const int64_t n = hg.n, nnz = hg.off[n];
    auto arc_of = [&](int32_t u, int32_t v) { return int64_t(std::lower_bound(hg.row(u), hg.row(u) + hg.deg(u), v) - hg.adj); };
    std::vector<int32_t> disc(size_t(n), -1), low(size_t(n), 0), parent(size_t(n), -1);
    std::vector<int64_t> next(size_t(n), 0), raw(size_t(nnz), -1), edges;  // the edge stack holds arc indices
    std::vector<int32_t> stack;
    int32_t clock = 0;
    int64_t nraw = 0;
    for (int32_t root = 0; root < n; ++root) {
        if (disc[size_t(root)] >= 0) continue;
        disc[size_t(root)] = low[size_t(root)] = clock++;
        next[size_t(root)] = hg.off[root];
        stack.assign(1, root);
        while (!stack.empty()) {
            const int32_t v = stack.back();
            if (next[size_t(v)] < hg.off[v + 1]) {
                const int64_t j = next[size_t(v)]++;
                const int32_t w = hg.adj[j];
                if (w == parent[size_t(v)]) continue;
                if (disc[size_t(w)] < 0) {
                    edges.push_back(j);
                    parent[size_t(w)] = v;
                    disc[size_t(w)] = low[size_t(w)] = clock++;
                    next[size_t(w)] = hg.off[w];
                    stack.push_back(w);
                } else if (disc[size_t(w)] < disc[size_t(v)]) {  // a back edge to an ancestor, met from its lower end only
                    edges.push_back(j);
                    low[size_t(v)] = std::min(low[size_t(v)], disc[size_t(w)]);
                }
            } else {
                stack.pop_back();
                const int32_t p = parent[size_t(v)];
                if (p < 0) continue;
                low[size_t(p)] = std::min(low[size_t(p)], low[size_t(v)]);
                if (low[size_t(v)] >= disc[size_t(p)]) {  // p separates v's subtree: the arcs above p -> v on the stack are one block
                    const int64_t tree = arc_of(p, v);
                    for (;;) {
                        const int64_t j = edges.back();
                        edges.pop_back();
                        raw[size_t(j)] = nraw;
                        if (j == tree) break;
                    }
                    ++nraw;
                }
            }
        }
    }
    // the twin of a stacked arc gets its number; then ids by the first `u < v` arc
    std::vector<int32_t> id(size_t(nraw), -1);
    std::vector<int64_t> edges_of(size_t(nraw), 0);
    block.assign(size_t(nnz), -1);
    blocks_at.assign(size_t(n), 0);
    keep.assign(size_t(nnz), 0);
    int32_t ids = 0;
    for (int32_t u = 0; u < n; ++u)
        for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
            if (raw[size_t(j)] < 0) raw[size_t(j)] = raw[size_t(arc_of(hg.adj[j], u))];
            if (hg.adj[j] > u) {
                if (id[size_t(raw[size_t(j)])] < 0) id[size_t(raw[size_t(j)])] = ids++;
                ++edges_of[size_t(raw[size_t(j)])];
            }
        }
    std::vector<int32_t> mine;
    for (int32_t u = 0; u < n; ++u) {
        mine.clear();
        for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
            block[size_t(j)] = id[size_t(raw[size_t(j)])];
            keep[size_t(j)] = edges_of[size_t(raw[size_t(j)])] > 1 ? 1 : 0;
            mine.push_back(block[size_t(j)]);
        }
        std::sort(mine.begin(), mine.end());
        blocks_at[size_t(u)] = int32_t(std::unique(mine.begin(), mine.end()) - mine.begin());
    }
}

// biconnected components (bicc) under the usual trial loop; -v holds every array to host_bicc
int run_bicc(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg) {
    const int64_t nnz = hg.n > 0 ? hg.off[hg.n] : 0;
    double total_seconds = 0;
    Timer t;
    std::vector<int32_t> block(size_t(nnz) + 1), blocks_at(size_t(hg.n) + 1);
    std::vector<uint8_t> keep(size_t(nnz) + 1);
    gmsx_bicc_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        gmsx::detail::check(gmsx_biconnected_components(g.device(), 0, block.data(), blocks_at.data(), keep.data(), &info, nullptr), "gmsx_biconnected_components");
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Blocks", std::to_string(info.blocks));
        PrintLabel("Bridges", std::to_string(info.bridges));
        PrintLabel("Articulation Points", std::to_string(info.articulation_points));
        PrintLabel("Largest Block", std::to_string(info.largest_block_edges) + " edges " + std::to_string(info.largest_block_vertices) + " vertices");
        PrintLabel("Components", std::to_string(info.components));
        PrintLabel("Levels", std::to_string(info.levels));
        if (args.verify) {
            std::vector<int32_t> hb, ha;
            std::vector<uint8_t> hk;
            host_bicc(hg, hb, ha, hk);
            int64_t cut = 0, bridges2 = 0, most = -1;
            for (int64_t v = 0; v < hg.n; ++v) cut += ha[size_t(v)] >= 2;
            for (int64_t j = 0; j < nnz; ++j) {
                bridges2 += hk[size_t(j)] == 0;
                most = std::max<int64_t>(most, hb[size_t(j)]);
            }
            const bool ok = std::equal(hb.begin(), hb.end(), block.begin()) && std::equal(ha.begin(), ha.end(), blocks_at.begin()) &&
                            std::equal(hk.begin(), hk.end(), keep.begin()) && cut == info.articulation_points && bridges2 == 2 * info.bridges &&
                            most + 1 == info.blocks;
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ biconnected components" << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// BFSVerifier (bfs.cc:212-258) as this driver's own loop: a serial BFS from the source; the source is its own parent, every other reached vertex
// has a parent that is a neighbour one level up, and exactly the unreachable vertices have -1.  `depth` is held to the serial depths, too.
bool verify_bfs(const HostGraph &hg, int32_t source, const std::vector<int32_t> &parent, const std::vector<int32_t> &depth_got) {
    std::vector<int32_t> depth(size_t(hg.n), -1), to_visit;
    to_visit.reserve(size_t(hg.n));
    depth[size_t(source)] = 0;
    to_visit.push_back(source);
    for (size_t at = 0; at < to_visit.size(); ++at) {
        const int32_t u = to_visit[at];
        for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j)
            if (depth[size_t(hg.adj[j])] == -1) {
                depth[size_t(hg.adj[j])] = depth[size_t(u)] + 1;
                to_visit.push_back(hg.adj[j]);
            }
    }
    for (int64_t u = 0; u < hg.n; ++u) {
        if (depth_got[size_t(u)] != depth[size_t(u)]) return false;
        const int32_t p = parent[size_t(u)];
        if (depth[size_t(u)] != -1 && p != -1) {
            if (u == source) {
                if (p != u) return false;
                continue;
            }
            if (p < 0 || p >= hg.n || depth[size_t(p)] != depth[size_t(u)] - 1) return false;
            if (!std::binary_search(hg.row(int32_t(u)), hg.row(int32_t(u)) + hg.deg(int32_t(u)), p)) return false;
        } else if (depth[size_t(u)] != p) {
            return false;
        }
    }
    return true;
}

// BCVerifier (bc.cc:172-232) in double: serial Brandes from the same sources, normalised; returns whether `got` (normalised) lies within
// 2 eps (L (d + 2) + S + 1) want + 2 eps want of it — the bound of include/gmsx.h's definition while every path count is exact (below 2^53);
// beyond that 2 eps (L ((d + 2) + 2 L d) + S + 1) want + 2 eps want, and a line says so
bool verify_bc(const HostGraph &hg, const std::vector<int32_t> &sources, const std::vector<double> &got) {
    const size_t n = size_t(hg.n);
    std::vector<double> scores(n, 0.0), sigma(n), delta(n);
    std::vector<int32_t> depth(n), order;
    order.reserve(n);
    int64_t max_levels = 0, max_degree = 0;
    double max_sigma = 0.0;
    for (int64_t v = 0; v < hg.n; ++v) max_degree = std::max(max_degree, hg.deg(int32_t(v)));
    for (const int32_t s : sources) {
        std::fill(depth.begin(), depth.end(), -1);
        std::fill(sigma.begin(), sigma.end(), 0.0);
        std::fill(delta.begin(), delta.end(), 0.0);
        order.clear();
        depth[size_t(s)] = 0;
        sigma[size_t(s)] = 1.0;
        order.push_back(s);
        for (size_t at = 0; at < order.size(); ++at) {
            const int32_t u = order[at];
            for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
                const int32_t v = hg.adj[j];
                if (depth[size_t(v)] == -1) {
                    depth[size_t(v)] = depth[size_t(u)] + 1;
                    order.push_back(v);
                }
                if (depth[size_t(v)] == depth[size_t(u)] + 1) sigma[size_t(v)] += sigma[size_t(u)];
            }
        }
        for (size_t at = order.size(); at-- > 0;) {
            const int32_t u = order[at];
            for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) {
                const int32_t v = hg.adj[j];
                if (depth[size_t(v)] == depth[size_t(u)] + 1) delta[size_t(u)] += sigma[size_t(u)] / sigma[size_t(v)] * (1 + delta[size_t(v)]);
            }
            scores[size_t(u)] += delta[size_t(u)];
            max_sigma = std::max(max_sigma, sigma[size_t(u)]);
        }
        max_levels = std::max<int64_t>(max_levels, depth[size_t(order.back())] + 1);
    }
    const double biggest = n ? *std::max_element(scores.begin(), scores.end()) : 0.0;
    const double eps = 1.1102230246251565e-16, L = double(max_levels), d = double(max_degree), S = double(sources.size());
    // beyond 2^53 the counts themselves carry up to L d eps and enter a term twice: the wider bound of the same derivation, per source
    const bool exact = max_sigma < 9007199254740992.0;
    if (!exact) std::printf("%-21s%s\n", "Path Counts:", "beyond 2^53: held to the bound of inexact counts");
    const double factor = (exact ? 2.0 * eps * (L * (d + 2.0) + S + 1.0) : 2.0 * eps * (L * ((d + 2.0) + 2.0 * L * d) + S + 1.0)) + 2.0 * eps;
    for (size_t v = 0; v < n; ++v) {
        const double want = biggest > 0.0 ? scores[v] / biggest : 0.0;
        if (!(std::fabs(got[v] - want) <= factor * want)) return false;
    }
    return true;
}

// breadth-first search (bfs) and betweenness centrality (bc) under the usual trial loop, with PrintBFSStats' / PrintTopScores' lines at the end
int run_traversal(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg, const gmsx_csr *csr) {
    const bool bc = args.kernel == "bc";
    if (args.start >= hg.n) { std::printf("-r %lld: the graph has %lld vertices\n", (long long)args.start, (long long)hg.n); return 100; }
    const int64_t per_trial = bc ? args.iters : 1;
    std::vector<int32_t> picks(size_t(per_trial * std::max<int64_t>(args.trials, 0)) + 1);
    if (int rc = gmsx_csr_pick_sources(csr, int64_t(picks.size()) - 1, int32_t(args.start), picks.data())) {
        std::printf("no source to pick: %s\n", gmsx_strerror(rc));
        return 2;
    }
    double total_seconds = 0;
    Timer t;
    std::vector<int32_t> parent, depth;
    std::vector<double> scores;
    gmsx_bfs_info info{};
    gmsx_bc_info bi{};
    for (int64_t it = 0; it < args.trials; ++it) {
        const std::vector<int32_t> sources(picks.begin() + it * per_trial, picks.begin() + (it + 1) * per_trial);
        t.Start();
        if (bc) gmsx::betweenness(g, sources, scores, GMSX_BC_NORMALIZE_MAX, &bi);
        else gmsx::bfs(g, sources[0], parent, &depth, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        if (bc) {
            std::printf("%-21s%g\n", "Max Score:", bi.max_score);
            if (args.verify) PrintLabel("Verification", verify_bc(hg, sources, scores) ? "PASS" : "FAIL");
            std::cout << "@@@ betweenness" << std::endl;
        } else {
            PrintLabel("Source", std::to_string(sources[0]));
            PrintLabel("Levels", std::to_string(info.levels));
            PrintLabel("Bottom-up Levels", std::to_string(info.bottom_up_levels));
            if (args.verify) PrintLabel("Verification", verify_bfs(hg, sources[0], parent, depth) ? "PASS" : "FAIL");
            std::cout << "@@@ bfs" << std::endl;
        }
    }
    if (args.trials > 0 && !bc) std::cout << "BFS Tree has " << info.reached << " nodes and " << info.reached_arcs << " edges" << std::endl;
    if (args.trials > 0 && bc) {
        std::vector<std::pair<double, int32_t>> top;  // (-score, id): ascending = largest first, ties by the smaller id
        for (int64_t v = 0; v < hg.n; ++v) top.emplace_back(-scores[size_t(v)], int32_t(v));
        const size_t k = std::min<size_t>(5, top.size());
        std::partial_sort(top.begin(), top.begin() + k, top.end());
        for (size_t i = 0; i < k; ++i) std::cout << top[i].second << ":" << -top[i].first << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// closeness centrality of the picked sources by batched multi-source BFS (gmsx_bfs_multi), under the usual trial loop; -v: a serial BFS per
// source of this driver's own must give the same reached, depth_sum and levels
int run_closeness(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg, const gmsx_csr *csr) {
    if (args.start >= hg.n) { std::printf("-r %lld: the graph has %lld vertices\n", (long long)args.start, (long long)hg.n); return 100; }
    if (args.iters < 1) { std::printf("-i %lld: at least one source per trial\n", (long long)args.iters); return 100; }
    const int64_t per_trial = args.iters;
    std::vector<int32_t> picks(size_t(per_trial * std::max<int64_t>(args.trials, 0)) + 1);
    if (int rc = gmsx_csr_pick_sources(csr, int64_t(picks.size()) - 1, int32_t(args.start), picks.data())) {
        std::printf("no source to pick: %s\n", gmsx_strerror(rc));
        return 2;
    }
    double total_seconds = 0;
    Timer t;
    std::vector<int32_t> sources;
    std::vector<gmsx_bfs_source> per;
    for (int64_t it = 0; it < args.trials; ++it) {
        sources.assign(picks.begin() + it * per_trial, picks.begin() + (it + 1) * per_trial);
        t.Start();
        gmsx::bfs_multi(g, sources, per);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        double top = 0.0;
        for (const gmsx_bfs_source &x : per) top = std::max(top, x.closeness);
        std::printf("%-21s%g\n", "Max Score:", top);
        if (args.verify) {
            bool ok = true;
            std::vector<int32_t> depth(size_t(hg.n)), to_visit;
            to_visit.reserve(size_t(hg.n));
            for (size_t i = 0; i < sources.size(); ++i) {
                std::fill(depth.begin(), depth.end(), -1);
                to_visit.clear();
                depth[size_t(sources[i])] = 0;
                to_visit.push_back(sources[i]);
                int64_t depth_sum = 0;
                for (size_t at = 0; at < to_visit.size(); ++at) {
                    const int32_t u = to_visit[at];
                    depth_sum += depth[size_t(u)];
                    for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j)
                        if (depth[size_t(hg.adj[j])] == -1) {
                            depth[size_t(hg.adj[j])] = depth[size_t(u)] + 1;
                            to_visit.push_back(hg.adj[j]);
                        }
                }
                if (per[i].reached != int64_t(to_visit.size()) || per[i].depth_sum != depth_sum || per[i].levels != depth[size_t(to_visit.back())] + 1) ok = false;
            }
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ closeness" << std::endl;
    }
    if (args.trials > 0) {
        std::vector<std::pair<double, size_t>> top;  // (-score, position in the list): ascending = largest first, ties by the earlier source
        for (size_t i = 0; i < per.size(); ++i) top.emplace_back(-per[i].closeness, i);
        const size_t k = std::min<size_t>(5, top.size());
        std::partial_sort(top.begin(), top.begin() + k, top.end());
        for (size_t i = 0; i < k; ++i) std::cout << sources[top[i].second] << ":" << -top[i].first << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// PageRank (pr) under the usual trial loop: PageRankPull's sweeps on the device, PRVerifier's rule from gmsx_pagerank_residual and from this
// driver's own serial push sweep (pr.cc:79-97, in double), PrintTopScores' lines at the end
int run_pagerank(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg) {
    const double damping = 0.85;  // kDamp
    const int32_t iters = args.iters_given ? int32_t(std::min<int64_t>(args.iters, INT32_MAX)) : 20;
    double total_seconds = 0;
    Timer t;
    std::vector<double> scores;
    gmsx_pagerank_info pi{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        gmsx::pagerank(g, scores, damping, iters, args.tol, nullptr, GMSX_PR_DEFAULT, &pi);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Iterations", std::to_string(pi.iterations));
        std::printf("%-21s%g\n", "Error:", pi.error);
        if (args.verify) {
            const double residual = gmsx::pagerank_residual(g, scores, damping);
            std::vector<double> incoming(size_t(hg.n), 0.0);
            for (int64_t u = 0; u < hg.n; ++u) {
                const int64_t deg = hg.off[u + 1] - hg.off[u];
                if (deg == 0) continue;
                const double contrib = scores[size_t(u)] / double(deg);
                for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j) incoming[size_t(hg.adj[j])] += contrib;
            }
            double mine = 0.0, mass = 0.0;
            const double base = (1.0 - damping) / double(hg.n > 0 ? hg.n : 1);
            for (int64_t v = 0; v < hg.n; ++v) {
                mine += std::fabs(base + damping * incoming[size_t(v)] - scores[size_t(v)]);
                mass += scores[size_t(v)];
            }
            // the two residuals are the same sum taken in two orders: they differ by rounding only (2^-40 of the mass is far above it)
            const bool ok = residual < args.tol && mine < args.tol && std::fabs(residual - mine) <= std::ldexp(mass > 1.0 ? mass : 1.0, -40);
            std::printf("%-21s%g\n", "Residual:", residual);
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ pagerank" << std::endl;
    }
    if (args.trials > 0)
        for (const auto &kv : gmsx::top_scores(scores, 5)) std::cout << kv.first << ":" << kv.second << std::endl;
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// shortest paths (sssp) under the usual trial loop: DeltaStep on the device from the t-th picked source, SSSPVerifier as gmsx_sssp_verify's four
// numbers, PrintSSSPStats' line (sssp.cc:137-141) at the end
int run_sssp(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg, const gmsx_csr *csr) {
    if (args.start >= hg.n) { std::printf("-r %lld: the graph has %lld vertices\n", (long long)args.start, (long long)hg.n); return 100; }
    std::vector<int32_t> picks(size_t(std::max<int64_t>(args.trials, 0)) + 1);
    if (int rc = gmsx_csr_pick_sources(csr, int64_t(picks.size()) - 1, int32_t(args.start), picks.data())) {
        std::printf("no source to pick: %s\n", gmsx_strerror(rc));
        return 2;
    }
    gmsx::detail::check(gmsx_graph_set_weights(const_cast<gmsx_graph *>(g.device()), gmsx_csr_weights(csr)), "gmsx_graph_set_weights");
    double total_seconds = 0;
    Timer t;
    std::vector<int64_t> dist;
    gmsx_sssp_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        const int32_t source = picks[size_t(it)];
        t.Start();
        gmsx::sssp(g, source, dist, args.delta, nullptr, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Source", std::to_string(source));
        PrintLabel("Delta", std::to_string(info.delta));
        PrintLabel("Buckets", std::to_string(info.buckets));
        if (args.verify) {
            gmsx_sssp_check c{};
            const bool ok = gmsx::sssp_verify(g, source, dist, &c);
            std::printf("%-21s%lld violated, %lld untight, %lld wrongly unreached\n", "Check:", (long long)c.violated_arcs, (long long)c.untight,
                        (long long)c.wrong_unreached);
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ sssp" << std::endl;
    }
    if (args.trials > 0) std::cout << "SSSP Tree reaches " << info.reached << " nodes" << std::endl;
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// serial Kruskal over the host CSR under the order of gmsx.h: the u < v arcs by (weight — heavier first for the maximum —, u, v), a union-find
// with path halving; the forest's edges ascending by (u, v)
std::vector<gmsx::WeightedEdge> host_kruskal(const HostGraph &hg, const int32_t *wgt, bool maximum) {
    std::vector<gmsx::WeightedEdge> all;
    for (int64_t u = 0; u < hg.n; ++u)
        for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j)
            if (int64_t(hg.adj[j]) > u) all.push_back({int32_t(u), hg.adj[j], wgt[j]});
    const auto by_uv = [](const gmsx::WeightedEdge &a, const gmsx::WeightedEdge &b) { return a.u != b.u ? a.u < b.u : a.v < b.v; };
    std::sort(all.begin(), all.end(), [&](const gmsx::WeightedEdge &a, const gmsx::WeightedEdge &b) {
        return a.w != b.w ? (maximum ? a.w > b.w : a.w < b.w) : by_uv(a, b);
    });
    std::vector<int32_t> parent(size_t(hg.n));
    for (int64_t v = 0; v < hg.n; ++v) parent[size_t(v)] = int32_t(v);
    const auto find = [&](int32_t x) {
        while (parent[size_t(x)] != x) x = parent[size_t(x)] = parent[size_t(parent[size_t(x)])];
        return x;
    };
    std::vector<gmsx::WeightedEdge> forest;
    for (const gmsx::WeightedEdge &e : all) {
        const int32_t a = find(e.u), b = find(e.v);
        if (a == b) continue;
        parent[size_t(std::max(a, b))] = std::min(a, b);
        forest.push_back(e);
    }
    std::sort(forest.begin(), forest.end(), by_uv);
    return forest;
}

// the spanning forest (msf) under the usual trial loop; -v: the edge list and the total weight against host_kruskal
int run_msf(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg, const gmsx_csr *csr) {
    gmsx::detail::check(gmsx_graph_set_weights(const_cast<gmsx_graph *>(g.device()), gmsx_csr_weights(csr)), "gmsx_graph_set_weights");
    const uint32_t flags = args.maximum ? uint32_t(GMSX_MSF_MAXIMUM) : 0u;
    double total_seconds = 0, host_seconds = 0;
    Timer t;
    std::vector<gmsx::WeightedEdge> edges, want;
    gmsx_msf_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        gmsx::min_spanning_forest(g, edges, flags, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Trees", std::to_string(info.trees));
        PrintLabel("Edges", std::to_string(info.edges));
        PrintLabel("Total Weight", std::to_string(info.total_weight));
        PrintLabel("Rounds", std::to_string(info.rounds));
        if (args.verify) {
            if (want.empty() && hg.n > 0) {
                t.Start();
                want = host_kruskal(hg, gmsx_csr_weights(csr), args.maximum);
                t.Stop();
                host_seconds = t.Seconds();
            }
            int64_t want_weight = 0;
            for (const gmsx::WeightedEdge &e : want) want_weight += e.w;
            PrintTime("Host Kruskal", host_seconds);
            PrintLabel("Verification", edges == want && want_weight == info.total_weight && int64_t(want.size()) == info.edges ? "PASS" : "FAIL");
        }
        std::cout << "@@@ msf " << (args.maximum ? "maximum" : "minimum") << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// the sequential propagation of gmsx.h over the host CSR: the vertices ascending by (colour, id); a vertex keeps its label if that is a heaviest
// one among its neighbours, else takes the smallest heaviest label; wgt == nullptr: every arc weighs 1
std::vector<int32_t> host_label_propagation(const HostGraph &hg, const int32_t *wgt, const std::vector<int32_t> &color, int64_t max_sweeps) {
    std::vector<int32_t> order(size_t(hg.n)), label(size_t(hg.n));
    for (int64_t v = 0; v < hg.n; ++v) order[size_t(v)] = label[size_t(v)] = int32_t(v);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return color[size_t(a)] != color[size_t(b)] ? color[size_t(a)] < color[size_t(b)] : a < b; });
    std::vector<std::pair<int32_t, int64_t>> seen;  // (label, weight) of the row at hand, ascending by the label
    for (int64_t sweep = 0; sweep < (max_sweeps > 0 ? max_sweeps : 1000); ++sweep) {
        int64_t changes = 0;
        for (const int32_t v : order) {
            seen.clear();
            for (int64_t j = hg.off[v]; j < hg.off[v + 1]; ++j) seen.push_back({label[size_t(hg.adj[j])], wgt ? int64_t(wgt[j]) : 1});
            if (seen.empty()) continue;
            std::sort(seen.begin(), seen.end());
            int64_t best_weight = 0, own = 0;
            int32_t best = -1;
            for (size_t i = 0; i < seen.size();) {
                int64_t sum = 0;
                const int32_t l = seen[i].first;
                for (; i < seen.size() && seen[i].first == l; ++i) sum += seen[i].second;
                if (sum > best_weight) best_weight = sum, best = l;  // (ascending labels: the first at the maximum is the smallest)
                if (l == label[size_t(v)]) own = sum;
            }
            if (own == best_weight) continue;
            label[size_t(v)] = best;
            ++changes;
        }
        if (changes == 0) break;
    }
    return label;
}

// communities by label propagation under the usual trial loop; -v: every label against host_label_propagation
int run_communities(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg, const gmsx_csr *csr) {
    if (args.weighted) gmsx::detail::check(gmsx_graph_set_weights(const_cast<gmsx_graph *>(g.device()), gmsx_csr_weights(csr)), "gmsx_graph_set_weights");
    const uint32_t flags = args.weighted ? uint32_t(GMSX_LP_WEIGHTED) : 0u;
    const int32_t max_sweeps = args.iters_given ? int32_t(args.iters) : 0;
    double total_seconds = 0, host_seconds = 0;
    Timer t;
    std::vector<int32_t> label, want;
    gmsx_lp_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        gmsx::label_propagation(g, label, flags, nullptr, max_sweeps, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        const gmsx_modularity_info mod = gmsx::modularity(g, label, flags);
        PrintLabel("Communities", std::to_string(info.communities));
        PrintLabel("Sweeps", std::to_string(info.sweeps));
        std::printf("%-21s%.6f\n", "Modularity:", mod.modularity);
        if (args.verify) {
            if (want.empty() && hg.n > 0) {
                const std::vector<int32_t> color = gmsx::coloring(g, "id");
                t.Start();
                want = host_label_propagation(hg, args.weighted ? gmsx_csr_weights(csr) : nullptr, color, max_sweeps);
                t.Stop();
                host_seconds = t.Seconds();
            }
            PrintTime("Host Propagation", host_seconds);
            PrintLabel("Verification", label == want && mod.communities == info.communities && (!info.converged || mod.unstable == 0) ? "PASS" : "FAIL");
        }
        std::cout << "@@@ communities " << (args.weighted ? "weighted" : "unweighted") << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// the sequential greedy matching over the host CSR under the order of gmsx.h: the u < v arcs by (heavier weight first, h(u, v), u, v); an edge
// is kept iff both ends are still free
std::vector<int32_t> host_greedy_matching(const HostGraph &hg, const int32_t *wgt) {
    struct Edge { uint32_t k0, h; int32_t u, v; };
    const auto mix = [](uint32_t lo, uint32_t hi) {
        uint32_t h = lo * 0x9E3779B1u + hi;
        h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
        return h;
    };
    std::vector<Edge> all;
    for (int64_t u = 0; u < hg.n; ++u)
        for (int64_t j = hg.off[u]; j < hg.off[u + 1]; ++j)
            if (int64_t(hg.adj[j]) > u) all.push_back({wgt ? ~uint32_t(wgt[j]) : 0u, mix(uint32_t(u), uint32_t(hg.adj[j])), int32_t(u), hg.adj[j]});
    std::sort(all.begin(), all.end(), [](const Edge &a, const Edge &b) {
        return a.k0 != b.k0 ? a.k0 < b.k0 : a.h != b.h ? a.h < b.h : a.u != b.u ? a.u < b.u : a.v < b.v;
    });
    std::vector<int32_t> mate(size_t(hg.n), -1);
    for (const Edge &e : all)
        if (mate[size_t(e.u)] < 0 && mate[size_t(e.v)] < 0) {
            mate[size_t(e.u)] = e.v;
            mate[size_t(e.v)] = e.u;
        }
    return mate;
}

// the greedy matching under the usual trial loop; -v: every mate against host_greedy_matching, and the device's own certificate
int run_matching(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg, const gmsx_csr *csr) {
    if (args.weighted) gmsx::detail::check(gmsx_graph_set_weights(const_cast<gmsx_graph *>(g.device()), gmsx_csr_weights(csr)), "gmsx_graph_set_weights");
    const uint32_t flags = args.weighted ? uint32_t(GMSX_MATCH_WEIGHTED) : 0u;
    double total_seconds = 0, host_seconds = 0;
    Timer t;
    std::vector<int32_t> mate, want;
    gmsx_matching_info info{};
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        gmsx::greedy_matching(g, mate, flags, nullptr, &info);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        PrintLabel("Pairs", std::to_string(info.pairs));
        PrintLabel("Total Weight", std::to_string(info.total_weight));
        PrintLabel("Free", std::to_string(info.free_vertices));
        PrintLabel("Rounds", std::to_string(info.rounds));
        if (args.verify) {
            if (want.empty() && hg.n > 0) {
                t.Start();
                want = host_greedy_matching(hg, args.weighted ? gmsx_csr_weights(csr) : nullptr);
                t.Stop();
                host_seconds = t.Seconds();
            }
            gmsx_matching_check check{};
            const bool certified = gmsx::matching_verify(g, mate, flags, &check);
            PrintTime("Host Greedy", host_seconds);
            PrintLabel("Verification", mate == want && certified && check.pairs == info.pairs && check.total_weight == info.total_weight ? "PASS" : "FAIL");
        }
        std::cout << "@@@ matching " << (args.weighted ? "weighted" : "unweighted") << std::endl;
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    return 0;
}

// subgraph matching: the reference's VF2 drivers (subgraphiso_vf2_sequential.cpp:33-51) over gmsx::subgraph_isomorphisms
int run_sgi(const Args &args, const gmsx::HipSetGraph &g, const HostGraph &hg) {
    gmsx_csr *pc = nullptr;
    const int rc = gmsx_csr_load(args.pattern_file.c_str(), 1, GMSX_RELABEL_NEVER, &pc);
    if (rc != GMSX_OK) {
        std::printf("could not load the pattern: %s\n", gmsx_strerror(rc));
        return 2;
    }
    const int32_t k = int32_t(gmsx_csr_num_nodes(pc));
    const int64_t *po = gmsx_csr_offsets(pc);
    const int32_t *pn = gmsx_csr_neighbors(pc);
    const uint32_t mode = args.mono ? GMSX_SGM_MONO : GMSX_SGM_INDUCED;
    double total_seconds = 0;
    Timer t;
    for (int64_t it = 0; it < args.trials; ++it) {
        t.Start();
        const std::vector<int32_t> row = gmsx::subgraph_isomorphisms(g, k, po, pn, mode | GMSX_SGM_FIRST);
        t.Stop();
        PrintTime("Trial Time", t.Seconds());
        total_seconds += t.Seconds();
        if (row.empty()) {
            std::cout << "No isomorphisms were found" << std::endl;
        } else {  // Result::isomorphism: target vertex -> pattern vertex, in key order
            std::vector<std::pair<int32_t, int32_t>> pairs;
            for (int32_t p = 0; p < k; ++p) pairs.push_back({row[size_t(p)], p});
            std::sort(pairs.begin(), pairs.end());
            std::cout << "isomorphism:";
            for (const auto &pr : pairs) std::cout << " " << pr.first << ":" << pr.second;
            std::cout << std::endl;
        }
        if (args.verify) {  // subgraphisomorphismVerification: every pattern edge a mapped target edge, and (induced) nothing else among the images
            bool ok = true;
            for (int32_t a = 0; a < k && !row.empty(); ++a)
                for (int32_t b = 0; b < k; ++b) {
                    if (a == b) continue;
                    const bool pe = std::binary_search(pn + po[a], pn + po[a + 1], b);
                    const bool te = std::binary_search(hg.row(row[size_t(a)]), hg.row(row[size_t(a)]) + hg.deg(row[size_t(a)]), row[size_t(b)]);
                    if (row[size_t(a)] == row[size_t(b)] || (pe && !te) || (!args.mono && te && !pe)) ok = false;
                }
            PrintLabel("Verification", ok ? "PASS" : "FAIL");
        }
        std::cout << "@@@ vf2 " << (args.mono ? "non-induced" : "induced") << std::endl;
    }
    if (!args.list.empty()) {  // outside the timed trials: every embedding
        const std::vector<int32_t> rows = gmsx::subgraph_isomorphisms(g, k, po, pn, mode);
        std::FILE *f = std::fopen(args.list.c_str(), "w");
        if (!f) { std::printf("could not write %s\n", args.list.c_str()); gmsx_csr_free(pc); return 2; }
        for (size_t i = 0; i < rows.size(); ++i) std::fprintf(f, "%d%c", rows[i], (i + 1) % size_t(k) == 0 ? '\n' : ' ');
        std::fclose(f);
        std::printf("wrote %zu embeddings to %s\n", rows.size() / size_t(k), args.list.c_str());
    }
    PrintTime("Average Time", total_seconds / double(args.trials > 0 ? args.trials : 1));
    gmsx_csr_free(pc);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    Args args = parse(argc, argv);
    if (args.error) { usage(argv[0]); return args.error; }  // the reference exits with 100 / 101 (cli/cli.h:122-133,159-160)
    if (args.kernel != "tc" && args.kernel != "vertex" && args.kernel != "kclique" && args.kernel != "kcstar" && args.kernel != "bk" && args.kernel != "lp" && args.kernel != "color" && args.kernel != "truss" && args.kernel != "sgi" && args.kernel != "cc" && args.kernel != "jp" && args.kernel != "motifs" && args.kernel != "bfs" && args.kernel != "bc" && args.kernel != "closeness" && args.kernel != "pr" && args.kernel != "sssp" && args.kernel != "msf" && args.kernel != "communities" && args.kernel != "matching" && args.kernel != "bicc") { usage(argv[0]); return 100; }
    if (args.gpus >= 1 && !std::getenv("GMSX_DRIVER_RANK")) {
        const int rc_launch = launch_ranks(args.gpus);
        if (rc_launch >= 0) return rc_launch;  // the supervisor; a child (-1) falls through as its rank
    }
    const char *env_rank = std::getenv("GMSX_DRIVER_RANK");
    const int rank = env_rank ? std::atoi(env_rank) : 0;
    const int nranks = env_rank ? std::atoi(std::getenv("GMSX_DRIVER_NRANKS")) : 1;
    const bool root = rank == 0;
    if (!root) {  // only rank 0 talks
        if (!std::freopen("/dev/null", "w", stdout)) return 4;
    }
    if (args.threads > 0) gmsx_set_host_threads(int(args.threads));

    // ---- parse_and_load ------------------------------------------------------------------------------------
    Timer t;
    gmsx_csr *csr = nullptr;
    t.Start();
    int rc;
    const int relabel = (args.kernel == "sgi" || args.kernel == "bicc") ? GMSX_RELABEL_NEVER : GMSX_RELABEL_AUTO;  // the reference's subgraph drivers never relabel; block ids are those of the graph as loaded
    if (args.kernel == "sssp" || args.kernel == "msf" || args.kernel == "matching" || (args.kernel == "communities" && args.weighted))  // WeightedBuilder: the weights of the file, or the generator's; never relabelled (sssp.cc:182-183)
        rc = !args.file.empty() ? gmsx_csr_load_weighted(args.file.c_str(), 1, GMSX_RELABEL_NEVER, &csr)
                                : gmsx_csr_generate_weighted(args.gen == "uniform" ? GMSX_GEN_UNIFORM : GMSX_GEN_KRONECKER, args.scale, args.deg,
                                                             GMSX_RELABEL_NEVER, int(args.threads), &csr);
    else if (!args.file.empty()) rc = gmsx_csr_load(args.file.c_str(), 1, relabel, &csr);
    else rc = gmsx_csr_generate(args.gen == "uniform" ? GMSX_GEN_UNIFORM : GMSX_GEN_KRONECKER, args.scale, args.deg, relabel,
                                int(args.threads), &csr);
    t.Stop();
    if (rc != GMSX_OK) {
        std::printf("could not load the graph: %s\n", gmsx_strerror(rc));
        return rc == GMSX_ERR_DIRECTED ? 100 : 2;
    }
    PrintTime("Load Time", t.Seconds());
    const int64_t n = gmsx_csr_num_nodes(csr), m = gmsx_csr_num_edges(csr);
    // CSRGraph::PrintStats (gapbs/graph.h:270-277)
    std::cout << "Graph has " << n << " nodes and " << m << " undirected edges for degree: " << (n ? m / n : 0) << std::endl;
    if (gmsx_init(env_rank ? rank : -1) != GMSX_OK) { std::printf("no HIP device: this driver has no CPU path\n"); return 3; }

    // ---- communicator (only with --gpus): the id travels through a file written by rank 0 ------------------------------
    gmsx_comm *comm = nullptr;
    if (env_rank) {
        const char *idfile = std::getenv("GMSX_DRIVER_ID_FILE");
        char id[GMSX_COMM_ID_BYTES];
        if (root) {
            if ((rc = gmsx_comm_unique_id(id)) != GMSX_OK) { std::printf("gmsx_comm_unique_id: %s\n", gmsx_strerror(rc)); return 5; }
            const std::string tmp = std::string(idfile) + ".tmp";
            std::FILE *f = std::fopen(tmp.c_str(), "wb");
            if (!f || std::fwrite(id, 1, sizeof(id), f) != sizeof(id)) return 5;
            std::fclose(f);
            if (std::rename(tmp.c_str(), idfile) != 0) return 5;
        } else {
            std::FILE *f = nullptr;
            for (int tries = 0; tries < 6000 && !(f = std::fopen(idfile, "rb")); ++tries) std::this_thread::sleep_for(std::chrono::milliseconds(50));
            if (!f || std::fread(id, 1, sizeof(id), f) != sizeof(id)) return 5;
            std::fclose(f);
        }
        if ((rc = gmsx_comm_init(rank, nranks, id, &comm)) != GMSX_OK) {
            std::fprintf(stderr, "gmsx_comm_init: %s\n", gmsx_strerror(rc));
            std::fflush(nullptr);
            if (rc == GMSX_ERR_TIMEOUT) _exit(5);  // a helper thread is parked inside RCCL: leave without the exit handlers (the supervisor reaps)
            return 5;
        }
        std::printf("RCCL communicator: %d rank(s), one per GPU; partial counts meet in one u64 all-reduce\n", nranks);
    }
    auto reduce = [&](uint64_t v) {
        if (comm) gmsx::detail::check(gmsx_comm_allreduce_u64(comm, &v), "gmsx_comm_allreduce_u64");
        return v;
    };

    // ---- BenchmarkKernelBk / BenchmarkKernelBkPP ---------------------------------------------------------------------------
    t.Start();
    if (nranks > 1 && args.kernel == "tc") gmsx::default_upload_shard() = {rank, nranks};  // this rank's task lists and inline rows only
    if (args.kernel == "tc") gmsx::default_upload_flags() = GMSX_UPLOAD_FOR_TC;              // … built here, inside "GraphExec buildTime"
    gmsx::HipSetGraph g = gmsx::HipSetGraph::FromCsr(csr);  // borrows the CSR arrays; uploads + builds the device containers
    (void)g.device();
    t.Stop();
    PrintTime("GraphExec buildTime", t.Seconds());
    const HostGraph hg{n, gmsx_csr_offsets(csr), gmsx_csr_neighbors(csr)};
    if (args.kernel == "color" || args.kernel == "truss" || args.kernel == "sgi" || args.kernel == "cc" || args.kernel == "jp" || args.kernel == "motifs" || args.kernel == "bfs" || args.kernel == "bc" || args.kernel == "closeness" || args.kernel == "pr" || args.kernel == "sssp" || args.kernel == "msf" || args.kernel == "communities" || args.kernel == "matching" || args.kernel == "bicc") {
        const int rc_run = args.kernel == "bicc" ? run_bicc(args, g, hg) : args.kernel == "matching" ? run_matching(args, g, hg, csr) : args.kernel == "communities" ? run_communities(args, g, hg, csr) : args.kernel == "msf" ? run_msf(args, g, hg, csr) : args.kernel == "sssp" ? run_sssp(args, g, hg, csr) : args.kernel == "pr" ? run_pagerank(args, g, hg) : args.kernel == "closeness" ? run_closeness(args, g, hg, csr) : (args.kernel == "bfs" || args.kernel == "bc") ? run_traversal(args, g, hg, csr) : args.kernel == "motifs" ? run_motifs(args, g, hg) : args.kernel == "color" ? run_color(args, g) : args.kernel == "truss" ? run_truss(args, g) : args.kernel == "sgi" ? run_sgi(args, g, hg)
                                                                                                                                        : run_components(args, g, hg);
        if (comm) gmsx_comm_finalize(comm);
        gmsx_csr_free(csr);
        return rc_run;
    }

    std::string label;
    double total = 0;
    for (int64_t it = 0; it < args.trials; ++it) {
        uint64_t result = 0;
        std::vector<int64_t> counts;
        std::vector<int32_t> order;
        gmsx::ScoredEdges lp_result;
        double pp_time = -1;
        if (args.kernel == "bk") {  // BenchmarkKernelBkPP: preprocess(rgraph, order) per trial (common/benchmark.h:163-170)
            t.Start();
            // the three preprocessors of maximal_clique_enum_bron_kerbosch.cc:36-56: BK-GMS-ADG (eps 0.001), BK-GMS-DEG, BK-GMS-DGR
            if (args.order == "deg") gmsx::degree_order(g, order, true);
            else if (args.order == "dgr") gmsx::degeneracy_order(g, order, true);
            else gmsx::adg_rank(g, 0.001, order, true);
            t.Stop();
            pp_time = t.Seconds();
            PrintTime("Preprocess Time", pp_time);
        }
        t.Start();
        if (args.kernel == "tc") {
            uint64_t part = 0;
            gmsx::detail::check(gmsx_tc_partial(g.device(), GMSX_TC_AUTO, rank, nranks, &part, nullptr), "gmsx_tc_partial");
            result = reduce(part);
            label = "tc-total-par-HipSetGraph";
        } else if (args.kernel == "vertex") {
            gmsx::vertex_count2(g, counts);  // per-vertex output: not sharded
            label = "tc-vertex-count2-par-HipSetGraph";
        } else if (args.kernel == "kclique") {
            uint64_t part = 0, fact = 1;
            gmsx::detail::check(gmsx_kclique_partial(g.device(), args.clique_size, rank, nranks, &part, nullptr), "gmsx_kclique_partial");
            for (int i = 2; i <= args.clique_size; ++i) fact *= uint64_t(i);
            result = reduce(part) * fact;  // the reference's value k!·C_k, mod 2^64 like size_t
            std::printf("total %d-cliques: %" PRIu64 "\n", args.clique_size, result);  // k_clique_count_set_based.h:29
            label = "HipSet HipSetGraph";
        } else if (args.kernel == "lp") {
            const int64_t q = args.q > 0 ? args.q : std::max<int64_t>(1, m / 4);
            lp_result = gmsx::link_prediction(g, lp_metric(args.metric), q);
            result = uint64_t(lp_result.found);
            std::printf("predicted links: %" PRIu64 " of %" PRId64 " requested (%s)\n", result, q, args.metric.c_str());
            label = "link-prediction-HipSetGraph";
        } else if (args.kernel == "kcstar") {  // the timed kernel is the listing's sizing pass: every pair is found, none is copied out
            gmsx_kclique_star_list_info info{};
            gmsx::detail::check(gmsx_kclique_star_list(g.device(), args.clique_size, GMSX_KCSTAR_DEFAULT, 0, 1, nullptr, nullptr, nullptr, 0, 0, &info, nullptr),
                                "gmsx_kclique_star_list");
            result = uint64_t(info.cliques);
            std::printf("total %d-cliques: %" PRIu64 "\n", args.clique_size, result);  // k_clique_star_list/parallel/recursive.h:34
            label = "kcstar-list-par-HipSetGraph";
        } else {
            uint64_t part = 0;
            gmsx::detail::check(gmsx_bk_partial(g.device(), order.data(), rank, nranks, &part, nullptr), "gmsx_bk_partial");
            result = reduce(part);
            label = "BK-GMS-ADG";
        }
        t.Stop();
        const double trial = t.Seconds();
        total += trial;
        PrintTime("Trial Time", trial);
        if (args.kernel == "tc") std::printf("triangles: %" PRIu64 "\n", result);
        if (args.kernel == "bk") std::printf("The Number of maximal clique counted: %" PRIu64 "\n", result);  // helper.h:120-133
        if (args.kernel == "bk" && !args.list.empty() && it + 1 == args.trials) {  // outside the timed trial: the listing build's `sol`
            const auto cliques = gmsx::maximal_cliques(g, order);
            FILE *fo = std::fopen(args.list.c_str(), "w");
            if (!fo) {
                std::fprintf(stderr, "gmsx_driver: --list %s: cannot open\n", args.list.c_str());
                return 2;
            }
            for (const auto &c : cliques) {
                bool first = true;
                for (auto v : c) {
                    std::fprintf(fo, first ? "%d" : " %d", int(v));
                    first = false;
                }
                std::fputc('\n', fo);
            }
            if (std::fclose(fo) != 0) return 2;
        }
        if (args.kernel == "lp" && !args.list.empty() && it + 1 == args.trials) {  // the reference's shape, padding included, worst first
            FILE *fo = std::fopen(args.list.c_str(), "w");
            if (!fo) {
                std::fprintf(stderr, "gmsx_driver: --list %s: cannot open\n", args.list.c_str());
                return 2;
            }
            for (size_t i = 0; i < lp_result.scores.size(); ++i)
                std::fprintf(fo, "%d %d %a\n", int(lp_result.edges[i].first), int(lp_result.edges[i].second), lp_result.scores[i]);
            if (std::fclose(fo) != 0) return 2;
        }
        if (args.kernel == "kcstar" && !args.list.empty() && it + 1 == args.trials) {  // outside the timed trial: the pairs themselves
            const auto pairs = gmsx::clique_stars(g, int32_t(args.clique_size));
            FILE *fo = std::fopen(args.list.c_str(), "w");
            if (!fo) {
                std::fprintf(stderr, "gmsx_driver: --list %s: cannot open\n", args.list.c_str());
                return 2;
            }
            for (const auto &p : pairs) {
                for (auto v : p[0]) std::fprintf(fo, "%d ", int(v));
                std::fputc('|', fo);
                for (auto v : p[1]) std::fprintf(fo, " %d", int(v));
                std::fputc('\n', fo);
            }
            if (std::fclose(fo) != 0) return 2;
        }
        if (args.verify && root) {  // rank 0 verifies; the others go on to the next trial's all-reduce and wait there
            t.Start();
            bool ok = true;
            std::string how;
            if (args.kernel == "tc" || args.kernel == "vertex") {
                const bool host = gmsx_csr_merge_elements(csr) * 2 <= kHostTcElements;
                if (host) {  // triangle_count/verifier.h:13-42 and :44-85
                    std::vector<int64_t> want;
                    const uint64_t tri = host_triangles(hg, args.kernel == "vertex" ? &want : nullptr);
                    ok = args.kernel == "tc" ? tri == result : want == counts;
                    how = "host recount over all directed pairs";
                } else if (args.kernel == "tc") {  // the reference formulation verbatim on the device: m full-row intersect_counts, /3
                    uint64_t again = 0;
                    ok = gmsx_tc_total(g.device(), GMSX_TC_FULL, &again, nullptr) == GMSX_OK && again == result;
                    how = "device full-row recount (graph beyond the host-recount limit)";
                } else {  // verifier.h:84: 3·T == Σ counts / 2
                    uint64_t tri = 0, sum = 0;
                    for (int64_t c : counts) sum += uint64_t(c);
                    ok = gmsx_tc_total(g.device(), GMSX_TC_FULL, &tri, nullptr) == GMSX_OK && sum == 6 * tri;
                    how = "sum identity against the device full-row count (graph beyond the host-recount limit)";
                }
            } else if (args.kernel == "kclique") {
                if (m <= kHostKcEdges) {
                    ok = host_kclique(hg, size_t(args.clique_size)) == result;
                    how = "host recursion on a degree-oriented DAG, times k!";
                } else {  // a different decomposition of the device run: three disjoint shards must add up
                    uint64_t sum = 0, fact = 1;
                    for (int p = 0; p < 3 && ok; ++p) {
                        uint64_t part = 0;
                        ok = gmsx_kclique_partial(g.device(), args.clique_size, p, 3, &part, nullptr) == GMSX_OK;
                        sum += part;
                    }
                    for (int i = 2; i <= args.clique_size; ++i) fact *= uint64_t(i);
                    ok = ok && sum * fact == result;
                    how = "three-shard device recount (graph beyond the host-recount limit)";
                }
            } else if (args.kernel == "lp") {  // a different decomposition of the device run: three shards merged under the rule must give the same entries
                const int64_t q = args.q > 0 ? args.q : std::max<int64_t>(1, m / 4);
                std::vector<gmsx::ScoredEdges> parts;
                for (int p = 0; p < 3; ++p) parts.push_back(gmsx::link_prediction_shard(g, lp_metric(args.metric), q, p, 3));
                const gmsx::ScoredEdges merged = gmsx::merge_link_predictions(parts, q);
                ok = merged.edges == lp_result.edges && merged.scores == lp_result.scores;
                how = "three-shard device recount, merged";
            } else if (args.kernel == "kcstar") {  // the number of pairs is C_k: the count kernels, a different formulation
                uint64_t stars = 0;
                ok = gmsx_kclique_star_count(g.device(), args.clique_size, &stars, nullptr, nullptr) == GMSX_OK && stars == result;
                how = "k-clique count kernels (gmsx_kclique_star_count)";
            } else {
                if (m <= kHostBkEdges) {  // maximal_clique_enum/verifier.h:41-49: recount with Tomita on the host
                    ok = host_bk(hg, order) == result;
                    how = "host Tomita recount";
                } else {
                    uint64_t sum = 0;
                    for (int p = 0; p < 2 && ok; ++p) {
                        uint64_t part = 0;
                        ok = gmsx_bk_partial(g.device(), nullptr, p, 2, &part, nullptr) == GMSX_OK;
                        sum += part;
                    }
                    ok = ok && sum == result;
                    how = "two-shard device recount (graph beyond the host-recount limit)";
                }
            }
            t.Stop();
            const std::string mark = ok ? "PASS" : "FAIL";
            PrintLabel("Verification", mark);
            std::printf("Verification method: %s\n", how.c_str());
            PrintTime("Verification Time", t.Seconds());
            std::cout << "@@@ " << trial << " " << mark << " " << t.Seconds();
            if (pp_time >= 0) std::cout << " " << pp_time;
            std::cout << " " << label << std::endl;
        } else {
            std::cout << "@@@ " << trial;
            if (pp_time >= 0) std::cout << " " << pp_time;
            std::cout << " " << label << std::endl;
        }
    }
    PrintTime("Average Time", total / double(args.trials > 0 ? args.trials : 1));
    if (comm) gmsx_comm_finalize(comm);
    gmsx_csr_free(csr);
    return 0;
}
