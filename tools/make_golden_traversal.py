#!/usr/bin/env python3
"""Writes tests/golden/traversal.json and tests/golden/traversal.npz: the goldens of gmsx_bfs, gmsx_betweenness and gmsx_csr_pick_sources.

Run on a machine that has the reference tree (REF, default /root/reference).  Two small programs of this project are compiled in a temporary
directory against the reference headers, each in its own translation unit: one #includes the reference's log_graph/bfs.cc, the other its
log_graph/bc.cc — with that file's own main renamed by a #define around the #include.  Every graph is saved as .sg by this project's loader and
read back by gapbs' own Builder (the fingerprints are compared).

BFS.  The records hold what the restatement of tests/test_traversal_golden_cpu.py (bfs_np) computes: the gmsx_bfs_info integers, the sha256 of
the <i4 depth and parent arrays, the arrays themselves in the .npz (depth up to 2^16 vertices; parent, which does not compress, up to 2^12 —
the parents of the 65 536-vertex graphs alone would pass the size a committed file may have — the sha256 covers them), and bottom_up_levels at BFS_DIRECTION 0 and the default
alpha / beta from the replay of the switching rule.  Before a record is written the tool asserts that the REFERENCE's DOBFS parents (bfs.cc:120-190)
give the same depths, and that the reference's BFSVerifier (:212-258) accepts both the reference's parents and the smallest-id parents.
Sources per graph: the picker's first four, the vertex of the largest degree and, where one exists, an isolated vertex and a vertex outside the
largest component (both from tests/golden/components.npz).

PICKER.  The first 16 picks of the reference's SourcePicker (gapbs/benchmark.h:51-75) per graph.

BC.  Source lists: the first 1, 4 and 8 picks, and all n sources for the graphs of at most 1024 vertices; flags both off and both on.  The
scores are those of the exact restatement (betweenness_exact: integers for sigma, rationals for delta, rounded once to double), with max_sigma,
max_levels and the graph's maximum degree.  Asserted before a record is written: max_sigma < 2^53; and, for the lists the reference can run (its
sources come from its picker), that the reference's float scores (Brandes, bc.cc:89-153, one OpenMP thread, accepted by its own BCVerifier) agree
with the restatement within the derived bound at eps = 2^-24 plus 2 eps for the normalisation — unless max_sigma >= 2^31, where the reference's
32-bit counts wrap: such a record is kept with "reference": false.  The all-sources lists cannot be given to the reference: "reference": false.
The graphs above 4096 vertices get the one-source list only: their score arrays are 512 KB each before compression, and the exact restatement is
pure Python."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gms_amd import capi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BC_MAX_N = 4096
ALL_SOURCES_MAX_N = 1024

COMMON = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
static uint64_t fnv(const unsigned char *p, size_t len) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}
static void print_fingerprint(const CSRGraph &g) {
    const int64_t n = g.num_nodes();
    std::vector<int64_t> off(size_t(n) + 1, 0);
    std::vector<int32_t> nb;
    for (int64_t v = 0; v < n; ++v) {
        for (NodeId w : g.out_neigh(v)) nb.push_back(int32_t(w));
        off[size_t(v) + 1] = int64_t(nb.size());
    }
    std::printf("F %llu %llu\n", (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(off.data()), off.size() * 8),
                (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(nb.data()), nb.size() * 4));
}
'''

BFS_PROGRAM = r'''
// TRAV_SOURCES = "s0,s1,…"; TRAV_CAND = file of the candidate parents (int32 [sources][n]); TRAV_OUT = per source: the reference's DOBFS
// parents (int32 [n]), BFSVerifier's answer for them (1 byte), BFSVerifier's answer for the candidate (1 byte).  stdout: the fingerprint and
// "P" + the first 16 picks of SourcePicker.
#define main reference_bfs_main_unused
#include <gms/representations/graphs/log_graph/bfs.cc>
#undef main
#include <gms/third_party/gapbs/builder.h>
''' + COMMON + r'''
int main(int argc, char **argv) {
    CLBase cli(argc, argv, "traversal golden: bfs");
    if (!cli.ParseArgs()) return 2;
    Builder b(cli);
    CSRGraph g = b.MakeGraph();
    const int64_t n = g.num_nodes();
    print_fingerprint(g);
    SourcePicker<CSRGraph> sp(g);
    std::printf("P");
    for (int i = 0; i < 16; ++i) std::printf(" %d", int(sp.PickNext()));
    std::printf("\n");
    static_assert(sizeof(NodeId) == 4, "parents are written as int32");
    std::FILE *cand = std::fopen(std::getenv("TRAV_CAND"), "rb"), *out = std::fopen(std::getenv("TRAV_OUT"), "wb");
    if (!cand || !out) return 3;
    std::string list = std::getenv("TRAV_SOURCES");
    for (size_t at = 0; at < list.size();) {
        size_t end = list.find(',', at);
        if (end == std::string::npos) end = list.size();
        const NodeId s = NodeId(std::stol(list.substr(at, end - at)));
        at = end + 1;
        pvector<NodeId> parent = DOBFS(g, s);
        // (the reference leaves -degree in the unvisited entries; its verifier wants -1 there, as its own PrintBFSStats counts them)
        for (int64_t v = 0; v < n; ++v) if (parent[v] < 0) parent[v] = -1;
        const bool ok = BFSVerifier(g, s, parent);
        pvector<NodeId> theirs(n);
        if (std::fread(theirs.data(), 4, size_t(n), cand) != size_t(n)) return 4;
        const bool ok2 = BFSVerifier(g, s, theirs);
        std::fwrite(parent.data(), 4, size_t(n), out);
        std::fputc(ok ? 1 : 0, out);
        std::fputc(ok2 ? 1 : 0, out);
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
'''

BC_PROGRAM = r'''
// -i K: Brandes from the first K picks; TRAV_OUT = the reference's normalised float scores (n), then BCVerifier's answer (1 byte)
#define main reference_bc_main_unused
#include <gms/representations/graphs/log_graph/bc.cc>
#undef main
''' + COMMON + r'''
int main(int argc, char **argv) {
    CLIterApp cli(argc, argv, "traversal golden: bc", 1);
    if (!cli.ParseArgs()) return 2;
    Builder b(cli);
    CSRGraph g = b.MakeGraph();
    print_fingerprint(g);
    SourcePicker<CSRGraph> sp(g), vsp(g);
    pvector<ScoreT> scores = Brandes(g, sp, cli.num_iters());
    const bool ok = BCVerifier(g, vsp, cli.num_iters(), scores);
    static_assert(sizeof(ScoreT) == 4, "scores are written as float");
    std::FILE *out = std::fopen(std::getenv("TRAV_OUT"), "wb");
    if (!out) return 3;
    std::fwrite(scores.data(), 4, size_t(g.num_nodes()), out);
    std::fputc(ok ? 1 : 0, out);
    return std::fclose(out) == 0 ? 0 : 3;
}
'''

GENERATED = [("kronecker", 10, 16, True), ("kronecker", 12, 16, True), ("kronecker", 16, 16, True), ("uniform", 10, 16, True), ("uniform", 16, 16, True),
             ("kronecker", 10, 16, False)]


def fingerprint_ok(txt, csr):
    f = [ln for ln in txt.splitlines() if ln.startswith("F ")][0].split()
    return (int(f[1]), int(f[2])) == csr.fingerprint()


def main():
    if not os.path.isdir(os.path.join(REF, "gms")):
        sys.exit(f"needs the reference tree at {REF}")
    if not os.path.exists(os.path.join(GOLDEN, "traversal.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "traversal.json"), "w").write('{"graphs": {}, "bfs": [], "bc": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "traversal.npz"))
    import test_traversal_golden_cpu as T  # the restatements
    comp = np.load(os.path.join(GOLDEN, "components.npz"))
    inputs = []
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            inputs.append(("file_" + name[:-3], {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name))))
    for kind, scale, deg, relabel in GENERATED:
        key = "%s_%d_%d%s" % (kind, scale, deg, "" if relabel else "_raw")
        inputs.append((key, {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": relabel},
                       capi.HostCSR.generate(kind, scale, deg, capi.RELABEL_AUTO if relabel else capi.RELABEL_NEVER)))
    graphs, bfs, bc, arrays = {}, [], [], {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = {}
        for name, text in (("bfs", BFS_PROGRAM), ("bc", BC_PROGRAM)):
            src, exe[name] = os.path.join(tmp, name + "_ref.cc"), os.path.join(tmp, name + "_ref")
            open(src, "w").write(text)
            subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, "-o", exe[name]], check=True)
        for key, source, csr in inputs:
            off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32)
            n, deg = off.size - 1, np.diff(off)
            sg, out, cand = os.path.join(tmp, "g.sg"), os.path.join(tmp, "out.bin"), os.path.join(tmp, "cand.bin")
            csr.save_sg(sg)
            # ---- the sources
            picks = csr.pick_sources(16).tolist()
            label = comp["label_" + key]
            roots, sizes = np.unique(label, return_counts=True)
            giant = roots[np.argmax(sizes)]
            srcs = [(int(s), "pick") for s in picks[:4]] + [(int(np.argmax(deg)), "hub")]
            if np.any(deg == 0):
                srcs.append((int(np.flatnonzero(deg == 0)[0]), "isolated"))
            if np.any((label != giant) & (deg > 0)):
                srcs.append((int(np.flatnonzero((label != giant) & (deg > 0))[0]), "outside"))
            seen, uniq = set(), []
            for s, kind in srcs:
                if s not in seen:
                    seen.add(s)
                    uniq.append((s, kind))
            # ---- BFS: the restatement, checked against the reference
            mine = [T.bfs_np(off, adj, s) for s, _ in uniq]
            np.concatenate([m[1] for m in mine]).astype("<i4").tofile(cand)
            env = dict(os.environ, TRAV_OUT=out, TRAV_CAND=cand, TRAV_SOURCES=",".join(str(s) for s, _ in uniq))
            txt = subprocess.run([exe["bfs"], "-f", sg], check=True, capture_output=True, text=True, env=env).stdout
            assert fingerprint_ok(txt, csr), "the reference loaded another CSR"
            ref_picks = [int(x) for x in [ln for ln in txt.splitlines() if ln.startswith("P")][0].split()[1:]]
            assert ref_picks == picks, (key, ref_picks, picks)  # recorded: the REFERENCE's picks
            raw = open(out, "rb").read()
            assert len(raw) == len(uniq) * (4 * n + 2)
            graphs[key] = {"source": source, "n": int(n), "nnz": int(adj.size), "max_degree": int(deg.max()), "picks": ref_picks,
                           "bfs_sources": [s for s, _ in uniq]}
            for i, ((s, kind), (depth, parent, info)) in enumerate(zip(uniq, mine)):
                blk = raw[i * (4 * n + 2):(i + 1) * (4 * n + 2)]
                ref_parent = np.frombuffer(blk[:4 * n], dtype="<i4").astype(np.int64)
                assert blk[4 * n] == 1, "BFSVerifier refused the reference's own parents"
                assert blk[4 * n + 1] == 1, "BFSVerifier refused the smallest-id parents"
                # the reference's parents give the same depths: depth[v] = depth[parent[v]] + 1, the same reached set
                assert np.array_equal(ref_parent >= 0, depth >= 0) and ref_parent[s] == s, (key, s)
                r = np.flatnonzero((ref_parent >= 0) & (np.arange(n) != s))
                assert np.array_equal(depth[r], depth[ref_parent[r]] + 1), (key, s)
                assert np.all(parent[r] <= ref_parent[r])  # (ours is the smallest id among the possible parents)
                rec = {"graph": key, "source": s, "kind": kind, "depth_sha256": T.sha(depth), "parent_sha256": T.sha(parent),
                       "literal": bool(n <= T.LITERAL_MAX_N), "literal_parent": bool(n <= T.PARENT_LITERAL_MAX_N)}
                rec.update(info)
                bfs.append(rec)
                if rec["literal"]:
                    arrays["depth_%s_%d" % (key, s)] = depth
                if rec["literal_parent"]:
                    arrays["parent_%s_%d" % (key, s)] = parent
                print(f"{key} bfs from {s} ({kind}): reached {info['reached']}, levels {info['levels']}, widest {info['widest']} at {info['widest_level']}, "
                      f"bottom-up levels {info['bottom_up_levels']}", flush=True)
            # ---- BC
            lists = [("1", picks[:1]), ("4", picks[:4]), ("8", picks[:8])] + ([("all", list(range(n)))] if n <= ALL_SOURCES_MAX_N else [])
            if n > BC_MAX_N:  # one list: the rows above kBcChunk entries (several chunks, slots added in slot order) are in these graphs
                lists = lists[:1]
            for name, srcl in lists:
                exact = {}
                for excl, norm in ((False, False), (True, True)) + (((False, True),) if name != "all" else ()):
                    exact[(excl, norm)] = T.betweenness_exact(off, adj, srcl, excl, norm)
                _, max_sigma, max_levels = exact[(False, False)]
                assert max_sigma < 2 ** 53, (key, name, max_sigma)
                compared = False
                if name != "all" and max_sigma < 2 ** 31:
                    txt = subprocess.run([exe["bc"], "-f", sg, "-i", name, "-n", "1"], check=True, capture_output=True, text=True,
                                         env=dict(os.environ, TRAV_OUT=out, OMP_NUM_THREADS="1")).stdout
                    assert fingerprint_ok(txt, csr)
                    raw = open(out, "rb").read()
                    assert len(raw) == 4 * n + 1 and raw[-1] == 1, "BCVerifier refused the reference's own scores"
                    ref = np.frombuffer(raw[:4 * n], dtype="<f4").astype(np.float64)
                    want = exact[(False, True)][0]
                    e24 = 2.0 ** -24
                    bound = T.bc_bound(want, max_levels, int(deg.max()), len(srcl), eps=e24) + 2 * e24 * want
                    assert np.all(np.abs(ref - want) <= bound), (key, name, float(np.max(np.abs(ref - want) - bound)))
                    compared = True
                for excl, norm in ((False, False), (True, True)):
                    rec = {"graph": key, "sources": name, "n_sources": len(srcl), "exclude_source": excl, "normalize": norm, "max_sigma": str(max_sigma),
                           "max_levels": int(max_levels), "reference": compared, "array": "bc_%s_%s_%d" % (key, name, int(excl))}
                    arrays[rec["array"]] = exact[(excl, norm)][0]
                    bc.append(rec)
                print(f"{key} bc over {name} sources: max sigma {max_sigma}, levels {max_levels}, reference compared: {compared}", flush=True)
    must = {k for k in graphs if k.startswith("file_")} | {"kronecker_10_16"}
    assert must <= {r["graph"] for r in bc if r["reference"]}, "choose other sources: never loosen the bound"
    with open(os.path.join(GOLDEN, "traversal.json"), "w") as fh:
        fh.write('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) + '\n },\n "bfs": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in bfs) + '\n ],\n "bc": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in bc) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "traversal.npz"), **arrays)
    print("wrote", len(graphs), "graphs,", len(bfs), "BFS records,", len(bc), "BC records,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
