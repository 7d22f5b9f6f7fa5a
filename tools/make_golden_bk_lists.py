#!/usr/bin/env python3
"""Writes tests/golden/bk_lists.json: the maximal cliques the REFERENCE lists (BkEppsteinPar::mceBench<RoaringGraph> with the degree
ordering, built with -DMINEBENCH_TEST so that `sol` is filled), per test graph.

Run on a machine that has the reference tree (REF, default /root/reference) and its compiled CRoaring (oracle/_ref/roaring.o: `make -C
oracle`).  A small program is compiled in a temporary directory against the reference headers; every graph is saved as .sg by this
project's loader and read back by the reference's own reader, and the program prints the CSR's fingerprints and every clique.  Checks
before anything is written: the number of cliques equals the BK count golden of the graph, the CSR the reference loaded equals this
project's (FNV-1a fingerprints of both arrays), and, where networkx imports, networkx.find_cliques gives the same set.

Recorded per graph: cliques, members, max_size, size_hist (as gmsx_bk_list_info), the literal list when it has at most 50 cliques, and the
sha256 of the canonical form (members ascending, cliques sorted lexicographically, each as little-endian uint32 size + int32 members)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gms_amd import capi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")

PROGRAM = r'''
#include "gms/third_party/gapbs/benchmark.h"
#include <gms/common/cli/cli.h>
#include <gms/common/types.h>
#include <gms/representations/graphs/set_graph.h>
#include <gms/algorithms/set_based/maximal_clique_enum/bron_kerbosch.h>
#include <gms/algorithms/preprocessing/preprocessing.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace GMS;

static uint64_t fnv(const unsigned char *p, size_t len) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}

int main(int argc, char **argv) {
    CLI::Parser parser;
    CLI::Args args = parser.parse(argc, argv);
    CSRGraph g = args.load_graph();
    const int64_t n = g.num_nodes();
    std::vector<int64_t> off(size_t(n) + 1, 0);
    std::vector<int32_t> nb;
    for (int64_t v = 0; v < n; ++v) {
        for (auto w : g.out_neigh(v)) nb.push_back(int32_t(w));
        off[size_t(v) + 1] = int64_t(nb.size());
    }
    std::printf("F %llu %llu\n", (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(off.data()), off.size() * 8),
                (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(nb.data()), nb.size() * 4));
    RoaringGraph sg = RoaringGraph::FromCGraph(g);
    pvector<NodeId> rank(sg.num_nodes());
    PpParallel::getDegreeOrdering<RoaringGraph, true, pvector<NodeId>>(sg, rank);
    auto sol = BkEppsteinPar::mceBench<RoaringGraph>(sg, rank);
    for (auto &s : sol) {
        std::vector<int32_t> m;
        for (auto v : s) m.push_back(int32_t(v));
        std::sort(m.begin(), m.end());
        std::printf("C");
        for (auto v : m) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
'''


def canonical(cliques):
    return sorted(tuple(sorted(int(x) for x in c)) for c in cliques)


def sha256_of(canon):
    h = hashlib.sha256()
    for c in canon:
        h.update(np.uint32(len(c)).astype("<u4").tobytes())
        h.update(np.asarray(c, dtype="<i4").tobytes())
    return h.hexdigest()


def record(canon):
    sizes = np.asarray([len(c) for c in canon], dtype=np.int64)
    hist = np.zeros(65, dtype=np.int64)
    np.add.at(hist, np.minimum(sizes, 64), 1)
    hist[0] = 0
    rec = {"cliques": len(canon), "members": int(sizes.sum()), "max_size": int(sizes.max()) if sizes.size else 0,
           "size_hist": hist.tolist(), "sha256": sha256_of(canon)}
    if len(canon) <= 50:
        rec["list"] = [list(c) for c in canon]
    return rec


def networkx_check(csr, canon):
    try:
        import networkx as nx
    except ImportError:
        return
    o, a = csr.offsets(), csr.neighbors()
    G = nx.Graph()
    G.add_nodes_from(range(o.size - 1))
    for u in range(o.size - 1):
        G.add_edges_from((u, int(w)) for w in a[o[u]:o[u + 1]] if w > u)
    assert canonical(nx.find_cliques(G)) == canon, "networkx disagrees"


def main():
    roaring = os.path.join(ROOT, "oracle", "_ref", "roaring.o")
    if not os.path.isdir(os.path.join(REF, "gms")) or not os.path.exists(roaring):
        sys.exit(f"needs the reference tree at {REF} and {roaring} (make -C oracle)")
    graphs = json.load(open(os.path.join(GOLDEN, "graphs.json")))
    testgraphs = json.load(open(os.path.join(GOLDEN, "testgraphs.json")))
    ka = json.load(open(os.path.join(GOLDEN, "known_answers.json")))
    inputs = []  # (key, source, csr, expected count)
    for name in sorted(testgraphs):
        inputs.append((name, {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name)), testgraphs[name]["bk"]))
    for i, c in enumerate(ka["bk_random"]):
        e = np.asarray(c["edges"], dtype=np.int32).reshape(-1, 2)
        inputs.append((f"bk_random-{i}", {"kind": "edges", "edges": c["edges"], "n": c["n"]},
                       capi.HostCSR.from_edges(e[:, 0], e[:, 1], num_nodes=c["n"]), c["bk"]))
    for c in ka["kclique"]:
        e = np.asarray(c["edges"], dtype=np.int32).reshape(-1, 2)
        inputs.append((f"kclique-{c['name']}", {"kind": "edges", "edges": c["edges"]}, capi.HostCSR.from_edges(e[:, 0], e[:, 1]), c["bk"]))
    for key in ("kronecker-4-16-relabel", "kronecker-6-16-relabel", "kronecker-8-16-relabel", "kronecker-10-16-relabel", "kronecker-12-16-relabel",
                "kronecker-12-4-relabel", "uniform-10-16-relabel", "uniform-14-16-relabel", "rmat-12-38-a45-b22-c22"):
        r = graphs[key]
        rl = capi.RELABEL_AUTO if r["relabel"] else capi.RELABEL_NEVER
        if r["generator"] == "rmat":
            csr = capi.HostCSR.generate_rmat(r["scale"], r["degree"], 0.45, 0.22, 0.22, rl)
        else:
            csr = capi.HostCSR.generate(r["generator"], r["scale"], r["degree"], rl)
        inputs.append((key, {"kind": "generated", "generator": r["generator"], "scale": r["scale"], "degree": r["degree"], "relabel": r["relabel"]},
                       csr, r["bk"]))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "bk_list_ref.cc"), os.path.join(tmp, "bk_list_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-DMINEBENCH_TEST", "-I", REF, src, roaring, "-o", exe], check=True)
        for key, source, csr, bk in inputs:
            sg = os.path.join(tmp, "g.sg")
            csr.save_sg(sg)
            txt = subprocess.run([exe, "-f", sg], check=True, capture_output=True, text=True).stdout
            lines = txt.splitlines()
            f = [ln for ln in lines if ln.startswith("F ")][0].split()
            assert (int(f[1]), int(f[2])) == csr.fingerprint(), f"{key}: the reference loaded another CSR"
            canon = canonical([int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("C"))
            assert len(canon) == bk, f"{key}: {len(canon)} cliques, BK golden {bk}"
            assert len(set(canon)) == len(canon)
            networkx_check(csr, canon)
            out[key] = dict(record(canon), source=source)
            print(key, out[key]["cliques"], out[key]["max_size"], flush=True)
    with open(os.path.join(GOLDEN, "bk_lists.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
