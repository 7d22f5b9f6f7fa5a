#!/usr/bin/env python3
"""Writes tests/golden/kcstar_lists.json: the (clique, star) pairs the REFERENCE lists (KCliqueStar::Par::CliqueStarList<RoaringGraph>,
k_clique_star_list/parallel/recursive.h:37-43), per test graph and k.

Run on a machine that has the reference tree (REF, default /root/reference) and its compiled CRoaring (oracle/_ref/roaring.o: `make -C
oracle`).  A small program of this project is compiled in a temporary directory against the reference headers (it only #includes them);
every graph is saved as .sg by this project's loader and read back by the reference's own reader, and the program prints the CSR's
fingerprints and its wall time and writes every pair into a binary file.  Checks before anything is written: the CSR the reference loaded
equals this project's (FNV-1a fingerprints of both arrays), the pairs are distinct, and (pairs, sum of the star sizes) equals the oracle's
kclique_star_count.  A (graph, k) above 2 M pairs or 30 M star ids is skipped (decided from the oracle's count) and printed.

Recorded per (graph, k): cliques, star_members, max_star, source, the literal list when it has at most 50 pairs, and the sha256 of the
canonical form: the pairs sorted by clique row, lexicographically; the hash covers, in this order, the sorted clique matrix as <i4, the star
sizes as <i8 and the stars concatenated in that order as <i4."""
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
from oracle.bindings import Oracle  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_PAIRS, MAX_STAR_IDS, MAX_LITERAL = 2_000_000, 30_000_000, 50

PROGRAM = r'''
#include "gms/third_party/gapbs/benchmark.h"
#include <gms/common/cli/cli.h>
#include <gms/common/types.h>
#include <gms/representations/graphs/set_graph.h>
#include <gms/algorithms/set_based/k_clique_star_list/k_clique_star_list.h>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace GMS;

static uint64_t fnv(const unsigned char *p, size_t len) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}

int main(int argc, char **argv) {
    const int k = std::atoi(std::getenv("KCSTAR_K"));
    const char *out_path = std::getenv("KCSTAR_OUT");
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
    const auto t0 = std::chrono::steady_clock::now();
    auto output = KCliqueStar::Par::CliqueStarList<RoaringGraph>(sg, k);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("T %.6f\n", secs);
    std::vector<int32_t> cl, ids;
    std::vector<int64_t> sizes;
    for (const auto &pair : output) {
        std::vector<int32_t> m, s;
        for (auto v : pair[0]) m.push_back(int32_t(v));
        for (auto v : pair[1]) s.push_back(int32_t(v));
        std::sort(m.begin(), m.end());
        std::sort(s.begin(), s.end());
        if (int(m.size()) != k) return 7;
        cl.insert(cl.end(), m.begin(), m.end());
        ids.insert(ids.end(), s.begin(), s.end());
        sizes.push_back(int64_t(s.size()));
    }
    std::FILE *f = std::fopen(out_path, "wb");
    if (!f) return 8;
    const int64_t head[2] = {int64_t(sizes.size()), int64_t(ids.size())};
    std::fwrite(head, 8, 2, f);
    std::fwrite(cl.data(), 4, cl.size(), f);
    std::fwrite(sizes.data(), 8, sizes.size(), f);
    std::fwrite(ids.data(), 4, ids.size(), f);
    return std::fclose(f) == 0 ? 0 : 8;
}
'''


def canonical(cl, sizes, ids):
    """The pairs sorted by clique row: (clique matrix, star sizes, concatenated stars), no Python loop per pair."""
    cl = np.asarray(cl, dtype=np.int32)  # (pairs, k)
    order = np.lexsort(cl[:, ::-1].T) if cl.shape[0] else np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    ssz = sizes[order]
    new_starts = np.concatenate([[0], np.cumsum(ssz)])[:-1]
    gather = np.repeat(starts[order] - new_starts, ssz) + np.arange(int(ssz.sum()), dtype=np.int64)
    return cl[order], ssz, np.asarray(ids, dtype=np.int32)[gather]


def sha256_of(cl, sizes, ids):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(cl, dtype="<i4").tobytes())
    h.update(np.ascontiguousarray(sizes, dtype="<i8").tobytes())
    h.update(np.ascontiguousarray(ids, dtype="<i4").tobytes())
    return h.hexdigest()


def record(cl, sizes, ids):
    rec = {"cliques": int(sizes.size), "star_members": int(ids.size), "max_star": int(sizes.max()) if sizes.size else 0,
           "sha256": sha256_of(cl, sizes, ids)}
    if sizes.size <= MAX_LITERAL:
        off = np.concatenate([[0], np.cumsum(sizes)])
        rec["list"] = [[cl[i].tolist(), ids[off[i]:off[i + 1]].tolist()] for i in range(sizes.size)]
    return rec


def main():
    roaring = os.path.join(ROOT, "oracle", "_ref", "roaring.o")
    if not os.path.isdir(os.path.join(REF, "gms")) or not os.path.exists(roaring):
        sys.exit(f"needs the reference tree at {REF} and {roaring} (make -C oracle)")
    oracle = Oracle()
    graphs = json.load(open(os.path.join(GOLDEN, "graphs.json")))
    testgraphs = json.load(open(os.path.join(GOLDEN, "testgraphs.json")))
    ka = json.load(open(os.path.join(GOLDEN, "known_answers.json")))
    inputs = []  # (key, source, csr, ks)
    all_k = (1, 2, 3, 4, 5)
    for name in sorted(testgraphs):
        inputs.append((name, {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name)), all_k))
    for c in ka["kclique"]:
        e = np.asarray(c["edges"], dtype=np.int32).reshape(-1, 2)
        inputs.append((f"kclique-{c['name']}", {"kind": "edges", "edges": c["edges"]}, capi.HostCSR.from_edges(e[:, 0], e[:, 1]), all_k))
    for key, ks in (("kronecker-4-16-relabel", all_k), ("kronecker-6-16-relabel", all_k), ("kronecker-8-16-relabel", all_k),
                    ("kronecker-10-16-relabel", all_k), ("uniform-10-16-relabel", all_k), ("kronecker-12-4-relabel", (2, 3, 4, 5)),
                    ("kronecker-12-16-relabel", (3,)), ("rmat-12-38-a45-b22-c22", (2, 3))):
        r = graphs[key]
        rl = capi.RELABEL_AUTO if r["relabel"] else capi.RELABEL_NEVER
        if r["generator"] == "rmat":
            csr = capi.HostCSR.generate_rmat(r["scale"], r["degree"], 0.45, 0.22, 0.22, rl)
        else:
            csr = capi.HostCSR.generate(r["generator"], r["scale"], r["degree"], rl)
        inputs.append((key, {"kind": "generated", "generator": r["generator"], "scale": r["scale"], "degree": r["degree"], "relabel": r["relabel"]},
                       csr, ks))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "kcstar_list_ref.cc"), os.path.join(tmp, "kcstar_list_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, roaring, "-o", exe], check=True)
        for key, source, csr, ks in inputs:
            sg, binf = os.path.join(tmp, "g.sg"), os.path.join(tmp, "pairs.bin")
            csr.save_sg(sg)
            for k in ks:
                want = tuple(int(x) for x in oracle.kclique_star_count(csr.offsets(), csr.neighbors(), k))
                if want[0] > MAX_PAIRS or want[1] > MAX_STAR_IDS:
                    print(f"SKIPPED {key} k={k}: {want[0]} pairs, {want[1]} star ids", flush=True)
                    continue
                env = dict(os.environ, KCSTAR_K=str(k), KCSTAR_OUT=binf)
                txt = subprocess.run([exe, "-f", sg], check=True, capture_output=True, text=True, env=env).stdout
                lines = txt.splitlines()
                f = [ln for ln in lines if ln.startswith("F ")][0].split()
                assert (int(f[1]), int(f[2])) == csr.fingerprint(), f"{key}: the reference loaded another CSR"
                secs = float([ln for ln in lines if ln.startswith("T ")][0].split()[1])
                raw = np.fromfile(binf, dtype=np.uint8)
                npairs, nids = (int(x) for x in raw[:16].view("<i8"))
                p = 16
                cl = raw[p:p + 4 * npairs * k].view("<i4").reshape(npairs, k)
                p += 4 * npairs * k
                sizes = raw[p:p + 8 * npairs].view("<i8")
                p += 8 * npairs
                ids = raw[p:p + 4 * nids].view("<i4")
                assert p + 4 * nids == raw.size and int(sizes.sum()) == nids
                cl, sizes, ids = canonical(cl, sizes, ids)
                assert npairs < 2 or np.all(np.any(cl[1:] != cl[:-1], axis=1)), f"{key} k={k}: a clique is listed twice"
                assert (npairs, nids) == want, f"{key} k={k}: reference {(npairs, nids)}, oracle {want}"
                out[f"{key}|k={k}"] = dict(record(cl, sizes, ids), source=source, k=k, graph=key)
                print(f"{key} k={k}: {npairs} pairs, {nids} star ids, max star {out[f'{key}|k={k}']['max_star']}; reference {secs:.3f} s", flush=True)
    with open(os.path.join(GOLDEN, "kcstar_lists.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(key)}: {json.dumps(out[key], sort_keys=True)}" for key in sorted(out)) + "\n}\n")  # a record per line


if __name__ == "__main__":
    main()
