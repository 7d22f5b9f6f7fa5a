#!/usr/bin/env python3
"""Writes tests/golden/truss.json and tests/golden/truss.npz: the trussness of every edge of the test graphs — the goldens of
gmsx_edge_support / gmsx_truss_decomposition.

The k-truss has no counterpart in the reference, so the goldens come from an INDEPENDENT implementation of this project's own: the serial
bucket peel (always remove one edge of the lowest remaining support; the trussness is the running maximum of the removal supports + 2), a
small C++ program written here and compiled in a temporary directory.  It shares nothing with the level-synchronous peel of truss.hip or with
its numpy restatement in tests/test_truss_golden_cpu.py but the definition; the trussness of an edge is unique for the graph, so all three
must agree bit for bit.  Needs only g++ and the built libgmsx.so (the loader and the generators); no GPU.

Per graph the JSON holds n, nnz, m, max truss, the trussness histogram, levels, the edges of the top truss, triangles, max support and the
sha256 of the <i4 per-arc trussness array (parallel to the CSR's neigh); graphs of m <= 50 000 also have the arrays truss_<graph> and
support_<graph> literally in the .npz."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_LITERAL_M = 50000

PROGRAM = r'''
// serial bucket peel: in  = n, nnz (int64), off[n + 1] (int64), adj[nnz] (int32); out = support[nnz], truss[nnz] (int32), per arc
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    int64_t n = 0, nnz = 0;
    if (!f || std::fread(&n, 8, 1, f) != 1 || std::fread(&nnz, 8, 1, f) != 1) return 3;
    std::vector<int64_t> off(size_t(n) + 1);
    std::vector<int32_t> adj(size_t(nnz) + 1);
    if (std::fread(off.data(), 8, size_t(n) + 1, f) != size_t(n) + 1 || std::fread(adj.data(), 4, size_t(nnz), f) != size_t(nnz)) return 3;
    std::fclose(f);
    const int64_t m = nnz / 2;
    // edge ids: the u < v arcs in CSR order; the other arc finds its twin by binary search
    std::vector<int64_t> eid(size_t(nnz) + 1);
    std::vector<int32_t> eu(size_t(m) + 1), ev(size_t(m) + 1);
    int64_t next = 0;
    for (int64_t u = 0; u < n; ++u)
        for (int64_t j = off[u]; j < off[u + 1]; ++j)
            if (u < adj[j]) { eu[next] = int32_t(u); ev[next] = adj[j]; eid[j] = next++; }
    if (next != m) return 4;
    for (int64_t u = 0; u < n; ++u)
        for (int64_t j = off[u]; j < off[u + 1]; ++j)
            if (adj[j] < u) {
                const int32_t v = adj[j];
                const int32_t *p = std::lower_bound(adj.data() + off[v], adj.data() + off[v + 1], int32_t(u));
                if (p == adj.data() + off[v + 1] || *p != u) return 4;
                eid[j] = eid[p - adj.data()];
            }
    // support by merging the two rows
    std::vector<int32_t> sup(size_t(m) + 1, 0);
    for (int64_t e = 0; e < m; ++e) {
        int64_t i = off[eu[e]], ie = off[eu[e] + 1], j = off[ev[e]], je = off[ev[e] + 1];
        int32_t c = 0;
        while (i < ie && j < je) {
            if (adj[i] < adj[j]) ++i;
            else if (adj[j] < adj[i]) ++j;
            else { ++c; ++i; ++j; }
        }
        sup[e] = c;
    }
    std::vector<int32_t> sup0(sup);
    // bucket sort by support: pos[e] = place of e in `order`, bin[s] = first place of support s
    int32_t maxs = 0;
    for (int64_t e = 0; e < m; ++e) maxs = std::max(maxs, sup[e]);
    std::vector<int64_t> bin(size_t(maxs) + 2, 0), pos(size_t(m) + 1), order(size_t(m) + 1);
    for (int64_t e = 0; e < m; ++e) ++bin[size_t(sup[e]) + 1];
    for (int32_t s = 0; s <= maxs; ++s) bin[size_t(s) + 1] += bin[s];
    {
        std::vector<int64_t> at(bin.begin(), bin.end() - 1);
        for (int64_t e = 0; e < m; ++e) { pos[e] = at[sup[e]]++; order[pos[e]] = e; }
    }
    std::vector<char> gone(size_t(m) + 1, 0);
    std::vector<int32_t> truss(size_t(m) + 1, 0);
    int32_t k = 0;
    auto lower = [&](int64_t x) {  // sup[x] drops by one: x swaps with the first edge of its bucket, whose start moves up
        const int32_t s = sup[x];
        const int64_t first = bin[s], y = order[first];
        if (x != y) { order[pos[x]] = y; pos[y] = pos[x]; order[first] = x; pos[x] = first; }
        ++bin[s];
        --sup[x];
    };
    for (int64_t at = 0; at < m; ++at) {
        const int64_t e = order[at];
        k = std::max(k, sup[e]);
        truss[e] = k + 2;
        gone[e] = 1;
        int64_t i = off[eu[e]], ie = off[eu[e] + 1], j = off[ev[e]], je = off[ev[e] + 1];
        while (i < ie && j < je) {
            if (adj[i] < adj[j]) ++i;
            else if (adj[j] < adj[i]) ++j;
            else {
                const int64_t e1 = eid[i], e2 = eid[j];
                if (!gone[e1] && !gone[e2]) {
                    if (sup[e1] > sup[e]) lower(e1);
                    if (sup[e2] > sup[e]) lower(e2);
                }
                ++i; ++j;
            }
        }
    }
    std::vector<int32_t> out(size_t(nnz) * 2 + 1);
    for (int64_t j = 0; j < nnz; ++j) { out[j] = sup0[eid[j]]; out[nnz + j] = truss[eid[j]]; }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    std::fwrite(out.data(), 4, size_t(nnz) * 2, f);
    return std::fclose(f) == 0 ? 0 : 5;
}
'''

# (key, source record, record of tests/golden/graphs.json with the compiled reference's triangle count, or None)
GENERATED = [
    ("kronecker", 8, 16, True, "kronecker-8-16-relabel"), ("kronecker", 10, 16, True, "kronecker-10-16-relabel"),
    ("kronecker", 12, 16, True, "kronecker-12-16-relabel"), ("kronecker", 14, 16, True, "kronecker-14-16-relabel"),
    ("kronecker", 16, 16, True, "kronecker-16-16-relabel"), ("kronecker", 12, 4, True, "kronecker-12-4-relabel"),
    ("kronecker", 10, 8, False, None), ("uniform", 10, 16, True, "uniform-10-16-relabel"), ("uniform", 12, 16, True, None),
    ("rmat", 12, 38, True, "rmat-12-38-a45-b22-c22"),
]


def generate(kind, scale, deg, relabel):
    flag = capi.RELABEL_AUTO if relabel else capi.RELABEL_NEVER
    if kind == "rmat":  # the parameters of BASELINE configs[3]
        return capi.HostCSR.generate_rmat(scale, deg, 0.45, 0.22, 0.22, flag)
    return capi.HostCSR.generate(kind, scale, deg, flag)


def main():
    inputs = []
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            inputs.append(("file_" + name[:-3], {"kind": "file", "name": name}, None, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name))))
    for kind, scale, deg, relabel, gkey in GENERATED:
        key = "%s_%d_%d%s" % (kind, scale, deg, "" if relabel else "_raw")
        inputs.append((key, {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": relabel}, gkey, generate(kind, scale, deg, relabel)))
    meta, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "truss_peel.cc"), os.path.join(tmp, "truss_peel")
        with open(src, "w") as fh:
            fh.write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", src, "-o", exe], check=True)
        for key, source, gkey, csr in inputs:
            off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32)
            n, nnz = off.size - 1, adj.size
            fin, fout = os.path.join(tmp, "g.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as fh:
                fh.write(np.array([n, nnz], dtype="<i8").tobytes() + off.astype("<i8").tobytes() + adj.astype("<i4").tobytes())
            subprocess.run([exe, fin, fout], check=True)
            raw = np.fromfile(fout, dtype="<i4")
            assert raw.size == 2 * nnz
            support, truss = raw[:nnz].astype(np.int32), raw[nnz:].astype(np.int32)
            src_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
            up = src_of < adj
            assert int(support.sum()) % 6 == 0 and int(up.sum()) * 2 == nnz
            values, counts = np.unique(truss[up], return_counts=True)
            mx = int(values.max()) if values.size else 0
            rec = {"source": source, "graphs_key": gkey, "n": int(n), "nnz": int(nnz), "m": int(nnz // 2), "max_truss": mx,
                   "hist": {str(int(v)): int(c) for v, c in zip(values, counts)}, "levels": int(values.size),
                   "top_edges": int(counts[-1]) if values.size else 0, "triangles": int(support.sum()) // 6,
                   "max_support": int(support.max()) if nnz else 0,
                   "truss_sha256": hashlib.sha256(np.ascontiguousarray(truss, dtype="<i4").tobytes()).hexdigest(),
                   "support_sha256": hashlib.sha256(np.ascontiguousarray(support, dtype="<i4").tobytes()).hexdigest(),
                   "literal": bool(nnz // 2 <= MAX_LITERAL_M)}
            meta[key] = rec
            if rec["literal"]:
                arrays["truss_" + key], arrays["support_" + key] = truss, support
            print(f"{key}: n {n}, m {nnz // 2}, triangles {rec['triangles']}, max truss {mx}, levels {rec['levels']}, top edges {rec['top_edges']}", flush=True)
    with open(os.path.join(GOLDEN, "truss.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(key)}: {json.dumps(meta[key], sort_keys=True)}" for key in sorted(meta)) + "\n}\n")  # a record per line
    np.savez_compressed(os.path.join(GOLDEN, "truss.npz"), **arrays)
    print("wrote", len(meta), "records,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
