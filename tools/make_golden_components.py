#!/usr/bin/env python3
"""Writes tests/golden/components.json and tests/golden/components.npz: the goldens of gmsx_connected_components / gmsx_jarvis_patrick.

CONNECTED COMPONENTS come from the REFERENCE.  Run on a machine that has the reference tree (REF, default /root/reference).  A small program of
this project is compiled in a temporary directory against the reference headers: it #includes the reference's log_graph/cc.cc — with that
file's own main renamed by a #define around the #include — and calls its ShiloachVishkin (cc.cc:40-72) and CCVerifier (:98-138) on every graph,
which this project's loader saved as .sg and gapbs' own Builder read back.  Before anything is written the tool asserts that the reference's
labels equal scipy.sparse.csgraph.connected_components relabelled to the smallest id of every component.

JARVIS–PATRICK has no reference code: the records are written by the numpy / scipy restatement kept in tests/test_components_golden_cpu.py
(jarvis_patrick_np).  The count-based metrics are exact on both sides.  The Adamic-Adar sums of the device differ from a host sum in the last
bits, so a threshold of that metric is kept only if no edge's host score lies within 1e-9 relative of it, and is nudged upwards otherwise.  A
record whose kept set is empty or is every edge is refused.

Per graph the JSON holds n, nnz, components, singletons, largest, largest label and the sha256 of the <i4 label array; the array itself is in
the .npz up to 2^16 vertices.  A Jarvis–Patrick record holds graph, metric, threshold (hex float), kept_edges, the same info and labels."""
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
LITERAL_MAX_N = 1 << 16
SEPARATION = 1e-9

PROGRAM = r'''
// labels of the reference's ShiloachVishkin for the graph named by -f: out = comp[n] (int32), then one byte: CCVerifier's answer
#define main reference_cc_main_unused
#include <gms/representations/graphs/log_graph/cc.cc>
#undef main
#include <cstdint>
#include <cstdio>
#include <cstdlib>

static uint64_t fnv(const unsigned char *p, size_t len) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}

int main(int argc, char **argv) {
    CLBase cli(argc, argv, "components golden");
    if (!cli.ParseArgs()) return 2;
    Builder b(cli);
    CSRGraph g = b.MakeGraph();
    const int64_t n = g.num_nodes();
    std::vector<int64_t> off(size_t(n) + 1, 0);
    std::vector<int32_t> nb;
    for (int64_t v = 0; v < n; ++v) {
        for (NodeId w : g.out_neigh(v)) nb.push_back(int32_t(w));
        off[size_t(v) + 1] = int64_t(nb.size());
    }
    std::printf("F %llu %llu\n", (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(off.data()), off.size() * 8),
                (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(nb.data()), nb.size() * 4));
    pvector<NodeId> comp = ShiloachVishkin(g);
    const bool ok = CCVerifier(g, comp);
    const char *path = std::getenv("CC_OUT");
    std::FILE *f = path ? std::fopen(path, "wb") : nullptr;
    if (!f) return 3;
    static_assert(sizeof(NodeId) == 4, "labels are written as int32");
    if (n) std::fwrite(comp.data(), 4, size_t(n), f);
    std::fputc(ok ? 1 : 0, f);
    return std::fclose(f) == 0 ? 0 : 3;
}
'''

GENERATED = [("kronecker", 10, 16, True), ("kronecker", 12, 16, True), ("kronecker", 16, 16, True), ("kronecker", 20, 16, True),
             ("uniform", 10, 16, True), ("uniform", 16, 16, True), ("kronecker", 10, 16, False)]
JP_COUNT = [("common_neighbors", [1.0, 2.0, 5.0, 20.0]), ("jaccard", [0.05, 0.15]), ("overlap", [0.25, 0.5])]
JP_COUNT_GRAPHS = ["kronecker_10_16", "kronecker_12_16", "kronecker_16_16"]
JP_AA = ("adamic_adar", [1.0, 4.0])
JP_AA_GRAPHS = ["kronecker_10_16", "kronecker_12_16"]


def separated(scores, thr):
    return not np.any(np.abs(scores - thr) <= SEPARATION * np.abs(thr))


def main():
    if not os.path.isdir(os.path.join(REF, "gms")):
        sys.exit(f"needs the reference tree at {REF}")
    if not os.path.exists(os.path.join(GOLDEN, "components.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "components.json"), "w").write('{"cc": {}, "jp": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "components.npz"))
    import test_components_golden_cpu as T  # the restatement: components_np, edge_scores_np, jarvis_patrick_np
    inputs = []
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            inputs.append(("file_" + name[:-3], {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name))))
    for kind, scale, deg, relabel in GENERATED:
        key = "%s_%d_%d%s" % (kind, scale, deg, "" if relabel else "_raw")
        inputs.append((key, {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": relabel},
                       capi.HostCSR.generate(kind, scale, deg, capi.RELABEL_AUTO if relabel else capi.RELABEL_NEVER)))
    cc, jp, arrays, csrs = {}, [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "cc_ref.cc"), os.path.join(tmp, "cc_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, "-o", exe], check=True)
        for key, source, csr in inputs:
            off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32)
            n = off.size - 1
            sg, out = os.path.join(tmp, "g.sg"), os.path.join(tmp, "comp.bin")
            csr.save_sg(sg)
            txt = subprocess.run([exe, "-f", sg], check=True, capture_output=True, text=True, env=dict(os.environ, CC_OUT=out)).stdout
            f = [ln for ln in txt.splitlines() if ln.startswith("F ")][0].split()
            assert (int(f[1]), int(f[2])) == csr.fingerprint(), "the reference loaded another CSR"
            raw = open(out, "rb").read()
            assert len(raw) == 4 * n + 1 and raw[-1] == 1, "CCVerifier refused the reference's own labels"
            label = np.frombuffer(raw[:4 * n], dtype="<i4").astype(np.int32)
            want, info = T.components_np(off, adj)
            assert np.array_equal(label, want), key  # the reference's labels ARE the smallest ids
            rec = {"source": source, "n": int(n), "nnz": int(adj.size), "label_sha256": T.sha(label), "literal": bool(n <= LITERAL_MAX_N)}
            rec.update({k: info[k] for k in T.INFO_KEYS if k != "kept_edges"})
            cc[key] = rec
            csrs[key] = (off, adj)
            if rec["literal"]:
                arrays["label_" + key] = label
            print(f"{key}: n {n}, nnz {adj.size}, components {rec['components']}, singletons {rec['singletons']}, largest {rec['largest']} "
                  f"(label {rec['largest_label']})", flush=True)

    def record(graph, metric, thr, scores, index):
        off, adj = csrs[graph]
        label, info, _ = T.jarvis_patrick_np(off, adj, metric, thr, scores)
        assert 0 < info["kept_edges"] < adj.size // 2, (graph, metric, thr, info)  # a record that keeps nothing or everything tests nothing
        rec = {"graph": graph, "metric": metric, "threshold": float(thr).hex(), "label_sha256": T.sha(label), "literal": bool(label.size <= LITERAL_MAX_N)}
        rec.update({k: info[k] for k in T.INFO_KEYS})
        if rec["literal"]:
            rec["array"] = "jp_%s_%s_%d" % (graph, metric, index)
            arrays[rec["array"]] = label
        jp.append(rec)
        print(f"{graph} {metric} >= {thr!r}: kept {info['kept_edges']}, components {info['components']}, largest {info['largest']}", flush=True)

    for graph in JP_COUNT_GRAPHS:
        counts = T.edge_counts_np(*csrs[graph])
        for metric, thresholds in JP_COUNT:
            scores = T.edge_scores_np(*csrs[graph], metric, counts)
            for i, thr in enumerate(thresholds):
                record(graph, metric, thr, scores, i)
    for graph in JP_AA_GRAPHS:
        scores = T.edge_scores_np(*csrs[graph], JP_AA[0])
        for i, thr in enumerate(JP_AA[1]):
            while not separated(scores[2], thr):
                thr = float(np.nextafter(thr * (1 + 4 * SEPARATION), np.inf))
            record(graph, JP_AA[0], thr, scores, i)
    with open(os.path.join(GOLDEN, "components.json"), "w") as fh:
        fh.write('{\n "cc": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(cc[k], sort_keys=True)}" for k in sorted(cc)) + '\n },\n "jp": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in jp) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "components.npz"), **arrays)
    print("wrote", len(cc), "component records,", len(jp), "Jarvis-Patrick records,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
