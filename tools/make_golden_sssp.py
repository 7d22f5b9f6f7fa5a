#!/usr/bin/env python3
"""Writes tests/golden/sssp.json, tests/golden/sssp.npz and the fixtures under tests/golden/sssp/: the goldens of the weighted loader and of
gmsx_sssp.

Run on a machine that has the reference tree (REF, default /root/reference).  A small program of this project is compiled in a temporary
directory against the reference headers; it #includes the reference's log_graph/sssp.cc with that file's own main renamed by a #define around
the #include, builds the graph with the reference's WeightedBuilder and runs its DeltaStep and SSSPVerifier.

Asserted before anything is written:
  (a) generator parity: the FNV fingerprints of the offsets, ids and weights of WeightedBuilder's CSR ("-g/-u SCALE -k DEGREE -s") equal those
      of gmsx_csr_generate_weighted;
  (b) file parity: the same for the two .wel fixtures the tool writes (duplicate edges with different weights, a self loop, two components),
      read by the reference's Reader and by gmsx_csr_load_weighted; and a .wsg saved by this project (the relabelled kronecker graph, whose
      weights the reference's own RelabelByDegree would reset to 1) is read back by gapbs' Reader with equal fingerprints;
  (c) distances: per graph, three SourcePicker sources plus source 0; the reference's DeltaStep at delta 1 and 16, each with one and with four
      OpenMP threads, gives one array, its SSSPVerifier accepts it, and it equals the restatement of tests/test_sssp_golden_cpu.py (kDistInf
      mapped to -1).
Stored: dist and the restatement's parent as int32 in the .npz; reached, dist_sum, max_dist, far_vertex in the .json."""
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

PROGRAM = r'''
// the reference's command line (-g/-u SCALE -k DEGREE -s | -f FILE -s); SSSP_SOURCES = "a,b,c"; SSSP_DELTA; SSSP_OUT = the distance arrays
// (int32 [n] per source, kDistInf as -1) followed by one byte per source: SSSPVerifier's answer.  stdout: the three fingerprints.
#define main reference_sssp_main_unused
#include <gms/representations/graphs/log_graph/sssp.cc>
#undef main
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
static uint64_t fnv(const unsigned char *p, size_t len) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}
int main(int argc, char **argv) {
    CLBase cli(argc, argv, "sssp golden");
    if (!cli.ParseArgs()) return 2;
    WeightedBuilder b(cli);
    WGraph g = b.MakeGraph();
    const int64_t n = g.num_nodes();
    std::vector<int64_t> off(size_t(n) + 1, 0);
    std::vector<int32_t> nb, wt;
    for (int64_t v = 0; v < n; ++v) {
        for (WNode wn : g.out_neigh(v)) { nb.push_back(int32_t(wn.v)); wt.push_back(int32_t(wn.w)); }
        off[size_t(v) + 1] = int64_t(nb.size());
    }
    std::printf("F %llu %llu %llu\n", (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(off.data()), off.size() * 8),
                (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(nb.data()), nb.size() * 4),
                (unsigned long long)fnv(reinterpret_cast<const unsigned char *>(wt.data()), wt.size() * 4));
    static_assert(sizeof(WeightT) == 4, "distances are written as int32");
    const char *list = std::getenv("SSSP_SOURCES");
    if (!list) return 0;
    const WeightT delta = WeightT(std::atoi(std::getenv("SSSP_DELTA")));
    std::FILE *out = std::fopen(std::getenv("SSSP_OUT"), "wb");
    if (!out) return 3;
    std::string verdicts;
    for (const char *p = list; *p;) {
        char *end = nullptr;
        const long s = std::strtol(p, &end, 10);
        p = *end == ',' ? end + 1 : end;
        pvector<WeightT> dist = DeltaStep(g, NodeId(s), delta);
        verdicts.push_back(SSSPVerifier(g, NodeId(s), dist) ? 1 : 0);
        std::vector<int32_t> d(size_t(n), 0);
        for (int64_t v = 0; v < n; ++v) d[size_t(v)] = dist[v] == kDistInf ? -1 : int32_t(dist[v]);
        std::fwrite(d.data(), 4, size_t(n), out);
    }
    std::fwrite(verdicts.data(), 1, verdicts.size(), out);
    return std::fclose(out) == 0 ? 0 : 3;
}
'''

# (generator, scale, degree, relabelled)
GENERATED = [("kronecker", 10, 16, False), ("kronecker", 12, 16, False), ("uniform", 10, 16, False), ("kronecker", 10, 16, True)]
DELTAS, THREADS = [1, 16], [1, 4]


def write_wel(path, seed, n_a, n_b, edges):
    """Two components (vertices [0, n_a) and [n_a, n_a + n_b)), duplicate edges with different weights in both directions, one self loop."""
    rng = np.random.RandomState(seed)
    rows = []
    for lo, size in ((0, n_a), (n_a, n_b)):
        for v in range(1, size):  # a spanning path keeps the component connected
            rows.append((lo + v - 1, lo + v, int(rng.randint(1, 60))))
        for _ in range(edges * size // (n_a + n_b)):
            u, v = int(rng.randint(size)), int(rng.randint(size))
            if u != v:
                rows.append((lo + u, lo + v, int(rng.randint(1, 60))))
    for k in range(0, len(rows), 5):  # a repeated edge with another weight, every other one reversed
        u, v, w = rows[k]
        rows.append((v, u, w + 7) if k % 2 else (u, v, max(1, w - 3)))
    rows.append((3, 3, 9))  # a self loop
    order = rng.permutation(len(rows))
    with open(path, "w") as fh:
        for i in order:
            fh.write("%d %d %d\n" % rows[i])


def main():
    if not os.path.isdir(os.path.join(REF, "gms")):
        sys.exit(f"needs the reference tree at {REF}")
    os.makedirs(os.path.join(GOLDEN, "sssp"), exist_ok=True)
    if not os.path.exists(os.path.join(GOLDEN, "sssp.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "sssp.json"), "w").write('{"graphs": {}, "records": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "sssp.npz"))
    import test_sssp_golden_cpu as T  # the restatement
    write_wel(os.path.join(GOLDEN, "sssp", "two_parts_a.wel"), 1, 40, 24, 160)
    write_wel(os.path.join(GOLDEN, "sssp", "two_parts_b.wel"), 2, 17, 30, 90)
    graphs, records, arrays = {}, [], {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "sssp_ref.cc"), os.path.join(tmp, "sssp_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, "-o", exe], check=True)
        inputs = []
        for name in ("two_parts_a.wel", "two_parts_b.wel"):
            path = os.path.join(GOLDEN, "sssp", name)
            inputs.append(("file_" + name[:-4], {"kind": "file", "name": name}, capi.HostCSR.load_weighted(path), ["-f", path, "-s"]))
        for kind, scale, deg, relabel in GENERATED:
            key = "%s_%d_%d%s" % (kind, scale, deg, "_relabelled" if relabel else "")
            csr = capi.HostCSR.generate_weighted(kind, scale, deg, capi.RELABEL_ALWAYS if relabel else capi.RELABEL_NEVER)
            args = ["-u" if kind == "uniform" else "-g", str(scale), "-k", str(deg), "-s"]
            if relabel:  # the reference reads this project's .wsg
                wsg = os.path.join(tmp, key + ".wsg")
                csr.save_wsg(wsg)
                args = ["-f", wsg]
            inputs.append((key, {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": relabel}, csr, args))
        for key, source, csr, args in inputs:
            off, adj, w = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int32), np.array(csr.weights(), dtype=np.int32)
            n = off.size - 1
            fp = [int(x) for x in csr.fingerprint()] + [csr.weights_fingerprint()]
            sources = [int(s) for s in csr.pick_sources(3)]
            sources = sources + [s for s in (0,) if s not in sources]
            out = os.path.join(tmp, "out.bin")
            ref = None
            for delta in DELTAS:
                for threads in THREADS:
                    txt = subprocess.run([exe] + args, check=True, capture_output=True, text=True,
                                         env=dict(os.environ, SSSP_SOURCES=",".join(map(str, sources)), SSSP_DELTA=str(delta), SSSP_OUT=out,
                                                  OMP_NUM_THREADS=str(threads))).stdout
                    f = [ln for ln in txt.splitlines() if ln.startswith("F ")][0].split()
                    assert [int(f[1]), int(f[2]), int(f[3])] == fp, (key, "the reference built another CSR", f, fp)  # (a), (b)
                    raw = open(out, "rb").read()
                    assert len(raw) == 4 * n * len(sources) + len(sources)
                    assert raw[4 * n * len(sources):] == b"\x01" * len(sources), (key, "SSSPVerifier refused DeltaStep's distances")
                    got = np.frombuffer(raw[:4 * n * len(sources)], dtype="<i4").reshape(len(sources), n)
                    assert ref is None or np.array_equal(ref, got), (key, delta, threads)
                    ref = got.copy()
            graphs[key] = {"source": source, "n": int(n), "nnz": int(adj.size), "max_degree": int(np.diff(off).max()), "wmax": int(w.max()),
                           "fingerprints": [str(x) for x in fp]}
            for i, s in enumerate(sources):
                dist = T.dijkstra_np(off, adj, w, s)
                assert np.array_equal(dist, ref[i].astype(np.int64)), (key, s)  # (c)
                info = T.info_np(off, dist)
                rec = {"graph": key, "source": s, "picked": i < 3, "reached": info["reached"], "dist_sum": info["dist_sum"], "max_dist": info["max_dist"],
                       "far_vertex": info["far_vertex"], "reference_deltas": DELTAS, "reference_threads": THREADS, "reference_verified": True}
                assert dist.max() < 2 ** 31
                arrays["dist_" + T.rec_id(rec)] = dist.astype(np.int32)
                arrays["parent_" + T.rec_id(rec)] = T.parent_np(off, adj, w, s, dist)
                records.append(rec)
                print(f"{key} source {s}: reached {info['reached']}, max_dist {info['max_dist']}, dist_sum {info['dist_sum']}", flush=True)
    with open(os.path.join(GOLDEN, "sssp.json"), "w") as fh:
        fh.write('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) + '\n },\n "records": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "sssp.npz"), **arrays)
    print("wrote", len(graphs), "graphs,", len(records), "records,", os.path.getsize(os.path.join(GOLDEN, "sssp.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
