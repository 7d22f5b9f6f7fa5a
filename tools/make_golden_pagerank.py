#!/usr/bin/env python3
"""Writes tests/golden/pagerank.json and tests/golden/pagerank.npz: the goldens of gmsx_pagerank.

Run on a machine that has the reference tree (REF, default /root/reference).  A small program of this project is compiled in a temporary
directory against the reference headers; it #includes the reference's log_graph/pr.cc with that file's own main renamed by a #define around the
#include.  Every graph is saved as .sg by this project's loader and read back by gapbs' own Builder (the fingerprints are compared).

A record is (graph, damping, max_iters, tolerance, teleport kind, flags) -> iterations, converged, argmax, the top five ids, error, sum and the
score array (in the .npz).  The values are those of the numpy float64 restatement of tests/test_pagerank_golden_cpu.py (pagerank_np: ascending row
sums) — also for the records whose flags ask for float32 storage: the device's float scores are held to them by the float bound.

Asserted before a record is written:
  (a) where the reference can run the record (damping 0.85, uniform teleport, no GMSX_PR_DANGLING): its PageRankPull float scores (one OpenMP
      thread) lie within pr_bound(k, 0.85, dmax, 2^-24) of the restatement in L1 — the reference adds a row in float, so the bound's eps is
      float's;
  (b) … and, where the record converged, the reference's own PRVerifier accepts the restatement's scores cast to float at the record's tolerance;
  (c) no sweep's error lies within four times the bound of the tolerance (tolerance 0 never stops a run: nothing to assert), so the iteration
      count is a fact that both sides must reproduce.
A record that fails (c) needs another tolerance here, never a wider bound there."""
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
// -f graph.sg; PR_ITERS, PR_TOL; PR_CAND = candidate scores (float [n]); PR_OUT = the reference's PageRankPull scores (float [n]), PRVerifier's
// answer for them (1 byte), PRVerifier's answer for the candidate (1 byte).  stdout: the fingerprint.
#define main reference_pr_main_unused
#include <gms/representations/graphs/log_graph/pr.cc>
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
    CLBase cli(argc, argv, "pagerank golden");
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
    static_assert(sizeof(ScoreT) == 4, "scores are written as float");
    const int iters = std::atoi(std::getenv("PR_ITERS"));
    const double tol = std::atof(std::getenv("PR_TOL"));
    pvector<ScoreT> scores = PageRankPull(g, iters, tol);
    const bool ok = PRVerifier(g, scores, tol);
    pvector<ScoreT> theirs(n);
    std::FILE *cand = std::fopen(std::getenv("PR_CAND"), "rb"), *out = std::fopen(std::getenv("PR_OUT"), "wb");
    if (!cand || !out || std::fread(theirs.data(), 4, size_t(n), cand) != size_t(n)) return 3;
    const bool ok2 = PRVerifier(g, theirs, tol);
    std::fwrite(scores.data(), 4, size_t(n), out);
    std::fputc(ok ? 1 : 0, out);
    std::fputc(ok2 ? 1 : 0, out);
    return std::fclose(out) == 0 ? 0 : 3;
}
'''

GENERATED = [("kronecker", 10, 16, True), ("kronecker", 12, 16, True), ("uniform", 10, 16, True), ("kronecker", 10, 16, False)]
# (damping, max_iters, tolerance, teleport kind, flags)
CASES = [(0.85, 20, 1e-4, "uniform", 0), (0.85, 20, 1e-4, "uniform", 1), (0.85, 20, 1e-4, "uniform", 2), (0.85, 8, 0.0, "uniform", 0),
         (0.5, 100, 1e-9, "degree", 0), (0.85, 30, 1e-3, "first", 3)]


def main():
    if not os.path.isdir(os.path.join(REF, "gms")):
        sys.exit(f"needs the reference tree at {REF}")
    if not os.path.exists(os.path.join(GOLDEN, "pagerank.json")):  # the test module loads the goldens when it is imported: a first run starts from empty ones
        open(os.path.join(GOLDEN, "pagerank.json"), "w").write('{"graphs": {}, "records": []}\n')
        np.savez_compressed(os.path.join(GOLDEN, "pagerank.npz"))
    import test_pagerank_golden_cpu as T  # the restatement
    inputs = []
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            inputs.append(("file_" + name[:-3], {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name))))
    for kind, scale, deg, relabel in GENERATED:
        key = "%s_%d_%d%s" % (kind, scale, deg, "" if relabel else "_raw")
        inputs.append((key, {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": relabel},
                       capi.HostCSR.generate(kind, scale, deg, capi.RELABEL_AUTO if relabel else capi.RELABEL_NEVER)))
    graphs, records, arrays = {}, [], {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "pr_ref.cc"), os.path.join(tmp, "pr_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, "-o", exe], check=True)
        for key, source, csr in inputs:
            off, adj = np.array(csr.offsets(), dtype=np.int64), np.array(csr.neighbors(), dtype=np.int64)
            n, deg = off.size - 1, np.diff(off)
            assert n <= 4096
            dmax, isolated = int(deg.max()), int((deg == 0).sum())
            sg, out, cand = os.path.join(tmp, "g.sg"), os.path.join(tmp, "out.bin"), os.path.join(tmp, "cand.bin")
            csr.save_sg(sg)
            graphs[key] = {"source": source, "n": int(n), "nnz": int(adj.size), "max_degree": dmax, "isolated": isolated}
            for i, (damping, max_iters, tol, tkind, flags) in enumerate(CASES):
                scores, info, errors = T.pagerank_np(off, adj, damping, max_iters, tol, T.teleport_of(tkind, off), dangling=bool(flags & T.PR_DANGLING))
                bound = T.pr_bound(max_iters, damping, dmax, T.EPS, float32=bool(flags & T.PR_FLOAT32), isolated=isolated if flags & T.PR_DANGLING else None)
                if tol > 0:  # (c)
                    near = [e for e in errors if abs(e - tol) <= 4.0 * T.scalar_bound(bound, n, e)]
                    assert not near, (key, i, near, "choose another tolerance: never loosen the bound")
                compared = False
                if damping == 0.85 and tkind == "uniform" and not flags & T.PR_DANGLING:
                    scores.astype("<f4").tofile(cand)
                    txt = subprocess.run([exe, "-f", sg], check=True, capture_output=True, text=True,
                                         env=dict(os.environ, PR_ITERS=str(max_iters), PR_TOL=repr(tol), PR_CAND=cand, PR_OUT=out, OMP_NUM_THREADS="1")).stdout
                    f = [ln for ln in txt.splitlines() if ln.startswith("F ")][0].split()
                    assert (int(f[1]), int(f[2])) == csr.fingerprint(), "the reference loaded another CSR"
                    raw = open(out, "rb").read()
                    assert len(raw) == 4 * n + 2
                    ref = np.frombuffer(raw[:4 * n], dtype="<f4").astype(np.float64)
                    ref_bound = T.pr_bound(max_iters, damping, dmax, T.EPS32)
                    dist = float(np.abs(ref - scores).sum())
                    assert dist <= ref_bound, (key, i, dist, ref_bound)  # (a)
                    if info["converged"]:
                        assert raw[4 * n] == 1, "PRVerifier refused the reference's own scores"
                        assert raw[4 * n + 1] == 1, "PRVerifier refused the restatement's scores"  # (b)
                    compared = True
                    print(f"{key} case {i}: reference within {dist:.3e} (bound {ref_bound:.3e})", flush=True)
                rec = {"graph": key, "damping": damping, "max_iters": max_iters, "tolerance": tol, "teleport": tkind, "flags": flags,
                       "iterations": info["iterations"], "converged": info["converged"], "argmax": info["argmax"], "top": T.top_five(scores),
                       "error": info["error"], "sum": info["sum"], "reference": compared, "array": "pr_%s_%d" % (key, i)}
                arrays[rec["array"]] = scores
                records.append(rec)
                print(f"{key} case {i}: {info['iterations']} sweeps, converged {info['converged']}, error {info['error']:.3e}, sum {info['sum']:.6f}", flush=True)
    with open(os.path.join(GOLDEN, "pagerank.json"), "w") as fh:
        fh.write('{\n "graphs": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(graphs[k], sort_keys=True)}" for k in sorted(graphs)) + '\n },\n "records": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]\n}\n")
    np.savez_compressed(os.path.join(GOLDEN, "pagerank.npz"), **arrays)
    print("wrote", len(graphs), "graphs,", len(records), "records,", os.path.getsize(os.path.join(GOLDEN, "pagerank.npz")), "bytes of arrays")


if __name__ == "__main__":
    main()
