#!/usr/bin/env python3
"""Writes tests/golden/core_orders.json and tests/golden/core_orders.npz: what the REFERENCE says about exact degeneracy, the degree order
and the quality of an order, per test graph — the goldens of gmsx_core_decomposition / gmsx_degree_rank / gmsx_order_quality.

Run on a machine that has the reference tree (REF, default /root/reference) and its compiled CRoaring (oracle/_ref/roaring.o: `make -C
oracle`).  A small program of this project is compiled in a temporary directory against the reference headers (it only #includes them);
every graph is saved as .sg by this project's loader and read back by the reference's own reader into a RoaringGraph (the SortedSetGraph
instantiation of Matula's loop is the quadratic one), and the program prints the CSR's fingerprints and writes its results into a binary file:

  matula     PpSequential::getDegeneracyOrderingMatula<RoaringGraph, rank format> (preprocessing/sequential/degeneracy_matula.h:13-66) + its wall time
  degeneracy CoreNumberEvaluator::getCoreNumberOfOrder(matula) (util/core_number_evaluator.h:115-139), and for n <= 2^10 additionally the naive
             DegeneracyOrderingVerifier::getDegeneracy (verifiers/degeneracy_verifier.h:39-67)
  degrank    PpParallel::getDegreeOrdering<RoaringGraph, rank format> (parallel/degree.h:15-61)
  quality    CoreNumberEvaluator::evaluateCoreNrAccuracy<rank format>(order, graph, degeneracy) (:73-112): the five CoreNumberInfo fields, for the degree
             order, the Matula order and — where tests/golden/orderings.npz has the key adg_<graph> and that rank belongs to this CSR — the
             reference's own `-t 1` ADG rank

Derived here, in numpy, and cross-checked against the above before anything is written: the core numbers (the running maximum of the
removal degrees along the Matula order; the removal degree of v = its neighbours after it), and per order the integers behind the three
doubles — faulty (vertices with more later neighbours than the degeneracy) and excess (the sum of the surplus); the doubles must be the
reference's expressions on those integers, bit for bit.

The arrays go into the .npz literally for n <= 2^14 (keys matula_<graph>, core_<graph>, degrank_<graph>); above that the JSON carries the
sha256 of the <i4 core-number array.  --largest S (18 or 20; default 20) also runs kronecker S beside kronecker 16."""
import argparse
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
MAX_LITERAL_N = 1 << 14
NAIVE_MAX_N = 1 << 10

PROGRAM = r'''
#include "gms/third_party/gapbs/benchmark.h"
#include <gms/common/cli/cli.h>
#include <gms/common/types.h>
#include <gms/representations/graphs/set_graph.h>
#include <gms/algorithms/preprocessing/preprocessing.h>
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
static void print_info(const char *tag, const CoreNumberEvaluator::CoreNumberInfo &ci) {
    std::printf("Q %s %zu %zu %a %a %a\n", tag, ci.coreNumberOfOrder, ci.coreNumber, ci.relativeError, ci.faultRate, ci.relativeMeanDifference);
}

int main(int argc, char **argv) {
    const char *out_path = std::getenv("CORE_OUT");
    const char *adg_path = std::getenv("CORE_ADG");  // n int32: an ADG rank to grade, or unset
    const long naive_max = std::atol(std::getenv("CORE_NAIVE_MAX"));
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
    std::vector<NodeId> matula(n), degrank(n);
    const auto t0 = std::chrono::steady_clock::now();
    PpSequential::getDegeneracyOrderingMatula<RoaringGraph, true>(sg, matula);
    std::printf("T %.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    PpParallel::getDegreeOrdering<RoaringGraph, true>(sg, degrank);
    const size_t degeneracy = CoreNumberEvaluator::getCoreNumberOfOrder<true>(matula, sg);
    long naive = -1;
    if (n <= naive_max) naive = long(DegeneracyOrderingVerifier::getDegeneracy(RoaringGraph::FromCGraph(g)));  // (by value: it erases the graph)
    std::printf("D %zu %ld\n", degeneracy, naive);
    print_info("degree", CoreNumberEvaluator::evaluateCoreNrAccuracy<true>(degrank, sg, degeneracy));
    print_info("matula", CoreNumberEvaluator::evaluateCoreNrAccuracy<true>(matula, sg, degeneracy));
    if (adg_path) {
        std::vector<NodeId> adg(n);
        std::FILE *f = std::fopen(adg_path, "rb");
        if (!f || std::fread(adg.data(), 4, size_t(n), f) != size_t(n)) return 9;
        std::fclose(f);
        print_info("adg", CoreNumberEvaluator::evaluateCoreNrAccuracy<true>(adg, sg, degeneracy));
    }
    static_assert(sizeof(NodeId) == 4, "ids are 32-bit");
    std::FILE *f = std::fopen(out_path, "wb");
    if (!f) return 8;
    std::fwrite(matula.data(), 4, size_t(n), f);
    std::fwrite(degrank.data(), 4, size_t(n), f);
    return std::fclose(f) == 0 ? 0 : 8;
}
'''


def later_counts(off, adj, rank):
    """later[v] = |{w in N(v): rank[w] > rank[v]}|"""
    n = off.size - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    return np.bincount(src[rank[adj] > rank[src]], minlength=n).astype(np.int64)


def quality_ints(later, cn):
    over = later > cn
    return {"max_later": int(later.max()) if later.size else 0, "faulty": int(over.sum()), "excess": int((later[over] - cn).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--largest", type=int, default=20, choices=(0, 18, 20))
    opts = ap.parse_args()
    roaring = os.path.join(ROOT, "oracle", "_ref", "roaring.o")
    if not os.path.isdir(os.path.join(REF, "gms")) or not os.path.exists(roaring):
        sys.exit(f"needs the reference tree at {REF} and {roaring} (make -C oracle)")
    oracle = Oracle()
    adg_golden = np.load(os.path.join(GOLDEN, "orderings.npz"))
    inputs = []  # (key, source, csr)
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            inputs.append(("file_" + name[:-3], {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name))))
    specs = [("kronecker", 8, 16), ("kronecker", 10, 16), ("kronecker", 12, 16), ("kronecker", 14, 16), ("kronecker", 12, 4), ("uniform", 12, 16),
             ("kronecker", 16, 16)]
    if opts.largest:
        specs.append(("kronecker", opts.largest, 16))
    for kind, scale, deg in specs:
        inputs.append(("%s_%d_%d" % (kind, scale, deg), {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": True},
                       capi.HostCSR.generate(kind, scale, deg, capi.RELABEL_AUTO)))
    meta, arrays = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "core_ref.cc"), os.path.join(tmp, "core_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, roaring, "-o", exe], check=True)
        for key, source, csr in inputs:
            off, adj = np.array(csr.offsets()), np.array(csr.neighbors())
            n = off.size - 1
            sg, binf, adgf = os.path.join(tmp, "g.sg"), os.path.join(tmp, "out.bin"), os.path.join(tmp, "adg.bin")
            csr.save_sg(sg)
            env = dict(os.environ, CORE_OUT=binf, CORE_NAIVE_MAX=str(NAIVE_MAX_N))
            env.pop("CORE_ADG", None)
            adg = None
            if "adg_" + key in adg_golden:
                adg = np.ascontiguousarray(adg_golden["adg_" + key], dtype=np.int32)
                # the golden rank was taken on the reference's own CSR: it is graded only if it is an ADG order of THIS one (the oracle's staircase)
                _, rnd, dat, _ = oracle.adg_rank(off, adj, 0.001)
                ok = adg.size == n and np.array_equal(np.sort(adg), np.arange(n))
                if ok:
                    by = np.argsort(adg)
                    ok = bool(np.all(np.diff(rnd[by].astype(np.int64) * (1 << 32) + dat[by]) >= 0))
                if ok:
                    adg.astype("<i4").tofile(adgf)
                    env["CORE_ADG"] = adgf
                else:
                    print(f"{key}: orderings.npz's adg rank is not an ADG order of this CSR — not graded", flush=True)
                    adg = None
            txt = subprocess.run([exe, "-f", sg], check=True, capture_output=True, text=True, env=env).stdout
            lines = txt.splitlines()
            f = [ln for ln in lines if ln.startswith("F ")][0].split()
            assert (int(f[1]), int(f[2])) == csr.fingerprint(), f"{key}: the reference loaded another CSR"
            secs = float([ln for ln in lines if ln.startswith("T ")][0].split()[1])
            d = [ln for ln in lines if ln.startswith("D ")][0].split()
            degeneracy, naive = int(d[1]), int(d[2])
            raw = np.fromfile(binf, dtype="<i4")
            assert raw.size == 2 * n
            matula, degrank = raw[:n].astype(np.int32), raw[n:].astype(np.int32)
            assert np.array_equal(np.sort(matula), np.arange(n)) and np.array_equal(np.sort(degrank), np.arange(n))
            # core numbers: the running maximum of the removal degrees along Matula's order
            later = later_counts(off, adj, matula)
            by = np.argsort(matula)
            core = np.empty(n, dtype=np.int32)
            core[by] = np.maximum.accumulate(later[by]).astype(np.int32) if n else 0
            assert (int(core.max()) if n else 0) == degeneracy and (naive < 0 or naive == degeneracy), (key, degeneracy, naive)
            rec = {"source": source, "n": int(n), "nnz": int(adj.size), "degeneracy": degeneracy, "naive_degeneracy": naive if naive >= 0 else None,
                   "levels": int(np.unique(core).size), "top_core": int((core == degeneracy).sum()), "matula_seconds": secs,
                   "core_sha256": hashlib.sha256(np.ascontiguousarray(core, dtype="<i4").tobytes()).hexdigest(), "literal": bool(n <= MAX_LITERAL_N),
                   "quality": {}}
            for tag, rank in (("degree", degrank), ("matula", matula), ("adg", adg)):
                if rank is None:
                    continue
                q = [ln for ln in lines if ln.startswith("Q " + tag + " ")][0].split()
                ref = {"core_number_of_order": int(q[2]), "core_number": int(q[3]), "relative_error": float.fromhex(q[4]),
                       "fault_rate": float.fromhex(q[5]), "relative_mean_difference": float.fromhex(q[6])}
                ints = quality_ints(later_counts(off, adj, rank), degeneracy)
                assert ref["core_number"] == degeneracy and ref["core_number_of_order"] == max(degeneracy, ints["max_later"]), (key, tag)
                assert ints["excess"] < 2 ** 32  # (the reference's difAcc is an unsigned int)
                assert ref["relative_error"] == (ref["core_number_of_order"] - degeneracy) / float(degeneracy), (key, tag)
                assert ref["fault_rate"] == float(ints["faulty"]) / float(n), (key, tag)
                assert ref["relative_mean_difference"] == (0.0 if ints["faulty"] == 0 else (float(ints["excess"]) / float(ints["faulty"])) / float(degeneracy))
                rec["quality"][tag] = dict(ref, **ints)
            meta[key] = rec
            if n <= MAX_LITERAL_N:
                arrays["matula_" + key], arrays["core_" + key], arrays["degrank_" + key] = matula, core, degrank
            print(f"{key}: n {n}, degeneracy {degeneracy}, levels {rec['levels']}, top core {rec['top_core']}; reference Matula {secs:.3f} s; "
                  + ", ".join(f"{t} order: {v['core_number_of_order']}" for t, v in rec["quality"].items()), flush=True)
    with open(os.path.join(GOLDEN, "core_orders.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(key)}: {json.dumps(meta[key], sort_keys=True)}" for key in sorted(meta)) + "\n}\n")  # a record per line
    np.savez_compressed(os.path.join(GOLDEN, "core_orders.npz"), **arrays)
    print("wrote", len(meta), "records,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
