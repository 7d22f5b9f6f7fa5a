#!/usr/bin/env python3
"""Writes tests/golden/subgraph.json: what the REFERENCE's VF2 returns per (target, pattern), and the full lists of a plain enumerator — the
goldens of gmsx_subgraph_match / gmsx_subgraph_order.

Run on a machine that has the reference tree (REF, default /root/reference).  Two small programs of this project are compiled in a temporary
directory against the reference headers (they only #include them): one around the SEQUENTIAL VF2 (vf2/sequential/vf2.hpp), one around the
parallel one (vf2/parallel/vf2.hpp; the two headers define the same class, hence two programs).  Target and patterns are saved as .sg by this
project's loader and read back by the reference's own Builder (MakeGraph, as subgraphiso_vf2_sequential.cpp:24-32 does); per pattern a program
prints

  R <index> <pairs> <verified> <seconds> <target>:<pattern> ...   Result::isomorphism of VF2::run (empty = none) and the verdict of
                                                                     subgraphisomorphismVerification (util/subgraphiso_verification.hpp:11-78)

The parallel program runs once per pattern with 4 OpenMP threads; where that run crashes (its tasks write `success`, a local of a frame that
may have returned, vf2/parallel/vf2.hpp:86-100) it is repeated with one thread, where every task runs undeferred; ref_parallel_threads says
which run answered.  The tool asserts that the parallel program's existence answer equals the sequential one's, that the sequential mapping equals row 0 of its own
INDUCED enumeration, and that the matching order equals capi.subgraph_order.

The tool's own enumerator (enumerate_all below: level by level over the matching order, plain boolean algebra on the dense adjacency matrix, no
degree filter) gives, for INDUCED and MONO: the embedding count, row 0 and the sha256 of the whole list in list order (<i4, rows indexed by
pattern vertex).  A list is recorded only where no level of the enumeration holds more than LIST_LIMIT partial embeddings (MONO C8 in G(48, 0.5)
has ~10^10 embeddings): count and sha256 are null otherwise.  Row 0 (first_embedding below, a depth-first search of its own) is recorded for
every pair and mode.  Lists are never literal beyond row 0, so the file stays below 200 KB.

"graphs": every target's source (a fixture file, a generator call, or literal edges).  "patterns": name -> edges.  A record: graph, pattern,
order, ref (the sequential mapping as f(p) per pattern vertex p, or null), ref_verified, ref_parallel_found, ref_seconds, induced / mono =
{count, row0, sha256}."""
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
LIST_LIMIT = 200000

PROGRAM = r'''
#include "gms/third_party/gapbs/benchmark.h"
#include <gms/algorithms/non_set_based/subgraphiso/util/command_line.hpp>
#include <gms/algorithms/non_set_based/subgraphiso/util/subgraphiso_verification.hpp>
#ifdef SGM_PARALLEL
#include <gms/algorithms/non_set_based/subgraphiso/vf2/parallel/vf2.hpp>
#else
#include <gms/algorithms/non_set_based/subgraphiso/vf2/sequential/vf2.hpp>
#endif
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace GMS;
using namespace GMS::SubGraphIso;

int main(int argc, char **argv) {
    SubGraphIsoCLApp cli = subgraph_iso_parse_args(argc, argv);
    Builder b(cli);
    CSRGraph target = b.MakeGraph();
    std::printf("T %lld %lld\n", (long long)target.num_nodes(), (long long)target.num_edges_directed());
    std::vector<std::string> paths;
    std::string cur;
    for (const char *p = std::getenv("SGM_PATTERNS");; ++p) {
        if (*p == ',' || *p == 0) { if (!cur.empty()) paths.push_back(cur); cur.clear(); if (!*p) break; }
        else cur.push_back(*p);
    }
    for (size_t i = 0; i < paths.size(); ++i) {
        Builder b2(cli);
        CSRGraph pattern = b2.MakeGraph(paths[i]);
        const auto t0 = std::chrono::steady_clock::now();
        VF2 solver(target, pattern);
        Result r = solver.run();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const bool pass = subgraphisomorphismVerification(r, target, pattern);
        std::printf("R %zu %zu %d %.6f", i, r.isomorphism.size(), pass ? 1 : 0, secs);
        for (auto pr : r.isomorphism) std::printf(" %d:%d", pr.first, pr.second);
        std::printf("\n");
        std::fflush(stdout);
    }
    return 0;
}
'''


def path_edges(vs):
    return [(vs[i], vs[i + 1]) for i in range(len(vs) - 1)]


def relabel(edges, perm):
    return [(perm[a], perm[b]) for a, b in edges]


HOUSE = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 4)]
PATTERNS = {
    "K2": [(0, 1)],
    "P3": path_edges([0, 1, 2]),
    "K3": [(0, 1), (0, 2), (1, 2)],
    "P4": path_edges([0, 1, 2, 3]),
    "claw": [(0, 1), (0, 2), (0, 3)],
    "C4": [(0, 1), (1, 2), (2, 3), (3, 0)],
    "paw": [(0, 1), (0, 2), (1, 2), (2, 3)],
    "diamond": [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)],
    "K4": [(a, b) for a in range(4) for b in range(a + 1, 4)],
    "C5": [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)],
    "house": HOUSE,
    "bull": [(0, 1), (0, 2), (1, 2), (1, 3), (2, 4)],
    "P5": path_edges([0, 1, 2, 3, 4]),
    "K5": [(a, b) for a in range(5) for b in range(a + 1, 5)],
    "C8": [(i, (i + 1) % 8) for i in range(8)],
    # vertex 0 an inner vertex: the matching order is not the identity
    "P4_r1": path_edges([2, 0, 3, 1]),
    "P4_r2": path_edges([3, 0, 2, 1]),
    "house_r1": relabel(HOUSE, [3, 0, 4, 1, 2]),
    "house_r2": relabel(HOUSE, [2, 4, 0, 3, 1]),
}
PETERSEN = [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]


def gnp(n, p, seed):
    r = np.random.RandomState(seed).random_sample((n, n))
    return [(a, b) for a in range(n) for b in range(a + 1, n) if r[a, b] < p]


def matching_order(pa):
    k = pa.shape[0]
    order, inside = [0], {0}
    while len(order) < k:
        order.append(min(v for v in range(k) if v not in inside and any(pa[v, u] for u in order)))
        inside.add(order[-1])
    return order


def dense(edges, n):
    a = np.zeros((n, n), dtype=bool)
    for u, v in edges:
        a[u, v] = a[v, u] = True
    return a


def enumerate_all(A, pa, order, induced, limit):
    """every embedding, rows indexed by pattern vertex, in list order; None when a level exceeds `limit` rows"""
    n, k = A.shape[0], pa.shape[0]
    if k > n:
        return np.zeros((0, k), dtype=np.int32)
    rows = np.arange(n, dtype=np.int64)[:, None]
    for i in range(1, k):
        cand = np.ones((rows.shape[0], n), dtype=bool)
        for j in range(i):
            col = rows[:, j]
            if pa[order[i], order[j]]:
                cand &= A[col]
            elif induced:
                cand &= ~A[col]
            cand[np.arange(rows.shape[0]), col] = False
        r, w = np.nonzero(cand)
        rows = np.concatenate([rows[r], w[:, None]], axis=1)
        if rows.shape[0] > limit:
            return None
    out = np.zeros((rows.shape[0], k), dtype=np.int32)
    out[:, order] = rows
    return out


def first_embedding(A, pa, order, induced):
    """the first embedding of a depth-first search over the matching order, target vertices ascending; None if there is none"""
    n, k = A.shape[0], pa.shape[0]
    img = []

    def go(i):
        if i == k:
            return True
        cand = np.ones(n, dtype=bool)
        for j in range(i):
            if pa[order[i], order[j]]:
                cand &= A[img[j]]
            elif induced:
                cand &= ~A[img[j]]
            cand[img[j]] = False
        for w in np.nonzero(cand)[0]:
            img.append(int(w))
            if go(i + 1):
                return True
            img.pop()
        return False

    if k > n or not go(0):
        return None
    out = [0] * k
    for i, p in enumerate(order):
        out[p] = img[i]
    return out


def csr_of(edges, n):
    e = np.array(edges, dtype=np.int32).reshape(-1, 2)
    return capi.HostCSR.from_edges(e[:, 0], e[:, 1], num_nodes=n)


def parse(txt):
    out, shape = {}, None
    for ln in txt.splitlines():
        t = ln.split()
        if t and t[0] == "T":
            shape = (int(t[1]), int(t[2]))
        elif t and t[0] == "R":
            out[int(t[1])] = (int(t[2]), bool(int(t[3])), float(t[4]), [tuple(int(x) for x in p.split(":")) for p in t[5:]])
    return shape, out


def main():
    if not os.path.isdir(os.path.join(REF, "gms")):
        sys.exit(f"needs the reference tree at {REF}")
    graphs, targets = {}, []
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            csr = capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name), relabel=capi.RELABEL_NEVER)
            graphs["file_" + name[:-3]] = {"kind": "file", "name": name}
            targets.append(("file_" + name[:-3], csr))
    for key, n, p, seed in (("gnp_48_15", 48, 0.15, 20261019), ("gnp_48_50", 48, 0.5, 20261020)):
        edges = gnp(n, p, seed)
        graphs[key] = {"kind": "edges", "n": n, "p": p, "seed": seed, "edges": edges}
        targets.append((key, csr_of(edges, n)))
    for kind in ("kronecker", "uniform"):
        key = "%s_8_8" % kind
        graphs[key] = {"kind": "generated", "generator": kind, "scale": 8, "degree": 8, "relabel": False}
        targets.append((key, capi.HostCSR.generate(kind, 8, 8, capi.RELABEL_NEVER)))
    graphs["petersen"] = {"kind": "edges", "n": 10, "edges": PETERSEN}
    targets.append(("petersen", csr_of(PETERSEN, 10)))

    names = list(PATTERNS)
    pas = {nm: dense(PATTERNS[nm], max(max(e) for e in PATTERNS[nm]) + 1) for nm in names}
    orders = {nm: matching_order(pas[nm]) for nm in names}
    for nm in names:
        assert orders[nm] == capi.subgraph_order(PATTERNS[nm]).tolist(), nm
        if "_r" in nm:
            assert orders[nm] != list(range(len(orders[nm]))), nm
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sgm_ref.cc")
        open(src, "w").write(PROGRAM)
        exes = {}
        for mode, define in (("seq", []), ("par", ["-DSGM_PARALLEL"])):
            exes[mode] = os.path.join(tmp, "sgm_ref_" + mode)
            subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF] + define + [src, "-o", exes[mode]], check=True)
        ppaths = []
        for i, nm in enumerate(names):
            ppaths.append(os.path.join(tmp, "p%d.sg" % i))
            csr_of(PATTERNS[nm], pas[nm].shape[0]).save_sg(ppaths[-1])
        for key, csr in targets:
            n = csr.num_nodes
            graphs[key].update(n=int(n), nnz=int(csr.nnz))
            off, adj = np.array(csr.offsets()), np.array(csr.neighbors())
            A = np.zeros((n, n), dtype=bool)
            A[np.repeat(np.arange(n), np.diff(off)), adj] = True
            assert np.array_equal(A, A.T) and not A.diagonal().any()
            tpath = os.path.join(tmp, "t.sg")
            csr.save_sg(tpath)
            def run_ref(mode, paths, threads):
                env = dict(os.environ, SGM_PATTERNS=",".join(paths), OMP_NUM_THREADS=str(threads))
                r = subprocess.run([exes[mode], "-f", tpath, "-p", "pattern-file=" + paths[0]], capture_output=True, text=True, env=env)
                if r.returncode != 0:
                    return None
                shape, out = parse(r.stdout)
                assert shape == (n, csr.nnz) and len(out) == len(paths), (key, shape)
                return out

            res = {"seq": run_ref("seq", ppaths, 1), "par": {}}
            assert res["seq"] is not None
            par_threads = {}
            for i, p in enumerate(ppaths):  # one process per pattern: the parallel driver's tasks write to a local of a frame that has returned
                for threads in (4, 1):     # (vf2/parallel/vf2.hpp:86-100) and can crash; with one thread every task runs undeferred
                    out = run_ref("par", [p], threads)
                    if out is not None:
                        res["par"][i], par_threads[i] = out[0], threads
                        break
                assert i in res["par"], (key, names[i])
            secs_total = 0.0
            for i, nm in enumerate(names):
                pa, order = pas[nm], orders[nm]
                k = pa.shape[0]
                size, verified, secs, pairs = res["seq"][i]
                ref = None
                if size:
                    assert size == k and sorted(p for _, p in pairs) == list(range(k))
                    ref = [0] * k
                    for tv, pv in pairs:  # Result::isomorphism: key = target vertex, value = pattern vertex
                        ref[pv] = tv
                assert (res["par"][i][0] > 0) == (size > 0), (key, nm)
                assert verified and res["par"][i][1], (key, nm)
                rec = {"graph": key, "pattern": nm, "order": order, "ref": ref, "ref_verified": verified,
                       "ref_parallel_found": res["par"][i][0] > 0, "ref_parallel_threads": par_threads[i], "ref_seconds": round(secs, 6)}
                for mode, induced in (("induced", True), ("mono", False)):
                    row0 = first_embedding(A, pa, order, induced)
                    lst = enumerate_all(A, pa, order, induced, LIST_LIMIT)
                    ent = {"count": None, "row0": row0, "sha256": None}
                    if lst is not None:
                        assert (lst.shape[0] == 0) == (row0 is None) and (row0 is None or lst[0].tolist() == row0)
                        ent.update(count=int(lst.shape[0]), sha256=hashlib.sha256(np.ascontiguousarray(lst, dtype="<i4").tobytes()).hexdigest())
                    rec[mode] = ent
                assert rec["induced"]["row0"] == ref, (key, nm, rec["induced"]["row0"], ref)
                records.append(rec)
                secs_total += secs
            print(f"{key}: n {n}, nnz {csr.nnz}, {len(names)} patterns, reference sequential VF2 {secs_total:.3f} s", flush=True)
    path = os.path.join(GOLDEN, "subgraph.json")
    with open(path, "w") as fh:
        fh.write('{\n "list_limit": %d,\n "graphs": ' % LIST_LIMIT + json.dumps(graphs, sort_keys=True, separators=(",", ":")) + ',\n "patterns": ' +
                 json.dumps(PATTERNS, sort_keys=True, separators=(",", ":")) + ',\n "records": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True, separators=(",", ":")) for r in records) + "\n ]\n}\n")
    size = os.path.getsize(path)
    assert size <= 200 * 1024, size
    print("wrote", len(records), "records,", size, "bytes")


if __name__ == "__main__":
    main()
