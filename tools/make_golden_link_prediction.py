#!/usr/bin/env python3
"""Writes tests/golden/link_prediction.json: what the REFERENCE's link prediction returns, per test graph, metric and q — the goldens of
gmsx_link_prediction / gmsx_link_prediction_precision.

Run on a machine that has the reference tree (REF, default /root/reference) and its compiled CRoaring (oracle/_ref/roaring.o: `make -C
oracle`).  A small program of this project is compiled in a temporary directory against the reference headers (it only #includes them);
every graph is saved as .sg by this project's loader and read back by the reference's own reader into a RoaringGraph (what bench_ranking
uses, link_prediction.cc:30), and the program prints

  R <metric> <q> <size> <seconds>   GMS::LinkPrediction::link_prediction_similarity<Metric>(graph, q) (link_prediction.h:42-101), then its
  E <u> <v> <score as hex float>    `size` entries verbatim, padding included
  P <metric> <q> <precision> <recall>  score_link_prediction_precision (evaluation.h:99-124) of the Jaccard and the CommonNeighbors prediction on a train graph against
                                    the test edges of a fixed split (a seeded numpy permutation of the edges; the reference's own sampler
                                    depends on the OpenMP thread count)

for the seven metrics and q in {1, 7, 100, 2000}.  Adamic-Adar and Resource sum their terms in an order the device does not repeat, so a
test can compare them only up to a tolerance; for every record of these two the generator ASSERTS a separation condition and lowers q until
it holds: the reference's q-th and (q+1)-th scores differ by more than 1e-9 relative, and no two distinct scores among the kept ones are
closer than that; where not even q = 1 satisfies it (the best scores tie) q is raised to the first value that does.  (The scores behind
the q-th come from one longer run.)

"graphs" holds every graph's source, n and nnz.  A record: graph, metric, q_requested, q, padding (leading (-1.0, (0,0)) entries; 1 when nothing qualifies), found, sha256 of the
real entries (u as <i4, v as <i4, scores as <f8, concatenated) and the entries themselves, worst first: literally (u, v, scores_rle = runs of
[hex float, count]) up to 128 of them; for longer Adamic-Adar / Resource records packed (edges_z: base64 of zlib of the <i4 (u, v) rows; scores_z:
base64 of zlib of the <u8 differences of consecutive order-preserving score images — the scores ascend —, first difference from 0); longer
records of the count-based metrics carry the sha256 only: they are compared byte for byte, which the hash does as well, and the file stays
below 200 KB."""
import base64
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gms_amd import capi  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
METRICS = ["jaccard", "overlap", "adamic_adar", "resource", "common", "total", "prefatt"]
TOLERANT = ("adamic_adar", "resource")
QS = [1, 7, 100, 2000]
LITERAL_MAX = 128
SEPARATION = 1e-9
SPLIT = {"generator": "kronecker", "scale": 10, "degree": 8, "relabel": False, "seed": 20261017, "test_fraction": 0.25}

PROGRAM = r'''
#include "gms/third_party/gapbs/benchmark.h"
#include <gms/common/cli/cli.h>
#include <gms/common/types.h>
#include <gms/representations/graphs/set_graph.h>
#include <gms/algorithms/set_based/link_prediction/evaluation.h>
#include <gms/algorithms/set_based/link_prediction/link_prediction.h>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace GMS;
using namespace GMS::VertexSim;
using namespace GMS::LinkPrediction;

static uint64_t fnv(const unsigned char *p, size_t len) {
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < len; ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}
template <Metric M>
static void run(const RoaringGraph &g, int idx, int64_t q) {
    const auto t0 = std::chrono::steady_clock::now();
    ScoredEdges se = link_prediction_similarity<M>(g, q);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("R %d %lld %zu %.6f\n", idx, (long long)q, se.edges.size(), secs);
    for (size_t i = 0; i < se.edges.size(); ++i) std::printf("E %d %d %a\n", int(se.edges[i].first), int(se.edges[i].second), se.scores[i]);
}
static std::vector<int64_t> numbers(const char *s) {
    std::vector<int64_t> out;
    if (!s) return out;
    std::string cur;
    for (const char *p = s;; ++p) {
        if (*p == ',' || *p == 0) { if (!cur.empty()) out.push_back(std::atoll(cur.c_str())); cur.clear(); if (!*p) break; }
        else cur.push_back(*p);
    }
    return out;
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
    const std::vector<int64_t> metrics = numbers(std::getenv("LP_METRICS")), qs = numbers(std::getenv("LP_QS"));
    for (int64_t m : metrics)
        for (int64_t q : qs) {
            switch (int(m)) {
                case 0: run<Metric::Jaccard>(sg, 0, q); break;
                case 1: run<Metric::Overlap>(sg, 1, q); break;
                case 2: run<Metric::AdamicAdar>(sg, 2, q); break;
                case 3: run<Metric::Resource>(sg, 3, q); break;
                case 4: run<Metric::CommNeigh>(sg, 4, q); break;
                case 5: run<Metric::TotalNeigh>(sg, 5, q); break;
                default: run<Metric::PrefAtt>(sg, 6, q); break;
            }
        }
    if (const char *test_path = std::getenv("LP_TEST")) {  // <i4 pairs: the test edges; the loaded graph is the train graph
        std::FILE *f = std::fopen(test_path, "rb");
        if (!f) return 9;
        std::vector<int32_t> e;
        int32_t pair[2];
        while (std::fread(pair, 4, 2, f) == 2) { e.push_back(pair[0]); e.push_back(pair[1]); }
        std::fclose(f);
        RoaringGraph g_test(n);
        for (size_t i = 0; i < e.size(); i += 2) add_undirected_edge(g_test, e[i], e[i + 1]);
        const int64_t q = int64_t(e.size() / 2);
        using EdgeSet = SortedSetBase<UndirectedEdge>;
        for (int m : {0, 4}) {  // Jaccard (bench_ranking's choice, link_prediction.cc:36) and CommonNeighbors
            ScoredEdges scoring = m == 0 ? link_prediction_similarity<Metric::Jaccard>(sg, q) : link_prediction_similarity<Metric::CommNeigh>(sg, q);
            EdgeSet predicted(scoring.edges.data(), scoring.edges.size());
            const LinkPredictionScore score = score_link_prediction_precision(predicted, g_test);
            std::printf("P %d %lld %a %a\n", m, (long long)q, score.precision, score.recall);
        }
    }
    return 0;
}
'''


def image(scores):
    """the order-preserving 64-bit image of float64 scores (linkpred.hip: score_image)"""
    b = np.ascontiguousarray(scores, dtype="<f8").view("<u8")
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def pack(u, v, s):
    edges = np.ascontiguousarray(np.stack([u, v], axis=1), dtype="<i4").tobytes()
    img = image(s)
    assert np.all(img[1:] >= img[:-1])
    diffs = np.diff(np.concatenate([np.zeros(1, dtype=np.uint64), img])).astype("<u8").tobytes()
    return base64.b64encode(zlib.compress(edges, 9)).decode(), base64.b64encode(zlib.compress(diffs, 9)).decode()


def rle(s):
    """[[hex float, count], ...]: the runs of equal scores"""
    out = []
    for x in s:
        h = float(x).hex()
        if out and out[-1][0] == h:
            out[-1][1] += 1
        else:
            out.append([h, 1])
    return out


def digest(u, v, s):
    return hashlib.sha256(np.ascontiguousarray(u, dtype="<i4").tobytes() + np.ascontiguousarray(v, dtype="<i4").tobytes() +
                          np.ascontiguousarray(s, dtype="<f8").tobytes()).hexdigest()


def separated(s_kept, s_next):
    """s_kept ascending (worst first), s_next = the (q+1)-th score or None"""
    d = np.unique(s_kept)
    if d.size > 1 and np.any(np.diff(d) <= SEPARATION * np.abs(d[1:])):
        return False
    return s_next is None or abs(s_kept[0] - s_next) > SEPARATION * abs(s_kept[0])


def parse(txt):
    """{(metric idx, q): (seconds, u, v, scores)} and the P line"""
    out, prec, cur = {}, None, None
    for ln in txt.splitlines():
        t = ln.split()
        if t[0] == "R":
            cur = (int(t[1]), int(t[2]))
            out[cur] = [float(t[4]), [], [], [], int(t[3])]
        elif t[0] == "E":
            out[cur][1].append(int(t[1]))
            out[cur][2].append(int(t[2]))
            out[cur][3].append(float.fromhex(t[3]))
        elif t[0] == "P":
            prec = (prec or []) + [(int(t[1]), int(t[2]), float.fromhex(t[3]), float.fromhex(t[4]))]
    for k, r in out.items():
        assert len(r[1]) == r[4], k
        out[k] = (r[0], np.array(r[1], dtype=np.int32), np.array(r[2], dtype=np.int32), np.array(r[3], dtype=np.float64))
    return out, prec


def strip(u, v, s):
    """(padding, real u, v, s): the leading (-1.0, (0,0)) entries off"""
    pad = 0
    while pad < s.size and s[pad] == -1.0:
        assert u[pad] == 0 and v[pad] == 0
        pad += 1
    return pad, u[pad:], v[pad:], s[pad:]


def main():
    roaring = os.path.join(ROOT, "oracle", "_ref", "roaring.o")
    if not os.path.isdir(os.path.join(REF, "gms")) or not os.path.exists(roaring):
        sys.exit(f"needs the reference tree at {REF} and {roaring} (make -C oracle)")
    inputs = []
    for name in sorted(os.listdir(os.path.join(GOLDEN, "testGraphs"))):
        if name.endswith(".el"):
            inputs.append(("file_" + name[:-3], {"kind": "file", "name": name}, capi.HostCSR.load(os.path.join(GOLDEN, "testGraphs", name))))
    for kind, scale, deg in (("kronecker", 8, 4), ("kronecker", 10, 8), ("uniform", 8, 4)):
        inputs.append(("%s_%d_%d" % (kind, scale, deg), {"kind": "generated", "generator": kind, "scale": scale, "degree": deg, "relabel": False},
                       capi.HostCSR.generate(kind, scale, deg, capi.RELABEL_NEVER)))
    records, graphs, precision = [], {}, []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lp_ref.cc"), os.path.join(tmp, "lp_ref")
        open(src, "w").write(PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-w", "-DNOPAPIW", "-I", REF, src, roaring, "-o", exe], check=True)

        def run_ref(csr, metrics, qs, test=None):
            sg = os.path.join(tmp, "g.sg")
            csr.save_sg(sg)
            env = dict(os.environ, LP_METRICS=",".join(str(m) for m in metrics), LP_QS=",".join(str(q) for q in qs))
            env.pop("LP_TEST", None)
            if test is not None:
                env["LP_TEST"] = test
            txt = subprocess.run([exe, "-f", sg], check=True, capture_output=True, text=True, env=env).stdout
            f = [ln for ln in txt.splitlines() if ln.startswith("F ")][0].split()
            assert (int(f[1]), int(f[2])) == csr.fingerprint(), "the reference loaded another CSR"
            return parse("\n".join(ln for ln in txt.splitlines() if ln[:2] in ("R ", "E ", "P ")))

        for key, source, csr in inputs:
            n = csr.num_nodes
            exact = [i for i, m in enumerate(METRICS) if m not in TOLERANT]
            res, _ = run_ref(csr, exact, QS)
            final = {}
            for (mi, q), r in res.items():
                final[(mi, q, q)] = r
            for mi in (METRICS.index(m) for m in TOLERANT):
                for q_req in QS:
                    probe, _ = run_ref(csr, [mi], [2 * q_req + 64])
                    _, pu, pv, ps = probe[(mi, 2 * q_req + 64)]
                    pad, pu, pv, ps = strip(pu, pv, ps)

                    def holds(q):  # the top q is the suffix of any longer top list
                        return separated(ps[-q:] if ps.size >= q else ps, ps[-q - 1] if ps.size > q else None)
                    # (The condition is judged on the 2 q + 64 best scores of ONE longer run: a near-tie among the kept scores rules a q out, so the q
                    # a request ends at depends on where such near-ties lie, not monotonically on the request — uniform_8_4 / resource: 7 -> 3, 100 -> 98,
                    # 2000 -> 369 — and a wider window can only matter where q is raised.)
                    # q is lowered until the condition holds; where not even q = 1 is separated (the best scores tie) it is raised instead to the
                    # first q above that is: every (graph, metric, q_requested) keeps a record
                    q = next((c for c in range(q_req, 0, -1) if holds(c)), None)
                    if q is None:
                        q = next(c for c in range(q_req + 1, q_req + 64) if holds(c))
                    got, _ = run_ref(csr, [mi], [q])
                    final[(mi, q_req, q)] = got[(mi, q)]
            graphs[key] = {"source": source, "n": int(n), "nnz": int(csr.nnz)}
            secs_total = 0.0
            for (mi, q_req, q), (secs, u, v, s) in sorted(final.items()):
                pad, ru, rv, rs = strip(u, v, s)
                found = int(rs.size)
                assert (pad == q - found) if found else (pad == 1 and u.size == 1), (key, METRICS[mi], q)
                assert np.all(ru < rv) and np.all(np.diff(rs) >= 0)
                rec = {"graph": key, "metric": METRICS[mi], "q_requested": q_req, "q": q, "padding": pad, "found": found,
                       "sha256": digest(ru, rv, rs)}
                if found <= LITERAL_MAX:
                    rec.update(form="literal", u=ru.tolist(), v=rv.tolist(), scores_rle=rle(rs))
                elif METRICS[mi] in TOLERANT:
                    ez, sz = pack(ru, rv, rs)
                    rec.update(form="packed", edges_z=ez, scores_z=sz)
                else:
                    rec.update(form="sha256")
                records.append(rec)
                secs_total += secs
            print(f"{key}: n {n}, {len(final)} records, reference wall time {secs_total:.3f} s (largest q: "
                  f"{max(r[0] for r in final.values()):.3f} s)", flush=True)

        # the fixed split behind the precision golden
        csr = capi.HostCSR.generate(SPLIT["generator"], SPLIT["scale"], SPLIT["degree"], capi.RELABEL_NEVER)
        off, adj = np.array(csr.offsets()), np.array(csr.neighbors())
        n = off.size - 1
        src_v = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
        keep = src_v < adj
        eu, ev = src_v[keep].astype(np.int32), adj[keep].astype(np.int32)
        perm = np.random.RandomState(SPLIT["seed"]).permutation(eu.size)
        n_test = int(SPLIT["test_fraction"] * eu.size)
        te, tr = perm[:n_test], perm[n_test:]
        train = capi.HostCSR.from_edges(eu[tr], ev[tr], num_nodes=n)
        testf = os.path.join(tmp, "test.bin")
        np.ascontiguousarray(np.stack([eu[te], ev[te]], axis=1), dtype="<i4").tofile(testf)
        res, prec = run_ref(train, [], [], test=testf)
        for mi, q, p, r in prec:
            assert q == n_test
            pred, _ = run_ref(train, [mi], [q])
            _, ju, jv, js = pred[(mi, q)]
            pad, ju, jv, js = strip(ju, jv, js)
            assert pad == 0
            tp = len(set(zip(ju.tolist(), jv.tolist())) & set(zip(eu[te].tolist(), ev[te].tolist())))
            assert p == tp / float(q) and r == tp / float(n_test), (p, r, tp)
            precision.append(dict(SPLIT, metric=METRICS[mi], n=int(n), edges=int(eu.size), q=q, true_positives=tp, true_count=n_test, precision=float(p).hex(),
                                  recall=float(r).hex(), prediction_sha256=digest(ju, jv, js)))
            print(f"precision ({METRICS[mi]}): q {q}, tp {tp}, precision {p:.6f}, recall {r:.6f}")
    path = os.path.join(GOLDEN, "link_prediction.json")
    with open(path, "w") as fh:
        fh.write('{\n "graphs": ' + json.dumps(graphs, sort_keys=True) + ',\n "precision": ' + json.dumps(precision, sort_keys=True) + ',\n "records": [\n' +
                 ",\n".join("  " + json.dumps(r, sort_keys=True, separators=(",", ":")) for r in records) + "\n ]\n}\n")
    size = os.path.getsize(path)
    assert size <= 200 * 1024, size
    print("wrote", len(records), "records,", size, "bytes")


if __name__ == "__main__":
    main()
