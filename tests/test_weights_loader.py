"""CPU: edge weights in the host substrate (gmsx_csr_generate_weighted, _from_weighted_edges, _load_weighted, _save_wsg, _from_arrays_weighted,
gmsx_csr_fingerprint(g, 2)) against the fingerprints the reference's WeightedBuilder gave (tests/golden/sssp.json), and what the weights
must not change: every unweighted call and fingerprint.  tests/cpp/test_weights_loader_asan.cpp runs the malformed inputs under
AddressSanitizer as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_graph, load_golden
from test_sssp_golden_cpu import J, golden_csr

GRAPHS = load_golden("graphs.json")


def arcs(csr):
    off = np.array(csr.offsets(), dtype=np.int64)
    row = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
    return row, np.array(csr.neighbors(), dtype=np.int64), np.array(csr.weights(), dtype=np.int64)


@pytest.mark.parametrize("key", sorted(J["graphs"]))
def test_fingerprints_equal_the_reference(capi, key):
    csr = golden_csr(capi, key)
    rec = J["graphs"][key]
    assert (csr.num_nodes, csr.nnz) == (rec["n"], rec["nnz"])
    assert [str(x) for x in csr.fingerprint()] + [str(csr.weights_fingerprint())] == rec["fingerprints"]
    u, v, w = arcs(csr)
    assert w.min() >= 1 and w.max() == rec["wmax"] and np.all(u != v)
    # symmetric in structure and in weights
    a = np.lexsort((w, v, u))
    b = np.lexsort((w, u, v))
    assert np.array_equal(u[a], v[b]) and np.array_equal(v[a], u[b]) and np.array_equal(w[a], w[b])


def test_generated_structure_is_the_unweighted_graph(capi):
    for kind, scale in (("kronecker", 10), ("uniform", 10)):
        plain = capi.HostCSR.generate(kind, scale, 16, capi.RELABEL_NEVER)
        weighted = capi.HostCSR.generate_weighted(kind, scale, 16, capi.RELABEL_NEVER)
        assert plain.fingerprint() == weighted.fingerprint()
        assert plain.weights() is None and plain.weights_fingerprint() == 0 and weighted.weights_fingerprint() != 0


def test_thread_count_does_not_change_the_output(capi):
    fps = set()
    for threads in (1, 4):
        c = capi.HostCSR.generate_weighted("kronecker", 12, 16, capi.RELABEL_NEVER, threads)
        fps.add(c.fingerprint() + (c.weights_fingerprint(),))
    assert len(fps) == 1
    assert [str(x) for x in fps.pop()] == J["graphs"]["kronecker_12_16"]["fingerprints"]


def test_duplicate_keeps_the_minimum_and_loops_are_dropped(capi):
    src = [0, 1, 0, 2, 2, 1, 3]
    dst = [1, 0, 1, 2, 1, 2, 0]
    w = [9, 4, 6, 5, 8, 2, 7]
    c = capi.HostCSR.from_weighted_edges(src, dst, w)
    assert c.offsets().tolist() == [0, 2, 4, 5, 6]
    assert c.neighbors().tolist() == [1, 3, 0, 2, 1, 0]
    assert c.weights().tolist() == [4, 7, 4, 2, 2, 7]
    d = capi.HostCSR.from_weighted_edges(src, dst, w, symmetrize=False)
    assert d.offsets().tolist() == [0, 1, 3, 4, 5] and d.neighbors().tolist() == [1, 0, 2, 1, 0] and d.weights().tolist() == [6, 4, 2, 8, 7]


def test_missing_weights_are_inserted_as_the_reference_does(capi, tmp_path):
    """w = None and a weightless .el: Generator::InsertWeights over the list, in list order."""
    csr = capi.HostCSR.load_weighted(os.path.join(GOLDEN, "sssp", "two_parts_a.wel"))
    rows = np.loadtxt(os.path.join(GOLDEN, "sssp", "two_parts_a.wel"), dtype=np.int64)
    el = tmp_path / "same.el"
    np.savetxt(el, rows[:, :2], fmt="%d")
    a = capi.HostCSR.load_weighted(str(el))
    b = capi.HostCSR.from_weighted_edges(rows[:, 0], rows[:, 1], None)
    assert a.fingerprint() == b.fingerprint() == csr.fingerprint()
    assert a.weights_fingerprint() == b.weights_fingerprint() != csr.weights_fingerprint()
    assert 1 <= a.weights().min() and a.weights().max() <= 255
    # edge e of a list gets the e-th draw of its block, whatever follows it
    c = capi.HostCSR.from_weighted_edges(np.arange(8), np.arange(8) + 1, None)
    d = capi.HostCSR.from_weighted_edges(np.arange(4), np.arange(4) + 1, None)
    wc = {(int(u), int(v)): int(x) for u, v, x in zip(*arcs(c))}
    wd = {(int(u), int(v)): int(x) for u, v, x in zip(*arcs(d))}
    assert all(wc[k] == wd[k] for k in wd) and len(wd) == 8


def test_wsg_round_trip(capi, tmp_path):
    csr = golden_csr(capi, "kronecker_10_16")
    p = str(tmp_path / "g.wsg")
    csr.save_wsg(p)
    back = capi.HostCSR.load_weighted(p)
    assert back.fingerprint() == csr.fingerprint() and back.weights_fingerprint() == csr.weights_fingerprint()
    raw = open(p, "rb").read()
    n, nnz = csr.num_nodes, csr.nnz
    assert len(raw) == 17 + 8 * (n + 1) + 8 * nnz and struct.unpack_from("<?qq", raw) == (False, nnz, n)
    pairs = np.frombuffer(raw[17 + 8 * (n + 1):], dtype="<i4").reshape(-1, 2)
    assert np.array_equal(pairs[:, 0], csr.neighbors()) and np.array_equal(pairs[:, 1], csr.weights())
    open(str(tmp_path / "cut.wsg"), "wb").write(raw[:-5])
    with pytest.raises(capi.GmsxError) as ei:
        capi.HostCSR.load_weighted(str(tmp_path / "cut.wsg"))
    assert ei.value.status == capi.ERR_FORMAT
    with pytest.raises(capi.GmsxError) as ei:
        capi.HostCSR.generate("kronecker", 6, 4).save_wsg(str(tmp_path / "no.wsg"))
    assert ei.value.status == capi.ERR_INVALID


def test_what_load_weighted_refuses(capi, tmp_path):
    plain = capi.HostCSR.generate("kronecker", 6, 4)
    for suffix, save in ((".sg", plain.save_sg), (".sgx", plain.save_sgx)):
        p = str(tmp_path / ("g" + suffix))
        save(p)
        with pytest.raises(capi.GmsxError) as ei:
            capi.HostCSR.load_weighted(p)
        assert ei.value.status == capi.ERR_FORMAT
    for suffix in (".mtx", ".graph"):
        with pytest.raises(capi.GmsxError) as ei:
            capi.HostCSR.load_weighted(str(tmp_path / ("g" + suffix)))
        assert ei.value.status == capi.ERR_UNSUPPORTED
    gr = tmp_path / "g.gr"
    gr.write_text("c a comment\np sp 3 2\na 1 2 5\na 2 3 7\na 1 2 4\n")
    c = capi.HostCSR.load_weighted(str(gr))
    assert c.neighbors().tolist() == [1, 0, 2, 1] and c.weights().tolist() == [4, 4, 7, 7]
    wel = tmp_path / "g.wel"
    wel.write_text("0 1 5\n1 2 99999999999\n")
    with pytest.raises(capi.GmsxError) as ei:
        capi.HostCSR.load_weighted(str(wel))
    assert ei.value.status == capi.ERR_OVERFLOW


def test_relabelling_keeps_edge_weight_pairs(capi):
    raw = golden_csr(capi, "kronecker_10_16")
    rel = raw.relabel_by_degree()
    auto = golden_csr(capi, "kronecker_10_16_relabelled")
    assert rel.fingerprint() == auto.fingerprint() and rel.weights_fingerprint() == auto.weights_fingerprint()
    assert rel.fingerprint() == capi.HostCSR.generate("kronecker", 10, 16, capi.RELABEL_ALWAYS).fingerprint()
    deg = np.diff(raw.offsets())
    order = np.lexsort((-np.arange(deg.size), -deg))  # descending (degree, id)
    new_id = np.empty(deg.size, dtype=np.int64)
    new_id[order] = np.arange(deg.size)
    u, v, w = arcs(raw)
    ru, rv, rw = arcs(rel)
    a = np.lexsort((w, new_id[v], new_id[u]))
    b = np.lexsort((rw, rv, ru))
    assert np.array_equal(new_id[u][a], ru[b]) and np.array_equal(new_id[v][a], rv[b]) and np.array_equal(w[a], rw[b])
    assert np.all(np.diff(rel.neighbors())[np.diff(ru) == 0] > 0)  # rows ascending


def test_unweighted_calls_see_the_structure_only(capi, tmp_path):
    weighted = golden_csr(capi, "kronecker_10_16")
    plain = capi.HostCSR.generate("kronecker", 10, 16, capi.RELABEL_NEVER)
    for suffix, name in ((".sg", "save_sg"), (".sgx", "save_sgx")):
        a, b = str(tmp_path / ("a" + suffix)), str(tmp_path / ("b" + suffix))
        getattr(weighted, name)(a)
        getattr(plain, name)(b)
        assert open(a, "rb").read() == open(b, "rb").read()
    assert capi.HostCSR.load(str(tmp_path / "a.sg"), relabel=capi.RELABEL_NEVER).weights() is None
    assert weighted.merge_elements() == plain.merge_elements() and np.array_equal(weighted.pick_sources(8), plain.pick_sources(8))
    # the plain loader still drops the third column of a .wel
    dropped = capi.HostCSR.load(os.path.join(GOLDEN, "sssp", "two_parts_a.wel"), relabel=capi.RELABEL_NEVER)
    kept = capi.HostCSR.load_weighted(os.path.join(GOLDEN, "sssp", "two_parts_a.wel"))
    assert dropped.weights() is None and dropped.fingerprint() == kept.fingerprint()
    c = capi.HostCSR.from_arrays_weighted(weighted.offsets(), weighted.neighbors(), weighted.weights())
    assert c.fingerprint() == weighted.fingerprint() and c.weights_fingerprint() == weighted.weights_fingerprint()


@pytest.mark.parametrize("key", [k for k, v in GRAPHS.items() if "offsets_fnv64" in v and v["scale"] <= 14 and v["generator"] != "rmat"])
def test_unweighted_fingerprints_are_unchanged(capi, key):
    rec = GRAPHS[key]
    csr = host_graph(capi, rec["generator"], rec["scale"], rec["degree"], rec["relabel"])
    fo, fn = csr.fingerprint()
    assert "%016x" % fo == rec["offsets_fnv64"] and "%016x" % fn == rec["neigh_fnv64"] and csr.weights() is None


def test_malformed_inputs_under_address_sanitizer(tmp_path):
    """tests/cpp/test_weights_loader_asan.cpp + loader.cpp, compiled with -fsanitize=address,undefined into a plain executable and run."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "weights_asan")
    csrc = os.path.join(ROOT, "gms_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(csrc, "host"), os.path.join(ROOT, "tests", "cpp", "test_weights_loader_asan.cpp"),
                    os.path.join(csrc, "host", "loader.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all weighted-loader cases passed" in r.stdout
