"""CPU: gms_amd/csrc/hip/device_buffer.hpp holds the one owner of a device allocation (DevBuf, and DevArr<T> which reads like a T*).  The graph's
device arrays are DevArr members of gmsx_graph and of its lifetime groups (TcContainers, KcReverse, PrBins), so nothing is freed by a hand-kept
list: hipFree is spelled in the owner, and at the process-lifetime allocations that must not have one (the k-clique pool, the communicator)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gms_amd", "csrc")
OWNER = os.path.join("hip", "device_buffer.hpp")
GRAPH = os.path.join("hip", "device_graph.hpp")
GONE = ("DevGuard", "struct Guard", "free_graph", "release<")
# every device array that device_graph.hip, kclique.hip (ensure_kc_reverse) or pagerank.hip (ensure_pr_bins) allocates for a graph, by the struct that owns it
OWNED = {
    "gmsx_graph": ["off", "adj", "newid", "oldid", "hoff", "hadj", "toff", "tadj", "bmoff", "bmpool", "dplus", "order", "scratch", "acc"],
    "TcContainers": ["srow", "srow2", "ksplit", "spool", "trow", "tpool", "tsplit", "htask_lo", "htask_hi", "ttask_lo", "ttask_hi", "hitem", "titem",
                     "tunits", "ledge", "lpack", "core_bits"],
    "ShardItems": ["hitem", "titem"],
    "KcReverse": ["rel", "aoff", "arena", "rec", "item", "relt", "rect", "itemt"],
    "PrBins": ["bins", "first", "slot_row"],
}


def _sources():
    for base, _, files in os.walk(CSRC):
        for f in sorted(files):
            if f.endswith((".hip", ".hpp", ".cpp")):
                path = os.path.join(base, f)
                yield os.path.relpath(path, CSRC), open(path, errors="ignore").read()


def _struct_body(text, name):
    """the text between the braces of `struct name {`, nested structs included"""
    start = text.index("struct %s {" % name)
    depth, i = 0, text.index("{", start)
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
    raise AssertionError(name)


def _code(body):
    return re.sub(r"//[^\n]*", "", body)


def test_hipfree_is_spelled_by_the_owner_and_the_process_lifetime_allocations_only():
    texts = dict(_sources())
    assert len(texts) > 20 and OWNER in texts
    users = {name: text.count("hipFree(") for name, text in texts.items() if "hipFree(" in text}
    kclique, comm = os.path.join("hip", "kclique.hip"), os.path.join("hip", "comm.hip")
    assert sorted(users) == sorted([OWNER, kclique, comm]), users
    assert users[kclique] == 1 and "(void)hipFree(p.base);" in texts[kclique]   # the pool regrow of ensure_kc_pool
    for word in GONE:
        assert [name for name, text in texts.items() if word in text] == [], word


def test_the_graph_owns_its_device_arrays():
    hpp = open(os.path.join(CSRC, GRAPH)).read()
    for struct, names in OWNED.items():
        body = _code(_struct_body(hpp, struct))
        if struct == "TcContainers":   # its nested group is checked on its own
            body = body.replace(_code(_struct_body(hpp, "ShardItems")), "")
        owned = set()
        for decl in re.findall(r"DevArr<[^;>]*>\s*([^;]*);", body):
            owned |= set(re.findall(r"\w+", decl))
        assert owned == set(names), (struct, sorted(owned ^ set(names)))
        # … and no raw pointer member beside them (TaskList, a view that goes to the kernels by value, is a struct of its own)
        assert not re.search(r"^\s*(mutable\s+)?(const\s+)?(struct\s+)?[\w:]+(\s+[\w:]+)*\s*\*+\s*\w+\s*(=[^;]*)?[;,]", body, re.M), struct
    owner = open(os.path.join(CSRC, OWNER)).read()
    for line in ("!std::is_copy_constructible<DevArr<int>>::value", "std::is_nothrow_move_constructible<DevArr<int>>::value",
                 "std::is_convertible<const DevArr<int> &, int *>::value"):
        assert "static_assert(" + line in owner, line
    assert "static_assert(!std::is_copy_constructible<gmsx_graph>::value" in hpp


def test_no_owner_has_static_storage():
    """a DevBuf / DevArr that outlives the HIP runtime would free into it: none is static, global or thread_local"""
    for name, text in _sources():
        assert not re.search(r"^\s*(static|thread_local)\b[^;(]*\bDev(Buf|Arr)\b", _code(text), re.M), name
