"""ctypes binding of the gmsx C-ABI (include/gmsx.h -> gms_amd/lib/libgmsx.so).

This is plumbing for tests and bench.py; the product is the shared library.  There is no CPU fallback:
if libgmsx.so is missing this module raises at import of the library handle, and every device entry
point returns GMSX_ERR_NO_DEVICE without a GPU.
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GMSX_LIB") or os.path.join(_HERE, "lib", "libgmsx.so")  # GMSX_LIB: an A/B build of the same library (tools/)

_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")

GEN_KRONECKER, GEN_UNIFORM = 0, 1
RELABEL_NEVER, RELABEL_AUTO, RELABEL_ALWAYS = 0, 1, 2
TC_AUTO, TC_ORIENTED, TC_FULL = 0, 1, 2
UPLOAD_DEFAULT, UPLOAD_TRUSTED, UPLOAD_FOR_TC = 0, 1, 2
PREPARE_TC = 1
SETOP_INTERSECT, SETOP_DIFFERENCE = 0, 1
OK, ERR_INVALID, ERR_NOMEM, ERR_IO, ERR_FORMAT, ERR_DIRECTED, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5, -6
ERR_DEVICE_MEM, ERR_NOT_CANONICAL, ERR_OVERFLOW, ERR_UNSUPPORTED, ERR_KERNEL, ERR_COMM, ERR_TIMEOUT = -7, -8, -9, -10, -11, -12, -13
COMM_ID_BYTES = 128

# every symbol include/gmsx.h declares (tests/test_capi_symbols.py checks the header against this list)
SYMBOLS = [
    "gmsx_strerror", "gmsx_version",
    "gmsx_csr_generate", "gmsx_csr_generate_rmat", "gmsx_csr_from_edges", "gmsx_csr_load", "gmsx_csr_save_sg", "gmsx_csr_save_sgx", "gmsx_csr_is_mapped", "gmsx_csr_from_arrays",
    "gmsx_csr_pick_sources", "gmsx_csr_worth_relabelling", "gmsx_csr_relabel_by_degree", "gmsx_csr_num_nodes", "gmsx_csr_num_edges",
    "gmsx_csr_num_edges_directed", "gmsx_csr_offsets", "gmsx_csr_neighbors", "gmsx_csr_merge_elements",
    "gmsx_csr_fingerprint", "gmsx_csr_free", "gmsx_set_host_threads", "gmsx_set_option", "gmsx_reset_options", "gmsx_option_name",
    "gmsx_init", "gmsx_set_stream", "gmsx_device_info", "gmsx_hbm_read_probe",
    "gmsx_graph_upload", "gmsx_graph_upload_csr", "gmsx_graph_upload_shard", "gmsx_graph_upload_csr_shard", "gmsx_graph_prepare", "gmsx_graph_tc_passes", "gmsx_graph_free", "gmsx_graph_num_nodes", "gmsx_graph_num_edges",
    "gmsx_graph_device_bytes", "gmsx_graph_max_out_degree",
    "gmsx_tc_total", "gmsx_tc_partial", "gmsx_tc_divisor", "gmsx_tc_stream_breakdown", "gmsx_tc_row_histogram", "gmsx_tc_comembership", "gmsx_tc_vertex_count2",
    "gmsx_intersect_count_batch", "gmsx_set_op_batch", "gmsx_vertex_similarity_batch", "gmsx_kclique_count", "gmsx_kclique_partial", "gmsx_kclique_star_count", "gmsx_kclique_star_list", "gmsx_bk_count", "gmsx_bk_partial", "gmsx_bk_list",
    "gmsx_adg_rank", "gmsx_tc_ordering", "gmsx_core_decomposition", "gmsx_degree_rank", "gmsx_order_quality",
    "gmsx_coloring_jp", "gmsx_coloring_verify",
    "gmsx_edge_support", "gmsx_truss_decomposition",
    "gmsx_link_prediction", "gmsx_link_prediction_precision",
    "gmsx_subgraph_order", "gmsx_subgraph_match",
    "gmsx_connected_components", "gmsx_jarvis_patrick",
    "gmsx_bfs", "gmsx_betweenness", "gmsx_bfs_multi",
    "gmsx_pagerank", "gmsx_pagerank_residual",
    "gmsx_csr_weights", "gmsx_csr_generate_weighted", "gmsx_csr_from_weighted_edges", "gmsx_csr_load_weighted", "gmsx_csr_save_wsg",
    "gmsx_csr_from_arrays_weighted", "gmsx_graph_set_weights", "gmsx_graph_has_weights", "gmsx_sssp", "gmsx_sssp_verify",
    "gmsx_min_spanning_forest",
    "gmsx_label_propagation", "gmsx_modularity",
    "gmsx_greedy_matching", "gmsx_matching_verify",
    "gmsx_biconnected_components",
    "gmsx_cycle4_count", "gmsx_cycle4_partial", "gmsx_motif_census4",
    "gmsx_comm_unique_id", "gmsx_comm_init", "gmsx_comm_allreduce_u64", "gmsx_comm_rank", "gmsx_comm_size", "gmsx_comm_finalize",
]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("setup_ms", C.c_double), ("units", C.c_uint64),
                ("alg_elements", C.c_uint64), ("probes", C.c_uint64), ("launches", C.c_int32), ("reserved", C.c_int32),
                ("stream_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class BkListInfo(C.Structure):
    _fields_ = [("cliques", C.c_int64), ("members", C.c_int64), ("max_size", C.c_int32), ("size_hist", C.c_int64 * 65)]

    def as_dict(self):
        return {"cliques": int(self.cliques), "members": int(self.members), "max_size": int(self.max_size),
                "size_hist": [int(x) for x in self.size_hist]}


class KcliqueStarListInfo(C.Structure):
    _fields_ = [("cliques", C.c_int64), ("star_members", C.c_int64), ("k", C.c_int32), ("max_star", C.c_int32)]

    def as_dict(self):
        return {"cliques": int(self.cliques), "star_members": int(self.star_members), "k": int(self.k), "max_star": int(self.max_star)}


KCSTAR_DEFAULT, KCSTAR_CLIQUES_ONLY = 0, 1


class CoreInfo(C.Structure):
    _fields_ = [("degeneracy", C.c_int32), ("levels", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32), ("top_core", C.c_int64)]

    def as_dict(self):
        return {"degeneracy": int(self.degeneracy), "levels": int(self.levels), "rounds": int(self.rounds), "top_core": int(self.top_core)}


class OrderQualityInfo(C.Structure):
    _fields_ = [("max_later", C.c_int32), ("core_number", C.c_int32), ("core_number_of_order", C.c_int32), ("reserved", C.c_int32),
                ("faulty", C.c_int64), ("excess", C.c_int64), ("relative_error", C.c_double), ("fault_rate", C.c_double),
                ("relative_mean_difference", C.c_double)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k in ("max_later", "core_number", "core_number_of_order", "faulty", "excess")}
        d.update({k: float(getattr(self, k)) for k in ("relative_error", "fault_rate", "relative_mean_difference")})
        return d


class ColoringInfo(C.Structure):
    _fields_ = [("colors", C.c_int32), ("rounds", C.c_int32), ("max_pred", C.c_int32), ("reserved", C.c_int32), ("first_round", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("colors", "rounds", "max_pred", "first_round")}


class ColoringCheck(C.Structure):
    _fields_ = [("conflicts", C.c_int64), ("invalid", C.c_int64), ("max_color", C.c_int32), ("distinct", C.c_int32), ("max_degree", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("conflicts", "invalid", "max_color", "distinct", "max_degree")}


COLOR_HEURISTICS = ("id", "ff", "lf", "sl", "adg")


class TrussInfo(C.Structure):
    _fields_ = [("max_truss", C.c_int32), ("levels", C.c_int32), ("rounds", C.c_int32), ("max_support", C.c_int32), ("top_edges", C.c_int64),
                ("triangles", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("max_truss", "levels", "rounds", "max_support", "top_edges", "triangles")}


class LinkPredictionInfo(C.Structure):
    _fields_ = [("found", C.c_int64), ("scored", C.c_int64), ("positive", C.c_int64), ("chunks", C.c_int32), ("classes", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("found", "scored", "positive", "chunks", "classes")}


class ComponentsInfo(C.Structure):
    _fields_ = [("components", C.c_int64), ("singletons", C.c_int64), ("largest", C.c_int64), ("kept_edges", C.c_int64),
                ("largest_label", C.c_int32), ("passes", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("components", "singletons", "largest", "kept_edges", "largest_label", "passes")}


MOTIFS = ("wedge", "triangle", "star3", "path4", "paw", "cycle4", "diamond", "clique4")  # GMSX_MOTIF_*: the index of a name is its value


class BfsInfo(C.Structure):
    _fields_ = [("reached", C.c_int64), ("reached_arcs", C.c_int64), ("depth_sum", C.c_int64), ("widest", C.c_int64),
                ("levels", C.c_int32), ("widest_level", C.c_int32), ("bottom_up_levels", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("reached", "reached_arcs", "depth_sum", "widest", "levels", "widest_level", "bottom_up_levels")}


BC_DEFAULT, BC_EXCLUDE_SOURCE, BC_NORMALIZE_MAX = 0, 1, 2


class BcInfo(C.Structure):
    _fields_ = [("sources", C.c_int64), ("reached_total", C.c_int64), ("max_levels", C.c_int32), ("reserved", C.c_int32),
                ("max_score", C.c_double), ("max_sigma", C.c_double)]

    def as_dict(self):
        return {"sources": int(self.sources), "reached_total": int(self.reached_total), "max_levels": int(self.max_levels),
                "max_score": float(self.max_score), "max_sigma": float(self.max_sigma)}


class BfsSource(C.Structure):
    _fields_ = [("reached", C.c_int64), ("reached_arcs", C.c_int64), ("depth_sum", C.c_int64), ("levels", C.c_int32), ("reserved", C.c_int32),
                ("closeness", C.c_double), ("harmonic", C.c_double)]


# gmsx_bfs_source as a numpy record (the same 48 bytes)
BFS_SOURCE_DTYPE = np.dtype([("reached", "<i8"), ("reached_arcs", "<i8"), ("depth_sum", "<i8"), ("levels", "<i4"), ("reserved", "<i4"),
                             ("closeness", "<f8"), ("harmonic", "<f8")])


class BfsMultiInfo(C.Structure):
    _fields_ = [("sources", C.c_int64), ("passes", C.c_int64), ("reached_total", C.c_int64), ("max_levels", C.c_int32), ("max_far", C.c_int32),
                ("push_levels", C.c_int32), ("pull_levels", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


PR_DEFAULT, PR_DANGLING, PR_FLOAT32 = 0, 1, 2


class PagerankInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("argmax", C.c_int32), ("reserved", C.c_int32), ("error", C.c_double),
                ("sum", C.c_double), ("max_score", C.c_double), ("isolated", C.c_int64)]

    def as_dict(self):
        return {"iterations": int(self.iterations), "converged": int(self.converged), "argmax": int(self.argmax), "error": float(self.error),
                "sum": float(self.sum), "max_score": float(self.max_score), "isolated": int(self.isolated)}


class SsspInfo(C.Structure):
    _fields_ = [("reached", C.c_int64), ("reached_arcs", C.c_int64), ("dist_sum", C.c_int64), ("max_dist", C.c_int64), ("delta", C.c_int64),
                ("buckets", C.c_int64), ("rounds", C.c_int64), ("relaxations", C.c_int64), ("far_vertex", C.c_int32), ("wide", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SsspCheck(C.Structure):
    _fields_ = [("violated_arcs", C.c_int64), ("untight", C.c_int64), ("wrong_unreached", C.c_int64), ("source_ok", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


MSF_MAXIMUM = 1


class MsfInfo(C.Structure):
    _fields_ = [("edges", C.c_int64), ("total_weight", C.c_int64), ("trees", C.c_int64), ("isolated", C.c_int64), ("largest_tree", C.c_int64),
                ("min_weight", C.c_int32), ("max_weight", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


LP_WEIGHTED = 1


class LpInfo(C.Structure):
    _fields_ = [("communities", C.c_int64), ("largest", C.c_int64), ("singletons", C.c_int64), ("changes", C.c_int64),
                ("first_sweep_changes", C.c_int64), ("sweeps", C.c_int32), ("colors", C.c_int32), ("converged", C.c_int32),
                ("largest_label", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ModularityInfo(C.Structure):
    _fields_ = [("total_weight", C.c_int64), ("intra_weight", C.c_int64), ("sumsq_hi", C.c_uint64), ("sumsq_lo", C.c_uint64),
                ("communities", C.c_int64), ("largest", C.c_int64), ("unstable", C.c_int64), ("modularity", C.c_double)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "modularity"}
        d["sumsq"] = (d["sumsq_hi"] << 64) | d["sumsq_lo"]
        d["modularity"] = float(self.modularity)
        return d


MATCH_WEIGHTED = 1


class MatchingInfo(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("total_weight", C.c_int64), ("free_vertices", C.c_int64), ("exposed", C.c_int64),
                ("min_weight", C.c_int32), ("max_weight", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class MatchingCheck(C.Structure):
    _fields_ = [("invalid", C.c_int64), ("pairs", C.c_int64), ("total_weight", C.c_int64), ("free_vertices", C.c_int64),
                ("augmentable", C.c_int64), ("undominated", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class BiccInfo(C.Structure):
    _fields_ = [("blocks", C.c_int64), ("bridges", C.c_int64), ("articulation_points", C.c_int64), ("largest_block_edges", C.c_int64),
                ("largest_block_vertices", C.c_int64), ("components", C.c_int64), ("isolated", C.c_int64), ("largest_block", C.c_int32),
                ("max_blocks_at", C.c_int32), ("levels", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class MotifInfo(C.Structure):
    _fields_ = [("subgraphs", C.c_uint64 * 8), ("induced", C.c_uint64 * 8), ("wedges_walked", C.c_uint64), ("max_codegree", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self):
        return {"subgraphs": {k: int(self.subgraphs[i]) for i, k in enumerate(MOTIFS)},
                "induced": {k: int(self.induced[i]) for i, k in enumerate(MOTIFS)},
                "wedges_walked": int(self.wedges_walked), "max_codegree": int(self.max_codegree)}


def clusters(label):
    """The vertex ids of every component of a label array (connected_components, jarvis_patrick): a list of ascending int32 arrays, ordered
    by label."""
    label = np.asarray(label)
    order = np.argsort(label, kind="stable")
    cuts = np.flatnonzero(np.diff(label[order])) + 1
    return [part.astype(np.int32) for part in np.split(order, cuts)] if label.size else []


LP_CLASS_ONE, LP_CLASS_POS, LP_CLASS_ZERO, LP_CLASS_ALL = 1, 2, 4, 8
SIM_METRICS = {"jaccard": 0, "overlap": 1, "adamic_adar": 2, "resource": 3, "common": 4, "total": 5, "prefatt": 6}


def merge_link_predictions(parts, q):
    """Merges link_prediction outputs (u, v, scores[, info]) of the shards of one (graph, metric, q) under the rule of gmsx.h — decreasing
    score, ties by ascending (u, v) — truncates to q and returns (u, v, scores) worst first: the whole graph's output, byte for byte."""
    u = np.concatenate([np.asarray(p[0], dtype=np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    v = np.concatenate([np.asarray(p[1], dtype=np.int32) for p in parts]) if parts else np.zeros(0, np.int32)
    s = np.concatenate([np.asarray(p[2], dtype=np.float64) for p in parts]) if parts else np.zeros(0, np.float64)
    order = np.lexsort((v, u, -s))[:max(int(q), 0)][::-1]
    return u[order], v[order], s[order]


class SubgraphInfo(C.Structure):
    _fields_ = [("embeddings", C.c_int64), ("tasks", C.c_int64), ("k", C.c_int32), ("reserved", C.c_int32), ("order", C.c_int32 * 32)]

    def as_dict(self):
        return {"embeddings": int(self.embeddings), "tasks": int(self.tasks), "k": int(self.k), "order": [int(x) for x in self.order[:max(int(self.k), 0)]]}


SGM_INDUCED, SGM_MONO, SGM_FIRST = 0, 1, 2


def pattern_arrays(pattern):
    """(offsets int64[k + 1], neigh int32[nnz]) of a pattern given as a HostCSR, an (offsets, neigh) pair or an edge list (pairs; symmetrized,
    k = the largest id + 1).  A pair of arrays is handed on as it is: the library validates it."""
    if isinstance(pattern, HostCSR):
        return np.array(pattern.offsets(), dtype=np.int64), np.array(pattern.neighbors(), dtype=np.int32)
    # (two arrays that are not two edges: offsets of 2 entries are k = 1, whose neigh is empty)
    if isinstance(pattern, tuple) and len(pattern) == 2 and np.ndim(pattern[0]) == 1 and np.ndim(pattern[1]) == 1 and \
            not (len(pattern[0]) == 2 and len(pattern[1]) == 2):
        return np.ascontiguousarray(pattern[0], dtype=np.int64), np.ascontiguousarray(pattern[1], dtype=np.int32)
    e = np.asarray(pattern, dtype=np.int64).reshape(-1, 2)
    k = int(e.max()) + 1 if e.size else 1
    a = np.zeros((k, k), dtype=bool)
    a[e[:, 0], e[:, 1]] = True
    a[e[:, 1], e[:, 0]] = True
    off = np.concatenate([[0], np.cumsum(a.sum(axis=1))]).astype(np.int64)
    return off, np.nonzero(a)[1].astype(np.int32)


def _pattern_args(pattern):
    off, neigh = pattern_arrays(pattern)
    return off, neigh, int(off.size - 1), off.ctypes.data_as(C.c_void_p), (neigh if neigh.size else np.zeros(1, np.int32)).ctypes.data_as(C.c_void_p)


def subgraph_order(pattern):
    """gmsx_subgraph_order: the matching order pi of a pattern (int32[k]); host only."""
    off, neigh, k, po, pn = _pattern_args(pattern)
    order = np.zeros(max(k, 1), dtype=np.int32)
    _check(lib().gmsx_subgraph_order(k, po, pn, order.ctypes.data_as(C.c_void_p)), "gmsx_subgraph_order")
    return order[:k]


def merge_subgraph_matches(parts, order):
    """The row-wise merge of the shard lists of one (graph, pattern, flags): rows by ascending (f(pi_0), .., f(pi_(k-1))), the whole list byte
    for byte.  parts: (E_i, k) int32 arrays; order: the matching order pi."""
    order = [int(x) for x in order]
    rows = np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1, len(order)) for p in parts]) if parts else np.zeros((0, len(order)), np.int32)
    if rows.shape[0] == 0:
        return rows
    return np.ascontiguousarray(rows[np.lexsort([rows[:, p] for p in reversed(order)])])


class GmsxError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__(f"{what}: gmsx status {status} ({lib().gmsx_strerror(status).decode()})")


_LIB = None


def lib():
    """The loaded libgmsx.so; raises if it has not been built (python __graft_entry__.py / make -C gms_amd/csrc)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C gms_amd/csrc` (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
    L.gmsx_strerror.restype = C.c_char_p
    L.gmsx_strerror.argtypes = [C.c_int]
    L.gmsx_csr_generate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vpp]
    L.gmsx_csr_generate_rmat.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, vpp]
    L.gmsx_csr_from_edges.argtypes = [C.c_int64, C.c_int64, _i32p, _i32p, C.c_int, C.c_int, vpp]
    L.gmsx_csr_load.argtypes = [C.c_char_p, C.c_int, C.c_int, vpp]
    L.gmsx_csr_save_sg.argtypes = [vp, C.c_char_p]
    L.gmsx_csr_save_sgx.argtypes = [vp, C.c_char_p]
    L.gmsx_csr_is_mapped.argtypes = [vp]
    L.gmsx_csr_from_arrays.argtypes = [C.c_int64, _i64p, _i32p, vpp]
    L.gmsx_csr_worth_relabelling.argtypes = [vp]
    L.gmsx_csr_relabel_by_degree.argtypes = [vp, vpp]
    for f in (L.gmsx_csr_num_nodes, L.gmsx_csr_num_edges, L.gmsx_csr_num_edges_directed):
        f.restype = C.c_int64
        f.argtypes = [vp]
    L.gmsx_csr_offsets.restype = C.POINTER(C.c_int64)
    L.gmsx_csr_offsets.argtypes = [vp]
    L.gmsx_csr_neighbors.restype = C.POINTER(C.c_int32)
    L.gmsx_csr_neighbors.argtypes = [vp]
    L.gmsx_csr_merge_elements.restype = C.c_uint64
    L.gmsx_csr_merge_elements.argtypes = [vp]
    L.gmsx_csr_fingerprint.restype = C.c_uint64
    L.gmsx_csr_fingerprint.argtypes = [vp, C.c_int]
    L.gmsx_csr_free.argtypes = [vp]
    L.gmsx_init.argtypes = [C.c_int]
    L.gmsx_set_stream.argtypes = [vp]
    L.gmsx_device_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.gmsx_graph_upload.argtypes = [C.c_int64, _i64p, _i32p, C.c_uint32, vpp]
    L.gmsx_graph_upload_csr.argtypes = [vp, C.c_uint32, vpp]
    L.gmsx_graph_upload_shard.argtypes = [C.c_int64, _i64p, _i32p, C.c_uint32, C.c_int, C.c_int, vpp]
    L.gmsx_graph_upload_csr_shard.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, vpp]
    L.gmsx_graph_free.argtypes = [vp]
    L.gmsx_graph_prepare.argtypes = [vp, C.c_uint32]
    L.gmsx_graph_tc_passes.argtypes = [vp]
    for f in (L.gmsx_graph_num_nodes, L.gmsx_graph_num_edges, L.gmsx_graph_device_bytes):
        f.restype = C.c_int64
        f.argtypes = [vp]
    L.gmsx_graph_max_out_degree.restype = C.c_int32
    L.gmsx_graph_max_out_degree.argtypes = [vp]
    sp = C.POINTER(Stats)
    u64p = C.POINTER(C.c_uint64)
    L.gmsx_tc_total.argtypes = [vp, C.c_int, u64p, sp]
    L.gmsx_tc_partial.argtypes = [vp, C.c_int, C.c_int, C.c_int, u64p, sp]
    L.gmsx_tc_divisor.argtypes = [C.c_int]
    L.gmsx_tc_stream_breakdown.argtypes = [vp, np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")]
    L.gmsx_tc_row_histogram.argtypes = [vp, np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")]
    L.gmsx_tc_comembership.argtypes = [vp, C.c_int, np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")]
    L.gmsx_tc_vertex_count2.argtypes = [vp, _i64p, sp]
    L.gmsx_intersect_count_batch.argtypes = [vp, C.c_int64, _i32p, _i32p, _u32p, sp]
    L.gmsx_set_op_batch.argtypes = [vp, C.c_int, C.c_int64, _i32p, _i32p, _i64p, C.c_void_p, C.c_int64, sp]
    L.gmsx_vertex_similarity_batch.argtypes = [vp, C.c_int, C.c_int64, _i32p, _i32p, np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), sp]
    L.gmsx_kclique_count.argtypes = [vp, C.c_int, u64p, u64p, sp]
    L.gmsx_kclique_partial.argtypes = [vp, C.c_int, C.c_int, C.c_int, u64p, sp]
    L.gmsx_kclique_star_count.argtypes = [vp, C.c_int, u64p, u64p, sp]
    L.gmsx_kclique_star_list.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                         C.POINTER(KcliqueStarListInfo), sp]
    L.gmsx_bk_count.argtypes = [vp, C.c_void_p, u64p, sp]
    L.gmsx_bk_partial.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, u64p, sp]
    L.gmsx_bk_list.argtypes = [vp, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(BkListInfo), sp]
    L.gmsx_adg_rank.argtypes = [vp, C.c_double, C.c_int, _i32p, C.POINTER(C.c_int32), sp]
    L.gmsx_tc_ordering.argtypes = [vp, _i32p, sp]
    L.gmsx_core_decomposition.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(CoreInfo), sp]
    L.gmsx_degree_rank.argtypes = [vp, C.c_int, _i32p, sp]
    L.gmsx_order_quality.argtypes = [vp, C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.POINTER(OrderQualityInfo), sp]
    L.gmsx_coloring_jp.argtypes = [vp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ColoringInfo), sp]
    L.gmsx_coloring_verify.argtypes = [vp, C.c_void_p, C.POINTER(ColoringCheck), sp]
    L.gmsx_edge_support.argtypes = [vp, C.c_void_p, u64p, sp]
    L.gmsx_truss_decomposition.argtypes = [vp, C.c_void_p, C.c_void_p, C.POINTER(TrussInfo), sp]
    L.gmsx_link_prediction.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.POINTER(LinkPredictionInfo), sp]
    L.gmsx_link_prediction_precision.argtypes = [vp, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), sp]
    L.gmsx_subgraph_order.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gmsx_subgraph_match.argtypes = [vp, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                      C.POINTER(SubgraphInfo), sp]
    L.gmsx_connected_components.argtypes = [vp, C.c_void_p, C.c_void_p, C.POINTER(ComponentsInfo), sp]
    L.gmsx_jarvis_patrick.argtypes = [vp, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(ComponentsInfo), sp]
    L.gmsx_bfs.argtypes = [vp, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(BfsInfo), sp]
    L.gmsx_betweenness.argtypes = [vp, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(BcInfo), sp]
    L.gmsx_bfs_multi.argtypes = [vp, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BfsMultiInfo), sp]
    L.gmsx_pagerank.argtypes = [vp, C.c_double, C.c_int32, C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(PagerankInfo), sp]
    L.gmsx_pagerank_residual.argtypes = [vp, C.c_void_p, C.c_double, C.c_void_p, C.c_uint32, C.POINTER(C.c_double), sp]
    L.gmsx_csr_pick_sources.argtypes = [vp, C.c_int64, C.c_int32, C.c_void_p]
    L.gmsx_csr_weights.restype = C.POINTER(C.c_int32)
    L.gmsx_csr_weights.argtypes = [vp]
    L.gmsx_csr_generate_weighted.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vpp]
    L.gmsx_csr_from_weighted_edges.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, vpp]
    L.gmsx_csr_load_weighted.argtypes = [C.c_char_p, C.c_int, C.c_int, vpp]
    L.gmsx_csr_save_wsg.argtypes = [vp, C.c_char_p]
    L.gmsx_csr_from_arrays_weighted.argtypes = [C.c_int64, _i64p, C.c_void_p, C.c_void_p, vpp]
    L.gmsx_graph_set_weights.argtypes = [vp, C.c_void_p]
    L.gmsx_graph_has_weights.argtypes = [vp]
    L.gmsx_sssp.argtypes = [vp, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(SsspInfo), sp]
    L.gmsx_sssp_verify.argtypes = [vp, C.c_int32, C.c_void_p, C.POINTER(SsspCheck), sp]
    L.gmsx_min_spanning_forest.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MsfInfo), sp]
    L.gmsx_label_propagation.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(LpInfo), sp]
    L.gmsx_modularity.argtypes = [vp, C.c_uint32, C.c_void_p, C.POINTER(ModularityInfo), sp]
    L.gmsx_greedy_matching.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MatchingInfo), sp]
    L.gmsx_matching_verify.argtypes = [vp, C.c_uint32, C.c_void_p, C.POINTER(MatchingCheck), sp]
    L.gmsx_biconnected_components.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BiccInfo), sp]
    L.gmsx_cycle4_count.argtypes = [vp, u64p, C.c_void_p, sp]
    L.gmsx_cycle4_partial.argtypes = [vp, C.c_int, C.c_int, u64p, sp]
    L.gmsx_motif_census4.argtypes = [vp, C.POINTER(MotifInfo), sp]
    L.gmsx_comm_unique_id.argtypes = [C.c_char_p]
    L.gmsx_comm_init.argtypes = [C.c_int, C.c_int, C.c_char_p, vpp]
    L.gmsx_comm_allreduce_u64.argtypes = [vp, u64p]
    L.gmsx_comm_rank.argtypes = [vp]
    L.gmsx_comm_size.argtypes = [vp]
    L.gmsx_comm_finalize.argtypes = [vp]
    L.gmsx_hbm_read_probe.argtypes = [C.c_int64, C.c_int, C.POINTER(C.c_double)]
    L.gmsx_set_option.argtypes = [C.c_char_p, C.c_char_p]
    L.gmsx_reset_options.restype = None
    L.gmsx_option_name.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    _LIB = L
    # convenience of the tools (tools/*.sh, probes): GMSX_OPT_<NAME>=<value> in the environment of a PYTHON process becomes
    # gmsx_set_option(NAME, value) here, in the binding — the library itself reads no tuning from the environment
    for k, v in os.environ.items():
        if k.startswith("GMSX_OPT_"):
            _check(L.gmsx_set_option(k[len("GMSX_OPT_"):].encode(), v.encode()), f"gmsx_set_option({k})")
    return L


def _check(status, what):
    if status != 0:
        raise GmsxError(status, what)


class HostCSR:
    """gmsx_csr*: the host CSR the loader builds (replaces CSRGraph + Builder + Generator + Reader)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def generate(cls, generator="kronecker", scale=10, degree=16, relabel=RELABEL_AUTO, threads=0):
        h = C.c_void_p()
        gen = GEN_UNIFORM if generator in ("uniform", "u", GEN_UNIFORM) else GEN_KRONECKER
        _check(lib().gmsx_csr_generate(gen, scale, degree, relabel, threads, C.byref(h)), "gmsx_csr_generate")
        return cls(h)

    @classmethod
    def generate_rmat(cls, scale, degree, a, b, c, relabel=RELABEL_AUTO, threads=0):
        h = C.c_void_p()
        _check(lib().gmsx_csr_generate_rmat(scale, degree, a, b, c, relabel, threads, C.byref(h)), "gmsx_csr_generate_rmat")
        return cls(h)

    @classmethod
    def from_edges(cls, src, dst, num_nodes=-1, symmetrize=True, relabel=RELABEL_NEVER):
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        h = C.c_void_p()
        _check(lib().gmsx_csr_from_edges(num_nodes, src.size, src, dst, int(symmetrize), relabel, C.byref(h)),
               "gmsx_csr_from_edges")
        return cls(h)

    @classmethod
    def load(cls, path, symmetrize=True, relabel=RELABEL_AUTO):
        h = C.c_void_p()
        _check(lib().gmsx_csr_load(os.fsencode(path), int(symmetrize), relabel, C.byref(h)), "gmsx_csr_load")
        return cls(h)

    @classmethod
    def from_arrays(cls, off, neigh):
        off = np.ascontiguousarray(off, dtype=np.int64)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        h = C.c_void_p()
        _check(lib().gmsx_csr_from_arrays(off.size - 1, off, neigh if neigh.size else np.zeros(1, np.int32), C.byref(h)),
               "gmsx_csr_from_arrays")
        return cls(h)

    @classmethod
    def generate_weighted(cls, generator="kronecker", scale=10, degree=16, relabel=RELABEL_NEVER, threads=0):
        """gmsx_csr_generate_weighted: the reference's WeightedBuilder on a generated graph (weights 1 … 255 by InsertWeights)."""
        h = C.c_void_p()
        gen = GEN_UNIFORM if generator in ("uniform", "u", GEN_UNIFORM) else GEN_KRONECKER
        _check(lib().gmsx_csr_generate_weighted(gen, scale, degree, relabel, threads, C.byref(h)), "gmsx_csr_generate_weighted")
        return cls(h)

    @classmethod
    def from_weighted_edges(cls, src, dst, w=None, num_nodes=-1, symmetrize=True, relabel=RELABEL_NEVER):
        """gmsx_csr_from_weighted_edges; w = None: InsertWeights over the list."""
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        ww = None if w is None else np.ascontiguousarray(w, dtype=np.int32)
        pad = np.zeros(1, np.int32)
        h = C.c_void_p()
        _check(lib().gmsx_csr_from_weighted_edges(num_nodes, src.size, (src if src.size else pad).ctypes.data_as(C.c_void_p),
                                                  (dst if dst.size else pad).ctypes.data_as(C.c_void_p),
                                                  None if ww is None else (ww if ww.size else pad).ctypes.data_as(C.c_void_p),
                                                  int(symmetrize), relabel, C.byref(h)), "gmsx_csr_from_weighted_edges")
        return cls(h)

    @classmethod
    def load_weighted(cls, path, symmetrize=True, relabel=RELABEL_NEVER):
        h = C.c_void_p()
        _check(lib().gmsx_csr_load_weighted(os.fsencode(path), int(symmetrize), relabel, C.byref(h)), "gmsx_csr_load_weighted")
        return cls(h)

    @classmethod
    def from_arrays_weighted(cls, off, neigh, weights):
        off = np.ascontiguousarray(off, dtype=np.int64)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        weights = np.ascontiguousarray(weights, dtype=np.int32)
        pad = np.zeros(1, np.int32)
        h = C.c_void_p()
        _check(lib().gmsx_csr_from_arrays_weighted(off.size - 1, off, (neigh if neigh.size else pad).ctypes.data_as(C.c_void_p),
                                                   (weights if weights.size else pad).ctypes.data_as(C.c_void_p), C.byref(h)),
               "gmsx_csr_from_arrays_weighted")
        return cls(h)

    def save_wsg(self, path):
        _check(lib().gmsx_csr_save_wsg(self._h, os.fsencode(path)), "gmsx_csr_save_wsg")

    def weights(self):
        """int32[nnz] view of the weight array (valid while this object lives), or None for an unweighted CSR."""
        p = lib().gmsx_csr_weights(self._h)
        if not p:
            return None
        nnz = self.nnz
        return np.ctypeslib.as_array(p, shape=(nnz,)) if nnz else np.zeros(0, dtype=np.int32)

    def weights_fingerprint(self):
        return int(lib().gmsx_csr_fingerprint(self._h, 2))

    def save_sg(self, path):
        _check(lib().gmsx_csr_save_sg(self._h, os.fsencode(path)), "gmsx_csr_save_sg")

    def save_sgx(self, path):
        """The mappable cache form (gmsx_csr_save_sgx); HostCSR.load of a ".sgx" maps it instead of reading it."""
        _check(lib().gmsx_csr_save_sgx(self._h, os.fsencode(path)), "gmsx_csr_save_sgx")

    @property
    def is_mapped(self):
        return bool(lib().gmsx_csr_is_mapped(self._h))

    def relabel_by_degree(self):
        h = C.c_void_p()
        _check(lib().gmsx_csr_relabel_by_degree(self._h, C.byref(h)), "gmsx_csr_relabel_by_degree")
        return HostCSR(h)

    def worth_relabelling(self):
        return bool(lib().gmsx_csr_worth_relabelling(self._h))

    @property
    def num_nodes(self):
        return lib().gmsx_csr_num_nodes(self._h)

    @property
    def num_edges(self):
        return lib().gmsx_csr_num_edges(self._h)

    @property
    def nnz(self):
        return lib().gmsx_csr_num_edges_directed(self._h)

    def offsets(self):
        """Zero-copy numpy view (valid while this object lives)."""
        return np.ctypeslib.as_array(lib().gmsx_csr_offsets(self._h), shape=(self.num_nodes + 1,))

    def neighbors(self):
        nnz = self.nnz
        if nnz == 0:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(lib().gmsx_csr_neighbors(self._h), shape=(nnz,))

    def merge_elements(self):
        return int(lib().gmsx_csr_merge_elements(self._h))

    def pick_sources(self, count, given=-1):
        """gmsx_csr_pick_sources: the first `count` picks of the reference's SourcePicker (int32[count]); given >= 0: `count` copies of it."""
        out = np.zeros(max(int(count), 1), dtype=np.int32)
        _check(lib().gmsx_csr_pick_sources(self._h, int(count), int(given), out.ctypes.data_as(C.c_void_p)), "gmsx_csr_pick_sources")
        return out[:int(count)]

    def fingerprint(self):
        return int(lib().gmsx_csr_fingerprint(self._h, 0)), int(lib().gmsx_csr_fingerprint(self._h, 1))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().gmsx_csr_free(self._h)
            self._h = None


def set_host_threads(n=0):
    """Threads of the host substrate (OpenMP); n <= 0 = all processors.  Returns the previous maximum."""
    return int(lib().gmsx_set_host_threads(int(n)))


def set_option(name, value):
    """gmsx_set_option: value None = back to the default.  Unknown names raise (GMSX_ERR_INVALID)."""
    _check(lib().gmsx_set_option(name.encode(), None if value is None else str(value).encode()), f"gmsx_set_option({name})")


def reset_options():
    lib().gmsx_reset_options()


def option_names():
    out, i, p = [], 0, C.c_char_p()
    while lib().gmsx_option_name(i, C.byref(p)) == 0:
        out.append(p.value.decode())
        i += 1
    return out


class options:
    """with capi.options(KC_MAXD=8, BK_BUDGET=64): … — sets the options for the block and restores the defaults after it."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            set_option(k, None)
        return False


def init(device=-1):
    _check(lib().gmsx_init(device), "gmsx_init")


def set_stream(stream_ptr):
    _check(lib().gmsx_set_stream(C.c_void_p(stream_ptr)), "gmsx_set_stream")


def hbm_read_probe(nbytes=4 << 30, iterations=20):
    """GB/s of a read-only stream over a buffer of `nbytes` (gmsx_hbm_read_probe)."""
    v = C.c_double(0)
    _check(lib().gmsx_hbm_read_probe(int(nbytes), int(iterations), C.byref(v)), "gmsx_hbm_read_probe")
    return v.value


def device_info():
    name = C.create_string_buffer(256)
    cu, mem = C.c_int(0), C.c_int64(0)
    _check(lib().gmsx_device_info(name, 256, C.byref(cu), C.byref(mem)), "gmsx_device_info")
    return {"name": name.value.decode(), "compute_units": cu.value, "hbm_bytes": mem.value}


class DeviceGraph:
    """gmsx_graph*: the HBM-resident graph (replaces SetGraph<Set>::FromCGraph)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def upload(cls, off, neigh, flags=UPLOAD_DEFAULT):
        off = np.ascontiguousarray(off, dtype=np.int64)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        h = C.c_void_p()
        _check(lib().gmsx_graph_upload(off.size - 1, off, neigh if neigh.size else np.zeros(1, np.int32), flags, C.byref(h)),
               "gmsx_graph_upload")
        g = cls(h)
        g._host = (weakref.ref(off), weakref.ref(neigh))  # what ktruss_edges(k) filters; weak: the handle keeps no host copy alive
        return g

    @classmethod
    def from_csr(cls, csr, flags=UPLOAD_DEFAULT, shard=None):
        """shard = (part, nparts): gmsx_graph_upload_csr_shard — the triangle-count containers of that shard's pivots only."""
        h = C.c_void_p()
        if shard is None:
            _check(lib().gmsx_graph_upload_csr(csr._h, flags, C.byref(h)), "gmsx_graph_upload_csr")
        else:
            _check(lib().gmsx_graph_upload_csr_shard(csr._h, flags, int(shard[0]), int(shard[1]), C.byref(h)), "gmsx_graph_upload_csr_shard")
        g = cls(h)
        g._host = (weakref.ref(csr),)
        return g

    num_nodes = property(lambda self: lib().gmsx_graph_num_nodes(self._h))
    num_edges = property(lambda self: lib().gmsx_graph_num_edges(self._h))
    device_bytes = property(lambda self: lib().gmsx_graph_device_bytes(self._h))
    max_out_degree = property(lambda self: lib().gmsx_graph_max_out_degree(self._h))
    tc_passes = property(lambda self: lib().gmsx_graph_tc_passes(self._h))

    def prepare(self, what=PREPARE_TC):
        """gmsx_graph_prepare: build the optional containers (triangle-count task lists) now instead of on first use."""
        _check(lib().gmsx_graph_prepare(self._h, what), "gmsx_graph_prepare")

    def tc_total(self, algo=TC_AUTO, stats=False):
        out, st = C.c_uint64(0), Stats()
        _check(lib().gmsx_tc_total(self._h, algo, C.byref(out), C.byref(st)), "gmsx_tc_total")
        return (int(out.value), st.as_dict()) if stats else int(out.value)

    def tc_partial(self, part, nparts, algo=TC_AUTO, stats=False):
        out, st = C.c_uint64(0), Stats()
        _check(lib().gmsx_tc_partial(self._h, algo, part, nparts, C.byref(out), C.byref(st)), "gmsx_tc_partial")
        return (int(out.value), st.as_dict()) if stats else int(out.value)

    BREAKDOWN = ["hub_rows_list", "hub_rows_bitset", "hub_rows_delta", "tail_rows_list", "tail_rows_delta", "entries", "pivot_containers",
                 "of_which_inline_rows", "light_streamed_hub_rows", "light_streamed_tail_rows", "light_pivot_lists_and_descriptors",
                 "count_entries", "count_inline_entries", "count_work_items", "count_light_streamed_members",
                 "core_matrix", "core_k", "gathered_rows", "row_line_bytes", "partial_line_entries", "gather_limit"]
    BREAKDOWN_BYTES = ("hub_rows_list", "hub_rows_bitset", "hub_rows_delta", "tail_rows_list", "tail_rows_delta", "entries", "pivot_containers",
                       "light_streamed_hub_rows", "light_streamed_tail_rows", "light_pivot_lists_and_descriptors", "core_matrix")  # these add up to stats.stream_bytes

    def tc_stream_breakdown(self):
        out = np.zeros(21, dtype=np.uint64)
        _check(lib().gmsx_tc_stream_breakdown(self._h, out), "gmsx_tc_stream_breakdown")
        return dict(zip(self.BREAKDOWN, (int(x) for x in out)))

    def tc_row_histogram(self):
        """(hist[5 classes][24 bins][rows, units], light[8]) — see gmsx_tc_row_histogram."""
        out = np.zeros(256, dtype=np.uint64)
        _check(lib().gmsx_tc_row_histogram(self._h, out), "gmsx_tc_row_histogram")
        return out[:240].reshape(5, 24, 2).astype(np.int64), out[240:].astype(np.int64)

    def tc_comembership(self, batch):
        """gmsx_tc_comembership: dict(entries, units, distinct_rows, batched_units, items) for batches of `batch` consecutive heavy pivots."""
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().gmsx_tc_comembership(self._h, int(batch), out), "gmsx_tc_comembership")
        return dict(entries=int(out[0]), units=int(out[1]), distinct_rows=int(out[2]), batched_units=int(out[3]), items=int(out[4]))

    def tc_vertex_count2(self, stats=False):
        c, st = np.zeros(self.num_nodes, dtype=np.int64), Stats()
        _check(lib().gmsx_tc_vertex_count2(self._h, c, C.byref(st)), "gmsx_tc_vertex_count2")
        return (c, st.as_dict()) if stats else c

    def intersect_count_batch(self, u, v, stats=False):
        u = np.ascontiguousarray(u, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.int32)
        out, st = np.zeros(max(u.size, 1), dtype=np.uint32), Stats()
        _check(lib().gmsx_intersect_count_batch(self._h, u.size, u if u.size else np.zeros(1, np.int32),
                                                v if v.size else np.zeros(1, np.int32), out, C.byref(st)),
               "gmsx_intersect_count_batch")
        out = out[:u.size]
        return (out, st.as_dict()) if stats else out

    def set_op_batch(self, op, u, v, stats=False):
        """gmsx_set_op_batch: (offsets[n_pairs + 1], ids) of N(u[i]) ∩ N(v[i]) (op = "intersect") or N(u[i]) \\ N(v[i]) ("difference"), ascending — the sizing
        call first, then the fill into an array of exactly that size."""
        code = {"intersect": SETOP_INTERSECT, "difference": SETOP_DIFFERENCE}[op]
        u = np.ascontiguousarray(u, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.int32)
        uu, vv = (u if u.size else np.zeros(1, np.int32)), (v if v.size else np.zeros(1, np.int32))
        off, st = np.zeros(u.size + 1, dtype=np.int64), Stats()
        _check(lib().gmsx_set_op_batch(self._h, code, u.size, uu, vv, off, None, 0, C.byref(st)), "gmsx_set_op_batch (sizing)")
        ids = np.zeros(max(int(off[-1]), 1), dtype=np.int32)
        _check(lib().gmsx_set_op_batch(self._h, code, u.size, uu, vv, off, ids.ctypes.data_as(C.c_void_p), int(off[-1]), C.byref(st)), "gmsx_set_op_batch")
        ids = ids[:int(off[-1])]
        return (off, ids, st.as_dict()) if stats else (off, ids)

    SIM = {"jaccard": 0, "overlap": 1, "adamic_adar": 2, "resource": 3, "common_neighbors": 4, "total_neighbors": 5, "pref_attachment": 6}

    def vertex_similarity_batch(self, metric, u, v, stats=False):
        u = np.ascontiguousarray(u, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.int32)
        out, st = np.zeros(max(u.size, 1), dtype=np.float64), Stats()
        m = self.SIM[metric] if isinstance(metric, str) else int(metric)
        _check(lib().gmsx_vertex_similarity_batch(self._h, m, u.size, u if u.size else np.zeros(1, np.int32),
                                                  v if v.size else np.zeros(1, np.int32), out, C.byref(st)), "gmsx_vertex_similarity_batch")
        out = out[:u.size]
        return (out, st.as_dict()) if stats else out

    def kclique_count(self, k, stats=False):
        ordered, cliques, st = C.c_uint64(0), C.c_uint64(0), Stats()
        _check(lib().gmsx_kclique_count(self._h, k, C.byref(ordered), C.byref(cliques), C.byref(st)), "gmsx_kclique_count")
        r = (int(ordered.value), int(cliques.value))
        return (r + (st.as_dict(),)) if stats else r

    def kclique_star_count(self, k, members=True, stats=False):
        """KCliqueStar::Par::CliqueStar in count mode: (number of k-clique-stars = C_k, total cardinality of the stars = (k+1) C_{k+1})."""
        stars, mem, st = C.c_uint64(0), C.c_uint64(0), Stats()
        _check(lib().gmsx_kclique_star_count(self._h, k, C.byref(stars), C.byref(mem) if members else None, C.byref(st)), "gmsx_kclique_star_count")
        r = (int(stars.value), int(mem.value) if members else None)
        return (r + (st.as_dict(),)) if stats else r

    def kclique_star_list_info(self, k, cliques_only=False, part=0, nparts=1):
        """gmsx_kclique_star_list, sizing call: {cliques, star_members, k, max_star} of shard (part, nparts)."""
        info = KcliqueStarListInfo()
        flags = KCSTAR_CLIQUES_ONLY if cliques_only else KCSTAR_DEFAULT
        _check(lib().gmsx_kclique_star_list(self._h, k, flags, part, nparts, None, None, None, 0, 0, C.byref(info), None),
               "gmsx_kclique_star_list (sizing)")
        return info.as_dict()

    def kclique_star_list(self, k, cliques_only=False, part=0, nparts=1, stats=False):
        """gmsx_kclique_star_list: the (clique, star) pairs of shard (part, nparts) as (cliques int32[C, k], star_offsets int64[C + 1],
        star_members int32[M]) — star i is star_members[star_offsets[i]:star_offsets[i + 1]]; all ids ascending caller ids.  With
        cliques_only the last two are None (k-clique listing).  The sizing call, then the fill into arrays of exactly that size."""
        info, st = KcliqueStarListInfo(), Stats()
        flags = KCSTAR_CLIQUES_ONLY if cliques_only else KCSTAR_DEFAULT
        _check(lib().gmsx_kclique_star_list(self._h, k, flags, part, nparts, None, None, None, 0, 0, C.byref(info), C.byref(st)),
               "gmsx_kclique_star_list (sizing)")
        sizing = st.as_dict()
        nc, nm = int(info.cliques), int(info.star_members)
        cl = np.zeros(max(nc * k, 1), dtype=np.int32)
        soff = mem = None
        if not cliques_only:
            soff = np.zeros(nc + 1, dtype=np.int64)
            mem = np.zeros(max(nm, 1), dtype=np.int32)
        _check(lib().gmsx_kclique_star_list(self._h, k, flags, part, nparts, cl.ctypes.data_as(C.c_void_p),
                                            None if cliques_only else soff.ctypes.data_as(C.c_void_p),
                                            None if cliques_only else mem.ctypes.data_as(C.c_void_p), nc, nm, C.byref(info), C.byref(st)),
               "gmsx_kclique_star_list")
        cl = cl[:nc * k].reshape(nc, k)
        if mem is not None:
            mem = mem[:nm]
        if stats:
            return cl, soff, mem, {"sizing": sizing, "fill": st.as_dict(), "info": info.as_dict()}
        return cl, soff, mem

    def kclique_partial(self, k, part, nparts, stats=False):
        out, st = C.c_uint64(0), Stats()
        _check(lib().gmsx_kclique_partial(self._h, k, part, nparts, C.byref(out), C.byref(st)), "gmsx_kclique_partial")
        return (int(out.value), st.as_dict()) if stats else int(out.value)

    def bk_count(self, rank=None, stats=False):
        out, st = C.c_uint64(0), Stats()
        rp = None
        if rank is not None:
            rank = np.ascontiguousarray(rank, dtype=np.int32)
            rp = rank.ctypes.data_as(C.c_void_p)
        _check(lib().gmsx_bk_count(self._h, rp, C.byref(out), C.byref(st)), "gmsx_bk_count")
        return (int(out.value), st.as_dict()) if stats else int(out.value)

    def bk_partial(self, part, nparts, rank=None, stats=False):
        out, st = C.c_uint64(0), Stats()
        rp = None
        if rank is not None:
            rank = np.ascontiguousarray(rank, dtype=np.int32)
            rp = rank.ctypes.data_as(C.c_void_p)
        _check(lib().gmsx_bk_partial(self._h, rp, part, nparts, C.byref(out), C.byref(st)), "gmsx_bk_partial")
        return (int(out.value), st.as_dict()) if stats else int(out.value)

    def bk_list_info(self, rank=None, part=0, nparts=1):
        """gmsx_bk_list, sizing call: {cliques, members, max_size, size_hist[65]} of shard (part, nparts)."""
        info = BkListInfo()
        rp = None
        if rank is not None:
            rank = np.ascontiguousarray(rank, dtype=np.int32)
            rp = rank.ctypes.data_as(C.c_void_p)
        _check(lib().gmsx_bk_list(self._h, rp, part, nparts, None, None, 0, 0, C.byref(info), None), "gmsx_bk_list (sizing)")
        return info.as_dict()

    def bk_list(self, rank=None, part=0, nparts=1, stats=False):
        """gmsx_bk_list: the maximal cliques of shard (part, nparts) as (offsets int64[n + 1], members int32[m]) — clique i is
        members[offsets[i]:offsets[i + 1]], ascending caller ids.  The sizing call, then the fill into arrays of exactly that size."""
        info, st = BkListInfo(), Stats()
        rp = None
        if rank is not None:
            rank = np.ascontiguousarray(rank, dtype=np.int32)
            rp = rank.ctypes.data_as(C.c_void_p)
        _check(lib().gmsx_bk_list(self._h, rp, part, nparts, None, None, 0, 0, C.byref(info), C.byref(st)), "gmsx_bk_list (sizing)")
        sizing = st.as_dict()
        off = np.zeros(int(info.cliques) + 1, dtype=np.int64)
        mem = np.zeros(max(int(info.members), 1), dtype=np.int32)
        _check(lib().gmsx_bk_list(self._h, rp, part, nparts, off.ctypes.data_as(C.c_void_p), mem.ctypes.data_as(C.c_void_p), off.size,
                                  int(info.members), C.byref(info), C.byref(st)), "gmsx_bk_list")
        mem = mem[:int(info.members)]
        if stats:
            return off, mem, {"sizing": sizing, "fill": st.as_dict(), "info": info.as_dict()}
        return off, mem

    def adg_rank(self, epsilon=0.001, rank_format=True, stats=False):
        """gmsx_adg_rank: (rank or order vector, number of peeling rounds)"""
        out, rounds, st = np.zeros(max(self.num_nodes, 1), dtype=np.int32), C.c_int32(0), Stats()
        _check(lib().gmsx_adg_rank(self._h, float(epsilon), int(bool(rank_format)), out, C.byref(rounds), C.byref(st)), "gmsx_adg_rank")
        r = (out[:self.num_nodes], int(rounds.value))
        return (r + (st.as_dict(),)) if stats else r

    def tc_ordering(self, stats=False):
        out, st = np.zeros(max(self.num_nodes, 1), dtype=np.int32), Stats()
        _check(lib().gmsx_tc_ordering(self._h, out, C.byref(st)), "gmsx_tc_ordering")
        out = out[:self.num_nodes]
        return (out, st.as_dict()) if stats else out

    def core_decomposition(self, order=True, rank_format=True, stats=False):
        """gmsx_core_decomposition: (core numbers int32[n], exact degeneracy order as rank or order vector — None with order=False —,
        {degeneracy, levels, rounds, top_core})."""
        n = self.num_nodes
        core, info, st = np.zeros(max(n, 1), dtype=np.int32), CoreInfo(), Stats()
        ordv = np.zeros(max(n, 1), dtype=np.int32) if order else None
        _check(lib().gmsx_core_decomposition(self._h, core.ctypes.data_as(C.c_void_p), ordv.ctypes.data_as(C.c_void_p) if order else None,
                                             int(bool(rank_format)), C.byref(info), C.byref(st)), "gmsx_core_decomposition")
        r = (core[:n], ordv[:n] if order else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def degree_rank(self, rank_format=True, stats=False):
        """gmsx_degree_rank: the vertices by ascending (degree, id) as a rank or an order vector."""
        out, st = np.zeros(max(self.num_nodes, 1), dtype=np.int32), Stats()
        _check(lib().gmsx_degree_rank(self._h, int(bool(rank_format)), out, C.byref(st)), "gmsx_degree_rank")
        out = out[:self.num_nodes]
        return (out, st.as_dict()) if stats else out

    def order_quality(self, ordering, rank_format=True, core_number=None, later=False, stats=False):
        """gmsx_order_quality: the info dict of `ordering` graded against core_number (None: the exact degeneracy, computed on the device);
        with later=True (info, later int32[n])."""
        n = self.num_nodes
        ordering = np.ascontiguousarray(ordering, dtype=np.int32)
        if ordering.size != n:
            raise GmsxError(ERR_INVALID, "gmsx_order_quality (ordering must have n entries)")
        lat = np.zeros(max(n, 1), dtype=np.int32) if later else None
        info, st = OrderQualityInfo(), Stats()
        op = ordering.ctypes.data_as(C.c_void_p) if n else np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)
        _check(lib().gmsx_order_quality(self._h, op, int(bool(rank_format)), -1 if core_number is None else int(core_number),
                                        lat.ctypes.data_as(C.c_void_p) if later else None, C.byref(info), C.byref(st)), "gmsx_order_quality")
        r = (info.as_dict(), lat[:n]) if later else (info.as_dict(),)
        if stats:
            r = r + (st.as_dict(),)
        return r if len(r) > 1 else r[0]

    def coloring_jp(self, ordering=None, rank_format=True, want_rounds=False, stats=False):
        """gmsx_coloring_jp: (coloring int32[n], {colors, rounds, max_pred, first_round}) — Jones–Plassmann under `ordering` (a rank or an order
        vector; the vertex of the highest position is coloured first; None = order[v] = v); with want_rounds=True (coloring, round_of, info)."""
        n = self.num_nodes
        op = None
        if ordering is not None:
            ordering = np.ascontiguousarray(ordering, dtype=np.int32)
            if ordering.size != n:
                raise GmsxError(ERR_INVALID, "gmsx_coloring_jp (ordering must have n entries)")
            op = ordering.ctypes.data_as(C.c_void_p) if n else None
        col = np.zeros(max(n, 1), dtype=np.int32)
        rnd = np.zeros(max(n, 1), dtype=np.int32) if want_rounds else None
        info, st = ColoringInfo(), Stats()
        _check(lib().gmsx_coloring_jp(self._h, op, int(bool(rank_format)), col.ctypes.data_as(C.c_void_p),
                                      rnd.ctypes.data_as(C.c_void_p) if want_rounds else None, C.byref(info), C.byref(st)), "gmsx_coloring_jp")
        r = (col[:n], rnd[:n], info.as_dict()) if want_rounds else (col[:n], info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def coloring_verify(self, coloring, stats=False):
        """gmsx_coloring_verify: {conflicts, invalid, max_color, distinct, max_degree} of a colouring (int32[n]); GCVerifierMaxColor(g, c, m) is
        invalid == 0 and conflicts == 0 and max_color <= m."""
        coloring = np.ascontiguousarray(coloring, dtype=np.int32)
        if coloring.size != self.num_nodes:
            raise GmsxError(ERR_INVALID, "gmsx_coloring_verify (coloring must have n entries)")
        out, st = ColoringCheck(), Stats()
        _check(lib().gmsx_coloring_verify(self._h, coloring.ctypes.data_as(C.c_void_p) if coloring.size else None, C.byref(out), C.byref(st)),
               "gmsx_coloring_verify")
        return (out.as_dict(), st.as_dict()) if stats else out.as_dict()

    def color_order(self, heuristic, epsilon=0.001):
        """The rank vector of a colouring heuristic, composed from the existing producers (rank format; None for "id"): "ff" = n-1-v (first-fit in
        id order, graph_coloring_naive_sequential), "lf" = gmsx_degree_rank (largest first), "sl" = gmsx_core_decomposition's order (smallest last),
        "adg" = gmsx_adg_rank(epsilon)."""
        n = self.num_nodes
        if heuristic == "id":
            return None
        if heuristic == "ff":
            return np.arange(n - 1, -1, -1, dtype=np.int32)
        if heuristic == "lf":
            return self.degree_rank(rank_format=True)
        if heuristic == "sl":
            return self.core_decomposition(order=True, rank_format=True)[1]
        if heuristic == "adg":
            return self.adg_rank(epsilon, rank_format=True)[0]
        raise GmsxError(ERR_INVALID, f"color (heuristic must be one of {COLOR_HEURISTICS})")

    def color(self, heuristic, epsilon=0.001):
        """Jones–Plassmann under one of COLOR_HEURISTICS: (coloring int32[n], info dict)."""
        return self.coloring_jp(self.color_order(heuristic, epsilon), rank_format=True)

    def edge_support(self, stats=False):
        """gmsx_edge_support: (support int32[nnz] — |N(u) ∩ N(v)| per arc of the uploaded CSR, both arcs of an edge alike —, triangles)."""
        nnz = 2 * self.num_edges
        sup, tri, st = np.zeros(max(nnz, 1), dtype=np.int32), C.c_uint64(0), Stats()
        _check(lib().gmsx_edge_support(self._h, sup.ctypes.data_as(C.c_void_p), C.byref(tri), C.byref(st)), "gmsx_edge_support")
        r = (sup[:nnz], int(tri.value))
        return (r + (st.as_dict(),)) if stats else r

    def truss_decomposition(self, rounds=False, stats=False):
        """gmsx_truss_decomposition: (truss int32[nnz] per arc of the uploaded CSR, {max_truss, levels, rounds, max_support, top_edges,
        triangles}); with rounds=True (truss, round_of, info)."""
        nnz = 2 * self.num_edges
        tr = np.zeros(max(nnz, 1), dtype=np.int32)
        rnd = np.zeros(max(nnz, 1), dtype=np.int32) if rounds else None
        info, st = TrussInfo(), Stats()
        _check(lib().gmsx_truss_decomposition(self._h, tr.ctypes.data_as(C.c_void_p), rnd.ctypes.data_as(C.c_void_p) if rounds else None,
                                              C.byref(info), C.byref(st)), "gmsx_truss_decomposition")
        r = (tr[:nnz], rnd[:nnz], info.as_dict()) if rounds else (tr[:nnz], info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def _host_csr(self):
        """(off, neigh) of the CSR this graph was uploaded from, while the caller still holds it (the handle keeps only weak references)"""
        refs = [r() for r in getattr(self, "_host", ())]
        if len(refs) == 1 and refs[0] is not None and getattr(refs[0], "_h", None):
            return refs[0].offsets(), refs[0].neighbors()
        if len(refs) == 2 and refs[0] is not None and refs[1] is not None:
            return refs[0], refs[1]
        raise GmsxError(ERR_INVALID, "ktruss_edges (the uploaded CSR is gone from the host: pass off and neigh)")

    def ktruss_edges(self, k, off=None, neigh=None, truss=None):
        """The k-truss as an edge list: (u, v) int32 arrays of the u < v edges with truss >= k, in CSR order.  A host-side filter of
        truss_decomposition (or of `truss`, a per-arc array it returned earlier) over the CSR the graph was uploaded from: the handle keeps no
        host copy, so ktruss_edges(k) works while the caller still holds that CSR, and off / neigh hand its arrays over otherwise."""
        if off is None or neigh is None:
            off, neigh = self._host_csr()
        off, neigh = np.asarray(off, dtype=np.int64), np.asarray(neigh, dtype=np.int32)
        if truss is None:
            truss = self.truss_decomposition()[0]
        if off.size != self.num_nodes + 1 or neigh.size != truss.size or (off.size and int(off[-1]) != neigh.size):
            raise GmsxError(ERR_INVALID, "ktruss_edges (off / neigh must be the uploaded CSR)")
        src = np.repeat(np.arange(off.size - 1, dtype=np.int32), np.diff(off))
        keep = (src < neigh) & (truss >= int(k))
        return src[keep], neigh[keep]

    def link_prediction(self, metric, q, part=0, nparts=1, stats=False):
        """gmsx_link_prediction: the q best-scoring non-edges under `metric` (a SIM_* value or one of SIM_METRICS' names), worst first:
        (u int32[found], v int32[found], scores float64[found], info dict)."""
        metric = SIM_METRICS.get(metric, metric) if isinstance(metric, str) else int(metric)
        q = int(q)
        if q > (1 << 27):  # the library's limit (gmsx.h): refused here, before q slots are allocated for nothing
            raise GmsxError(ERR_UNSUPPORTED, "gmsx_link_prediction (q > 2^27)")
        cap = max(q, 1)  # (q < 1 is refused by the library)
        u, v, sc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        info, st = LinkPredictionInfo(), Stats()
        _check(lib().gmsx_link_prediction(self._h, metric, q, int(part), int(nparts), u.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                          sc.ctypes.data_as(C.c_void_p), cap, C.byref(info), C.byref(st)), "gmsx_link_prediction")
        f = int(info.found)
        r = (u[:f].copy(), v[:f].copy(), sc[:f].copy(), info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def link_prediction_precision(self, u, v, stats=False):
        """gmsx_link_prediction_precision with this graph as g_test: {true_positives, true_count, precision, recall} of the predicted list."""
        u, v = np.ascontiguousarray(u, dtype=np.int32), np.ascontiguousarray(v, dtype=np.int32)
        if u.size != v.size:
            raise GmsxError(ERR_INVALID, "gmsx_link_prediction_precision (u and v must have the same length)")
        tp, tc, pr, rc, st = C.c_int64(0), C.c_int64(0), C.c_double(0.0), C.c_double(0.0), Stats()
        pu = u.ctypes.data_as(C.c_void_p) if u.size else None
        pv = v.ctypes.data_as(C.c_void_p) if v.size else None
        _check(lib().gmsx_link_prediction_precision(self._h, int(u.size), pu, pv, C.byref(tp), C.byref(tc), C.byref(pr), C.byref(rc), C.byref(st)),
               "gmsx_link_prediction_precision")
        r = {"true_positives": int(tp.value), "true_count": int(tc.value), "precision": float(pr.value), "recall": float(rc.value)}
        return (r, st.as_dict()) if stats else r

    def subgraph_match_info(self, pattern, induced=True, first=False, part=0, nparts=1, stats=False):
        """gmsx_subgraph_match with maps = NULL: {embeddings, tasks, k, order} of shard (part, nparts) — the count, or with first=True the
        existence answer (embeddings 0 or 1)."""
        off, neigh, k, po, pn = _pattern_args(pattern)
        flags = (0 if induced else SGM_MONO) | (SGM_FIRST if first else 0)
        info, st = SubgraphInfo(), Stats()
        _check(lib().gmsx_subgraph_match(self._h, k, po, pn, flags, int(part), int(nparts), None, 0, C.byref(info), C.byref(st)),
               "gmsx_subgraph_match (sizing)")
        return (info.as_dict(), st.as_dict()) if stats else info.as_dict()

    def subgraph_match(self, pattern, induced=True, first=False, part=0, nparts=1, stats=False):
        """gmsx_subgraph_match: the embeddings of `pattern` (a HostCSR, an (offsets, neigh) pair or an edge list) in shard (part, nparts) as an
        (E, k) int32 array — row i is embedding i, column p the image of pattern vertex p; rows ascending in the matching order.  induced=False:
        GMSX_SGM_MONO.  first=True: GMSX_SGM_FIRST, one call, E is 0 or 1.  Otherwise the sizing call, then the fill into an array of exactly
        that size."""
        off, neigh, k, po, pn = _pattern_args(pattern)
        flags = (0 if induced else SGM_MONO) | (SGM_FIRST if first else 0)
        info, st = SubgraphInfo(), Stats()
        sizing = None
        if first:
            ne = 1
        else:
            _check(lib().gmsx_subgraph_match(self._h, k, po, pn, flags, int(part), int(nparts), None, 0, C.byref(info), C.byref(st)),
                   "gmsx_subgraph_match (sizing)")
            sizing = st.as_dict()
            ne = int(info.embeddings)
        maps = np.zeros(max(ne * k, 1), dtype=np.int32)
        _check(lib().gmsx_subgraph_match(self._h, k, po, pn, flags, int(part), int(nparts), maps.ctypes.data_as(C.c_void_p), ne, C.byref(info),
                                         C.byref(st)), "gmsx_subgraph_match")
        ne = int(info.embeddings)
        maps = maps[:ne * k].reshape(ne, k)
        if stats:
            return maps, {"sizing": sizing, "fill": st.as_dict(), "info": info.as_dict()}
        return maps

    def connected_components(self, arc_keep=None, stats=False):
        """gmsx_connected_components: (label int32[n] — the smallest vertex id of every vertex's component —, {components, singletons, largest,
        kept_edges, largest_label, passes}).  arc_keep: nnz bytes parallel to the uploaded CSR's neigh; an edge is kept if either arc's byte is
        non-zero; None = every edge."""
        n, nnz = self.num_nodes, 2 * self.num_edges
        keep = None
        if arc_keep is not None:
            keep = np.ascontiguousarray(arc_keep, dtype=np.uint8)
            if keep.size != nnz:
                raise GmsxError(ERR_INVALID, "gmsx_connected_components (arc_keep must have one byte per arc)")
            if nnz == 0:
                keep = np.zeros(1, dtype=np.uint8)
        label, info, st = np.zeros(max(n, 1), dtype=np.int32), ComponentsInfo(), Stats()
        _check(lib().gmsx_connected_components(self._h, keep.ctypes.data_as(C.c_void_p) if keep is not None else None,
                                               label.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(st)), "gmsx_connected_components")
        r = (label[:n], info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def jarvis_patrick(self, metric, threshold, want_mask=False, stats=False):
        """gmsx_jarvis_patrick: (label, info) of the components over the edges whose endpoints score >= threshold under `metric` (a GMSX_SIM_*
        value or a name of SIM / SIM_METRICS); with want_mask=True (label, info, mask uint8[nnz]), the kept arcs."""
        if isinstance(metric, str):
            metric = self.SIM[metric] if metric in self.SIM else SIM_METRICS[metric]
        n, nnz = self.num_nodes, 2 * self.num_edges
        label, info, st = np.zeros(max(n, 1), dtype=np.int32), ComponentsInfo(), Stats()
        mask = np.zeros(max(nnz, 1), dtype=np.uint8) if want_mask else None
        _check(lib().gmsx_jarvis_patrick(self._h, int(metric), float(threshold), label.ctypes.data_as(C.c_void_p),
                                         mask.ctypes.data_as(C.c_void_p) if want_mask else None, C.byref(info), C.byref(st)), "gmsx_jarvis_patrick")
        r = (label[:n], info.as_dict()) + ((mask[:nnz],) if want_mask else ())
        return (r + (st.as_dict(),)) if stats else r

    def bfs(self, source, want_depth=True, want_parent=True, stats=False):
        """gmsx_bfs from `source`: (depth int32[n] or None, parent int32[n] or None, {reached, reached_arcs, depth_sum, widest, levels,
        widest_level, bottom_up_levels}).  parent[v] is the smallest-id neighbour of v one level up; -1 = unreachable."""
        n = self.num_nodes
        depth = np.zeros(max(n, 1), dtype=np.int32) if want_depth else None
        parent = np.zeros(max(n, 1), dtype=np.int32) if want_parent else None
        info, st = BfsInfo(), Stats()
        _check(lib().gmsx_bfs(self._h, int(source), depth.ctypes.data_as(C.c_void_p) if want_depth else None,
                              parent.ctypes.data_as(C.c_void_p) if want_parent else None, C.byref(info), C.byref(st)), "gmsx_bfs")
        r = (depth[:n] if want_depth else None, parent[:n] if want_parent else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def betweenness(self, sources, exclude_source=False, normalize=False, stats=False):
        """gmsx_betweenness over the listed sources: (scores float64[n], {sources, reached_total, max_levels, max_score, max_sigma})."""
        n = self.num_nodes
        src = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        flags = (BC_EXCLUDE_SOURCE if exclude_source else 0) | (BC_NORMALIZE_MAX if normalize else 0)
        scores, info, st = np.zeros(max(n, 1), dtype=np.float64), BcInfo(), Stats()
        _check(lib().gmsx_betweenness(self._h, src.size, src.ctypes.data_as(C.c_void_p) if src.size else None, flags,
                                      scores.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(st)), "gmsx_betweenness")
        r = (scores[:n], info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def bfs_multi(self, sources, want_depth=False, want_vertex=True, stats=False):
        """gmsx_bfs_multi over the listed sources: (per_source — a structured array of BFS_SOURCE_DTYPE, one record per list entry —,
        depth int32[len(sources), n] or None, (dist_sum int64[n], reach int32[n], far int32[n]) or None, {sources, passes, reached_total,
        max_levels, max_far, push_levels, pull_levels})."""
        n = self.num_nodes
        src = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        per = np.zeros(max(src.size, 1), dtype=BFS_SOURCE_DTYPE)
        depth = np.zeros(max(src.size * n, 1), dtype=np.int32) if want_depth else None
        dist = np.zeros(max(n, 1), dtype=np.int64) if want_vertex else None
        reach = np.zeros(max(n, 1), dtype=np.int32) if want_vertex else None
        far = np.zeros(max(n, 1), dtype=np.int32) if want_vertex else None
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        info, st = BfsMultiInfo(), Stats()
        _check(lib().gmsx_bfs_multi(self._h, src.size, p(src) if src.size else None, p(per), p(depth), p(dist), p(reach), p(far), C.byref(info),
                                    C.byref(st)), "gmsx_bfs_multi")
        r = (per[:src.size], depth[:src.size * n].reshape(src.size, n) if want_depth else None,
             (dist[:n], reach[:n], far[:n]) if want_vertex else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def pagerank(self, damping=0.85, max_iters=20, tolerance=1e-4, teleport=None, dangling=False, float32=False, stats=False):
        """gmsx_pagerank: (scores float64[n], {iterations, converged, argmax, error, sum, max_score, isolated}).  teleport: n non-negative
        weights (normalised by the library), None = uniform.  The defaults are the reference's (pr.cc: kDamp, -i 20, -t 1e-4)."""
        n = self.num_nodes
        tp = None if teleport is None else np.ascontiguousarray(teleport, dtype=np.float64).reshape(-1)
        if tp is not None and tp.size != n:
            raise ValueError("teleport must have one entry per vertex")
        flags = (PR_DANGLING if dangling else 0) | (PR_FLOAT32 if float32 else 0)
        scores, info, st = np.zeros(max(n, 1), dtype=np.float64), PagerankInfo(), Stats()
        _check(lib().gmsx_pagerank(self._h, float(damping), int(max_iters), float(tolerance), tp.ctypes.data_as(C.c_void_p) if tp is not None and n else None,
                                   flags, scores.ctypes.data_as(C.c_void_p), C.byref(info), C.byref(st)), "gmsx_pagerank")
        r = (scores[:n], info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def pagerank_residual(self, scores, damping=0.85, teleport=None, dangling=False, float32=False, stats=False):
        """gmsx_pagerank_residual: Σ_u |one sweep over `scores` - scores| (the reference's PRVerifier accepts scores iff this is below its tolerance)."""
        n = self.num_nodes
        sc = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
        tp = None if teleport is None else np.ascontiguousarray(teleport, dtype=np.float64).reshape(-1)
        if sc.size != n or (tp is not None and tp.size != n):
            raise ValueError("scores and teleport must have one entry per vertex")
        flags = (PR_DANGLING if dangling else 0) | (PR_FLOAT32 if float32 else 0)
        out, st = C.c_double(0.0), Stats()
        _check(lib().gmsx_pagerank_residual(self._h, sc.ctypes.data_as(C.c_void_p) if n else None, float(damping),
                                            tp.ctypes.data_as(C.c_void_p) if tp is not None and n else None, flags, C.byref(out), C.byref(st)),
               "gmsx_pagerank_residual")
        return (out.value, st.as_dict()) if stats else out.value

    def set_weights(self, w):
        """gmsx_graph_set_weights: int32 w[nnz] parallel to the uploaded neighbour array; None detaches."""
        if w is None:
            _check(lib().gmsx_graph_set_weights(self._h, None), "gmsx_graph_set_weights")
            return
        w = np.ascontiguousarray(w, dtype=np.int32)
        _check(lib().gmsx_graph_set_weights(self._h, (w if w.size else np.zeros(1, np.int32)).ctypes.data_as(C.c_void_p)), "gmsx_graph_set_weights")

    has_weights = property(lambda self: bool(lib().gmsx_graph_has_weights(self._h)))

    def sssp(self, source, delta=0, want_dist=True, want_parent=True, stats=False):
        """gmsx_sssp from `source`: (dist int64[n] or None, parent int32[n] or None, {reached, reached_arcs, dist_sum, max_dist, delta, buckets,
        rounds, relaxations, far_vertex, wide}).  -1 = unreachable; parent[v] is the smallest-id neighbour on a lightest path."""
        n = self.num_nodes
        dist = np.zeros(max(n, 1), dtype=np.int64) if want_dist else None
        parent = np.zeros(max(n, 1), dtype=np.int32) if want_parent else None
        info, st = SsspInfo(), Stats()
        _check(lib().gmsx_sssp(self._h, int(source), int(delta), dist.ctypes.data_as(C.c_void_p) if want_dist else None,
                               parent.ctypes.data_as(C.c_void_p) if want_parent else None, C.byref(info), C.byref(st)), "gmsx_sssp")
        r = (dist[:n] if want_dist else None, parent[:n] if want_parent else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def sssp_verify(self, source, dist, stats=False):
        """gmsx_sssp_verify of a caller's distances: {violated_arcs, untight, wrong_unreached, source_ok}."""
        d = np.ascontiguousarray(dist, dtype=np.int64)
        out, st = SsspCheck(), Stats()
        _check(lib().gmsx_sssp_verify(self._h, int(source), (d if d.size else np.zeros(1, np.int64)).ctypes.data_as(C.c_void_p), C.byref(out),
                                      C.byref(st)), "gmsx_sssp_verify")
        return (out.as_dict(), st.as_dict()) if stats else out.as_dict()

    def min_spanning_forest(self, maximum=False, want_edges=True, want_mask=False, want_labels=False, stats=False):
        """gmsx_min_spanning_forest over the attached weights: (u, v, w, mask, label, info[, stats]).  u, v, w: int32[edges], the forest's edges
        with u < v, ascending by (u, v), or None each; mask: uint8[nnz], 1 on both arcs of every forest edge, or None; label: int32[n], the
        smallest vertex id of every vertex's tree, or None; info: {edges, total_weight, trees, isolated, largest_tree, min_weight, max_weight,
        rounds}.  maximum=True: the maximum spanning forest (GMSX_MSF_MAXIMUM)."""
        n, nnz = self.num_nodes, 2 * self.num_edges
        eu, ev, ew = (np.zeros(max(n - 1, 1), dtype=np.int32) for _ in range(3)) if want_edges else (None, None, None)
        mask = np.zeros(max(nnz, 1), dtype=np.uint8) if want_mask else None
        label = np.zeros(max(n, 1), dtype=np.int32) if want_labels else None
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        info, st = MsfInfo(), Stats()
        _check(lib().gmsx_min_spanning_forest(self._h, MSF_MAXIMUM if maximum else 0, p(eu), p(ev), p(ew), p(mask), p(label), C.byref(info),
                                              C.byref(st)), "gmsx_min_spanning_forest")
        ne = int(info.edges)
        r = (eu[:ne] if want_edges else None, ev[:ne] if want_edges else None, ew[:ne] if want_edges else None,
             mask[:nnz] if want_mask else None, label[:n] if want_labels else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def label_propagation(self, weighted=False, coloring=None, max_sweeps=0, want_labels=True, stats=False):
        """gmsx_label_propagation: (label, info[, stats]).  label: int32[n], the community of every vertex as the id of one of its members (None
        with want_labels=False); info: {communities, largest, singletons, changes, first_sweep_changes, sweeps, colors, converged,
        largest_label}.  coloring: a proper colouring int32[n] with colours >= 1 that fixes the order of the asynchronous sweeps; None = the
        colouring coloring_jp() returns.  weighted=True sums the attached weights (GMSX_LP_WEIGHTED) instead of counting arcs."""
        n = self.num_nodes
        col = None if coloring is None else np.ascontiguousarray(coloring, dtype=np.int32)
        if col is not None and col.size != n:
            raise ValueError("coloring must have one entry per vertex")
        label = np.zeros(max(n, 1), dtype=np.int32) if want_labels else None
        info, st = LpInfo(), Stats()
        _check(lib().gmsx_label_propagation(self._h, LP_WEIGHTED if weighted else 0,
                                            (col if col.size else np.zeros(1, np.int32)).ctypes.data_as(C.c_void_p) if col is not None else None,
                                            int(max_sweeps), label.ctypes.data_as(C.c_void_p) if want_labels else None, C.byref(info), C.byref(st)),
               "gmsx_label_propagation")
        r = (label[:n] if want_labels else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def modularity(self, label, weighted=False, stats=False):
        """gmsx_modularity of a labelling int32[n] with labels in [0, n): {total_weight, intra_weight, sumsq_hi, sumsq_lo, sumsq, communities,
        largest, unstable, modularity}.  The integers are exact; modularity = I / W - S / W^2 is computed from them once."""
        lab = np.ascontiguousarray(label, dtype=np.int32)
        if lab.size != self.num_nodes:
            raise ValueError("label must have one entry per vertex")
        info, st = ModularityInfo(), Stats()
        _check(lib().gmsx_modularity(self._h, LP_WEIGHTED if weighted else 0, (lab if lab.size else np.zeros(1, np.int32)).ctypes.data_as(C.c_void_p),
                                     C.byref(info), C.byref(st)), "gmsx_modularity")
        return (info.as_dict(), st.as_dict()) if stats else info.as_dict()

    def greedy_matching(self, weighted=False, want_mate=True, want_edges=False, stats=False):
        """gmsx_greedy_matching: (mate, u, v, w, info[, stats]).  mate: int32[n], every vertex's partner or -1 (None with want_mate=False);
        u, v, w: int32[pairs], the pairs with u < v ascending by u and their weights, or None each; info: {pairs, total_weight, free_vertices,
        exposed, min_weight, max_weight, rounds}.  weighted=True orders the edges by the attached weights, heavier first (GMSX_MATCH_WEIGHTED);
        else every edge weighs 1.  The matching is the sequential greedy one under the strict order of gmsx.h: the same bytes in every run."""
        n = self.num_nodes
        mate = np.zeros(max(n, 1), dtype=np.int32) if want_mate else None
        eu, ev, ew = (np.zeros(max(n // 2, 1), dtype=np.int32) for _ in range(3)) if want_edges else (None, None, None)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        info, st = MatchingInfo(), Stats()
        _check(lib().gmsx_greedy_matching(self._h, MATCH_WEIGHTED if weighted else 0, p(mate), p(eu), p(ev), p(ew), C.byref(info), C.byref(st)),
               "gmsx_greedy_matching")
        ne = int(info.pairs)
        r = (mate[:n] if want_mate else None, eu[:ne] if want_edges else None, ev[:ne] if want_edges else None, ew[:ne] if want_edges else None,
             info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def matching_verify(self, mate, weighted=False, stats=False):
        """gmsx_matching_verify of a mate array int32[n] (-1 = free): {invalid, pairs, total_weight, free_vertices, augmentable, undominated}.
        invalid == 0 and undominated == 0 iff mate is the greedy matching under the order of gmsx.h; augmentable == 0 iff it is maximal."""
        m = np.ascontiguousarray(mate, dtype=np.int32)
        if m.size != self.num_nodes:
            raise ValueError("mate must have one entry per vertex")
        out, st = MatchingCheck(), Stats()
        _check(lib().gmsx_matching_verify(self._h, MATCH_WEIGHTED if weighted else 0, (m if m.size else np.zeros(1, np.int32)).ctypes.data_as(C.c_void_p),
                                          C.byref(out), C.byref(st)), "gmsx_matching_verify")
        return (out.as_dict(), st.as_dict()) if stats else out.as_dict()

    def biconnected_components(self, want_block=True, want_blocks_at=True, want_mask=False, stats=False):
        """gmsx_biconnected_components: (block, blocks_at, arc_keep, info[, stats]).  block: int32[nnz], the id of the block of every arc of the
        uploaded CSR (ids ascend with each block's smallest `u < v` arc); blocks_at: int32[n], the blocks that contain a vertex (>= 2: an
        articulation point); arc_keep: uint8[nnz], 0 on both arcs of a bridge, else 1 (want_mask=True); an output that was not asked for is
        None.  info: {blocks, bridges, articulation_points, largest_block_edges, largest_block_vertices, components, isolated,
        largest_block, max_blocks_at, levels}.  Facts about the graph: the same bytes in every run."""
        n, nnz = self.num_nodes, 2 * self.num_edges
        block = np.zeros(max(nnz, 1), dtype=np.int32) if want_block else None
        at = np.zeros(max(n, 1), dtype=np.int32) if want_blocks_at else None
        mask = np.zeros(max(nnz, 1), dtype=np.uint8) if want_mask else None
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        info, st = BiccInfo(), Stats()
        _check(lib().gmsx_biconnected_components(self._h, 0, p(block), p(at), p(mask), C.byref(info), C.byref(st)), "gmsx_biconnected_components")
        r = (block[:nnz] if want_block else None, at[:n] if want_blocks_at else None, mask[:nnz] if want_mask else None, info.as_dict())
        return (r + (st.as_dict(),)) if stats else r

    def cycle4_count(self, at_vertex=False, stats=False):
        """gmsx_cycle4_count: the 4-cycles of the graph; with at_vertex=True (cycles, int64[n] — the 4-cycles through every vertex of the
        uploaded CSR, which add up to 4 * cycles)."""
        n = self.num_nodes
        out, st = C.c_uint64(0), Stats()
        at = np.zeros(max(n, 1), dtype=np.int64) if at_vertex else None
        _check(lib().gmsx_cycle4_count(self._h, C.byref(out), at.ctypes.data_as(C.c_void_p) if at_vertex else None, C.byref(st)), "gmsx_cycle4_count")
        r = (int(out.value), at[:n]) if at_vertex else int(out.value)
        if stats:
            return (r + (st.as_dict(),)) if at_vertex else (r, st.as_dict())
        return r

    def cycle4_partial(self, part, nparts, stats=False):
        """gmsx_cycle4_partial: the 4-cycles whose source (their vertex of the smallest rank id) belongs to shard `part` of `nparts`."""
        out, st = C.c_uint64(0), Stats()
        _check(lib().gmsx_cycle4_partial(self._h, int(part), int(nparts), C.byref(out), C.byref(st)), "gmsx_cycle4_partial")
        return (int(out.value), st.as_dict()) if stats else int(out.value)

    def motif_census4(self, stats=False):
        """gmsx_motif_census4: {subgraphs: {motif: non-induced copies}, induced: {motif: induced copies}, wedges_walked, max_codegree} over the
        eight motifs of MOTIFS."""
        info, st = MotifInfo(), Stats()
        _check(lib().gmsx_motif_census4(self._h, C.byref(info), C.byref(st)), "gmsx_motif_census4")
        return (info.as_dict(), st.as_dict()) if stats else info.as_dict()

    def free(self):
        if getattr(self, "_h", None):
            lib().gmsx_graph_free(self._h)
            self._h = None

    def __del__(self):
        self.free()


class Comm:
    """gmsx_comm*: the native RCCL communicator of the path's single collective (one u64 all-reduce)."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(lib().gmsx_comm_unique_id(buf), "gmsx_comm_unique_id")
        return buf.raw

    @classmethod
    def init(cls, rank, nranks, uid):
        assert len(uid) == COMM_ID_BYTES
        h = C.c_void_p()
        _check(lib().gmsx_comm_init(rank, nranks, uid, C.byref(h)), "gmsx_comm_init")
        return cls(h)

    rank = property(lambda self: lib().gmsx_comm_rank(self._h))
    size = property(lambda self: lib().gmsx_comm_size(self._h))

    def allreduce_u64(self, value):
        v = C.c_uint64(value & 0xFFFFFFFFFFFFFFFF)
        _check(lib().gmsx_comm_allreduce_u64(self._h, C.byref(v)), "gmsx_comm_allreduce_u64")
        return int(v.value)

    def finalize(self):
        if getattr(self, "_h", None):
            _check(lib().gmsx_comm_finalize(self._h), "gmsx_comm_finalize")
            self._h = None
