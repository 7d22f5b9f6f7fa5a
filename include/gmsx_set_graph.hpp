// gmsx_set_graph.hpp — C++17 adaptor that plugs the gmsx C-ABI (gmsx.h) under GMS's compile-time Set / SGraph
// concept, so drivers written against the reference's templates instantiate unchanged with the graph types below.
//
// What the reference requires of a Set (union of testing/sets.cpp and the three algorithm families):
//   gms/representations/sets/sorted_set.h:21-272     (SortedSetBase)     — mirrored by gmsx::SortedSpanSet
//   gms/representations/sets/sorted_set_ref.h:9-78   (SortedSetRefBase)  — mirrored by gmsx::SortedSpanRef (borrowed view)
//   gms/representations/sets/roaring_set.h:15-229    (RoaringSetBase)    — mirrored by gmsx::RoaringSpanSet (uint32 iteration)
//   gms/representations/graphs/set_graph.h:86-118    (SetGraph)          — mirrored by gmsx::HipGraphT<Set>:
//        HipSetGraph = HipGraphT<SortedSpanSet>, HipRoaringGraph = HipGraphT<RoaringSpanSet>, HipSetRefGraph = HipGraphT<SortedSpanRef>
//
// ZERO-COPY: a row of the graph is a *view* (pointer + count, 16 bytes) into ONE adjacency array — the caller's CSRGraph /
// gmsx_csr memory when its rows are contiguous and sorted (the reference does the same for SetGraph<SortedSetRef>,
// set_graph.h:162-168), otherwise one private copy.  No per-row allocation, no second copy of the adjacency.  A set turns
// into an owning one only when it is mutated or produced by an operator.
//
// The per-element operators below run on the host (they exist so that every generic template still compiles and
// runs); the whole-graph algorithms — the hot path — are forwarded to the device through the C-ABI:
//   gmsx::count_total(g)                 -> gmsx_tc_total          (triangle_count/parallel/total.h:7-24)
//   gmsx::vertex_count2(g, out)          -> gmsx_tc_vertex_count2  (triangle_count/parallel/vertex.h:14-49)
//   gmsx::clique_count(g, k)             -> gmsx_kclique_count     (k_clique_count_set_based.h:19-31)
//   gmsx::clique_star_count(g, k)        -> gmsx_kclique_star_count (k_clique_star_list/parallel/recursive.h:19-35, count mode)
//   gmsx::clique_stars(g, k) / cliques(g, k) -> gmsx_kclique_star_list (k_clique_star_list/parallel/recursive.h:37-43: the pairs themselves)
//   gmsx::maximal_clique_count(g, rank)  -> gmsx_bk_count          (maximal_clique_enum/parallel/eppsteinPAR.h:18-53)
//   gmsx::adg_rank(g, eps, out)          -> gmsx_adg_rank          (preprocessing/parallel/degeneracy_approx_set.h:14-86)
//   gmsx::triangle_count_ordering(g,out) -> gmsx_tc_ordering       (preprocessing/parallel/triangle_count.h:11-30)
//   gmsx::core_numbers(g, out)           -> gmsx_core_decomposition (the core numbers behind preprocessing/sequential/degeneracy_matula.h:13-66; returns the degeneracy)
//   gmsx::degeneracy_order(g, out)       -> gmsx_core_decomposition (an exact degeneracy order; not Matula's own tie sequence, gmsx.h)
//   gmsx::degree_order(g, out)           -> gmsx_degree_rank       (preprocessing/parallel/degree.h:15-61)
//   gmsx::order_quality(g, order)        -> gmsx_order_quality     (preprocessing/util/core_number_evaluator.h:73-139)
//   gmsx::coloring(g, order) / coloring(g, "sl") -> gmsx_coloring_jp (non_set_based/coloring/coloring_jones_v3.h:38-68: Jones–Plassmann under a priority)
//   gmsx::coloring_check(g, coloring)    -> gmsx_coloring_verify   (non_set_based/coloring/coloring_common.h:102-157, 205-209: the verifiers as integers)
//   gmsx::edge_support(g, out)           -> gmsx_edge_support      (per arc |N(u) ∩ N(v)|: one Set::intersect_count per edge; no reference driver; returns the triangles)
//   gmsx::truss_numbers(g, out)          -> gmsx_truss_decomposition (the trussness per arc; returns the largest)
//   gmsx::ktruss_edges(g, k)             -> gmsx_truss_decomposition (the u < v edges of the k-truss, a host-side filter)
//   gmsx::connected_components(g, out)   -> gmsx_connected_components (representations/graphs/log_graph/cc.cc:40-72, ShiloachVishkin: out[v] = smallest id of v's component)
//   gmsx::jarvis_patrick(g, metric, threshold, out) -> gmsx_jarvis_patrick (the components over the edges whose endpoints are similar enough; no reference driver)
//   gmsx::ktruss_components(g, k, out)   -> gmsx_truss_decomposition + gmsx_connected_components (the communities of the k-truss: the mask truss >= k)
//   gmsx::bfs(g, source, parent)         -> gmsx_bfs                (representations/graphs/log_graph/bfs.cc:120-190, DOBFS: parent[v] = the smallest-id neighbour one level up)
//   gmsx::betweenness(g, sources, scores) -> gmsx_betweenness       (log_graph/bc.cc:89-153, Brandes from the listed sources, in double)
//   gmsx::bfs_multi(g, sources, per_source, …) -> gmsx_bfs_multi    (a BFS from every listed source, 64 per sweep: per-source sums, optional depths and per-vertex farness; no reference driver)
//   gmsx::closeness(g, sources, out_scores, harmonic = false) -> gmsx_bfs_multi (closeness or harmonic centrality of the listed sources; returns the largest)
//   gmsx::pagerank(g, scores, damping, max_iters, tolerance, …) -> gmsx_pagerank  (log_graph/pr.cc:34-61, PageRankPull; in double unless GMSX_PR_FLOAT32)
//   gmsx::pagerank_residual(g, scores, …) -> gmsx_pagerank_residual  (pr.cc:79-97, PRVerifier as a number);  gmsx::top_scores(scores, k): PrintTopScores' top k on the host
//   gmsx::set_weights(g, weights)        -> gmsx_graph_set_weights  (int32 weights parallel to g.neighbors(); what makes the graph a WGraph)
//   gmsx::sssp(g, source, dist, delta, …) -> gmsx_sssp               (log_graph/sssp.cc:54-134, DeltaStep; dist in 64 bits, -1 = unreachable)
//   gmsx::sssp_verify(g, source, dist)   -> gmsx_sssp_verify        (sssp.cc:145-175, SSSPVerifier)
//   gmsx::min_spanning_forest(g, edges, flags, info) -> gmsx_min_spanning_forest (the forest's (u, v, w), u < v, ascending; GMSX_MSF_MAXIMUM: the maximum one; no reference driver)
//   gmsx::msf_arc_mask(g, flags)         -> gmsx_min_spanning_forest (a byte per arc of g.neighbors(): 1 on both arcs of every forest edge — what gmsx_connected_components takes)
//   gmsx::label_propagation(g, label, flags, coloring, max_sweeps, info) -> gmsx_label_propagation (communities by asynchronous label propagation, colour class by colour class; no reference driver)
//   gmsx::modularity(g, label, flags)    -> gmsx_modularity         (W, I, Σ D_c² in 128 bits, unstable and Q = I / W - S / W² of any labelling)
//   gmsx::greedy_matching(g, mate, flags, edges, info) -> gmsx_greedy_matching (the greedy matching under a strict edge order; GMSX_MATCH_WEIGHTED: heavier first; no reference driver)
//   gmsx::matching_verify(g, mate, flags, out) -> gmsx_matching_verify (true iff mate is that matching: an O(m) certificate)
//   gmsx::biconnected_components(g, block, blocks_at, info) -> gmsx_biconnected_components (the block id of every arc of g.neighbors(), the blocks at every vertex; no reference driver)
//   gmsx::articulation_points(g)         -> gmsx_biconnected_components (the cut vertices, ascending)
//   gmsx::bridges(g)                     -> gmsx_biconnected_components (the bridges as (u, v), u < v, ascending)
//   gmsx::pick_sources(csr, count)       -> gmsx_csr_pick_sources   (gapbs/benchmark.h:51-75, SourcePicker)
//   gmsx::cycle4_count(g) / cycle4_count(g, at_vertex) -> gmsx_cycle4_count (the 4-cycles, and those through every vertex; no reference driver)
//   gmsx::motif_census4(g)               -> gmsx_motif_census4     (the eight 3- and 4-vertex motifs, non-induced and induced; no reference driver)
//   gmsx::link_prediction(g, metric, q)  -> gmsx_link_prediction  (set_based/link_prediction/link_prediction.h:42-101; the reference's padding reproduced)
//   gmsx::link_prediction_precision(g_test, edges) -> gmsx_link_prediction_precision (set_based/link_prediction/evaluation.h:99-124)
//   gmsx::subgraph_isomorphisms(g, pattern, flags) -> gmsx_subgraph_match (every embedding of a small connected pattern, induced or not; no reference driver lists them)
//   gmsx::subgraph_isomorphism(g, pattern) -> gmsx_subgraph_match, GMSX_SGM_FIRST (non_set_based/subgraphiso/vf2/sequential/vf2.hpp:39-81: the one mapping, target -> pattern)
// include/gmsx_gms_glue.hpp holds the explicit specialisations that route the reference's own function names to these
// (INTEGRATION.md §2).  Header-only; link with -lgmsx.
#pragma once

#include <algorithm>
#include <array>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "gmsx.h"

namespace gmsx {

using SetElement = int32_t;  // sorted_set.h:25, roaring_set.h:28

namespace detail {
inline void check(int rc, const char *what) {
    if (rc != GMSX_OK) {  // the reference's convention for loader / CLI failures: message + exit (gapbs/reader.h:45,228)
        std::fprintf(stderr, "gmsx: %s failed: %s\n", what, gmsx_strerror(rc));
        std::exit(-33);
    }
}
// the four merges of sorted_set_operations.h:29-106 on raw sorted ranges; `out` may alias `a` for intersect/difference
inline size_t isect_count(const SetElement *a, size_t na, const SetElement *b, size_t nb) {
    size_t i = 0, j = 0, c = 0;
    while (i < na && j < nb) {
        if (a[i] < b[j]) ++i;
        else if (b[j] < a[i]) ++j;
        else { ++c; ++i; ++j; }
    }
    return c;
}
inline size_t isect(const SetElement *a, size_t na, const SetElement *b, size_t nb, SetElement *out) {
    size_t i = 0, j = 0, c = 0;
    while (i < na && j < nb) {
        if (a[i] < b[j]) ++i;
        else if (b[j] < a[i]) ++j;
        else { out[c++] = a[i]; ++i; ++j; }
    }
    return c;
}
inline size_t diff(const SetElement *a, size_t na, const SetElement *b, size_t nb, SetElement *out) {
    size_t i = 0, j = 0, c = 0;
    while (i < na) {
        if (j == nb || a[i] < b[j]) out[c++] = a[i++];
        else if (b[j] < a[i]) ++j;
        else { ++i; ++j; }
    }
    return c;
}
inline size_t unite(const SetElement *a, size_t na, const SetElement *b, size_t nb, SetElement *out) {
    return size_t(std::set_union(a, a + na, b, b + nb, out) - out);
}
}  // namespace detail

// ------------------------------------------------------------------------------------------------------------------
// SpanSetT: sorted duplicate-free set of int32 that is either a borrowed VIEW of caller memory (cap_ == 0) or an owning
// buffer.  16 bytes.  Move-only like the reference's sets (copying is explicit via clone(), sorted_set.h:31-39,84-87).
// IterElem is what iteration yields: int32_t for the SortedSet flavour, uint32_t for the RoaringSet flavour
// (roaring_set.h:82-105 hands out Roaring's uint32 iterators).
// ------------------------------------------------------------------------------------------------------------------
template <class IterElem>
class SpanSetT {
   public:
    using SetElement = gmsx::SetElement;
    static_assert(sizeof(IterElem) == sizeof(gmsx::SetElement), "iteration element must be 32 bits wide");
    using Container = std::vector<SetElement>;
    using const_iterator = const IterElem *;

    SpanSetT() = default;
    SpanSetT(SpanSetT &&o) noexcept : p_(o.p_), n_(o.n_), cap_(o.cap_) { o.forget(); }
    SpanSetT &operator=(SpanSetT &&o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; n_ = o.n_; cap_ = o.cap_;
            o.forget();
        }
        return *this;
    }
    SpanSetT(const SpanSetT &) = delete;
    SpanSetT &operator=(const SpanSetT &) = delete;
    ~SpanSetT() { release(); }

    // copies; the input need not be sorted (sorted_set.h:64-66, roaring_set.h:49-54)
    SpanSetT(const SetElement *start, size_t count) { assign_unsorted(start, count); }
    explicit SpanSetT(const Container &c) { assign_unsorted(c.data(), c.size()); }
    explicit SpanSetT(Container &&c, bool sorted = false) {
        if (sorted) assign_sorted(c.data(), c.size()); else assign_unsorted(c.data(), c.size());
    }
    SpanSetT(std::initializer_list<SetElement> il) { assign_unsorted(il.begin(), il.size()); }
    explicit SpanSetT(SetElement single) { assign_sorted(&single, 1); }

    // zero-copy view of a sorted, duplicate-free range that outlives the set (a CSR row): sorted_set_ref.h:17-20 without the
    // in-place sort — canonical rows are sorted already
    static SpanSetT borrow(const SetElement *sorted_unique, size_t count) {
        SpanSetT s;
        s.p_ = const_cast<SetElement *>(sorted_unique);
        s.n_ = uint32_t(count);
        return s;
    }
    bool borrowed() const { return cap_ == 0 && n_ != 0; }

    SpanSetT clone() const { SpanSetT s; s.assign_sorted(p_, n_); return s; }
    static SpanSetT Range(unsigned bound) {  // sorted_set.h:257-262, roaring_set.h:219-224
        SpanSetT s;
        s.reserve(bound);
        for (unsigned i = 0; i < bound; ++i) s.p_[i] = SetElement(i);
        s.n_ = bound;
        return s;
    }

    size_t cardinality() const { return n_; }
    const_iterator begin() const { return reinterpret_cast<const IterElem *>(p_); }
    const_iterator end() const { return reinterpret_cast<const IterElem *>(p_) + n_; }
    const SetElement *data() const { return p_; }
    bool contains(SetElement e) const { return std::binary_search(p_, p_ + n_, e); }
    template <class T>
    void toArray(T *out) const {  // sorted_set.h:234-239 (memcpy), roaring_set.h:190-201 (toUint32Array)
        static_assert(sizeof(T) == sizeof(SetElement), "toArray needs a 32-bit element type");
        if (n_) std::memcpy(out, p_, size_t(n_) * sizeof(SetElement));
    }
    bool operator==(const SpanSetT &o) const { return n_ == o.n_ && (n_ == 0 || std::memcmp(p_, o.p_, size_t(n_) * sizeof(SetElement)) == 0); }
    bool operator!=(const SpanSetT &o) const { return !(*this == o); }

    // ---- intersection (sorted_set.h:160-182, roaring_set.h:134-152) ----
    template <class Other>
    size_t intersect_count(const Other &o) const { return detail::isect_count(p_, n_, o.data(), o.cardinality()); }
    template <class Other>
    SpanSetT intersect(const Other &o) const {
        SpanSetT r;
        r.reserve(std::min<size_t>(n_, o.cardinality()));
        r.n_ = uint32_t(detail::isect(p_, n_, o.data(), o.cardinality(), r.p_));
        return r;
    }
    void intersect_inplace(const SpanSetT &o) {
        if (cap_) n_ = uint32_t(detail::isect(p_, n_, o.p_, o.n_, p_));  // the write index never passes the read index
        else *this = intersect(o);
    }

    // ---- union (sorted_set.h:104-158, roaring_set.h:107-132) ----
    template <class Other>
    SpanSetT union_with(const Other &o) const {
        SpanSetT r;
        r.reserve(size_t(n_) + o.cardinality());
        r.n_ = uint32_t(detail::unite(p_, n_, o.data(), o.cardinality(), r.p_));
        return r;
    }
    SpanSetT union_with(SetElement e) const { SpanSetT r = clone(); r.union_inplace(e); return r; }
    void union_inplace(const SpanSetT &o) { *this = union_with(o); }
    void union_inplace(SetElement e) {
        const size_t pos = size_t(std::lower_bound(p_, p_ + n_, e) - p_);
        if (pos < n_ && p_[pos] == e) return;
        if (cap_ == 0 || n_ == cap_) grow(std::max<size_t>(4, size_t(n_) * 2));
        std::memmove(p_ + pos + 1, p_ + pos, (size_t(n_) - pos) * sizeof(SetElement));
        p_[pos] = e;
        ++n_;
    }
    template <class Other>
    size_t union_count(const Other &o) const { return size_t(n_) + o.cardinality() - intersect_count(o); }

    // ---- difference (sorted_set.h:184-216, roaring_set.h:154-178) ----
    template <class Other>
    SpanSetT difference(const Other &o) const {
        SpanSetT r;
        r.reserve(n_);
        r.n_ = uint32_t(detail::diff(p_, n_, o.data(), o.cardinality(), r.p_));
        return r;
    }
    SpanSetT difference(SetElement e) const { SpanSetT r = clone(); r.difference_inplace(e); return r; }
    void difference_inplace(const SpanSetT &o) {
        if (cap_) n_ = uint32_t(detail::diff(p_, n_, o.p_, o.n_, p_));
        else *this = difference(o);
    }
    void difference_inplace(SetElement e) {
        const size_t pos = size_t(std::lower_bound(p_, p_ + n_, e) - p_);
        if (pos == n_ || p_[pos] != e) return;  // removing an absent element is a no-op (sets.cpp:344-357,404-408)
        if (cap_ == 0) grow(n_);
        std::memmove(p_ + pos, p_ + pos + 1, (size_t(n_) - pos - 1) * sizeof(SetElement));
        --n_;
    }
    void add(SetElement e) { union_inplace(e); }
    void remove(SetElement e) { difference_inplace(e); }

   private:
    void forget() { p_ = nullptr; n_ = cap_ = 0; }
    void release() { if (cap_) delete[] p_; forget(); }
    void reserve(size_t cap) {  // fresh owning buffer (at least one slot so that owning == cap_ > 0)
        release();
        cap_ = uint32_t(std::max<size_t>(cap, 1));
        p_ = new SetElement[cap_];
    }
    void grow(size_t cap) {  // owning buffer of >= cap that keeps the current contents
        cap = std::max<size_t>(std::max<size_t>(cap, n_), 1);
        SetElement *q = new SetElement[cap];
        if (n_) std::memcpy(q, p_, size_t(n_) * sizeof(SetElement));
        if (cap_) delete[] p_;
        p_ = q;
        cap_ = uint32_t(cap);
    }
    void assign_sorted(const SetElement *s, size_t count) {
        reserve(count);
        if (count) std::memcpy(p_, s, count * sizeof(SetElement));
        n_ = uint32_t(count);
    }
    void assign_unsorted(const SetElement *s, size_t count) {
        assign_sorted(s, count);
        std::sort(p_, p_ + n_);
        n_ = uint32_t(std::unique(p_, p_ + n_) - p_);
    }
    SetElement *p_ = nullptr;
    uint32_t n_ = 0, cap_ = 0;  // cap_ == 0: borrowed view (or empty)
};

using SortedSpanSet = SpanSetT<int32_t>;    // the SortedSet flavour   (sorted_set.h:274-276)
using RoaringSpanSet = SpanSetT<uint32_t>;  // the RoaringSet flavour  (roaring_set.h:227-229): same contents, uint32 iteration;
                                            // the Roaring containers themselves live on the device (device_graph.hpp)

// Borrowed, trivially copyable view of a sorted row whose operators return owning SortedSpanSets: the surface of
// SortedSetRefBase (sorted_set_ref.h:9-78).  Unlike the reference it neither sorts the caller's memory in its constructor
// (:17-20; rows handed to it are canonical) nor inherits the missing equality test of its contains() (:70-73).
class SortedSpanRef {
   public:
    using SetElement = gmsx::SetElement;
    using Container = std::vector<SetElement>;
    SortedSpanRef() = default;
    SortedSpanRef(const SetElement *start, size_t count) : p_(start), n_(count) {}
    static SortedSpanRef borrow(const SetElement *start, size_t count) { return SortedSpanRef(start, count); }
    size_t cardinality() const { return n_; }
    const SetElement *begin() const { return p_; }
    const SetElement *end() const { return p_ + n_; }
    const SetElement *data() const { return p_; }
    template <class Set> SortedSpanSet union_with(const Set &s) const { return as_set().union_with(s); }
    template <class Set> SortedSpanSet intersect(const Set &s) const { return as_set().intersect(s); }
    template <class Set> size_t intersect_count(const Set &s) const { return detail::isect_count(p_, n_, s.data(), s.cardinality()); }
    template <class Set> SortedSpanSet difference(const Set &s) const { return as_set().difference(s); }
    bool contains(SetElement x) const { return std::binary_search(p_, p_ + n_, x); }

   private:
    SortedSpanSet as_set() const { return SortedSpanSet::borrow(p_, n_); }
    const SetElement *p_ = nullptr;
    size_t n_ = 0;
};

// ------------------------------------------------------------------------------------------------------------------
// SGraph over a device-resident graph (SetGraph<Set>, set_graph.h:10-233).  One host adjacency (borrowed or private),
// n 16-byte row views, and the device handle.  FromCGraph uploads eagerly, so the H2D copy and the device-side container
// build are part of what the reference harness times as "GraphExec buildTime" (common/benchmark.h:105-109); on a host
// without a HIP device the upload is skipped and the first whole-graph call fails loudly instead — the generic host
// templates keep working.
// ------------------------------------------------------------------------------------------------------------------
// Upload flags FromCGraph / FromCsr / clone use when none are given.  GMSX_UPLOAD_DEFAULT builds the degree-oriented containers and
// bitsets only (what k-clique and Bron–Kerbosch need) and leaves the triangle-count task lists to the first count_total call; a
// triangle-count driver sets GMSX_UPLOAD_FOR_TC — one line in main(), or -DGMSX_ADAPTOR_UPLOAD_FLAGS=GMSX_UPLOAD_FOR_TC — so that their
// build lands in the harness's untimed "GraphExec buildTime" (common/benchmark.h:105-109) like the reference's SetGraph construction.
#ifndef GMSX_ADAPTOR_UPLOAD_FLAGS
#define GMSX_ADAPTOR_UPLOAD_FLAGS GMSX_UPLOAD_DEFAULT
#endif
inline uint32_t &default_upload_flags() {
    static uint32_t flags = uint32_t(GMSX_ADAPTOR_UPLOAD_FLAGS);
    return flags;
}
// (part, nparts) of the uploads of THIS process: a rank of a multi-GPU run sets it once (before the first FromCGraph / FromCsr), so that
// only its own shard's triangle-count containers are built (gmsx_graph_upload_shard); {0, 1} = the whole graph
inline std::pair<int, int> &default_upload_shard() {
    static std::pair<int, int> shard{0, 1};
    return shard;
}

template <class SetT>
class HipGraphT {
   public:
    using Set = SetT;

    HipGraphT() = default;
    HipGraphT(HipGraphT &&o) noexcept { *this = std::move(o); }
    HipGraphT &operator=(HipGraphT &&o) noexcept {
        if (this != &o) {
            release();
            off_own_ = std::move(o.off_own_);
            adj_own_ = std::move(o.adj_own_);
            sets_ = std::move(o.sets_);
            off_ = o.off_; adj_ = o.adj_; n_ = o.n_;
            dev_ = o.dev_; upload_rc_ = o.upload_rc_; flags_ = o.flags_; shard_ = o.shard_;
            o.dev_ = nullptr; o.off_ = nullptr; o.adj_ = nullptr; o.n_ = 0; o.shard_ = {0, 1};
        }
        return *this;
    }
    HipGraphT(const HipGraphT &) = delete;
    HipGraphT &operator=(const HipGraphT &) = delete;
    ~HipGraphT() { release(); }

    // SetGraph::FromCGraph (set_graph.h:86-89,152-181): CGraph needs num_nodes(), out_degree(u) and an iterable out_neigh(u).
    // When out_neigh(u) hands out pointers into one contiguous, row-sorted int32 array (gapbs CSRGraph, graph.h:361-364) the
    // adjacency is BORROWED — the CGraph must outlive this object, as it does in the reference harness (set_graph.h:162-168
    // makes the same assumption for SortedSetRef) — otherwise it is copied once and sorted.
    template <class CGraph>
    static HipGraphT FromCGraph(const CGraph &g) { return FromCGraph(g, default_upload_flags()); }
    template <class CGraph>
    static HipGraphT FromCGraph(const CGraph &g, uint32_t upload_flags) {
        HipGraphT r;
        r.flags_ = upload_flags;
        const int64_t n = g.num_nodes();
        r.n_ = n;
        r.off_own_.resize(size_t(n) + 1);
        r.off_own_[0] = 0;
        for (int64_t u = 0; u < n; ++u) r.off_own_[size_t(u) + 1] = r.off_own_[size_t(u)] + int64_t(g.out_degree(u));
        r.off_ = r.off_own_.data();
        const int64_t nnz = r.off_[n];
        const SetElement *base = nullptr;
        if (n > 0 && nnz > 0) base = contiguous_base(g, r.off_, n);
        if (base) {
            r.adj_ = base;
        } else {
            r.adj_own_.resize(size_t(nnz));
            for (int64_t u = 0; u < n; ++u) {
                int64_t k = r.off_[u];
                for (auto v : g.out_neigh(u)) r.adj_own_[size_t(k++)] = SetElement(v);
                std::sort(r.adj_own_.begin() + r.off_[u], r.adj_own_.begin() + r.off_[u + 1]);
            }
            r.adj_ = r.adj_own_.data();
        }
        r.make_views();
        r.try_upload();
        return r;
    }
    // borrows the arrays of a gmsx_csr (which must outlive the graph)
    static HipGraphT FromCsr(const gmsx_csr *c, uint32_t upload_flags = default_upload_flags()) {
        HipGraphT r;
        r.flags_ = upload_flags;
        r.n_ = gmsx_csr_num_nodes(c);
        r.off_ = gmsx_csr_offsets(c);
        r.adj_ = gmsx_csr_neighbors(c);
        r.make_views();
        r.try_upload();
        return r;
    }
    HipGraphT clone() const {  // set_graph.h:120-127: an independent deep copy
        HipGraphT r;
        r.flags_ = flags_;
        r.n_ = n_;
        r.off_own_.assign(off_, off_ + n_ + 1);
        r.adj_own_.assign(adj_, adj_ + off_[n_]);
        r.off_ = r.off_own_.data();
        r.adj_ = r.adj_own_.data();
        r.make_views();
        r.try_upload();
        return r;
    }

    int64_t num_nodes() const { return n_; }                                              // set_graph.h:115-118
    const Set &out_neigh(SetElement v) const { return sets_[size_t(v)]; }                 // set_graph.h:102-105
    int64_t out_degree(SetElement v) const { return off_[size_t(v) + 1] - off_[size_t(v)]; }  // set_graph.h:91-94
    bool borrows_adjacency() const { return adj_own_.empty() && n_ > 0 && off_[n_] > 0; }
    const int64_t *offsets() const { return off_; }
    const SetElement *neighbors() const { return adj_; }

    std::pair<int, int> upload_shard() const { return shard_; }  // (part, nparts) of the device copy ({0, 1} = the whole graph)
    // device handle; failures follow the reference's convention: message + exit (gapbs/reader.h:45,228; cli/cli.h:159-171) —
    // nothing is thrown across the C-ABI
    const gmsx_graph *device() const {
        if (!dev_) {
            if (upload_rc_ == GMSX_OK || upload_rc_ == GMSX_ERR_NO_DEVICE) const_cast<HipGraphT *>(this)->try_upload();  // e.g. device bound later
            if (!dev_) {
                std::fprintf(stderr, "gmsx: graph upload failed: %s\n", gmsx_strerror(upload_rc_));
                std::exit(-32);
            }
        }
        return dev_;
    }

   private:
    template <class CGraph>
    static const SetElement *contiguous_base(const CGraph &g, const int64_t *off, int64_t n) {
        using It = decltype(g.out_neigh(0).begin());
        if constexpr (std::is_pointer_v<It> && sizeof(std::remove_pointer_t<It>) == sizeof(SetElement) &&
                      std::is_integral_v<std::remove_cv_t<std::remove_pointer_t<It>>>) {
            const SetElement *base = reinterpret_cast<const SetElement *>(g.out_neigh(0).begin());
            int ok = 1;
#ifdef _OPENMP
#pragma omp parallel for schedule(static, 4096) reduction(& : ok)
#endif
            for (int64_t u = 0; u < n; ++u) {
                const SetElement *row = reinterpret_cast<const SetElement *>(g.out_neigh(u).begin());
                if (row != base + off[u]) ok = 0;
                else
                    for (int64_t j = off[u] + 1; j < off[u + 1]; ++j) ok &= int(base[j - 1] < base[j]);
            }
            return ok ? base : nullptr;
        } else {
            (void)g; (void)off; (void)n;
            return nullptr;
        }
    }
    void make_views() {
        sets_.clear();
        sets_.reserve(size_t(n_));
        for (int64_t u = 0; u < n_; ++u) sets_.push_back(Set::borrow(adj_ + off_[u], size_t(off_[u + 1] - off_[u])));
    }
    void try_upload() {
        release_device();
        shard_ = default_upload_shard();
        upload_rc_ = gmsx_graph_upload_shard(n_, off_, adj_, flags_, shard_.first, shard_.second, &dev_);
        if (upload_rc_ != GMSX_OK) dev_ = nullptr;
    }
    void release_device() {
        if (dev_) gmsx_graph_free(dev_);
        dev_ = nullptr;
    }
    void release() { release_device(); }

    std::vector<int64_t> off_own_;
    std::vector<SetElement> adj_own_;
    std::vector<Set> sets_;
    const int64_t *off_ = nullptr;
    const SetElement *adj_ = nullptr;
    int64_t n_ = 0;
    gmsx_graph *dev_ = nullptr;
    int upload_rc_ = GMSX_OK;
    uint32_t flags_ = GMSX_UPLOAD_DEFAULT;
    std::pair<int, int> shard_{0, 1};  // (part, nparts) the device copy was uploaded with
};

using HipSetGraph = HipGraphT<SortedSpanSet>;       // the SortedSetGraph flavour       (set_graph.h:235)
using HipRoaringGraph = HipGraphT<RoaringSpanSet>;  // the RoaringGraph flavour         (set_graph.h:236)
using HipSetRefGraph = HipGraphT<SortedSpanRef>;    // the SetGraph<SortedSetRef> one   (k_clique_count_set_based.cc:38)

// ---- whole-graph algorithms: the hot path, forwarded to the device ---------------------------------------------------

// GMS::TriangleCount::Par::count_total / Seq::count_total (triangle_count/parallel/total.h:7-24, sequential/total.h:7-23)
// A graph uploaded as shard (part, nparts) of a multi-GPU run (default_upload_shard) holds the triangle-count containers of that shard
// only: count_total then returns the shard's PARTIAL count (gmsx_tc_partial) — the rank's term of the reference's reduction(+:total),
// which the caller sums over the ranks (gmsx_comm_allreduce_u64), as gmsx_driver --gpus does.
template <class S>
inline size_t count_total(const HipGraphT<S> &g) {
    uint64_t t = 0;
    if (g.upload_shard().second > 1)
        detail::check(gmsx_tc_partial(g.device(), GMSX_TC_AUTO, g.upload_shard().first, g.upload_shard().second, &t, nullptr), "gmsx_tc_partial");
    else
        detail::check(gmsx_tc_total(g.device(), GMSX_TC_AUTO, &t, nullptr), "gmsx_tc_total");
    return size_t(t);
}
// GMS::TriangleCount::Par::vertex_count2 / vertex_count2_once / Seq::vertex_count2 (parallel/vertex.h:14-49)
template <class S, class Output = std::vector<int64_t>>
inline void vertex_count2(const HipGraphT<S> &g, Output &counts) {
    counts.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*counts.data()) == sizeof(int64_t), "vertex counts are 64-bit");
    detail::check(gmsx_tc_vertex_count2(g.device(), reinterpret_cast<int64_t *>(counts.data()), nullptr), "gmsx_tc_vertex_count2");
}
// CliqueCount<…, SGraph, …> (k_clique_count_set_based.h:19-31): returns k! * C_k like the reference and prints its line (:29)
template <class S>
inline size_t clique_count(const HipGraphT<S> &g, size_t k = 4) {
    uint64_t ordered = 0;
    detail::check(gmsx_kclique_count(g.device(), int(k), &ordered, nullptr, nullptr), "gmsx_kclique_count");
    std::printf("total %zu-cliques: %llu\n", k, static_cast<unsigned long long>(ordered));
    return size_t(ordered);
}
// KCliqueStar::Par::CliqueStar<SGraph, OutputMode::Count> (k_clique_star_list/parallel/recursive.h:19-35): the number of k-clique-stars —
// what `output.size()` is in count mode — printed like the reference does (:33); *star_members (optional) = the total size of the stars a
// listing would carry.  The listing itself (`CliqueStarList`) is gmsx::clique_stars below.
template <class S>
inline int64_t clique_star_count(const HipGraphT<S> &g, int32_t k, uint64_t *star_members = nullptr) {
    uint64_t stars = 0;
    detail::check(gmsx_kclique_star_count(g.device(), int(k), &stars, star_members, nullptr), "gmsx_kclique_star_count");
    std::printf("total %d-cliques: %llu\n", int(k), static_cast<unsigned long long>(stars));
    return int64_t(stars);
}
// BkEppsteinPar::mceBench under -DBK_COUNT (eppsteinPAR.h:18-53): the maximal-clique count.  `rank` (rank format, any
// random-access container of n integers) is validated to be a permutation by the library; the count does not depend on it.
template <class S, class Ranking>
inline size_t maximal_clique_count(const HipGraphT<S> &g, const Ranking &rank) {
    uint64_t c = 0;
    const auto *r = rank.data();
    if constexpr (sizeof(*r) == sizeof(int32_t) && std::is_integral_v<std::remove_cv_t<std::remove_reference_t<decltype(*r)>>>) {
        detail::check(gmsx_bk_count(g.device(), reinterpret_cast<const int32_t *>(r), &c, nullptr), "gmsx_bk_count");
    } else {
        std::unique_ptr<int32_t[]> tmp(new int32_t[size_t(g.num_nodes())]);
        for (int64_t i = 0; i < g.num_nodes(); ++i) tmp[size_t(i)] = int32_t(rank[size_t(i)]);
        detail::check(gmsx_bk_count(g.device(), tmp.get(), &c, nullptr), "gmsx_bk_count");
    }
    return size_t(c);
}
template <class S>
inline size_t maximal_clique_count(const HipGraphT<S> &g) {
    uint64_t c = 0;
    detail::check(gmsx_bk_count(g.device(), nullptr, &c, nullptr), "gmsx_bk_count");
    return size_t(c);
}
// PpParallel::getDegeneracyOrderingApproxSGraph<averageDegree, useRankFormat> (degeneracy_approx_set.h:14-86)
template <class S, class Output>
inline void adg_rank(const HipGraphT<S> &g, double epsilon, Output &res, bool rank_format = true) {
    res.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*res.data()) == sizeof(int32_t), "orderings are NodeId = int32 vectors");
    detail::check(gmsx_adg_rank(g.device(), epsilon, rank_format ? 1 : 0, reinterpret_cast<int32_t *>(res.data()), nullptr, nullptr), "gmsx_adg_rank");
}
// PpParallel::triangleCountOrdering (preprocessing/parallel/triangle_count.h:11-30): vertices by increasing per-vertex count
template <class S, class Output>
inline void triangle_count_ordering(const HipGraphT<S> &g, Output &ordering) {
    ordering.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*ordering.data()) == sizeof(int32_t), "orderings are NodeId = int32 vectors");
    detail::check(gmsx_tc_ordering(g.device(), reinterpret_cast<int32_t *>(ordering.data()), nullptr), "gmsx_tc_ordering");
}
// The core numbers of all vertices (the running maximum of the removal degrees along PpSequential::getDegeneracyOrderingMatula's order,
// degeneracy_matula.h:13-66); returns the degeneracy.  `info` (optional) receives levels, rounds and the size of the top core.
template <class S, class Output>
inline int32_t core_numbers(const HipGraphT<S> &g, Output &core, gmsx_core_info *info = nullptr) {
    core.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*core.data()) == sizeof(int32_t), "core numbers are NodeId = int32 vectors");
    gmsx_core_info ci{};
    detail::check(gmsx_core_decomposition(g.device(), reinterpret_cast<int32_t *>(core.data()), nullptr, 1, &ci, nullptr), "gmsx_core_decomposition");
    if (info) *info = ci;
    return ci.degeneracy;
}
// An EXACT degeneracy order — what getDegeneracyOrderingMatula<SGraph, useRankFormat> is for: every vertex has at most degeneracy
// neighbours after it.  The vertices by (peel round, id), not Matula's own sequence (gmsx.h); returns the degeneracy.
template <class S, class Output>
inline int32_t degeneracy_order(const HipGraphT<S> &g, Output &res, bool rank_format = true) {
    res.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*res.data()) == sizeof(int32_t), "orderings are NodeId = int32 vectors");
    gmsx_core_info ci{};
    detail::check(gmsx_core_decomposition(g.device(), nullptr, reinterpret_cast<int32_t *>(res.data()), rank_format ? 1 : 0, &ci, nullptr),
                  "gmsx_core_decomposition");
    return ci.degeneracy;
}
// PpParallel::getDegreeOrdering<AnyGraph, useRankFormat> (preprocessing/parallel/degree.h:15-61): ascending (degree, id), bit-identical
template <class S, class Output>
inline void degree_order(const HipGraphT<S> &g, Output &res, bool rank_format = true) {
    res.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*res.data()) == sizeof(int32_t), "orderings are NodeId = int32 vectors");
    detail::check(gmsx_degree_rank(g.device(), rank_format ? 1 : 0, reinterpret_cast<int32_t *>(res.data()), nullptr), "gmsx_degree_rank");
}
// CoreNumberEvaluator::evaluateCoreNrAccuracy<useRankFormat> (core_number_evaluator.h:73-112, :141-154 when core_number < 0: graded against
// the exact degeneracy, computed on the device) — info.max_later is getCoreNumberOfOrder (:115-139)
template <class S, class Input>
inline gmsx_order_quality_info order_quality(const HipGraphT<S> &g, const Input &order, bool rank_format = true, int32_t core_number = -1) {
    static_assert(sizeof(*order.data()) == sizeof(int32_t), "orderings are NodeId = int32 vectors");
    gmsx_order_quality_info qi{};
    if (int64_t(order.size()) != g.num_nodes()) detail::check(GMSX_ERR_INVALID, "gmsx_order_quality");
    detail::check(gmsx_order_quality(g.device(), reinterpret_cast<const int32_t *>(order.data()), rank_format ? 1 : 0, core_number, nullptr, &qi, nullptr),
                  "gmsx_order_quality");
    return qi;
}

// support[j] = |N(u) ∩ N(v)| of arc j = (u -> v) of the graph's CSR — the triangles through that edge, both arcs of an edge alike (gmsx.h);
// returns the number of triangles.
template <class S, class Output>
inline uint64_t edge_support(const HipGraphT<S> &g, Output &support) {
    const int64_t nnz = g.num_nodes() ? g.offsets()[g.num_nodes()] : 0;
    support.resize(size_t(nnz));
    static_assert(sizeof(*support.data()) == sizeof(int32_t), "supports are int32 vectors");
    uint64_t triangles = 0;
    detail::check(gmsx_edge_support(g.device(), reinterpret_cast<int32_t *>(support.data()), &triangles, nullptr), "gmsx_edge_support");
    return triangles;
}
// truss[j] = trussness of the edge of arc j (gmsx.h: the level-synchronous peel; unique for the graph); returns the largest.  `info` (optional)
// receives levels, rounds, the largest support, the size of the top truss and the triangles.
template <class S, class Output>
inline int32_t truss_numbers(const HipGraphT<S> &g, Output &truss, gmsx_truss_info *info = nullptr) {
    const int64_t nnz = g.num_nodes() ? g.offsets()[g.num_nodes()] : 0;
    truss.resize(size_t(nnz));
    static_assert(sizeof(*truss.data()) == sizeof(int32_t), "truss numbers are int32 vectors");
    gmsx_truss_info ti{};
    detail::check(gmsx_truss_decomposition(g.device(), reinterpret_cast<int32_t *>(truss.data()), nullptr, &ti, nullptr), "gmsx_truss_decomposition");
    if (info) *info = ti;
    return ti.max_truss;
}
// The k-truss as an edge list: the u < v edges with trussness >= k, in CSR order.
template <class S>
inline std::vector<std::pair<int32_t, int32_t>> ktruss_edges(const HipGraphT<S> &g, int32_t k) {
    std::vector<int32_t> truss;
    truss_numbers(g, truss);
    std::vector<std::pair<int32_t, int32_t>> res;
    for (int64_t u = 0; u < g.num_nodes(); ++u)
        for (int64_t j = g.offsets()[u]; j < g.offsets()[u + 1]; ++j)
            if (u < g.neighbors()[j] && truss[size_t(j)] >= k) res.emplace_back(int32_t(u), int32_t(g.neighbors()[j]));
    return res;
}

// ShiloachVishkin(g) (representations/graphs/log_graph/cc.cc:40-72), shaped like its pvector<NodeId> comp: comp[v] = the label of v's
// component, which is the smallest vertex id in it (what the reference's hooking converges to); returns the number of components.  `info`
// (optional) receives singletons, the largest component and its label.
template <class S, class Output>
inline int64_t connected_components(const HipGraphT<S> &g, Output &comp, gmsx_components_info *info = nullptr) {
    comp.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*comp.data()) == sizeof(int32_t), "component labels are int32 vectors");
    gmsx_components_info ci{};
    detail::check(gmsx_connected_components(g.device(), nullptr, reinterpret_cast<int32_t *>(comp.data()), &ci, nullptr), "gmsx_connected_components");
    if (info) *info = ci;
    return ci.components;
}
// Jarvis–Patrick clustering (no reference counterpart): comp[v] = the label of v's cluster — the components over the edges whose endpoints
// score >= threshold under `metric` (GMSX_SIM_*; the scores of gmsx_vertex_similarity_batch); returns the number of clusters.
template <class S, class Output>
inline int64_t jarvis_patrick(const HipGraphT<S> &g, int metric, double threshold, Output &comp, gmsx_components_info *info = nullptr) {
    comp.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*comp.data()) == sizeof(int32_t), "cluster labels are int32 vectors");
    gmsx_components_info ci{};
    detail::check(gmsx_jarvis_patrick(g.device(), metric, threshold, reinterpret_cast<int32_t *>(comp.data()), nullptr, &ci, nullptr), "gmsx_jarvis_patrick");
    if (info) *info = ci;
    return ci.components;
}
// The communities of the k-truss: trussness per arc -> the mask truss >= k -> components over the kept edges (vertices outside the k-truss are
// singletons); returns the number of components.  info->kept_edges is the number of edges of the k-truss.
template <class S, class Output>
inline int64_t ktruss_components(const HipGraphT<S> &g, int32_t k, Output &comp, gmsx_components_info *info = nullptr) {
    std::vector<int32_t> truss;
    truss_numbers(g, truss);
    std::vector<uint8_t> keep(truss.size() + 1);
    for (size_t j = 0; j < truss.size(); ++j) keep[j] = truss[j] >= k;
    comp.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*comp.data()) == sizeof(int32_t), "component labels are int32 vectors");
    gmsx_components_info ci{};
    detail::check(gmsx_connected_components(g.device(), keep.data(), reinterpret_cast<int32_t *>(comp.data()), &ci, nullptr), "gmsx_connected_components");
    if (info) *info = ci;
    return ci.components;
}

// DOBFS(g, source) (representations/graphs/log_graph/bfs.cc:120-190), shaped like its pvector<NodeId> parent: parent[v] = the smallest-id
// neighbour of v one level nearer the source, parent[source] = source, -1 = unreachable (the reference leaves -degree there); BFSVerifier
// (:212-258) accepts it.  `depth` (optional, a vector of int32) receives the distances, `info` (optional) the level statistics; returns the
// number of reached vertices: the "nodes" of PrintBFSStats.
template <class S, class Output>
inline int64_t bfs(const HipGraphT<S> &g, int32_t source, Output &parent, std::vector<int32_t> *depth = nullptr, gmsx_bfs_info *info = nullptr) {
    parent.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*parent.data()) == sizeof(int32_t), "parents are int32 vectors");
    if (depth) depth->resize(size_t(g.num_nodes()));
    gmsx_bfs_info bi{};
    detail::check(gmsx_bfs(g.device(), source, depth ? depth->data() : nullptr, reinterpret_cast<int32_t *>(parent.data()), &bi, nullptr), "gmsx_bfs");
    if (info) *info = bi;
    return bi.reached;
}
// Brandes(g, sp, num_iters) (log_graph/bc.cc:89-153) from an explicit source list (pick_sources gives the reference's), in double where the
// reference has float and 32-bit path counts; flags: GMSX_BC_*.  GMSX_BC_NORMALIZE_MAX gives the reference's normalised scores.  Returns the
// largest score before normalisation.
template <class S>
inline double betweenness(const HipGraphT<S> &g, const std::vector<int32_t> &sources, std::vector<double> &scores, uint32_t flags = GMSX_BC_DEFAULT,
                          gmsx_bc_info *info = nullptr) {
    scores.resize(size_t(g.num_nodes()));
    gmsx_bc_info bi{};
    double none = 0.0;  // (n = 0: the library wants no array, the vector has none)
    detail::check(gmsx_betweenness(g.device(), int64_t(sources.size()), sources.data(), flags, scores.empty() ? &none : scores.data(), &bi, nullptr),
                  "gmsx_betweenness");
    if (info) *info = bi;
    return bi.max_score;
}
// A BFS from every listed source, 64 (or 128) of them per sweep of the graph (gmsx_bfs_multi; no reference counterpart): per_source[i] holds
// reached, reached_arcs, depth_sum, levels, closeness and harmonic of sources[i].  Optional: depth (sources.size() rows of n, -1 = unreachable;
// meant for small graphs) and the per-vertex dist_sum (64-bit), reach and far (int32).  Returns the number of reached vertices summed over the
// sources.
template <class S>
inline int64_t bfs_multi(const HipGraphT<S> &g, const std::vector<int32_t> &sources, std::vector<gmsx_bfs_source> &per_source,
                         std::vector<int32_t> *depth = nullptr, std::vector<int64_t> *dist_sum = nullptr, std::vector<int32_t> *reach = nullptr,
                         std::vector<int32_t> *far = nullptr, gmsx_bfs_multi_info *info = nullptr) {
    const size_t n = size_t(g.num_nodes());
    per_source.resize(sources.size());
    if (depth) depth->resize(sources.size() * n);
    if (dist_sum) dist_sum->resize(n);
    if (reach) reach->resize(n);
    if (far) far->resize(n);
    gmsx_bfs_multi_info mi{};
    detail::check(gmsx_bfs_multi(g.device(), int64_t(sources.size()), sources.data(), per_source.data(), depth ? depth->data() : nullptr,
                                 dist_sum ? dist_sum->data() : nullptr, reach ? reach->data() : nullptr, far ? far->data() : nullptr, &mi, nullptr),
                  "gmsx_bfs_multi");
    if (info) *info = mi;
    return mi.reached_total;
}
// Closeness centrality of the listed sources inside their components: out_scores[i] = (reached - 1) / depth_sum of sources[i] (0 for an isolated
// source), or with `harmonic` the harmonic centrality Σ_{v != s} 1 / depth(v).  Returns the largest score.
template <class S>
inline double closeness(const HipGraphT<S> &g, const std::vector<int32_t> &sources, std::vector<double> &out_scores, bool harmonic = false,
                        gmsx_bfs_multi_info *info = nullptr) {
    std::vector<gmsx_bfs_source> per;
    bfs_multi(g, sources, per, nullptr, nullptr, nullptr, nullptr, info);
    out_scores.resize(per.size());
    double top = 0.0;
    for (size_t i = 0; i < per.size(); ++i) {
        out_scores[i] = harmonic ? per[i].harmonic : per[i].closeness;
        if (out_scores[i] > top) top = out_scores[i];
    }
    return top;
}
// PageRankPull(g, max_iters, epsilon) (log_graph/pr.cc:34-61) with its constants as arguments (the defaults are the reference's) and in double
// unless GMSX_PR_FLOAT32 asks for its float; teleport: n non-negative weights or nullptr = uniform; flags: GMSX_PR_*.  Returns the number of
// sweeps executed.
template <class S>
inline int32_t pagerank(const HipGraphT<S> &g, std::vector<double> &scores, double damping = 0.85, int32_t max_iters = 20, double tolerance = 1e-4,
                        const std::vector<double> *teleport = nullptr, uint32_t flags = GMSX_PR_DEFAULT, gmsx_pagerank_info *info = nullptr) {
    scores.resize(size_t(g.num_nodes()));
    if (teleport && teleport->size() != scores.size()) detail::check(GMSX_ERR_INVALID, "gmsx_pagerank");
    gmsx_pagerank_info pi{};
    detail::check(gmsx_pagerank(g.device(), damping, max_iters, tolerance, teleport && !teleport->empty() ? teleport->data() : nullptr, flags,
                                scores.empty() ? nullptr : scores.data(), &pi, nullptr),
                  "gmsx_pagerank");
    if (info) *info = pi;
    return pi.iterations;
}
// PRVerifier(g, scores, target_error) (pr.cc:79-97) as a number: the L1 change of one sweep over `scores`; the reference accepts iff it is
// below its tolerance
template <class S>
inline double pagerank_residual(const HipGraphT<S> &g, const std::vector<double> &scores, double damping = 0.85,
                                const std::vector<double> *teleport = nullptr, uint32_t flags = GMSX_PR_DEFAULT) {
    if (scores.size() != size_t(g.num_nodes()) || (teleport && teleport->size() != scores.size())) detail::check(GMSX_ERR_INVALID, "gmsx_pagerank_residual");
    double r = 0.0;
    detail::check(gmsx_pagerank_residual(g.device(), scores.empty() ? nullptr : scores.data(), damping,
                                         teleport && !teleport->empty() ? teleport->data() : nullptr, flags, &r, nullptr),
                  "gmsx_pagerank_residual");
    return r;
}
// Edge weights for gmsx::sssp: weights[j] belongs to g.neighbors()[j] (every weight >= 1, w(u,v) == w(v,u)); an empty vector detaches.  The
// weights live with the device copy of g: a graph that is uploaded again needs them attached again.
template <class S>
inline void set_weights(const HipGraphT<S> &g, const std::vector<int32_t> &weights) {
    const int64_t nnz = g.num_nodes() > 0 ? g.offsets()[g.num_nodes()] : 0;
    if (!weights.empty() && int64_t(weights.size()) != nnz) detail::check(GMSX_ERR_INVALID, "gmsx_graph_set_weights");
    detail::check(gmsx_graph_set_weights(const_cast<gmsx_graph *>(g.device()), weights.empty() ? nullptr : weights.data()), "gmsx_graph_set_weights");
}
// DeltaStep(g, source, delta) (log_graph/sssp.cc:54-134), shaped like its pvector<WeightT> dist but in 64 bits and with -1 (not kDistInf) for an
// unreachable vertex; delta = 0: the library's choice.  parent (optional): the smallest-id neighbour on a lightest path.  Returns the number of
// reached vertices — what PrintSSSPStats prints.
template <class S>
inline int64_t sssp(const HipGraphT<S> &g, int32_t source, std::vector<int64_t> &dist, int64_t delta = 0, std::vector<int32_t> *parent = nullptr,
                    gmsx_sssp_info *info = nullptr) {
    dist.resize(size_t(g.num_nodes()));
    if (parent) parent->resize(size_t(g.num_nodes()));
    gmsx_sssp_info si{};
    detail::check(gmsx_sssp(g.device(), source, delta, dist.empty() ? nullptr : dist.data(), parent && !parent->empty() ? parent->data() : nullptr, &si, nullptr),
                  "gmsx_sssp");
    if (info) *info = si;
    return si.reached;
}
// SSSPVerifier(g, source, dist) (sssp.cc:145-175): true iff no arc is violated, every reached vertex but the source has a tight arc, no
// unreached vertex has a reached neighbour and dist[source] == 0
template <class S>
inline bool sssp_verify(const HipGraphT<S> &g, int32_t source, const std::vector<int64_t> &dist, gmsx_sssp_check *out = nullptr) {
    if (dist.size() != size_t(g.num_nodes())) detail::check(GMSX_ERR_INVALID, "gmsx_sssp_verify");
    gmsx_sssp_check c{};
    detail::check(gmsx_sssp_verify(g.device(), source, dist.empty() ? nullptr : dist.data(), &c, nullptr), "gmsx_sssp_verify");
    if (out) *out = c;
    return c.violated_arcs == 0 && c.untight == 0 && c.wrong_unreached == 0 && c.source_ok == 1;
}
// One edge of a spanning forest: u < v and the weight attached to the arc u -> v.
struct WeightedEdge {
    int32_t u, v, w;
    friend bool operator==(const WeightedEdge &a, const WeightedEdge &b) { return a.u == b.u && a.v == b.v && a.w == b.w; }
    friend bool operator!=(const WeightedEdge &a, const WeightedEdge &b) { return !(a == b); }
};
// The minimum spanning forest of g under the weights attached with gmsx::set_weights — the maximum one with flags = GMSX_MSF_MAXIMUM — under
// the strict order of gmsx.h (weight, then the smaller (min id, max id)), so the forest is unique: `edges` receives its n - trees edges
// ascending by (u, v).  No reference counterpart.  Returns the total weight; `info` (optional) receives trees, rounds, the bottleneck weights …
template <class S>
inline int64_t min_spanning_forest(const HipGraphT<S> &g, std::vector<WeightedEdge> &edges, uint32_t flags = 0, gmsx_msf_info *info = nullptr) {
    const size_t room = size_t(std::max<int64_t>(g.num_nodes() - 1, 1));
    std::vector<int32_t> u(room), v(room), w(room);
    gmsx_msf_info mi{};
    detail::check(gmsx_min_spanning_forest(g.device(), flags, u.data(), v.data(), w.data(), nullptr, nullptr, &mi, nullptr), "gmsx_min_spanning_forest");
    edges.resize(size_t(mi.edges));
    for (size_t i = 0; i < edges.size(); ++i) edges[i] = WeightedEdge{u[i], v[i], w[i]};
    if (info) *info = mi;
    return mi.total_weight;
}
// The same forest as a byte per arc, parallel to g.neighbors(): 1 on both arcs of every forest edge.  gmsx_connected_components over this mask
// gives the labels of the whole graph.
template <class S>
inline std::vector<uint8_t> msf_arc_mask(const HipGraphT<S> &g, uint32_t flags = 0, gmsx_msf_info *info = nullptr) {
    const int64_t nnz = g.num_nodes() > 0 ? g.offsets()[g.num_nodes()] : 0;
    std::vector<uint8_t> keep(size_t(nnz) + 1);
    gmsx_msf_info mi{};
    detail::check(gmsx_min_spanning_forest(g.device(), flags, nullptr, nullptr, nullptr, keep.data(), nullptr, &mi, nullptr), "gmsx_min_spanning_forest");
    keep.resize(size_t(nnz));
    if (info) *info = mi;
    return keep;
}
// Communities by label propagation (gmsx.h): label[v] = the id of a member of v's community.  flags = GMSX_LP_WEIGHTED sums the weights attached
// with gmsx::set_weights instead of counting arcs; coloring (optional, one colour >= 1 per vertex, proper) fixes the order of the asynchronous
// sweeps — nullptr: the colouring gmsx::coloring(g) returns; max_sweeps = 0: the library's cap.  No reference counterpart.  Returns the number
// of communities; `info` (optional) receives sweeps, changes, converged …
template <class S>
inline int64_t label_propagation(const HipGraphT<S> &g, std::vector<int32_t> &label, uint32_t flags = 0, const std::vector<int32_t> *coloring = nullptr,
                                 int32_t max_sweeps = 0, gmsx_lp_info *info = nullptr) {
    if (coloring && coloring->size() != size_t(g.num_nodes())) detail::check(GMSX_ERR_INVALID, "gmsx_label_propagation");
    label.resize(size_t(g.num_nodes()));
    gmsx_lp_info li{};
    detail::check(gmsx_label_propagation(g.device(), flags, coloring && !coloring->empty() ? coloring->data() : nullptr, max_sweeps,
                                         label.empty() ? nullptr : label.data(), &li, nullptr),
                  "gmsx_label_propagation");
    if (info) *info = li;
    return li.communities;
}
// The exact modularity integers of any labelling with labels in [0, n) (gmsx.h): W, I, S = Σ D_c² as (hi, lo), communities, largest, unstable,
// and modularity = I / W - S / W² computed from them once.
template <class S>
inline gmsx_modularity_info modularity(const HipGraphT<S> &g, const std::vector<int32_t> &label, uint32_t flags = 0) {
    if (label.size() != size_t(g.num_nodes())) detail::check(GMSX_ERR_INVALID, "gmsx_modularity");
    gmsx_modularity_info mi{};
    detail::check(gmsx_modularity(g.device(), flags, label.empty() ? nullptr : label.data(), &mi, nullptr), "gmsx_modularity");
    return mi;
}
// The greedy matching of g under the strict order of gmsx.h (heavier weight first with flags = GMSX_MATCH_WEIGHTED and the weights attached
// with gmsx::set_weights, else unit weights; ties by the hash of the ends, then by the ids), so the matching is unique: mate[v] = v's partner
// or -1; `edges` (optional) receives the pairs (u, v, w), u < v, ascending by u.  No reference counterpart.  Returns the number of pairs;
// `info` (optional) receives total_weight, free_vertices, exposed, rounds …
template <class S>
inline int64_t greedy_matching(const HipGraphT<S> &g, std::vector<int32_t> &mate, uint32_t flags = 0, std::vector<WeightedEdge> *edges = nullptr,
                               gmsx_matching_info *info = nullptr) {
    mate.resize(size_t(g.num_nodes()));
    const size_t room = edges ? size_t(std::max<int64_t>(g.num_nodes() / 2, 1)) : 0;
    std::vector<int32_t> u(room), v(room), w(room);
    gmsx_matching_info mi{};
    detail::check(gmsx_greedy_matching(g.device(), flags, mate.empty() ? nullptr : mate.data(), edges ? u.data() : nullptr, edges ? v.data() : nullptr,
                                       edges ? w.data() : nullptr, &mi, nullptr),
                  "gmsx_greedy_matching");
    if (edges) {
        edges->resize(size_t(mi.pairs));
        for (size_t i = 0; i < edges->size(); ++i) (*edges)[i] = WeightedEdge{u[i], v[i], w[i]};
    }
    if (info) *info = mi;
    return mi.pairs;
}
// gmsx_matching_verify of any mate array (-1 = free) under the same flags: true iff it is THE greedy matching (invalid == 0 and
// undominated == 0, gmsx.h); `out` (optional) receives the six integers — augmentable == 0 iff the matching is maximal.
template <class S>
inline bool matching_verify(const HipGraphT<S> &g, const std::vector<int32_t> &mate, uint32_t flags = 0, gmsx_matching_check *out = nullptr) {
    if (mate.size() != size_t(g.num_nodes())) detail::check(GMSX_ERR_INVALID, "gmsx_matching_verify");
    gmsx_matching_check mc{};
    detail::check(gmsx_matching_verify(g.device(), flags, mate.empty() ? nullptr : mate.data(), &mc, nullptr), "gmsx_matching_verify");
    if (out) *out = mc;
    return mc.invalid == 0 && mc.undominated == 0;
}
// The biconnected components (blocks) of g (gmsx.h): block[j] = the id of the block of the arc j of g.neighbors() — ids ascend with each block's
// smallest `u < v` arc, both arcs of an edge carry the same id —, blocks_at[v] = the blocks that contain v.  No reference counterpart.  Returns
// the number of blocks; `info` (optional) receives bridges, articulation_points, the largest block, components, levels …
template <class S>
inline int64_t biconnected_components(const HipGraphT<S> &g, std::vector<int32_t> &block, std::vector<int32_t> &blocks_at, gmsx_bicc_info *info = nullptr) {
    const int64_t nnz = g.num_nodes() > 0 ? g.offsets()[g.num_nodes()] : 0;
    block.resize(size_t(nnz));
    blocks_at.resize(size_t(g.num_nodes()));
    gmsx_bicc_info bi{};
    detail::check(gmsx_biconnected_components(g.device(), 0, block.empty() ? nullptr : block.data(), blocks_at.empty() ? nullptr : blocks_at.data(), nullptr,
                                              &bi, nullptr),
                  "gmsx_biconnected_components");
    if (info) *info = bi;
    return bi.blocks;
}
// The articulation points (cut vertices) of g, ascending: the vertices that lie in two blocks or more.
template <class S>
inline std::vector<int32_t> articulation_points(const HipGraphT<S> &g, gmsx_bicc_info *info = nullptr) {
    std::vector<int32_t> at(size_t(g.num_nodes())), cut;
    gmsx_bicc_info bi{};
    detail::check(gmsx_biconnected_components(g.device(), 0, nullptr, at.empty() ? nullptr : at.data(), nullptr, &bi, nullptr), "gmsx_biconnected_components");
    cut.reserve(size_t(bi.articulation_points));
    for (size_t v = 0; v < at.size(); ++v)
        if (at[v] >= 2) cut.push_back(int32_t(v));
    if (info) *info = bi;
    return cut;
}
// The bridges of g as (u, v) with u < v, ascending: the edges whose removal disconnects their component (the arcs with arc_keep == 0).
template <class S>
inline std::vector<std::pair<int32_t, int32_t>> bridges(const HipGraphT<S> &g, gmsx_bicc_info *info = nullptr) {
    const int64_t n = g.num_nodes(), nnz = n > 0 ? g.offsets()[n] : 0;
    std::vector<uint8_t> keep(size_t(nnz) + 1);
    gmsx_bicc_info bi{};
    detail::check(gmsx_biconnected_components(g.device(), 0, nullptr, nullptr, keep.data(), &bi, nullptr), "gmsx_biconnected_components");
    std::vector<std::pair<int32_t, int32_t>> out;
    out.reserve(size_t(bi.bridges));
    for (int64_t u = 0; u < n; ++u)
        for (int64_t j = g.offsets()[u]; j < g.offsets()[u + 1]; ++j)
            if (!keep[size_t(j)] && int64_t(g.neighbors()[j]) > u) out.emplace_back(int32_t(u), g.neighbors()[j]);
    if (info) *info = bi;
    return out;
}
// PrintTopScores' top k (pr.cc:64-74, gapbs/util.h TopK) on the host: the k largest scores as (id, score), largest first, ties by the smaller id
inline std::vector<std::pair<int32_t, double>> top_scores(const std::vector<double> &scores, size_t k) {
    std::vector<std::pair<double, int32_t>> key(scores.size());  // (-score, id): ascending = largest first, ties by the smaller id
    for (size_t v = 0; v < scores.size(); ++v) key[v] = {-scores[v], int32_t(v)};
    k = std::min(k, key.size());
    std::partial_sort(key.begin(), key.begin() + std::ptrdiff_t(k), key.end());
    std::vector<std::pair<int32_t, double>> out(k);
    for (size_t i = 0; i < k; ++i) out[i] = {key[i].second, -key[i].first};
    return out;
}
// SourcePicker (gapbs/benchmark.h:51-75): its first `count` picks, or `count` copies of `given`
inline std::vector<int32_t> pick_sources(const gmsx_csr *csr, int64_t count, int32_t given = -1) {
    std::vector<int32_t> out(size_t(count > 0 ? count : 0));
    int32_t none = 0;
    detail::check(gmsx_csr_pick_sources(csr, count, given, out.empty() ? &none : out.data()), "gmsx_csr_pick_sources");
    return out;
}

// The 4-cycles of the graph (no reference counterpart).  With `at_vertex` (a vector of 64-bit integers, resized to n): the 4-cycles through
// every vertex as well, which add up to four times the return value.
template <class S>
inline uint64_t cycle4_count(const HipGraphT<S> &g) {
    uint64_t cycles = 0;
    detail::check(gmsx_cycle4_count(g.device(), &cycles, nullptr, nullptr), "gmsx_cycle4_count");
    return cycles;
}
template <class S, class Output>
inline uint64_t cycle4_count(const HipGraphT<S> &g, Output &at_vertex) {
    at_vertex.resize(size_t(g.num_nodes()));
    static_assert(sizeof(*at_vertex.data()) == sizeof(int64_t), "per-vertex cycle counts are 64-bit vectors");
    uint64_t cycles = 0;
    int64_t none = 0;  // (n = 0: data() may be null, and the library writes nothing)
    detail::check(gmsx_cycle4_count(g.device(), &cycles, at_vertex.empty() ? &none : reinterpret_cast<int64_t *>(at_vertex.data()), nullptr), "gmsx_cycle4_count");
    return cycles;
}
// The census of the eight 3- and 4-vertex motifs (GMSX_MOTIF_*): info.subgraphs[] non-induced, info.induced[] induced.  Throws on
// GMSX_ERR_OVERFLOW (a count that does not fit 64 bits), like every other failed call.
template <class S>
inline gmsx_motif_info motif_census4(const HipGraphT<S> &g) {
    gmsx_motif_info info{};
    detail::check(gmsx_motif_census4(g.device(), &info, nullptr), "gmsx_motif_census4");
    return info;
}

// JonesV3::graph_coloring_jones(g, coloring, order) (coloring_jones_v3.h:38-68): the colouring (1..info->colors) under `order` — rank format
// (order[v] = position of v) is the reference's own; the vertex of the highest position is coloured first.
template <class S, class Input>
inline std::vector<int32_t> coloring(const HipGraphT<S> &g, const Input &order, bool rank_format = true, gmsx_coloring_info *info = nullptr) {
    static_assert(sizeof(*order.data()) == sizeof(int32_t), "orderings are NodeId = int32 vectors");
    if (int64_t(order.size()) != g.num_nodes()) detail::check(GMSX_ERR_INVALID, "gmsx_coloring_jp");
    std::vector<int32_t> res(size_t(g.num_nodes()));
    gmsx_coloring_info ci{};
    detail::check(gmsx_coloring_jp(g.device(), g.num_nodes() ? reinterpret_cast<const int32_t *>(order.data()) : nullptr, rank_format ? 1 : 0, res.data(), nullptr,
                                   &ci, nullptr), "gmsx_coloring_jp");
    if (info) *info = ci;
    return res;
}
// The rank vector of a colouring heuristic, composed from the existing producers: "ff" = n-1-v (graph_coloring_naive_sequential's first-fit,
// coloring_sequential.h:17-42), "lf" = degree_order (largest first), "sl" = degeneracy_order (smallest last), "adg" = adg_rank(epsilon).
// Returns false for "id" (order[v] = v, getSimpleIdOrdering: gmsx_coloring_jp's NULL) and leaves `order` empty; an unknown name exits.
template <class S>
inline bool coloring_order(const HipGraphT<S> &g, const char *heuristic, double epsilon, std::vector<int32_t> &order) {
    const std::string h = heuristic ? heuristic : "";
    order.clear();
    if (h == "id") return false;
    if (h == "ff") {
        order.resize(size_t(g.num_nodes()));
        for (size_t v = 0; v < order.size(); ++v) order[v] = int32_t(order.size() - 1 - v);
    } else if (h == "lf") {
        degree_order(g, order, true);
    } else if (h == "sl") {
        degeneracy_order(g, order, true);
    } else if (h == "adg") {
        adg_rank(g, epsilon, order, true);
    } else {
        detail::check(GMSX_ERR_INVALID, "gmsx::coloring (heuristic: id, ff, lf, sl or adg)");
    }
    return true;
}
template <class S>
inline std::vector<int32_t> coloring(const HipGraphT<S> &g, const char *heuristic, double epsilon = 0.001, gmsx_coloring_info *info = nullptr) {
    std::vector<int32_t> order;
    if (coloring_order(g, heuristic, epsilon, order)) return coloring(g, order, true, info);
    std::vector<int32_t> res(size_t(g.num_nodes()));
    gmsx_coloring_info ci{};
    detail::check(gmsx_coloring_jp(g.device(), nullptr, 1, res.data(), nullptr, &ci, nullptr), "gmsx_coloring_jp");
    if (info) *info = ci;
    return res;
}
// GCVerifierMaxColor(g, c, m) (coloring_common.h:102-122) is invalid == 0 && conflicts == 0 && max_color <= m; GCVerifierDeltaPlusOne (:125-157)
// the same with m = max_degree + 1; distinct is uniqueColorsCount (:205-209)
template <class S, class Input>
inline gmsx_coloring_check coloring_check(const HipGraphT<S> &g, const Input &coloring) {
    static_assert(sizeof(*coloring.data()) == sizeof(int32_t), "colourings are int32 vectors");
    gmsx_coloring_check out{};
    if (int64_t(coloring.size()) != g.num_nodes()) detail::check(GMSX_ERR_INVALID, "gmsx_coloring_verify");
    detail::check(gmsx_coloring_verify(g.device(), g.num_nodes() ? reinterpret_cast<const int32_t *>(coloring.data()) : nullptr, &out, nullptr),
                  "gmsx_coloring_verify");
    return out;
}

// Set::intersect / Set::difference of whole neighbourhoods for a BATCH of vertex pairs on the device (sorted_set.h:160-197): result i =
// out_neigh(u[i]) ∩ out_neigh(v[i]) (difference = false) or out_neigh(u[i]) \ out_neigh(v[i]), as sets of the graph's own flavour — what a
// listing consumer (tomita.h:51-70 with `sol`, k_clique_star_list/parallel/output.h:14-68) hands on.  One sizing call, one fill.
template <class S, class Ids>
inline std::vector<S> set_op_batch(const HipGraphT<S> &g, const Ids &u, const Ids &v, bool difference = false) {
    const int64_t np = int64_t(u.size());
    std::vector<int32_t> uu(u.begin(), u.end()), vv(v.begin(), v.end());
    std::vector<int64_t> off(size_t(np) + 1, 0);
    const int op = difference ? GMSX_SETOP_DIFFERENCE : GMSX_SETOP_INTERSECT;
    detail::check(gmsx_set_op_batch(g.device(), op, np, uu.data(), vv.data(), off.data(), nullptr, 0, nullptr), "gmsx_set_op_batch");
    std::vector<int32_t> ids(size_t(off[size_t(np)]) + 1);
    detail::check(gmsx_set_op_batch(g.device(), op, np, uu.data(), vv.data(), off.data(), ids.data(), off[size_t(np)], nullptr), "gmsx_set_op_batch");
    std::vector<S> out;
    out.reserve(size_t(np));
    for (int64_t i = 0; i < np; ++i) out.emplace_back(ids.data() + off[size_t(i)], size_t(off[size_t(i) + 1] - off[size_t(i)]));  // (owning copies)
    return out;
}

// BkEppsteinPar::mceBench WITHOUT -DBK_COUNT (eppsteinPAR.h:18-53, tomita.h:79-84): the maximal cliques themselves, each an owning set of the
// graph's own flavour (members ascending).  `rank` is validated like maximal_clique_count's and does not change the set.  One sizing call,
// one fill (gmsx_bk_list); the order of the cliques is deterministic but otherwise unspecified, like the reference's parallel `sol`.
template <class S>
inline std::vector<S> maximal_cliques_shard(const HipGraphT<S> &g, const int32_t *rank, int part, int nparts) {
    gmsx_bk_list_info info{};
    detail::check(gmsx_bk_list(g.device(), rank, part, nparts, nullptr, nullptr, 0, 0, &info, nullptr), "gmsx_bk_list");
    std::vector<int64_t> off(size_t(info.cliques) + 1, 0);
    std::vector<int32_t> ids(size_t(info.members) + 1);
    detail::check(gmsx_bk_list(g.device(), rank, part, nparts, off.data(), ids.data(), int64_t(off.size()), info.members, &info, nullptr), "gmsx_bk_list");
    std::vector<S> out;
    out.reserve(size_t(info.cliques));
    for (int64_t i = 0; i < info.cliques; ++i) out.emplace_back(ids.data() + off[size_t(i)], size_t(off[size_t(i) + 1] - off[size_t(i)]));  // (owning copies)
    return out;
}
template <class S>
inline std::vector<S> maximal_cliques(const HipGraphT<S> &g) {
    return maximal_cliques_shard(g, nullptr, 0, 1);
}
template <class S, class Ranking>
inline std::vector<S> maximal_cliques(const HipGraphT<S> &g, const Ranking &rank) {
    const auto *r = rank.data();
    if constexpr (sizeof(*r) == sizeof(int32_t) && std::is_integral_v<std::remove_cv_t<std::remove_reference_t<decltype(*r)>>>) {
        return maximal_cliques_shard(g, reinterpret_cast<const int32_t *>(r), 0, 1);
    } else {
        std::unique_ptr<int32_t[]> tmp(new int32_t[size_t(g.num_nodes())]);
        for (int64_t i = 0; i < g.num_nodes(); ++i) tmp[size_t(i)] = int32_t(rank[size_t(i)]);
        return maximal_cliques_shard(g, tmp.get(), 0, 1);
    }
}

// KCliqueStar::Par::CliqueStarList (k_clique_star_list/parallel/recursive.h:37-43): one {clique, star} pair per k-clique, each an owning
// set of the graph's own flavour — the shape of the reference's ListOutput<Set, List, 2>, a vector of std::array<Set, 2>.  One sizing call,
// one fill (gmsx_kclique_star_list); the order of the pairs is deterministic (gmsx.h) where the reference's parallel one is not.
template <class S>
inline std::vector<std::array<S, 2>> clique_stars_shard(const HipGraphT<S> &g, int32_t k, int part, int nparts) {
    gmsx_kclique_star_list_info info{};
    detail::check(gmsx_kclique_star_list(g.device(), int(k), GMSX_KCSTAR_DEFAULT, part, nparts, nullptr, nullptr, nullptr, 0, 0, &info, nullptr),
                  "gmsx_kclique_star_list");
    std::vector<int32_t> cl(size_t(info.cliques) * size_t(k) + 1), ids(size_t(info.star_members) + 1);
    std::vector<int64_t> off(size_t(info.cliques) + 1, 0);
    detail::check(gmsx_kclique_star_list(g.device(), int(k), GMSX_KCSTAR_DEFAULT, part, nparts, cl.data(), off.data(), ids.data(), info.cliques,
                                         info.star_members, &info, nullptr),
                  "gmsx_kclique_star_list");
    std::vector<std::array<S, 2>> out;
    out.reserve(size_t(info.cliques));
    for (int64_t i = 0; i < info.cliques; ++i)  // (owning copies)
        out.push_back({S(cl.data() + size_t(i) * size_t(k), size_t(k)), S(ids.data() + off[size_t(i)], size_t(off[size_t(i) + 1] - off[size_t(i)]))});
    return out;
}
template <class S>
inline std::vector<std::array<S, 2>> clique_stars(const HipGraphT<S> &g, int32_t k) {
    return clique_stars_shard(g, k, 0, 1);
}
// … with the stars switched off (GMSX_KCSTAR_CLIQUES_ONLY): the k-cliques themselves, members ascending; k = 3 lists the triangles
template <class S>
inline std::vector<S> cliques(const HipGraphT<S> &g, int32_t k, int part = 0, int nparts = 1) {
    gmsx_kclique_star_list_info info{};
    detail::check(gmsx_kclique_star_list(g.device(), int(k), GMSX_KCSTAR_CLIQUES_ONLY, part, nparts, nullptr, nullptr, nullptr, 0, 0, &info, nullptr),
                  "gmsx_kclique_star_list");
    std::vector<int32_t> cl(size_t(info.cliques) * size_t(k) + 1);
    detail::check(gmsx_kclique_star_list(g.device(), int(k), GMSX_KCSTAR_CLIQUES_ONLY, part, nparts, cl.data(), nullptr, nullptr, info.cliques, 0,
                                         &info, nullptr),
                  "gmsx_kclique_star_list");
    std::vector<S> out;
    out.reserve(size_t(info.cliques));
    for (int64_t i = 0; i < info.cliques; ++i) out.emplace_back(cl.data() + size_t(i) * size_t(k), size_t(k));
    return out;
}

// GMS::LinkPrediction::link_prediction_similarity<Metric> (link_prediction/link_prediction.h:42-101) in the reference's shape: the q best
// non-edges and their scores, ascending (index 0 the worst kept), WITH the reference's padding — q - found leading entries (-1.0, edge (0,0))
// when fewer than q candidates exist, exactly one such entry when none does.  metric: a GMSX_SIM_* value.
struct ScoredEdges {
    std::vector<std::pair<int32_t, int32_t>> edges;  // UndirectedEdge: first < second
    std::vector<double> scores;
    int64_t found = 0;  // the real entries: the last `found` of both vectors
};
template <class S>
inline ScoredEdges link_prediction_shard(const HipGraphT<S> &g, int metric, int64_t q, int part, int nparts, gmsx_link_prediction_info *info = nullptr) {
    if (q > (int64_t(1) << 27)) detail::check(GMSX_ERR_UNSUPPORTED, "gmsx_link_prediction (q > 2^27)");  // the library's limit: no q slots allocated for nothing
    const int64_t room = q >= 1 ? q : 1;  // (q < 1 is refused by the library)
    std::vector<int32_t> u(static_cast<size_t>(room)), v(static_cast<size_t>(room));
    std::vector<double> sc(static_cast<size_t>(room));
    gmsx_link_prediction_info li{};
    detail::check(gmsx_link_prediction(g.device(), metric, q, part, nparts, u.data(), v.data(), sc.data(), room, &li, nullptr), "gmsx_link_prediction");
    if (info) *info = li;
    ScoredEdges out;
    out.found = li.found;
    const int64_t pad = li.found > 0 ? q - li.found : 1;
    out.edges.assign(size_t(pad), std::pair<int32_t, int32_t>(0, 0));
    out.scores.assign(size_t(pad), -1.0);
    for (int64_t i = 0; i < li.found; ++i) {
        out.edges.emplace_back(u[size_t(i)], v[size_t(i)]);
        out.scores.push_back(sc[size_t(i)]);
    }
    return out;
}
template <class S>
inline ScoredEdges link_prediction(const HipGraphT<S> &g, int metric, int64_t q, gmsx_link_prediction_info *info = nullptr) {
    return link_prediction_shard(g, metric, q, 0, 1, info);
}
// The shards of one (graph, metric, q) merged under the rule of gmsx.h — decreasing score, ties by ascending (u, v) —, truncated to q and padded
// as the reference pads: the whole graph's result, entry for entry.
inline ScoredEdges merge_link_predictions(const std::vector<ScoredEdges> &parts, int64_t q) {
    struct E {
        double s;
        int32_t u, v;
    };
    std::vector<E> all;
    for (const ScoredEdges &p : parts)
        for (size_t i = p.scores.size() - size_t(p.found); i < p.scores.size(); ++i) all.push_back(E{p.scores[i], p.edges[i].first, p.edges[i].second});
    std::sort(all.begin(), all.end(), [](const E &a, const E &b) { return a.s != b.s ? a.s > b.s : a.u != b.u ? a.u < b.u : a.v < b.v; });
    if (int64_t(all.size()) > q) all.resize(size_t(std::max<int64_t>(q, 0)));
    ScoredEdges out;
    out.found = int64_t(all.size());
    const int64_t pad = out.found > 0 ? q - out.found : 1;
    out.edges.assign(size_t(pad), std::pair<int32_t, int32_t>(0, 0));
    out.scores.assign(size_t(pad), -1.0);
    for (size_t i = all.size(); i-- > 0;) {
        out.edges.emplace_back(all[i].u, all[i].v);
        out.scores.push_back(all[i].s);
    }
    return out;
}
// score_link_prediction_precision (link_prediction/evaluation.h:99-124): g_test's undirected edges against a predicted list
struct LinkPredictionScore {
    double precision = 0.0, recall = 0.0;
    int64_t true_positives = 0, true_count = 0;
};
template <class S, class Edges>
inline LinkPredictionScore link_prediction_precision(const HipGraphT<S> &g_test, const Edges &predicted) {
    std::vector<int32_t> u, v;
    u.reserve(predicted.size());
    v.reserve(predicted.size());
    for (const auto &e : predicted) {
        u.push_back(int32_t(e.first));
        v.push_back(int32_t(e.second));
    }
    LinkPredictionScore sc;
    detail::check(gmsx_link_prediction_precision(g_test.device(), int64_t(u.size()), u.data(), v.data(), &sc.true_positives, &sc.true_count, &sc.precision,
                                                 &sc.recall, nullptr),
                  "gmsx_link_prediction_precision");
    return sc;
}

// Subgraph matching (gmsx_subgraph_match): every embedding of a small connected pattern, row i = embedding i, column p = the image of pattern
// vertex p, E * k ids in the list order of gmsx.h.  The pattern is anything with num_nodes(), offsets() and neighbors() — a HipGraphT of any
// flavour (only its host arrays are read) — or the raw arrays, which need no graph object at all.  flags: GMSX_SGM_*; with
// GMSX_SGM_FIRST the one call of that mode (0 or 1 row).  *info (may be NULL): count, tasks and the matching order.
template <class S>
inline std::vector<int32_t> subgraph_isomorphisms(const HipGraphT<S> &g, int32_t k, const int64_t *p_offsets, const int32_t *p_neigh,
                                                  uint32_t flags = GMSX_SGM_INDUCED, int part = 0, int nparts = 1, gmsx_subgraph_info *info = nullptr) {
    gmsx_subgraph_info local{};
    gmsx_subgraph_info &inf = info ? *info : local;
    const int32_t none = 0;
    if (!p_neigh) p_neigh = &none;  // (k = 1: an empty array)
    if (flags & GMSX_SGM_FIRST) {
        inf.embeddings = 1;
    } else {
        detail::check(gmsx_subgraph_match(g.device(), k, p_offsets, p_neigh, flags, part, nparts, nullptr, 0, &inf, nullptr), "gmsx_subgraph_match");
    }
    std::vector<int32_t> maps(size_t(inf.embeddings) * size_t(k > 0 ? k : 0) + 1);
    detail::check(gmsx_subgraph_match(g.device(), k, p_offsets, p_neigh, flags, part, nparts, maps.data(), inf.embeddings, &inf, nullptr),
                  "gmsx_subgraph_match");
    maps.resize(size_t(inf.embeddings) * size_t(k));
    return maps;
}
template <class S, class Pattern>
inline std::vector<int32_t> subgraph_isomorphisms(const HipGraphT<S> &g, const Pattern &pattern, uint32_t flags = GMSX_SGM_INDUCED, int part = 0,
                                                  int nparts = 1, gmsx_subgraph_info *info = nullptr) {
    return subgraph_isomorphisms(g, int32_t(pattern.num_nodes()), pattern.offsets(), pattern.neighbors(), flags, part, nparts, info);
}
// GMS::SubGraphIso::VF2::run (non_set_based/subgraphiso/vf2/sequential/vf2.hpp:39-51) in the shape of its Result::isomorphism (util/result.hpp:15,
// filled by State::SaveToResult, vf2/util/vf2State.hpp:153-156): key = target vertex, value = pattern vertex; empty if there is no induced
// embedding.  The pairs are the reference's sequential result, element for element (GMSX_SGM_FIRST).
template <class S, class Pattern>
inline std::map<int, int> subgraph_isomorphism(const HipGraphT<S> &g, const Pattern &pattern, uint32_t flags = GMSX_SGM_INDUCED) {
    const std::vector<int32_t> row = subgraph_isomorphisms(g, pattern, flags | GMSX_SGM_FIRST);
    std::map<int, int> out;
    for (size_t p = 0; p < row.size(); ++p) out[int(row[p])] = int(p);
    return out;
}

}  // namespace gmsx
