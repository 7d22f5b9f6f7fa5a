// The per-call edge numbering and support pass of truss.hip, for the translation units that need the support of every edge without the peel
// (motifs.hip).  The kernels and truss_edges() itself live in truss.hip; this header only names what they fill.
#pragma once
#include "device_buffer.hpp"
#include "device_graph.hpp"

#include <cstdint>

namespace gmsx {

// accumulators of the numbering and the support pass (one small block, zeroed per call)
struct TrussAcc {
    unsigned long long sum;  // Σ support over undirected edges
    int32_t max_sup;
    int32_t error;           // an arc without its twin, a self loop, or an append past its bound
    int32_t nlong;           // edges parked by k_truss_support
    int32_t pad;
};

// what one call builds before anything is counted: the numbering, the costs and the support of every edge
struct TrussEdges {
    int64_t m = 0, total_cost = 0, long_cap = 0;  // total_cost: Σ cost over the edges, what coff ends in
    DevBuf eid, eu, ev, coff, sup, acc, longs;
    TrussAcc h;
    int launches = 0;
};

// Edge numbering and support.  rnd (m, device, or null) is set to -1.  Refuses m >= 2^31: edge ids are 32 bits.
int truss_edges(const gmsx_graph *g, TrussEdges &t, int32_t *rnd);

}  // namespace gmsx
