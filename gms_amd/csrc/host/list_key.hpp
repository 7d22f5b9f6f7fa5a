// What identifies a cached pass 1 of a device LISTING call (hip/two_pass_list.hpp: ListPass1, ensure_pass1).  Plain C++:
// tests/cpp/test_list_key.cpp checks it on the host.
#pragma once
#include <cstdint>

namespace gmsx {

// A cached pass 1 belongs to ONE UPLOAD.  The handle's address and the device addresses of its arrays do not say which: after
// gmsx_graph_free the next upload of a graph with the same n and nnz tends to get the same blocks back (operator new and hipMalloc both
// re-use a freed block of the same size), and a key of addresses and sizes alone would hand that graph the task list, the slab offsets and
// the bases of the one before it.  So every upload takes a process-unique serial (gmsx_graph::serial, from 1 on; device_graph.hip) and the
// serial is part of the key.  The addresses and sizes stay in it: they cost nothing and say what the entry was built from.
struct ListKey {
    uint64_t serial = 0;  // 0 = no upload: a default-constructed key equals no key of a handle
    const void *g = nullptr;
    const void *off = nullptr;
    const void *adj = nullptr;
    int64_t n = -1, nnz = -1;
    int part = -1, nparts = -1;
    int64_t extra[2] = {0, 0};  // the call's own parameters (kcstar, subgraph: k, flags)
    ListKey() = default;
    ListKey(uint64_t serial_, const void *g_, const void *off_, const void *adj_, int64_t n_, int64_t nnz_, int part_, int nparts_, int64_t e0 = 0,
            int64_t e1 = 0)
        : serial(serial_), g(g_), off(off_), adj(adj_), n(n_), nnz(nnz_), part(part_), nparts(nparts_), extra{e0, e1} {}
    bool operator==(const ListKey &o) const {
        return serial == o.serial && g == o.g && off == o.off && adj == o.adj && n == o.n && nnz == o.nnz && part == o.part && nparts == o.nparts &&
               extra[0] == o.extra[0] && extra[1] == o.extra[1];
    }
    bool operator!=(const ListKey &o) const { return !(*this == o); }
};

}  // namespace gmsx
