// The host-side check of a caller's rank array (gmsx_bk_partial, gmsx_bk_list).  Plain C++: tests/cpp/test_rank_check.cpp checks it on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <new>

#include "gmsx.h"

namespace gmsx {

// `rank` is what the reference's drivers hand from the preprocessing step to mceBench(graph, ordering).  The maximal cliques do not depend on
// it and the device splits by its own degree rank, so it is validated (a permutation of 0..n-1, as every rank-format
// ordering is) and otherwise not needed.  GMSX_OK / GMSX_ERR_INVALID / GMSX_ERR_NOMEM.
// No exception may cross the C ABI: the scratch bitmap is a nothrow allocation.  Validated on EVERY call (an O(n) pass next to an
// enumeration): a memo keyed on the pointer would accept an array that was changed, or another one at the same address.
inline int check_rank_permutation(const int32_t *rank, int64_t n) {
    if (n <= 0) return GMSX_OK;
    if (!rank) return GMSX_ERR_INVALID;
    std::unique_ptr<uint64_t[]> seen(new (std::nothrow) uint64_t[size_t((n + 63) / 64)]());
    if (!seen) return GMSX_ERR_NOMEM;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = rank[i];
        if (r < 0 || r >= n) return GMSX_ERR_INVALID;
        uint64_t &w = seen[size_t(r >> 6)];
        const uint64_t bit = 1ull << (r & 63);
        if (w & bit) return GMSX_ERR_INVALID;
        w |= bit;
    }
    return GMSX_OK;
}

}  // namespace gmsx
