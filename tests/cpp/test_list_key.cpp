// ListKey (gms_amd/csrc/host/list_key.hpp): what makes a cached pass 1 of a listing call belong to one upload.  The free-and-re-upload case
// — the same handle address, the same device arrays, the same n and nnz, another serial — must not match.
#include "list_key.hpp"

#include <cstdio>

using gmsx::ListKey;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

int main() {
    int handle_a = 0, handle_b = 0;  // stand-ins: only their addresses are compared
    long long off_a[4] = {0, 1, 2, 2}, off_b[4] = {0, 1, 2, 2};
    int adj_a[2] = {1, 0}, adj_b[2] = {1, 0};
    const int64_t n = 3, nnz = 2;

    const ListKey base(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1);
    CHECK(base == ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1));  // identical keys match
    CHECK(!(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1)));
    CHECK(base == base);
    {  // a copy is the same key
        const ListKey copy = base;
        CHECK(copy == base && base == copy);
    }

    // free and re-upload: everything but the serial repeats
    CHECK(!(base == ListKey(8, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1)));
    CHECK(base != ListKey(8, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1));
    CHECK(ListKey(8, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1) != base);  // symmetric
    CHECK(base != ListKey(7 + (1ull << 32), &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1));  // all 64 bits of the serial count
    CHECK(base != ListKey(~0ull, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 1));

    // the call's parameters
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 1, 1, 3, 1));  // part
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 2, 3, 1));  // nparts
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 4, 1));  // extra[0] (k)
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3, 0));  // extra[1] (flags)
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 1, 3));  // the two extras are not interchangeable
    CHECK(ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 2) != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 1, 2));  // shards (0,2) and (1,2)
    CHECK(ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1) == ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 0, 0));  // the extras default to 0
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz, 0, 1, 3 + (1ll << 32), 1));  // 64-bit extras

    // what the key has always held still counts
    CHECK(base != ListKey(7, &handle_b, off_a, adj_a, n, nnz, 0, 1, 3, 1));
    CHECK(base != ListKey(7, &handle_a, off_b, adj_a, n, nnz, 0, 1, 3, 1));
    CHECK(base != ListKey(7, &handle_a, off_a, adj_b, n, nnz, 0, 1, 3, 1));
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n + 1, nnz, 0, 1, 3, 1));
    CHECK(base != ListKey(7, &handle_a, off_a, adj_a, n, nnz + 2, 0, 1, 3, 1));

    // a default-constructed key (a cleared cache entry) matches no key of a real handle: serials start at 1, and an empty graph (n = nnz = 0,
    // part 0 of 1) differs in the other fields as well
    const ListKey none;
    CHECK(none.serial == 0);
    CHECK(none != base);
    CHECK(base != none);
    CHECK(none != ListKey(1, &handle_a, off_a, adj_a, 0, 0, 0, 1));
    CHECK(none != ListKey(1, nullptr, nullptr, nullptr, -1, -1, -1, -1));  // the serial alone separates them
    CHECK(none != ListKey(0, &handle_a, off_a, adj_a, n, nnz, 0, 1));     // … and so do the fields of any handle without it

    if (failures) return 1;
    std::printf("list key ok\n");
    return 0;
}
