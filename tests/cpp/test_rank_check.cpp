// check_rank_permutation (gms_amd/csrc/host/rank_check.hpp): the edges of its bitmap (64-bit words) and every way an array fails to be a permutation.
#include "rank_check.hpp"

#include <cstdio>
#include <vector>

using gmsx::check_rank_permutation;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::vector<int32_t> identity(int64_t n) {
    std::vector<int32_t> r(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) r[size_t(i)] = int32_t(i);
    return r;
}

static int check(const std::vector<int32_t> &r) { return check_rank_permutation(r.data(), int64_t(r.size())); }

int main() {
    CHECK(check_rank_permutation(nullptr, 0) == GMSX_OK);  // no vertices: nothing to read
    const int32_t none = 7;
    CHECK(check_rank_permutation(&none, 0) == GMSX_OK);
    CHECK(check({}) == GMSX_OK);
    CHECK(check({0}) == GMSX_OK);  // n = 1
    CHECK(check({1}) == GMSX_ERR_INVALID);
    CHECK(check({-1}) == GMSX_ERR_INVALID);

    for (int64_t n : {int64_t(64), int64_t(65), int64_t(129)}) {  // the last id is bit 63 of a word, bit 0 of the next, bit 0 of the third
        const std::vector<int32_t> id = identity(n);
        CHECK(check(id) == GMSX_OK);
        CHECK(check(std::vector<int32_t>(id.rbegin(), id.rend())) == GMSX_OK);
        for (size_t at : {size_t(0), size_t(n / 2), size_t(n - 1)}) {
            std::vector<int32_t> r = id;
            r[at] = int32_t(n);  // one past the range
            CHECK(check(r) == GMSX_ERR_INVALID);
            r[at] = -1;
            CHECK(check(r) == GMSX_ERR_INVALID);
        }
        std::vector<int32_t> r = id;
        r[size_t(n - 1)] = int32_t(n - 2);  // a duplicate in the last position
        CHECK(check(r) == GMSX_ERR_INVALID);
        r = id;
        r[size_t(n - 1)] = 0;  // … whose first occurrence lies in another word (n = 64: in the same one)
        CHECK(check(r) == GMSX_ERR_INVALID);
    }
    {  // a duplicate across words, neither at an end: ids 3 (word 0) twice, 70 (word 1) missing
        std::vector<int32_t> r = identity(129);
        r[70] = 3;
        CHECK(check(r) == GMSX_ERR_INVALID);
        r = identity(129);
        r[3] = 128;  // first occurrence of 128 at position 3, the second in the last position; 3 missing
        CHECK(check(r) == GMSX_ERR_INVALID);
    }
    if (failures) return 1;
    std::printf("rank check ok\n");
    return 0;
}
