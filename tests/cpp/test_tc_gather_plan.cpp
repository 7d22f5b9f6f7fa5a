// gather_moved and its helpers (gms_amd/csrc/host/tc_gather_plan.hpp): the rule over every position in a line, units 1 … 40, every form and every
// limit R, then hand-derived cases.
#include "tc_gather_plan.hpp"

#include <cstdio>

using namespace gmsx;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

int main() {
    const uint64_t bases[3] = {0, 8000, (uint64_t(1) << 32) - 64};
    for (uint64_t base : bases)
        for (uint32_t a = 0; a < 8; ++a)
            for (uint32_t units = 1; units <= 40; ++units)
                for (uint32_t form = 0; form < 4; ++form) {
                    const uint64_t first = base + a;
                    uint32_t prev = 0;
                    for (int R = 0; R <= 7; ++R) {
                        const uint32_t m = gather_moved(first, units, form, R);
                        const unsigned long long d = ((unsigned long long)first << 24) | ((unsigned long long)form << 22) | units;
                        CHECK(gather_moved_of(d, R) == m);
                        CHECK(m <= uint32_t(R) && m <= units);                       // moved <= R
                        if (R == 0) CHECK(m == 0);                                    // R = 0 is the identity
                        if (form == kGatherFormBitset || form == kGatherFormGap12) CHECK(m == 0);  // bitset rows (and 12-bit gaps) are untouched
                        const uint32_t body = units - m;
                        if (m) {
                            CHECK(body == 0 || (first + body) % 8 == 0);              // the body ends on a line boundary or is empty
                            if (units >= 8 && a == 0) CHECK(body >= 8 && body % 8 == 0);  // an aligned row keeps whole lines, at least one
                            if (units >= 8) CHECK(body >= 1);
                            if (body == 0) CHECK(units < 8 && units <= uint32_t(R));  // only a small row of <= R units goes whole
                            const uint32_t r = uint32_t((first + units) % 8);
                            CHECK(r > 0 && r <= uint32_t(R));
                            CHECK(m == r || m == units);
                        }
                        // bytes are conserved: what the shrunk descriptor names plus what moved is the row; first unit and form stay
                        const unsigned long long s = gather_shrink(d, m);
                        if (body == 0) CHECK(s == 0);
                        else CHECK((s >> 24) == first && ((s >> 22) & 3) == form && (s & 0x3fffff) == body);
                        CHECK(16ull * body + 16ull * m == 16ull * units);
                        // a larger limit never moves less of a row that a smaller one moved
                        CHECK(m >= prev || prev == 0);
                        if (m) prev = m;
                    }
                }
    // by hand (list form): an aligned row of 9 units has remainder 1; of 15, 7; of 16, none
    CHECK(gather_moved(0, 9, 0, 1) == 1 && gather_moved(0, 9, 0, 7) == 1);
    CHECK(gather_moved(0, 15, 0, 6) == 0 && gather_moved(0, 15, 0, 7) == 7);
    CHECK(gather_moved(0, 16, 0, 7) == 0 && gather_moved(0, 8, 0, 7) == 0);
    CHECK(gather_moved(64, 33, 2, 3) == 1 && gather_moved(64, 35, 2, 3) == 3 && gather_moved(64, 36, 2, 3) == 0);
    // small rows: 3 units at position 6 of a line straddle (1 behind the boundary): whole at R >= 3, the one unit at R = 1, 2
    CHECK(gather_moved(6, 3, 0, 1) == 1 && gather_moved(6, 3, 0, 2) == 1 && gather_moved(6, 3, 0, 3) == 3);
    // … 3 units at position 2 end at 5: nothing below R = 5, whole from there
    CHECK(gather_moved(2, 3, 0, 4) == 0 && gather_moved(2, 3, 0, 5) == 3);
    // … 5 units at position 3 end on the boundary: never
    CHECK(gather_moved(3, 5, 0, 7) == 0);
    // … 7 units at position 4 end at 3: three move at R = 3 … 6, all seven at R = 7
    CHECK(gather_moved(4, 7, 0, 2) == 0 && gather_moved(4, 7, 0, 3) == 3 && gather_moved(4, 7, 0, 6) == 3 && gather_moved(4, 7, 0, 7) == 7);
    CHECK(gather_moved(0, 9, 1, 7) == 0 && gather_moved(0, 0, 0, 7) == 0);
    CHECK(gather_slot(0) == 0 && gather_slot(2) == 1);
    CHECK(gather_region_units(0) == 0 && gather_region_units(1) == 8 && gather_region_units(64) == 64 && gather_region_units(65) == 72);
    if (failures) return 1;
    std::printf("tc gather plan ok\n");
    return 0;
}
