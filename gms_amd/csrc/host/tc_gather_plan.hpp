// Gathered rows of the triangle count (hip/device_graph.hip, k_task_lists): which trailing 16-byte units of a stream row leave the row
// for the receiver's gathered row.  A row that ends inside a 128-byte line costs the whole line; its units behind the last line
// boundary are self-contained (ids, or base + count + gaps), so they can be streamed from anywhere.  Plain C++, host and device:
// tests/cpp/test_tc_gather_plan.cpp checks it on the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GMSX_GATHER_HD __host__ __device__
#else
#define GMSX_GATHER_HD
#endif

namespace gmsx {

constexpr uint32_t kGatherLineUnits = 8;   // 16-byte units per 128-byte line
constexpr uint32_t kGatherChunk = 64;      // units per entry of a gathered row (the chunk of the inline rows)
constexpr int kGatherMax = 7;              // the largest limit R: a remainder is at most a line less one unit
// What an unset GMSX_TC_GATHER means (chosen by measurement: profiles/tc_gather/README.md).
constexpr int kTcGatherDefault = 7;
constexpr int kGatherForms = 2;            // gathered rows per list of a receiver: one of list units, one of delta units
// forms as the stream rows number them (device_graph.hpp: kFormList …); bitsets never move — a unit's bit positions follow from its index
// in the row — and neither do the 12-bit-gap rows (off by default; they would need a gathered row of their own)
constexpr uint32_t kGatherFormList = 0, kGatherFormBitset = 1, kGatherFormDelta = 2, kGatherFormGap12 = 3;

GMSX_GATHER_HD inline bool gather_form_moves(uint32_t form) { return form == kGatherFormList || form == kGatherFormDelta; }
// the gathered row (0 = list units, 1 = delta units) a form's units go to
GMSX_GATHER_HD inline int gather_slot(uint32_t form) { return form == kGatherFormDelta ? 1 : 0; }

// How many trailing units of the row [first, first + units) of form `form` move, with limit R (0 … 7).  r = the units behind the last
// line boundary the row reaches.  Nothing moves unless 0 < r <= R.  A row of >= 8 units keeps its whole lines (r < units always).  A row
// of < 8 units moves whole when units <= R (its entry is dropped); otherwise units > R >= r: it straddles a boundary and the r units
// behind it move.  What stays ends on a line boundary or is empty.
GMSX_GATHER_HD inline uint32_t gather_moved(uint64_t first, uint32_t units, uint32_t form, int R) {
    if (R <= 0 || units == 0 || !gather_form_moves(form)) return 0;
    const uint32_t r = uint32_t((first + units) & (kGatherLineUnits - 1));
    if (r == 0 || r > uint32_t(R > kGatherMax ? kGatherMax : R)) return 0;
    if (units < kGatherLineUnits && units <= uint32_t(R)) return units;
    return r < units ? r : 0;
}
// the 64-bit descriptor first unit << 24 | form << 22 | units (device_graph.hpp) without its last `moved` units; 0 = no entry left
GMSX_GATHER_HD inline unsigned long long gather_shrink(unsigned long long d, uint32_t moved) {
    const uint32_t units = uint32_t(d) & 0x3fffffu;
    return moved >= units ? 0ull : d - moved;
}
GMSX_GATHER_HD inline uint32_t gather_moved_of(unsigned long long d, int R) {
    return gather_moved(d >> 24, uint32_t(d) & 0x3fffffu, (uint32_t(d) >> 22) & 3u, R);
}
// a gathered row of g units: the units its region takes (whole lines)
GMSX_GATHER_HD inline uint64_t gather_region_units(uint64_t g) { return (g + kGatherLineUnits - 1) & ~uint64_t(kGatherLineUnits - 1); }

}  // namespace gmsx
