// plan_launches (gms_amd/csrc/host/launch_plan.hpp): the hand-derived cases, then the planner's four properties over seeded random inputs.
#include "launch_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using gmsx::kNoTaskCap;
using gmsx::Launch;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::vector<int64_t> offsets(const std::vector<int64_t> &widths) {
    std::vector<int64_t> soff(1, 0);
    for (int64_t w : widths) soff.push_back(soff.back() + w);
    return soff;
}

static void expect(const std::vector<int64_t> &widths, unsigned long long budget, int64_t cap, const std::vector<Launch> &want,
                   unsigned long long want_arena) {
    unsigned long long arena = ~0ull;
    const std::vector<Launch> got = gmsx::plan_launches(offsets(widths), int64_t(widths.size()), budget, cap, &arena);
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i) CHECK(got[i].t0 == want[i].t0 && got[i].t1 == want[i].t1);
    CHECK(arena == want_arena);
}

int main() {
    for (unsigned long long budget : {1ull, 4ull, 1ull << 40})
        for (int64_t cap : {int64_t(1), int64_t(2), kNoTaskCap}) expect({}, budget, cap, {}, 0);  // no tasks
    expect({10}, 4, kNoTaskCap, {{0, 1}}, 10);                                                   // one task wider than the budget
    expect({4, 4, 4}, 8, kNoTaskCap, {{0, 2}, {2, 3}}, 8);                                       // an exact fit joins
    expect({4, 4, 4}, 7, kNoTaskCap, {{0, 1}, {1, 2}, {2, 3}}, 4);                               // one word less splits
    expect({4, 100, 4}, 8, kNoTaskCap, {{0, 1}, {1, 2}, {2, 3}}, 100);                           // a wide task in the middle
    expect({0, 0, 0, 0, 0}, 4, 2, {{0, 2}, {2, 4}, {4, 5}}, 0);                                  // all-zero slabs (kcstar with k <= 2), capped
    expect({0, 0, 0, 0, 0}, 4, kNoTaskCap, {{0, 5}}, 0);                                         // all-zero slabs, uncapped

    std::mt19937 rng(20240607u);
    for (int iter = 0; iter < 400; ++iter) {
        const int64_t n = int64_t(rng() % 41);
        std::vector<int64_t> widths(static_cast<size_t>(n));
        for (int64_t &w : widths) w = int64_t(rng() % 21);
        const unsigned long long budget = 1 + rng() % 30;
        const int64_t cap = rng() % 3 == 0 ? kNoTaskCap : int64_t(1 + rng() % 8);
        const std::vector<int64_t> soff = offsets(widths);
        unsigned long long arena = ~0ull;
        const std::vector<Launch> plan = gmsx::plan_launches(soff, n, budget, cap, &arena);
        auto span = [&](int64_t t0, int64_t t1) { return (unsigned long long)(soff[size_t(t1)] - soff[size_t(t0)]); };
        int64_t next = 0;
        unsigned long long widest = 0;
        for (const Launch &l : plan) {
            CHECK(l.t0 == next && l.t1 > l.t0 && l.t1 <= n);  // contiguous, non-empty
            if (l.t1 - l.t0 > 1) CHECK(span(l.t0, l.t1) <= budget && l.t1 - l.t0 <= cap);
            if (l.t1 < n) CHECK(span(l.t0, l.t1 + 1) > budget || l.t1 - l.t0 + 1 > cap);  // maximal
            widest = span(l.t0, l.t1) > widest ? span(l.t0, l.t1) : widest;
            next = l.t1;
        }
        CHECK(next == n);  // covers [0, n)
        CHECK(arena == widest);
    }
    if (failures) return 1;
    std::printf("launch plan ok\n");
    return 0;
}
