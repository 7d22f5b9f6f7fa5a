// How a pass over a task list is cut into kernel launches (hip/two_pass_list.hpp).  Plain C++: tests/cpp/test_launch_plan.cpp checks it on the host.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gmsx {

struct Launch {
    int64_t t0, t1;  // tasks [t0, t1)
};
constexpr int64_t kNoTaskCap = INT64_MAX;

// Task t owns the slab words [soff[t], soff[t + 1]) (n_tasks + 1 ascending offsets).  Greedy: a launch takes consecutive tasks while their
// slabs together fit budget_words and they are at most max_tasks_per_launch; a task wider than the budget runs alone.  *arena_words = the
// widest launch, which is what the pass allocates.
inline std::vector<Launch> plan_launches(const std::vector<int64_t> &soff, int64_t n_tasks, unsigned long long budget_words,
                                         int64_t max_tasks_per_launch, unsigned long long *arena_words) {
    std::vector<Launch> out;
    unsigned long long widest = 0;
    for (int64_t t0 = 0; t0 < n_tasks;) {
        int64_t t1 = t0 + 1;
        while (t1 < n_tasks && t1 - t0 < max_tasks_per_launch && (unsigned long long)(soff[size_t(t1 + 1)] - soff[size_t(t0)]) <= budget_words) ++t1;
        widest = std::max<unsigned long long>(widest, (unsigned long long)(soff[size_t(t1)] - soff[size_t(t0)]));
        out.push_back({t0, t1});
        t0 = t1;
    }
    *arena_words = widest;
    return out;
}

}  // namespace gmsx
