// The count / scan / fill scaffold of the device LISTING calls (bk_list.hip, kcstar_list.hip).
//
// A listing call builds one deterministic task list on the host; one wave searches one task, and every structure of a search lives in the
// task's slab of a global arena, so no width is refused.  Tasks run in launches whose slabs fit the arena budget (launch_plan.hpp; a test
// hook option shrinks it).  Two passes of the same kernel over the list:
//   FILL = false  per task: results and member total into cnt[t] / mem[t]; per call: a few accumulator words (maxima, histogram, flags)
//   scan          exclusive scans give every task its base in the caller's arrays: cbase / mbase, n_tasks + 1 entries
//   FILL = true   the identical search again, every result written at its task's base + a running offset
// Nothing that shapes a search may depend on timing, so pass 2 meets the results of pass 1 in the same order; a task that would write more
// or other than pass 1 counted raises a flag word instead (GMSX_ERR_KERNEL), it never writes past its span, and the caller's buffers are
// written only after the fill's flag word was read as zero.
// Pass 1 of the last call is kept: a sizing call always searches (it is what a caller times), a fill call whose key matches re-uses it
// instead of searching a third time.  The key (host/list_key.hpp) is the upload's serial, the handle, its device arrays and the call's
// parameters: a cached pass 1 belongs to one upload, and a handle that re-uses the addresses of a freed one searches again.
//
// A new listing call brings its kernel, its slab-size formula, the host loop that fills ListPass1::soff and its task arrays, the copy into
// the caller's arrays and the extern "C" entry; it calls, in this order: ensure_pass1 { upload_tasks, alloc_zeroed x3, run_list_pass,
// finish_count_pass }, then for a fill alloc_zeroed, run_list_pass, finish_fill_pass.
#pragma once
#include "device_buffer.hpp"
#include "device_graph.hpp"
#include "launch_plan.hpp"
#include "list_key.hpp"

#include <vector>

namespace gmsx {

// the wave's writes to its slab visible to the other lanes of the wave (readers: this wave only)
__device__ __forceinline__ void wave_slab_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// pass 1 of the last call; an algorithm derives from it to add its info struct
struct ListPass1 {
    ListKey key;
    bool valid = false;
    int64_t n_tasks = 0;
    std::vector<int64_t> soff;  // slab offsets (words), n_tasks + 1
    DevBuf task[2];             // the algorithm's int32 task arrays
    DevBuf slab_off, cbase, mbase;
    bool matches(const ListKey &k) const { return valid && key == k; }
    void clear() {
        valid = false;
        key = ListKey();
        soff.clear();
        soff.shrink_to_fit();
        for (DevBuf &t : task) t.reset();
        slab_off.reset();
        cbase.reset();
        mbase.reset();
    }
};

// the cache rule.  pass1() fills the cleared p1; on failure nothing is kept.
template <class Pass1>
int ensure_pass1(ListPass1 &p1, const ListKey &key, bool sizing, Pass1 &&pass1) {
    if (p1.matches(key) && !sizing) return GMSX_OK;
    p1.clear();
    if (int rc = pass1()) {
        p1.clear();
        return rc;
    }
    p1.key = key;
    p1.valid = true;
    return GMSX_OK;
}

// p1.soff and the task arrays (soff.size() - 1 entries each) to the device; cbase / mbase allocated
inline int upload_tasks(ListPass1 &p1, const std::vector<int32_t> *const *tasks, int n_arrays, hipStream_t s) {
    const int64_t nt = int64_t(p1.soff.size()) - 1;
    p1.n_tasks = nt;
    for (int i = 0; i < n_arrays; ++i) {
        GMSX_HIP(hipMalloc(&p1.task[i].p, size_t(nt > 0 ? nt : 1) * 4));
        if (nt > 0) GMSX_HIP(hipMemcpyAsync(p1.task[i].p, tasks[i]->data(), size_t(nt) * 4, hipMemcpyHostToDevice, s));
    }
    GMSX_HIP(hipMalloc(&p1.slab_off.p, size_t(nt + 1) * 8));
    GMSX_HIP(hipMalloc(&p1.cbase.p, size_t(nt + 1) * 8));
    GMSX_HIP(hipMalloc(&p1.mbase.p, size_t(nt + 1) * 8));
    GMSX_HIP(hipMemcpyAsync(p1.slab_off.p, p1.soff.data(), size_t(nt + 1) * 8, hipMemcpyHostToDevice, s));
    return GMSX_OK;
}

inline int alloc_zeroed(DevBuf &d, size_t bytes, hipStream_t s) {
    GMSX_HIP(hipMalloc(&d.p, bytes));
    GMSX_HIP(hipMemsetAsync(d.p, 0, bytes, s));
    return GMSX_OK;
}

// the arena of an algorithm: at most a quarter of the free memory and cap_bytes, shrunk to `option` MB when that is set, at least 4 words
struct ListArena {
    unsigned long long cap_bytes;
    const char *option;
    int64_t max_tasks_per_launch;
};

// One pass: ev[e0] | launch(l, arena, arena_words) for every launch of the plan | ev[e0 + 1], synchronised.  An empty plan allocates nothing.
template <class LaunchFn>
int run_list_pass(const ListPass1 &p1, const ListArena &a, int e0, int *launches, LaunchFn &&launch) {
    Ctx &cx = ctx();
    hipStream_t s = cx.stream;
    GMSX_HIP(hipEventRecord(cx.ev[e0], s));
    size_t free_b = 0, total_b = 0;
    GMSX_HIP(hipMemGetInfo(&free_b, &total_b));
    unsigned long long budget_words = std::min<unsigned long long>(free_b / 4, a.cap_bytes) / 4;
    const long long mb = opt_int(a.option, 0);
    if (mb >= 1) budget_words = std::min<unsigned long long>(budget_words, ((unsigned long long)mb << 20) / 4);
    unsigned long long arena_words = 0;
    const std::vector<Launch> plan =
        plan_launches(p1.soff, p1.n_tasks, std::max<unsigned long long>(budget_words, 4), a.max_tasks_per_launch, &arena_words);
    DevBuf arena;
    if (!plan.empty()) GMSX_HIP(hipMalloc(&arena.p, size_t(arena_words) * 4 + 64));
    for (const Launch &l : plan) {
        launch(l, arena.p, arena_words);
        GMSX_HIP(hipGetLastError());
        ++*launches;
    }
    if (!plan.empty()) GMSX_HIP(hipStreamSynchronize(s));
    GMSX_HIP(hipEventRecord(cx.ev[e0 + 1], s));
    return GMSX_OK;
}

// After the count pass (events ev[e0], ev[e0 + 1]): cnt / mem scanned into p1.cbase / p1.mbase; the accumulator words, the two totals and the
// pass's milliseconds read back in one synchronisation.
inline int finish_count_pass(ListPass1 &p1, const DevBuf &cnt, const DevBuf &mem, const DevBuf &acc, unsigned long long *host_acc, int acc_words,
                             int64_t tot[2], int e0, double *ms) {
    Ctx &cx = ctx();
    hipStream_t s = cx.stream;
    const int64_t nt = p1.n_tasks;
    if (int rc = exclusive_scan_i64(cnt.as<const int64_t>(), p1.cbase.as<int64_t>(), nt + 1, s)) return rc;
    if (int rc = exclusive_scan_i64(mem.as<const int64_t>(), p1.mbase.as<int64_t>(), nt + 1, s)) return rc;
    GMSX_HIP(hipMemcpyAsync(host_acc, acc.p, size_t(acc_words) * 8, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(&tot[0], p1.cbase.as<int64_t>() + nt, 8, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipMemcpyAsync(&tot[1], p1.mbase.as<int64_t>() + nt, 8, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    float f_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&f_ms, cx.ev[e0], cx.ev[e0 + 1]));
    *ms = double(f_ms);
    return GMSX_OK;
}

// After the fill pass (events ev[e0], ev[e0 + 1]): the accumulator words and the pass's milliseconds.
inline int finish_fill_pass(const DevBuf &acc, unsigned long long *host_acc, int acc_words, int e0, double *ms) {
    Ctx &cx = ctx();
    hipStream_t s = cx.stream;
    GMSX_HIP(hipMemcpyAsync(host_acc, acc.p, size_t(acc_words) * 8, hipMemcpyDeviceToHost, s));
    GMSX_HIP(hipStreamSynchronize(s));
    float f_ms = 0.f;
    GMSX_HIP(hipEventElapsedTime(&f_ms, cx.ev[e0], cx.ev[e0 + 1]));
    *ms = double(f_ms);
    return GMSX_OK;
}

}  // namespace gmsx
