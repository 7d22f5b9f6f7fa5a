// The one owner of a device allocation in the host code of the kernel translation units: freed when it leaves scope.  Beside it HostStage, the
// one way results leave device memory for a caller's arrays.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "gmsx.h"

namespace gmsx {

struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// Owns like DevBuf, reads like a T*: the fields of gmsx_graph and the typed temporaries of its builds.  Every site that only reads one — a
// kernel argument, g->off + k, g->hoff[v], a hipMemcpyAsync operand — takes it as the pointer; get() where deduction needs a real one.
// A finished buffer is handed to a longer-lived owner (the graph) by move-assignment.  Never static or global: an owner that outlives
// the HIP runtime would free into it.
template <class T>
struct DevArr : DevBuf {
    operator T *() const { return static_cast<T *>(p); }
    T *get() const { return static_cast<T *>(p); }
};
static_assert(!std::is_copy_constructible<DevArr<int>>::value, "one owner per allocation");
static_assert(std::is_nothrow_move_constructible<DevArr<int>>::value, "handed over by move");
static_assert(std::is_convertible<const DevArr<int> &, int *>::value, "reads like a T*");

// `count` elements of T (at least one) into the empty d.  Any failure is GMSX_ERR_DEVICE_MEM and leaves no sticky error behind; a site that
// tells out-of-memory from other failures writes GMSX_HIP(hipMalloc(&d.p, bytes)) instead.
template <class T>
int dalloc(DevBuf &d, int64_t count) {
    if (hipMalloc(&d.p, size_t(std::max<int64_t>(count, 1)) * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        d.p = nullptr;
        return GMSX_ERR_DEVICE_MEM;
    }
    return GMSX_OK;
}
template <class T>
int dalloc(DevArr<T> &d, int64_t count) {
    return dalloc<T>(static_cast<DevBuf &>(d), count);
}

// Results on their way from device memory to a caller's arrays.  THE ORDER: the call reads its flag words as zero, fetch() starts a copy into
// host memory of the stage's own, the call synchronizes, and only then deliver() writes the caller's memory — a call that fails on the way
// has not touched it.  A null dst or an empty array is skipped.
class HostStage {
    struct Item {
        void *dst;
        std::vector<unsigned char> tmp;
    };
    std::vector<Item> items;

  public:
    int fetch(void *dst, const void *src, size_t bytes, hipStream_t s) {
        if (!dst || bytes == 0) return GMSX_OK;
        items.push_back(Item{dst, std::vector<unsigned char>(bytes)});
        if (hipMemcpyAsync(items.back().tmp.data(), src, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) {
            (void)hipGetLastError();
            return GMSX_ERR_KERNEL;
        }
        return GMSX_OK;
    }
    // the three arrays of an edge list of ne entries (all given, or none)
    int fetch_edges(int32_t *eu, int32_t *ev, int32_t *ew, const DevBuf &du, const DevBuf &dv, const DevBuf &dw, size_t ne, hipStream_t s) {
        if (int rc = fetch(eu, du.p, ne * sizeof(int32_t), s)) return rc;
        if (int rc = fetch(ev, dv.p, ne * sizeof(int32_t), s)) return rc;
        return fetch(ew, dw.p, ne * sizeof(int32_t), s);
    }
    void deliver() const {
        for (const Item &it : items) std::memcpy(it.dst, it.tmp.data(), it.tmp.size());
    }
};

}  // namespace gmsx
