// The one owner of a device allocation in the host code of the kernel translation units: freed when it leaves scope.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

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

}  // namespace gmsx
