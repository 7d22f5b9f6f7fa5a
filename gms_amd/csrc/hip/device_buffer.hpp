// The one owner of a device allocation in the host code of the kernel translation units: freed when it leaves scope.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

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
    template <class T> T *release() {  // hands the allocation to a longer-lived owner (the graph)
        T *q = as<T>();
        p = nullptr;
        return q;
    }
};

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

}  // namespace gmsx
