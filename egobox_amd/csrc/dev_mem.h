// The library's owning buffers: a device allocation (DevMem) or a pinned host allocation (PinMem) of elements T that frees
// itself and records its size in bytes -- what the resource pool's byte counts are sums of.  Move-only.  Kernel-facing code
// takes the plain pointer (`buf.p`, or the implicit conversion).
#pragma once
#include <cstddef>
#include <utility>

#include "egx_internal.h"

namespace egx {

template <typename T, bool kPinned>
struct Mem {
    T *p = nullptr;
    size_t bytes = 0;
    Mem() = default;
    Mem(Mem &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Mem &operator=(Mem &&o) noexcept {  // (what this one held is freed with `o`)
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~Mem() { reset(); }
    void reset() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }
    operator T *() const { return p; }
    // grow-only: a buffer declared outside a chunk loop is allocated once (a hipMalloc / hipFree pair of a 1 GiB block per
    // 16 384 query points used to sit inside predict_var's loop).  Device memory comes from dev_malloc: the pool of destroyed
    // handles' resources is given back before out-of-memory is reported
    int alloc(size_t n) {
        if (n == 0) n = 1;
        if (p && bytes >= sizeof(T) * n) return EGX_SUCCESS;
        reset();
        EGX_HIP_CHECK(kPinned ? hipHostMalloc(reinterpret_cast<void **>(&p), sizeof(T) * n, hipHostMallocDefault)
                              : dev_malloc(&p, sizeof(T) * n));
        bytes = sizeof(T) * n;
        return EGX_SUCCESS;
    }
};
template <typename T>
using DevMem = Mem<T, false>;
template <typename T>
using PinMem = Mem<T, true>;
using DevBuf = DevMem<double>;  // the scoped temporaries of one call

}  // namespace egx
