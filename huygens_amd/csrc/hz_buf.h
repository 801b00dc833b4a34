// hz_buf.h -- move-only owners of device memory (hz::DevBuf) and pinned host memory (hz::PinBuf).
// Every handle's buffers are members of these types, so deleting a handle frees them; a buffer
// that grows on demand is reserve()d before use.  Self-contained host code: a plain C++ compiler
// can include it (tests/cpp/devbuf_host.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "../../include/huygens_hip.h"

namespace hz {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// pointer and capacity (elements) travel together: the capacity is nonzero only while the pointer
// is a live allocation of that many elements
template <typename T, bool kPinned>
class Buf {
public:
    Buf() = default;
    explicit Buf(unsigned host_flags) : flags_(host_flags) { static_assert(kPinned, "flags: pinned memory only"); }
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_), flags_(o.flags_) { o.p_ = nullptr, o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_, flags_ = o.flags_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }

    // at least n elements; the contents are not kept when it grows.  A failed allocation leaves
    // the buffer empty (null, capacity 0), so a later smaller request allocates again.
    int reserve(size_t n) { return n <= cap_ ? HZ_OK : grow(n); }
    void reset() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, cap_ = 0;
    }

private:
    // out of line: the callers' hot paths keep only the capacity test
    __attribute__((noinline)) int grow(size_t n) {
        reset();
        void* q = nullptr;
        hipError_t e;
        if constexpr (kPinned)
            e = hipHostMalloc(&q, n * sizeof(T), flags_);
        else
            e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) {
            set_error("%s(%zu bytes) failed: %s (%s:%d)", kPinned ? "hipHostMalloc" : "hipMalloc", n * sizeof(T),
                      hipGetErrorString(e), __FILE__, __LINE__);
            return HZ_E_HIP;
        }
        p_ = static_cast<T*>(q), cap_ = n;
        return HZ_OK;
    }

    T* p_ = nullptr;
    size_t cap_ = 0;
    unsigned flags_ = hipHostMallocDefault;   // hipHostMalloc flags (PinBuf's constructor argument)
};

template <typename T>
using DevBuf = Buf<T, false>;
template <typename T>
using PinBuf = Buf<T, true>;

}  // namespace hz
