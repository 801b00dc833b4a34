// hz_lds.h -- hz::allow_lds, the one place that raises a kernel's dynamic-LDS limit
// (hipFuncAttributeMaxDynamicSharedMemorySize).  The attribute belongs to the current device's
// copy of the function, so the grant is remembered per (device, kernel): the runtime is called
// again only for a larger size or after a call that failed.  A repeat is lock-free (a probe of the
// kernel's slot, one atomic load of the size granted), so a launch path may call it every time.
// The caller has made `device` current (hz::check_handle / hz::select_device).  Self-contained
// host code: a plain C++ compiler can include it (tests/cpp/mix_host.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <mutex>

#include "../../include/huygens_hip.h"

namespace hz {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

namespace lds_detail {

constexpr int kDevices = 16;    // a device past it, or a full table, asks the runtime every time
constexpr int kSlots = 1024;    // kernels with an opt-in, template instantiations counted: ~200

struct Slot {
    std::atomic<const void*> kernel{nullptr};
    std::atomic<size_t> granted[kDevices] = {};
};
struct Table {
    Slot slot[kSlots];   // open addressing; slots are claimed under `mu` and never released
    std::mutex mu;       // the slow path only
    Slot* find(const void* kernel, bool claim) {
        const size_t h = (size_t)((uintptr_t)kernel * 0x9E3779B97F4A7C15ull >> 40);
        for (int i = 0; i < kSlots; ++i) {
            Slot* s = &slot[(h + i) % kSlots];
            const void* k = s->kernel.load(std::memory_order_acquire);
            if (k == nullptr && claim) s->kernel.store(k = kernel, std::memory_order_release);
            if (k == kernel) return s;
            if (k == nullptr) break;
        }
        return nullptr;
    }
};

}  // namespace lds_detail

inline int allow_lds(int device, const void* kernel, size_t bytes) {
    static lds_detail::Table t;
    const bool keyed = device >= 0 && device < lds_detail::kDevices;
    lds_detail::Slot* s = keyed ? t.find(kernel, false) : nullptr;
    if (s && s->granted[device].load(std::memory_order_acquire) >= bytes) return HZ_OK;
    std::lock_guard<std::mutex> lock(t.mu);
    s = keyed ? t.find(kernel, true) : nullptr;
    if (s && s->granted[device].load(std::memory_order_relaxed) >= bytes) return HZ_OK;   // another thread's call
    if (hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) {
        set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed on device %d: %s", bytes, device,
                  hipGetErrorString(e));
        return HZ_E_HIP;
    }
    if (s) s->granted[device].store(bytes, std::memory_order_release);
    return HZ_OK;
}

// kernels that share one size
inline int allow_lds(int device, std::initializer_list<const void*> kernels, size_t bytes) {
    for (const void* k : kernels)
        if (int r = allow_lds(device, k, bytes)) return r;
    return HZ_OK;
}

}  // namespace hz
