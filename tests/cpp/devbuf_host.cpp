// Host-only check of huygens_amd/csrc/hz_buf.h (tests/test_devbuf_cpu.py): the HIP allocation
// calls are counting malloc / free stand-ins defined here, so the program links no HIP runtime.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../huygens_amd/csrc/hz_buf.h"

namespace {

int g_allocs = 0, g_frees = 0, g_live = 0;   // all four calls
int g_host_allocs = 0, g_host_frees = 0;     // the pinned pair's share
size_t g_last_bytes = 0;
unsigned g_last_flags = 0;
bool g_fail_next = false;
int g_errors_set = 0;
int g_failed = 0;

hipError_t fake_alloc(void** p, size_t bytes) {
    if (g_fail_next) {
        g_fail_next = false;
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    ++g_allocs, ++g_live;
    g_last_bytes = bytes;
    return hipSuccess;
}

hipError_t fake_free(void* p) {
    if (p) ++g_frees, --g_live;
    std::free(p);
    return hipSuccess;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

struct Bufs {   // a handle's sub-struct (hz_fb::Resp): buffers next to plain settings
    int mode = 3;
    hz::DevBuf<double> a, b[2];
    hz::DevBuf<int> c;
    hz::PinBuf<double> p;
};

template <typename B>
void reserve_cases(int* kind_allocs, int* kind_frees) {
    B buf;
    CHECK(buf.get() == nullptr && buf.cap() == 0);
    int a0 = g_allocs, f0 = g_frees;
    CHECK(buf.reserve(100) == HZ_OK);
    CHECK(g_allocs == a0 + 1 && g_frees == f0 && g_last_bytes == 100 * sizeof(double));
    CHECK(buf.get() != nullptr && buf.cap() == 100);
    double* const first = buf;   // implicit conversion
    CHECK(first == buf.get());
    // below (and at) the capacity: nothing is allocated, the buffer stays
    CHECK(buf.reserve(40) == HZ_OK && buf.reserve(100) == HZ_OK && buf.reserve(0) == HZ_OK);
    CHECK(g_allocs == a0 + 1 && g_frees == f0 && buf.get() == first && buf.cap() == 100);
    // above: one free, one allocation of exactly the requested size
    CHECK(buf.reserve(101) == HZ_OK);
    CHECK(g_allocs == a0 + 2 && g_frees == f0 + 1 && g_last_bytes == 101 * sizeof(double) && buf.cap() == 101);
    // a failed growth is a returned error and leaves the buffer empty ...
    const int e0 = g_errors_set;
    g_fail_next = true;
    CHECK(buf.reserve(5000) == HZ_E_HIP);
    CHECK(g_errors_set == e0 + 1);
    CHECK(buf.get() == nullptr && buf.cap() == 0);
    CHECK(g_allocs == a0 + 2 && g_frees == f0 + 2);
    // ... so a smaller request afterwards allocates again instead of passing the capacity test
    CHECK(buf.reserve(50) == HZ_OK);
    CHECK(buf.get() != nullptr && buf.cap() == 50 && g_allocs == a0 + 3 && g_last_bytes == 50 * sizeof(double));
    buf.reset();
    CHECK(buf.get() == nullptr && buf.cap() == 0 && g_frees == f0 + 3);
    buf.reset();   // idempotent
    CHECK(g_frees == f0 + 3);
    CHECK(buf.reserve(7) == HZ_OK);   // freed by the destructor
    a0 = g_allocs - a0, f0 = g_frees - f0;
    if (kind_allocs) CHECK(*kind_allocs == a0);
    if (kind_frees) CHECK(*kind_frees == f0);
}

void move_cases() {
    hz::DevBuf<double> dst, src;
    CHECK(dst.reserve(10) == HZ_OK && src.reserve(20) == HZ_OK);
    double* const sp = src.get();
    const int a0 = g_allocs, f0 = g_frees;
    dst = std::move(src);   // frees the target's old buffer exactly once, empties the source
    CHECK(g_frees == f0 + 1 && g_allocs == a0);
    CHECK(dst.get() == sp && dst.cap() == 20);
    CHECK(src.get() == nullptr && src.cap() == 0);
    hz::DevBuf<double>& self = dst;
    dst = std::move(self);   // self-assignment keeps the buffer
    CHECK(dst.get() == sp && dst.cap() == 20 && g_frees == f0 + 1);
    hz::DevBuf<double> made(std::move(dst));   // move construction
    CHECK(made.get() == sp && made.cap() == 20 && dst.get() == nullptr && dst.cap() == 0);
    CHECK(g_frees == f0 + 1 && g_allocs == a0);
    // the freezer's snapshot growth: allocate new, (copy), move-assign
    hz::DevBuf<double> grown;
    CHECK(grown.reserve(40) == HZ_OK);
    made = std::move(grown);
    CHECK(made.cap() == 40 && g_frees == f0 + 2);
}

void struct_cases() {
    Bufs s;
    s.mode = 1;
    CHECK(s.a.reserve(8) == HZ_OK && s.b[0].reserve(8) == HZ_OK && s.b[1].reserve(9) == HZ_OK);
    CHECK(s.c.reserve(3) == HZ_OK && s.p.reserve(4) == HZ_OK);
    const int f0 = g_frees, live0 = g_live;
    s = Bufs();   // the `R = hz_fb::Resp()` idiom
    CHECK(g_frees == f0 + 5 && g_live == live0 - 5);
    CHECK(!s.a && !s.b[0] && !s.b[1] && !s.c && !s.p && s.a.cap() == 0 && s.p.cap() == 0 && s.mode == 3);
}

void pinned_flags() {
    hz::PinBuf<double> plain;
    CHECK(plain.reserve(4) == HZ_OK && g_last_flags == hipHostMallocDefault);
    hz::PinBuf<double> mapped{hipHostMallocCoherent | hipHostMallocMapped};
    CHECK(mapped.reserve(4) == HZ_OK && g_last_flags == (hipHostMallocCoherent | hipHostMallocMapped));
    CHECK(mapped.reserve(8) == HZ_OK && g_last_flags == (hipHostMallocCoherent | hipHostMallocMapped));
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes); }
hipError_t hipFree(void* p) { return fake_free(p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
    g_last_flags = flags;
    const hipError_t e = fake_alloc(p, bytes);
    if (e == hipSuccess) ++g_host_allocs;
    return e;
}
hipError_t hipHostFree(void* p) {
    if (p) ++g_host_frees;
    return fake_free(p);
}
const char* hipGetErrorString(hipError_t) { return "out of memory (test)"; }
}

namespace hz {
void set_error(const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    ++g_errors_set;
}
}  // namespace hz

int main() {
    reserve_cases<hz::DevBuf<double>>(nullptr, nullptr);
    CHECK(g_host_allocs == 0 && g_host_frees == 0);   // device buffers never touch the pinned pair
    const int a0 = g_allocs, f0 = g_frees;
    reserve_cases<hz::PinBuf<double>>(&g_host_allocs, &g_host_frees);   // ... and pinned ones only it
    CHECK(g_allocs - a0 == g_host_allocs && g_frees - f0 == g_host_frees);
    move_cases();
    struct_cases();
    pinned_flags();
    CHECK(g_live == 0);   // every destructor ran by here
    CHECK(g_allocs == g_frees);
    if (g_failed) return 1;
    std::printf("devbuf ok: %d allocations, %d frees, live %d\n", g_allocs, g_frees, g_live);
    return 0;
}
