// Host-only check of huygens_amd/csrc/hz_mixplan.h and hz_lds.h (tests/test_mix_host_cpu.py):
// hz::mix_plan against the formula restated here, and hz::allow_lds against a counting stand-in
// for hipFuncSetAttribute (with a switch that fails the next call).  No HIP runtime is linked.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../huygens_amd/csrc/hz_lds.h"
#include "../../huygens_amd/csrc/hz_mixplan.h"

namespace {

std::atomic<int> g_calls{0}, g_errors_set{0};
std::atomic<bool> g_fail_next{false};
std::atomic<const void*> g_last_kernel{nullptr};
std::atomic<int> g_last_value{0}, g_last_attr{-1};
int g_failed = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

long ceil_div(long a, long b) { return (a + b - 1) / b; }

int plan_cases() {
    int cases = 0;
    for (long groups : {1L, 2L, 3L, 19L, 64L, 256L, 257L})
        for (int tile : {1024, 2048})
            for (long n : {1L, (long)tile - 1, (long)tile, (long)tile + 1, 5L * tile + 7, 480000L})
                for (int target : {1, 256, 304}) {
                    const hz::MixPlan p = hz::mix_plan(groups, n, tile, target);
                    // the formula, restated
                    const long ntiles = ceil_div(n, tile);
                    long nseg = ceil_div(target, groups);
                    if (nseg > ntiles) nseg = ntiles;
                    if (nseg < 1) nseg = 1;
                    const long seg_tiles = ceil_div(ntiles, nseg);
                    nseg = ceil_div(ntiles, seg_tiles);
                    CHECK(p.ntiles == ntiles && p.nseg == nseg && p.seg_tiles == seg_tiles);
                    CHECK(p.n_pad == ntiles * tile && p.seg_len == seg_tiles * tile);
                    CHECK(p.n_pad >= n && p.n_pad % tile == 0);
                    CHECK((p.nseg - 1) * p.seg_tiles < p.ntiles && p.ntiles <= p.nseg * p.seg_tiles);   // no empty segment
                    ++cases;
                }
    return cases;
}

// distinct addresses standing in for kernels
char g_k[8];
const void* K(int i) { return &g_k[i]; }

void lds_cases() {
    int c0 = g_calls;
    // one runtime call per (device, kernel); none on a repeat with an equal or smaller size
    CHECK(hz::allow_lds(0, K(0), 1000) == HZ_OK && g_calls == c0 + 1);
    CHECK(g_last_kernel == K(0) && g_last_value == 1000 &&
          g_last_attr == (int)hipFuncAttributeMaxDynamicSharedMemorySize);
    CHECK(hz::allow_lds(0, K(0), 1000) == HZ_OK && g_calls == c0 + 1);
    CHECK(hz::allow_lds(0, K(0), 10) == HZ_OK && g_calls == c0 + 1);
    CHECK(hz::allow_lds(0, K(1), 1000) == HZ_OK && g_calls == c0 + 2 && g_last_kernel == K(1));
    // one more when the size grows; the larger grant is the one remembered
    CHECK(hz::allow_lds(0, K(0), 2000) == HZ_OK && g_calls == c0 + 3 && g_last_value == 2000);
    CHECK(hz::allow_lds(0, K(0), 1500) == HZ_OK && g_calls == c0 + 3);
    // two devices each get their call
    CHECK(hz::allow_lds(1, K(0), 2000) == HZ_OK && g_calls == c0 + 4);
    CHECK(hz::allow_lds(1, K(0), 2000) == HZ_OK && g_calls == c0 + 4);
    CHECK(hz::allow_lds(0, K(0), 2000) == HZ_OK && g_calls == c0 + 4);
    // a failed call is reported and tried again next time
    const int e0 = g_errors_set;
    g_fail_next = true;
    CHECK(hz::allow_lds(0, K(2), 3000) == HZ_E_HIP && g_calls == c0 + 5 && g_errors_set == e0 + 1);
    CHECK(hz::allow_lds(0, K(2), 3000) == HZ_OK && g_calls == c0 + 6);
    CHECK(hz::allow_lds(0, K(2), 3000) == HZ_OK && g_calls == c0 + 6);
    // ... and a failed growth keeps the smaller grant
    g_fail_next = true;
    CHECK(hz::allow_lds(0, K(2), 4000) == HZ_E_HIP && g_calls == c0 + 7);
    CHECK(hz::allow_lds(0, K(2), 3000) == HZ_OK && g_calls == c0 + 7);
    CHECK(hz::allow_lds(0, K(2), 4000) == HZ_OK && g_calls == c0 + 8);
    // the list form: every kernel of the list, and the first error stops it
    c0 = g_calls;
    CHECK(hz::allow_lds(2, {K(3), K(4), K(5)}, 512) == HZ_OK && g_calls == c0 + 3);
    CHECK(hz::allow_lds(2, {K(3), K(4), K(5)}, 512) == HZ_OK && g_calls == c0 + 3);
    g_fail_next = true;
    CHECK(hz::allow_lds(3, {K(3), K(4)}, 512) == HZ_E_HIP && g_calls == c0 + 4);
    CHECK(hz::allow_lds(3, {K(3), K(4)}, 512) == HZ_OK && g_calls == c0 + 6);
    // a device outside the table is served by the runtime every time
    c0 = g_calls;
    CHECK(hz::allow_lds(1000, K(0), 64) == HZ_OK && hz::allow_lds(1000, K(0), 64) == HZ_OK && g_calls == c0 + 2);
}

// more kernels than the table holds: the overflow asks the runtime every time, the rest stay remembered
void full_table() {
    static std::vector<char> many(hz::lds_detail::kSlots + 50);
    for (char& k : many) CHECK(hz::allow_lds(0, &k, 128) == HZ_OK);
    const int c0 = g_calls;
    for (char& k : many) CHECK(hz::allow_lds(0, &k, 128) == HZ_OK);
    CHECK(g_calls - c0 > 0 && g_calls - c0 <= 50 + 16);   // (the slots the cases above took)
}

// eight threads asking for the same pair at once: exactly one runtime call
void threaded() {
    const int c0 = g_calls;
    std::atomic<int> ready{0}, bad{0};
    std::vector<std::thread> ts;
    for (int i = 0; i < 8; ++i)
        ts.emplace_back([&] {
            ++ready;
            while (ready.load() < 8) {
            }
            for (int r = 0; r < 1000; ++r)
                if (hz::allow_lds(5, K(6), 4096) != HZ_OK) ++bad;
        });
    for (std::thread& t : ts) t.join();
    CHECK(bad == 0 && g_calls == c0 + 1);
}

}  // namespace

extern "C" {
hipError_t hipFuncSetAttribute(const void* func, hipFuncAttribute attr, int value) {
    ++g_calls;
    g_last_kernel = func;
    g_last_attr = (int)attr;
    g_last_value = value;
    if (g_fail_next.exchange(false)) return hipErrorInvalidValue;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "invalid value (test)"; }
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
    const int cases = plan_cases();
    lds_cases();
    threaded();
    full_table();
    if (g_failed) return 1;
    std::printf("mix ok: %d plans, %d runtime calls\n", cases, g_calls.load());
    return 0;
}
