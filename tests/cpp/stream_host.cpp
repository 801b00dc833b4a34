// Host-only check of huygens_amd/csrc/hz_stream.h (tests/test_stream_host_cpu.py): the HIP stream
// and event calls are counting stand-ins defined here (every stream and event is a small heap
// block, so the sanitized build sees a double destroy or a leak), and no HIP runtime is linked.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../huygens_amd/csrc/hz_stream.h"

namespace {

int g_s_created = 0, g_s_destroyed = 0, g_s_live = 0, g_s_synced = 0;
int g_e_created = 0, g_e_destroyed = 0, g_e_live = 0, g_e_recorded = 0, g_e_timed = 0;
unsigned g_last_stream_flags = 0, g_last_event_flags = 0;
hipStream_t g_last_synced = nullptr, g_last_destroyed = nullptr;
bool g_fail_next_create = false;   // the next stream or event creation fails
int g_errors_set = 0;
int g_failed = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

// a caller's stream (torch's): made and destroyed outside the type under test
hipStream_t foreign_stream() { return static_cast<hipStream_t>(std::malloc(1)); }
void foreign_free(hipStream_t s) { std::free(s); }

void stream_lifetime() {
    const int c0 = g_s_created, d0 = g_s_destroyed;
    {
        hz::Stream s;
        CHECK(static_cast<hipStream_t>(s) == nullptr && !s.owned());
        CHECK(s.create() == HZ_OK);
        CHECK(s.owned() && static_cast<hipStream_t>(s) != nullptr && g_last_stream_flags == hipStreamNonBlocking);
        CHECK(g_s_created == c0 + 1 && g_s_destroyed == d0);
        hipStream_t raw = s;   // implicit conversion: what the launch sites use
        CHECK(s.sync() == HZ_OK && g_last_synced == raw);
    }
    CHECK(g_s_created == c0 + 1 && g_s_destroyed == d0 + 1);   // a private stream: destroyed exactly once
    {
        hz::Stream never;   // a half-built handle's
    }
    CHECK(g_s_destroyed == d0 + 1);
    hipStream_t f = foreign_stream();
    {
        hz::Stream s;
        CHECK(s.rebind(f, hz::NullMeans::Legacy) == HZ_OK);
        CHECK(!s.owned() && static_cast<hipStream_t>(s) == f);
    }
    CHECK(g_s_destroyed == d0 + 1);   // a borrowed stream: never destroyed
    foreign_free(f);
}

void rebind_cases(hz::NullMeans policy) {
    const bool priv = policy == hz::NullMeans::Private;
    hipStream_t f = foreign_stream(), g = foreign_stream();
    {
        hz::Stream s;
        CHECK(s.create() == HZ_OK);
        hipStream_t own = s;
        // owned -> non-null: the old stream is synchronized, then destroyed; the new one is borrowed
        int c0 = g_s_created, d0 = g_s_destroyed, y0 = g_s_synced;
        CHECK(s.rebind(f, policy) == HZ_OK);
        CHECK(g_s_synced == y0 + 1 && g_last_synced == own && g_last_destroyed == own);
        CHECK(g_s_created == c0 && g_s_destroyed == d0 + 1 && !s.owned() && static_cast<hipStream_t>(s) == f);
        // borrowed -> non-null: synchronized, nothing destroyed
        y0 = g_s_synced;
        CHECK(s.rebind(g, policy) == HZ_OK);
        CHECK(g_s_synced == y0 + 1 && g_last_synced == f);
        CHECK(g_s_created == c0 && g_s_destroyed == d0 + 1 && !s.owned() && static_cast<hipStream_t>(s) == g);
        // borrowed -> null
        CHECK(s.rebind(nullptr, policy) == HZ_OK);
        CHECK(g_s_destroyed == d0 + 1 && g_s_created == c0 + (priv ? 1 : 0));
        CHECK(s.owned() == priv && (static_cast<hipStream_t>(s) != nullptr) == priv);
        // owned -> null
        CHECK(s.create() == HZ_OK);
        c0 = g_s_created, d0 = g_s_destroyed;
        CHECK(s.rebind(nullptr, policy) == HZ_OK);
        CHECK(g_s_destroyed == d0 + 1 && g_s_created == c0 + (priv ? 1 : 0));
        CHECK(s.owned() == priv && (static_cast<hipStream_t>(s) != nullptr) == priv);
        // the null stream bound (Legacy) or a private one (Private) -> non-null
        d0 = g_s_destroyed;
        CHECK(s.rebind(f, policy) == HZ_OK);
        CHECK(g_s_destroyed == d0 + (priv ? 1 : 0) && !s.owned() && static_cast<hipStream_t>(s) == f);
    }
    foreign_free(f), foreign_free(g);
}

void failed_create() {
    const int e0 = g_errors_set;
    {
        hz::Stream s;
        g_fail_next_create = true;
        CHECK(s.create() == HZ_E_HIP && g_errors_set == e0 + 1);
        CHECK(!s.owned() && static_cast<hipStream_t>(s) == nullptr);
    }
    const int d0 = g_s_destroyed;
    {
        hz::Stream s;
        CHECK(s.create() == HZ_OK);
        g_fail_next_create = true;
        CHECK(s.rebind(nullptr, hz::NullMeans::Private) == HZ_E_HIP);   // the old one went, no new one came
        CHECK(g_s_destroyed == d0 + 1 && !s.owned() && static_cast<hipStream_t>(s) == nullptr);
    }
    CHECK(g_s_destroyed == d0 + 1);   // ... and its destructor destroyed nothing
    {
        hz::Event e;
        g_fail_next_create = true;
        CHECK(e.create(hipEventDisableTiming) == HZ_E_HIP && static_cast<hipEvent_t>(e) == nullptr);
    }
}

void move_cases() {
    const int d0 = g_s_destroyed, ed0 = g_e_destroyed;
    {
        hz::Stream a, b;
        CHECK(a.create() == HZ_OK && b.create() == HZ_OK);
        hipStream_t ra = a;
        b = std::move(a);   // the target's old stream goes exactly once, the source is left empty
        CHECK(g_s_destroyed == d0 + 1 && static_cast<hipStream_t>(b) == ra && b.owned());
        CHECK(static_cast<hipStream_t>(a) == nullptr && !a.owned());
        hz::Stream& self = b;
        b = std::move(self);
        CHECK(static_cast<hipStream_t>(b) == ra && b.owned() && g_s_destroyed == d0 + 1);
        hz::Stream c(std::move(b));
        CHECK(static_cast<hipStream_t>(c) == ra && c.owned() && !b.owned() && g_s_destroyed == d0 + 1);
    }
    CHECK(g_s_destroyed == d0 + 2);   // the moved-from objects destroyed nothing
    {
        hz::Event a, b;
        CHECK(a.create(hipEventDisableTiming) == HZ_OK && g_last_event_flags == hipEventDisableTiming);
        CHECK(b.create(hipEventDisableTiming) == HZ_OK);
        hipEvent_t ra = a;
        b = std::move(a);
        CHECK(g_e_destroyed == ed0 + 1 && static_cast<hipEvent_t>(b) == ra && static_cast<hipEvent_t>(a) == nullptr);
        std::vector<hz::Event> pool;   // hz_fb's ordering events
        for (int i = 0; i < 9; ++i) {
            pool.emplace_back();
            CHECK(pool.back().create(hipEventDisableTiming) == HZ_OK);
        }
        CHECK(g_e_destroyed == ed0 + 1);   // the vector's growth moved them
    }
    CHECK(g_e_destroyed == ed0 + 11 && g_e_live == 0);
    {
        hz::ProfEvents p, q;
        hipEvent_t* e = nullptr;
        CHECK(p.take(2, &e) == HZ_OK && g_e_live == 64);
        q = std::move(p);
        CHECK(g_e_live == 64 && q.used() == 2 && p.used() == 0);
        CHECK(p.take(2, &e) == HZ_OK && g_e_live == 128);   // the moved-from pool is an empty pool
    }
    CHECK(g_e_live == 0);
}

// groups of k across the 64-event growth steps: k consecutive live events each time
void take_cases(int k) {
    hz::ProfEvents p;
    hipStream_t f = foreign_stream();
    const int r0 = g_e_recorded;
    size_t taken = 0;
    for (int g = 0; g < 40; ++g) {   // 40 groups: 80, 120 or 200 events
        hipEvent_t* e = nullptr;
        CHECK(p.take(k, &e) == HZ_OK && e != nullptr);
        taken += k;
        CHECK(p.used() == taken);
        CHECK((size_t)g_e_live == (taken + 63) / 64 * 64);   // grown in steps of 64, only when needed
        CHECK(g_last_event_flags == hipEventDisableSystemFence);
        for (int j = 0; j < k; ++j) {
            CHECK(e[j] == p[taken - k + j]);
            CHECK(hipEventRecord(e[j], f) == hipSuccess);   // touches the block: a dead event trips the sanitizer
        }
    }
    CHECK(g_e_recorded == r0 + 40 * k);
    // complete groups only: the stand-in's elapsed time is 1 ms
    double ms = 0.5;
    int t0 = g_e_timed;
    CHECK(p.elapsed(k, 0, k - 1, &ms) == HZ_OK && ms == 40.5 && g_e_timed == t0 + 40);
    // a trailing incomplete group (a launch that failed between its events' take and the next one
    // cannot leave one, but the bound must not read past used()) is ignored
    hipEvent_t* e = nullptr;
    CHECK(p.take(k - 1, &e) == HZ_OK);
    ms = 0, t0 = g_e_timed;
    CHECK(p.elapsed(k, 0, k - 1, &ms) == HZ_OK && ms == 40.0 && g_e_timed == t0 + 40);
    // rewind keeps the events
    const int live = g_e_live, c0 = g_e_created;
    p.rewind();
    CHECK(p.used() == 0 && g_e_live == live);
    ms = 0;
    CHECK(p.elapsed(k, 0, k - 1, &ms) == HZ_OK && ms == 0.0);
    CHECK(p.take(k, &e) == HZ_OK && g_e_created == c0 && p.used() == (size_t)k);
    foreign_free(f);
}

void failed_growth() {
    const int e0 = g_errors_set;
    {
        hz::ProfEvents p;
        hipEvent_t* e = nullptr;
        for (int g = 0; g < 32; ++g) {   // exactly the first 64
            CHECK(p.take(2, &e) == HZ_OK);
            CHECK(hipEventRecord(e[0], nullptr) == hipSuccess && hipEventRecord(e[1], nullptr) == hipSuccess);
        }
        CHECK(g_e_live == 64);
        g_fail_next_create = true;
        e = nullptr;
        CHECK(p.take(2, &e) == HZ_E_HIP && e == nullptr && g_errors_set == e0 + 1);
        CHECK(p.used() == 64 && g_e_live == 64);
        double ms = 0;
        CHECK(p.elapsed(2, 0, 1, &ms) == HZ_OK && ms == 32.0);
        CHECK(p.take(2, &e) == HZ_OK && e != nullptr && p.used() == 66 && g_e_live == 128);
    }
    CHECK(g_e_live == 0);   // nothing leaked
}

struct Handle {   // the engines' layout: the stream first, so it is destroyed last
    hz::Stream stream;
    hz::Event up_ev;
    hz::ProfEvents ev;
    int device = 3;
};

int g_last_device = -1;

void handle_cases() {
    const int d0 = g_s_destroyed;
    {
        Handle* h = new Handle();
        CHECK(hz::check_handle(h, "hz_test") == HZ_OK && g_last_device == 3);
        CHECK(h->stream.create() == HZ_OK && h->up_ev.create(hipEventDisableTiming) == HZ_OK);
        hipEvent_t* e = nullptr;
        CHECK(h->ev.take(5, &e) == HZ_OK);
        delete h;
    }
    CHECK(g_s_destroyed == d0 + 1 && g_e_live == 0 && g_s_live == 0);
    const int e0 = g_errors_set;
    CHECK(hz::check_handle(static_cast<Handle*>(nullptr), "hz_test") == HZ_E_INVALID && g_errors_set == e0 + 1);
}

}  // namespace

extern "C" {
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    g_last_stream_flags = flags;
    if (g_fail_next_create) {
        g_fail_next_create = false;
        return hipErrorOutOfMemory;
    }
    *s = static_cast<hipStream_t>(std::malloc(1));
    ++g_s_created, ++g_s_live;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    CHECK(s != nullptr);   // the null stream is never destroyed
    ++g_s_destroyed, --g_s_live;
    g_last_destroyed = s;
    std::free(s);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    ++g_s_synced;
    g_last_synced = s;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    g_last_event_flags = flags;
    if (g_fail_next_create) {
        g_fail_next_create = false;
        return hipErrorOutOfMemory;
    }
    *e = static_cast<hipEvent_t>(std::calloc(1, 1));
    ++g_e_created, ++g_e_live;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    CHECK(e != nullptr);
    ++g_e_destroyed, --g_e_live;
    std::free(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
    *reinterpret_cast<volatile char*>(e) = 1;
    ++g_e_recorded;
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    CHECK(*reinterpret_cast<volatile char*>(a) == 1 && *reinterpret_cast<volatile char*>(b) == 1);   // both recorded
    ++g_e_timed;
    *ms = 1.0f;
    return hipSuccess;
}
hipError_t hipSetDevice(int d) {
    g_last_device = d;
    return hipSuccess;
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
    stream_lifetime();
    rebind_cases(hz::NullMeans::Private);
    rebind_cases(hz::NullMeans::Legacy);
    failed_create();
    move_cases();
    for (int k : {2, 3, 5}) take_cases(k);
    failed_growth();
    handle_cases();
    CHECK(g_s_live == 0 && g_e_live == 0);   // every destructor ran by here
    CHECK(g_s_created == g_s_destroyed && g_e_created == g_e_destroyed);
    if (g_failed) return 1;
    std::printf("stream ok: %d streams, %d events, live %d\n", g_s_created, g_e_created, g_s_live + g_e_live);
    return 0;
}
