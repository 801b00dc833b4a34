// hz_stream.h -- move-only owners of what a handle holds besides memory (hz_buf.h): its HIP stream
// (hz::Stream), a single ordering event (hz::Event) and the growing pool of profile timing events
// (hz::ProfEvents); and hz::check_handle, the null test + hipSetDevice every entry point starts
// with.  Deleting a handle destroys them.  Self-contained host code: a plain C++ compiler can
// include it (tests/cpp/stream_host.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

#include "../../include/huygens_hip.h"

namespace hz {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

inline int hip_status(hipError_t e, const char* call) {
    if (e == hipSuccess) return HZ_OK;
    set_error("%s failed: %s", call, hipGetErrorString(e));
    return HZ_E_HIP;
}

// Timing events of the profile counters: no system-scope fence on record, so a record between
// two kernels does not write back / invalidate L2 (it cost 5-10 us per record on the C2 step).
// Only hipEventElapsedTime after a stream synchronize reads them.
inline hipError_t prof_event_create(hipEvent_t* e) {
    return hipEventCreateWithFlags(e, hipEventDisableSystemFence);
}

// what hz_*_set_stream(h, NULL) binds: a new private non-blocking stream, or the null (legacy)
// stream itself -- torch's default stream is handle 0.  Each engine's choice: huygens_hip.h.
enum class NullMeans { Private, Legacy };

// the stream and whether the handle created it travel together; only an owned stream is destroyed
class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(o.s_), own_(o.own_) { o.s_ = nullptr, o.own_ = false; }
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            release();
            s_ = o.s_, own_ = o.own_;
            o.s_ = nullptr, o.own_ = false;
        }
        return *this;
    }
    ~Stream() { release(); }

    operator hipStream_t() const { return s_; }
    bool owned() const { return own_; }

    int create() {   // a private non-blocking stream
        release();
        if (hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)) {
            s_ = nullptr;
            return hip_status(e, "hipStreamCreateWithFlags");
        }
        own_ = true;
        return HZ_OK;
    }
    int sync() const { return hip_status(hipStreamSynchronize(s_), "hipStreamSynchronize"); }
    // waits for the work queued on the old stream, lets go of it, binds s.  A failure leaves the
    // null stream, unowned.
    int rebind(void* s, NullMeans null_means) {
        if (int r = sync()) return r;
        release();
        if (!s && null_means == NullMeans::Private) return create();
        s_ = static_cast<hipStream_t>(s);
        return HZ_OK;
    }

private:
    void release() {
        if (own_) (void)hipStreamDestroy(s_);
        s_ = nullptr, own_ = false;
    }

    hipStream_t s_ = nullptr;
    bool own_ = false;
};

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            release();
            e_ = o.e_, o.e_ = nullptr;
        }
        return *this;
    }
    ~Event() { release(); }

    operator hipEvent_t() const { return e_; }
    int create(unsigned flags) {
        release();
        return hip_status(hipEventCreateWithFlags(&e_, flags), "hipEventCreateWithFlags");
    }

private:
    void release() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

    hipEvent_t e_ = nullptr;
};

// The profile counters' events: each timed launch take()s a group of k consecutive events and
// records them; profile_read sums the time between two of each group's events.
class ProfEvents {
public:
    ProfEvents() = default;
    ProfEvents(ProfEvents&& o) noexcept : ev_(std::move(o.ev_)), used_(o.used_) { o.ev_.clear(), o.used_ = 0; }
    ProfEvents& operator=(ProfEvents&& o) noexcept {
        if (this != &o) {
            release();
            ev_ = std::move(o.ev_), used_ = o.used_;
            o.ev_.clear(), o.used_ = 0;
        }
        return *this;
    }
    ~ProfEvents() { release(); }

    // *e: k events, valid until the next take()
    int take(int k, hipEvent_t** e) {
        if (used_ + k > ev_.size()) {
            ev_.reserve(ev_.size() + 64);
            for (int q = 0; q < 64; ++q) {
                hipEvent_t ne;
                if (int r = hip_status(prof_event_create(&ne), "hipEventCreateWithFlags")) return r;
                ev_.push_back(ne);
            }
        }
        *e = &ev_[used_];
        used_ += k;
        return HZ_OK;
    }
    size_t used() const { return used_; }
    void rewind() { used_ = 0; }   // the events stay, for the next take()
    hipEvent_t operator[](size_t i) const { return ev_[i]; }
    size_t index_of(const hipEvent_t* e) const { return (size_t)(e - ev_.data()); }   // of a take()n event

    // adds to *ms_accum the time from event a to event b of every complete group taken
    int elapsed(size_t group, int a, int b, double* ms_accum) const {
        for (size_t i = 0; i + group <= used_; i += group) {
            float x = 0;
            if (int r = hip_status(hipEventElapsedTime(&x, ev_[i + a], ev_[i + b]), "hipEventElapsedTime")) return r;
            *ms_accum += x;
        }
        return HZ_OK;
    }

private:
    void release() {
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
        ev_.clear(), used_ = 0;
    }

    std::vector<hipEvent_t> ev_;
    size_t used_ = 0;
};

// the first line of every entry point: name is the handle's type ("hz_osc")
template <class H>
int check_handle(H* h, const char* name) {
    if (!h) {
        set_error("null %s handle", name);
        return HZ_E_INVALID;
    }
    return hip_status(hipSetDevice(h->device), "hipSetDevice");
}

}  // namespace hz
