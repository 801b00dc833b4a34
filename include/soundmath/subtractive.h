// soundmath/subtractive.h -- drop-in Subtractive<T, N> (src/subtractive.h:15-101, the MIMO variant
// the reference compiles) with the Minimizer note API and physics() (src/minimizer.h:61-187) over
// the HIP engine.  T = double.
// The reference's loop
//   out = sub(in); if (metro()) sub.physics(); sub.tick();
// runs as written after one added line, enable_physics(law), before the first physics(): law is
// HZ_GRAV_TRUNC (the reference as g++ / libstdc++ compile it) or HZ_GRAV_FABS (its text with
// std::abs(double)); see huygens_hip.h.  operator() renders the current sample without advancing,
// tick() advances with the sample operator() was last given; each is one device call, so this is
// the compatibility path.  The block path is physics_every(period, law) + process(in, out, n):
// in and out are [N][n], channel-major, and a step runs at every period-th sample on the device.
// tick() needs an operator() since the previous tick(): the reference's bare tick() moves the ring
// past a slot it never wrote, which the engine's register form of the ring does not keep.
#pragma once

#include <array>

#include "hz.h"

namespace soundmath {

template <typename T, std::size_t N>
class Subtractive {
    static_assert(std::is_same<T, double>::value, "the HIP Subtractive computes in double");

public:
    using TN = std::array<T, N>;

    Subtractive(uint voices, uint overtones, T decay, T resonance = 0.99999, T harmonicity = 1.0, T k = 0.1,
                int device = 0) {
        hz_sub* h = nullptr;
        detail::check(hz_sub_create((int)voices, (int)overtones, (int)N, decay, resonance, harmonicity, k, device, &h),
                      "Subtractive");
        h_ = decltype(h_)(h);
    }
    TN operator()(const TN& sample) {
        TN out{};
        detail::check(hz_sub_peek(h_.get(), sample.data(), out.data()), "Subtractive::operator()");
        pending_ = sample;
        computed_ = true;
        return out;
    }
    void tick() {
        if (!computed_) throw std::logic_error("Subtractive::tick: no operator() since the previous tick()");
        TN out{};
        detail::check(hz_sub_process(h_.get(), pending_.data(), out.data(), 1), "Subtractive::tick");
        computed_ = false;
    }
    // law: HZ_GRAV_TRUNC or HZ_GRAV_FABS
    void enable_physics(int law) {
        if (law != HZ_GRAV_TRUNC && law != HZ_GRAV_FABS)
            throw std::invalid_argument("Subtractive::enable_physics: law is HZ_GRAV_TRUNC or HZ_GRAV_FABS");
        law_ = law;
    }
    void physics() {
        if (!law_) throw std::logic_error("Subtractive::physics: call enable_physics(law) first");
        detail::check(hz_sub_physics(h_.get(), law_), "Subtractive::physics");
    }
    // block path: process() runs physics() at every sample T >= period with T % period == 0; 0 switches it off
    void physics_every(uint period, int law) {
        detail::check(hz_sub_physics_every(h_.get(), (int)period, law), "Subtractive::physics_every");
    }
    // n x { out[:, t] = operator()(in[:, t]); physics() when due; tick(); }, in / out [N][n]
    void process(const T* in, T* out, std::size_t n) {
        detail::check(hz_sub_process(h_.get(), in, out, n), "Subtractive::process");
        computed_ = false;
    }
    int request(T fundamental, T amplitude) {
        int v = -1;
        detail::check(hz_sub_request(h_.get(), fundamental, amplitude, &v), "Subtractive::request");
        return v;
    }
    void release(int voice) { detail::check(hz_sub_release(h_.get(), voice), "Subtractive::release"); }
    int makenote(T pitch, T amplitude) {
        int v = -1;
        detail::check(hz_sub_makenote(h_.get(), pitch, amplitude, &v), "Subtractive::makenote");
        return v;
    }
    void endnote(T pitch) { detail::check(hz_sub_endnote(h_.get(), pitch), "Subtractive::endnote"); }
    hz_sub* native() const { return h_.get(); }

private:
    handle<hz_sub, hz_sub_destroy> h_;
    TN pending_{};
    bool computed_ = false;
    int law_ = 0;
};

}  // namespace soundmath
