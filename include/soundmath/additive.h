// soundmath/additive.h -- drop-in Additive<T> (src/additive.h:11-71) with the Minimizer
// note API (src/minimizer.h:111-187) over the HIP engine.  T = double, form = &cycle.
// operator()() / tick() keep the reference's per-sample pair: operator() renders the
// current sample once (cached until tick()), tick() advances.
// physics() (Minimizer::physics(), src/minimizer.h:61-108: springs along each voice's overtone
// chain, gravity between partials of different voices) runs on the device after one added line,
// enable_physics(law), before the first operator(): the reference's loop
//   y = addi(); if (metro()) addi.physics(); addi.tick();
// is then exact.  law is HZ_GRAV_TRUNC (the reference as g++ / libstdc++ compile it) or HZ_GRAV_FABS
// (its text with std::abs(double)); see huygens_hip.h.  physics_every(period, law) is the block
// path: fill() then runs a step at every period-th sample on the device.
#pragma once

#include "hz.h"

namespace soundmath {

template <typename T>
class Additive {
    static_assert(std::is_same<T, double>::value, "the HIP Additive computes in double");

public:
    Additive(Wave<T>* form, uint voices, uint overtones, T decay, T harmonicity = 1.0, T k = 0.1, int device = 0) {
        if (!form || form->kind != Shape::cycle) throw std::runtime_error("Additive: only the cycle waveform runs on the device");
        hz_add* h = nullptr;
        detail::check(hz_add_create((int)voices, (int)overtones, decay, harmonicity, k, device, &h), "Additive");
        h_ = decltype(h_)(h);
    }
    T operator()() {
        if (law_) {   // physics may run between operator() and tick(): render without advancing
            T y;
            detail::check(hz_add_peek(h_.get(), &y), "Additive::operator()");
            return y;
        }
        if (!computed_) {
            detail::check(hz_add_fill(h_.get(), &last_, 1), "Additive::operator()");
            computed_ = true;
        }
        return last_;
    }
    void tick() {
        if (law_ || !computed_) {
            T y;
            detail::check(hz_add_fill(h_.get(), &y, 1), "Additive::tick");
        }
        computed_ = false;
    }
    // call before the first operator(); law: HZ_GRAV_TRUNC or HZ_GRAV_FABS
    void enable_physics(int law) {
        if (law != HZ_GRAV_TRUNC && law != HZ_GRAV_FABS) throw std::invalid_argument("Additive::enable_physics: law is HZ_GRAV_TRUNC or HZ_GRAV_FABS");
        if (computed_) throw std::logic_error("Additive::enable_physics: call it before the first operator()");
        law_ = law;
    }
    void physics() {
        if (!law_) throw std::logic_error("Additive::physics: call enable_physics(law) first");
        detail::check(hz_add_physics(h_.get(), law_), "Additive::physics");
    }
    // block path: fill() runs physics() at every sample T >= period with T % period == 0; 0 switches it off
    void physics_every(uint period, int law) {
        detail::check(hz_add_physics_every(h_.get(), (int)period, law), "Additive::physics_every");
    }
    int request(T fundamental, T amplitude) {
        int v = -1;
        detail::check(hz_add_request(h_.get(), fundamental, amplitude, &v), "Additive::request");
        return v;
    }
    void release(int voice) { detail::check(hz_add_release(h_.get(), voice), "Additive::release"); }
    int makenote(T pitch, T amplitude) {
        int v = -1;
        detail::check(hz_add_makenote(h_.get(), pitch, amplitude, &v), "Additive::makenote");
        return v;
    }
    void endnote(T pitch) { detail::check(hz_add_endnote(h_.get(), pitch), "Additive::endnote"); }
    // n x { out[t] = operator()(); tick(); }
    void fill(T* out, std::size_t n) { detail::check(hz_add_fill(h_.get(), out, n), "Additive::fill"); }
    hz_add* native() const { return h_.get(); }

private:
    handle<hz_add, hz_add_destroy> h_;
    bool computed_ = false;
    T last_ = 0;
    int law_ = 0;   // nonzero after enable_physics
};

}  // namespace soundmath
