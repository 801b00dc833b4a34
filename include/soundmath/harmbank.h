// soundmath/harmbank.h -- the heterodyne bank chain of tests/harmbank.cpp:77-101 as one
// fused drop-in over the HIP engine.
//
// The reference composes seven banks per sample in user code:
//     limiter(dry * in + gain * mixdown(demodulators(synthesis(), smoothbank(latchbank(&rmsbank,
//         slidebank(modulators(in, analysis())))))));
//     analysis.tick(); synthesis.tick(); slidebank.tick(); smoothbank.tick(); rmsbank.tick();
// with Oscbank (src/oscbank.h), Modbank (modbank.h), Slidebank (slidebank.h), Latchbank
// (latchbank.h), RMSbank (rmsbank.h), Stickbank (stickbank.h) and Mixer (mixer.h).  On the
// GPU the N-wide intermediate signals never leave registers, so the chain is one object:
// Heterodyne<N>(slide order, radii, Latchbank thresh/ratio, RMSbank width, Stickbank order/rad,
// dry, gain).  analysis() / synthesis() return the two Oscbanks' controls (freqmod, activate,
// deactivate, open, close); setup() is Slidebank::setup.  process() runs n iterations of the
// loop body above; operator()(in) is one.
//
// The same banks compose three more programs in the reference:
//   Heterodyne<N>(..., chain = HZ_HET_CHAIN_PHASE)   tests/phasebank.cpp:77-101, the phase
//       vocoder: phase_combiners(absbank(latchbank(..)), smoothbank(argbank(latchbank(..))))
//   set_output(HZ_HET_OUT_LIMITER, 4, 0.9)           tests/slidebank.cpp:95's tail,
//       limiter(dry * in + gain * softclip(drive * mixdown(...), 0.9))
//   StickChain<N>(pre, post, rad, gate)              tests/oscbank.cpp:106-110: dry * in +
//       mixdown(modbank2(oscbank2(), stickbank4(distbank(stickbank3(stickbank2(stickbank(
//       modbank1(in, oscbank1()))))))))
#pragma once

#include <complex>
#include <vector>

#include "hz.h"

namespace soundmath {

// the Oscbank controls of one bank (oscbank.h:49-56, multichannel.h:90-130)
class HetBank {
public:
    HetBank(hz_het* h, int b) : h_(h), b_(b) {}
    void freqmod(int index, double target) { detail::check(hz_het_freqmod(h_, b_, &index, &target, 1), "freqmod"); }
    void activate(const std::vector<int>& indices) {
        detail::check(hz_het_activate(h_, b_, indices.data(), (int)indices.size(), 1), "activate");
    }
    void deactivate(const std::vector<int>& indices) {
        detail::check(hz_het_activate(h_, b_, indices.data(), (int)indices.size(), 0), "deactivate");
    }
    void open() { detail::check(hz_het_open(h_, b_, 1), "open"); }
    void close() { detail::check(hz_het_open(h_, b_, 0), "close"); }

private:
    hz_het* h_;
    int b_;
};

// what every chain's object does with its handle: the two Oscbanks, the output stage, the loop
class HetChain {
public:
    using Bank = HetBank;
    Bank analysis() { return Bank(h_.get(), HZ_HET_ANALYSIS); }
    Bank synthesis() { return Bank(h_.get(), HZ_HET_SYNTHESIS); }

    // out = shaper(dry * in + gain * v); v = the mix, or softclip(drive * mix, clip_width)
    void set_output(int shaper, double drive = 0, double clip_width = 0) {
        detail::check(hz_het_set_output(h_.get(), shaper, drive, clip_width), "set_output");
    }

    double operator()(double in) {
        double y = 0;
        detail::check(hz_het_process(h_.get(), &in, &y, 1), "operator()");
        return y;
    }
    void process(const double* in, double* out, std::size_t n) {
        detail::check(hz_het_process(h_.get(), in, out, n), "process");
    }
    void process(const float* in, float* out, std::size_t n) {   // the Audio callback's float buffers
        std::vector<double> x(in, in + n), y(n);
        process(x.data(), y.data(), n);
        for (std::size_t i = 0; i < n; ++i) out[i] = (float)y[i];
    }
    hz_het* native() const { return h_.get(); }

protected:
    handle<hz_het, hz_het_destroy> h_;
};

template <int N>
class Heterodyne : public HetChain {
public:

    // defaults: tests/harmbank.cpp:47-52 (Latchbank(0.0005), RMSbank(SR / 20), Stickbank(1, -0.9)),
    // dry 0, gain 3 (harmbank.cpp:55-56); chain: HZ_HET_CHAIN_HARM or HZ_HET_CHAIN_PHASE
    Heterodyne(int order, const std::vector<std::complex<double>>& radii, double thresh = 0.0005, double ratio = 0.2,
               unsigned width = SR / 20, int stick_order = 1, double stick_rad = -0.9, double dry = 0,
               double gain = 3, int device = 0, int chain = HZ_HET_CHAIN_HARM) {
        hz_het* h = nullptr;
        const auto create = chain == HZ_HET_CHAIN_PHASE ? hz_het_create_phase : hz_het_create;
        detail::check(chain == HZ_HET_CHAIN_HARM || chain == HZ_HET_CHAIN_PHASE ? HZ_OK : HZ_E_INVALID,
                      "Heterodyne: chain");
        detail::check(create(N, order, reinterpret_cast<const double*>(radii.data()), thresh, ratio, width,
                             stick_order, stick_rad, dry, gain, device, &h),
                      "Heterodyne");
        h_ = decltype(h_)(h);
    }

    // Slidebank::setup (slidebank.h:63-100): new order and radii, zeroed stages
    void setup(int order, const std::vector<std::complex<double>>& radii) {
        detail::check(hz_het_setup(h_.get(), order, reinterpret_cast<const double*>(radii.data())), "setup");
    }
};

// tests/oscbank.cpp:64-72,106-110: `pre` Stickbank(1, rad), Distbank(&gate) (gate <= 0: none), `post`
// more; pre + post <= 4.  The program's scalar tail (Buffer under an LFO) stays with the caller.
template <int N>
class StickChain : public HetChain {
public:
    StickChain(int pre = 3, int post = 1, double rad = -0.999, double gate = 0.001, double dry = 0, double gain = 1,
               int device = 0) {
        hz_het* h = nullptr;
        detail::check(hz_het_create_sticks(N, pre, post, rad, gate, dry, gain, device, &h), "StickChain");
        h_ = decltype(h_)(h);
    }
};

}  // namespace soundmath
