// phasebank_dropin.cpp -- the reference's phase vocoder (tests/phasebank.cpp) over the drop-in
// header: 48 channels from mtof(28), transpose() / measure() with multiplicity 1, both Oscbanks
// open, Heterodyne<48>(..., HZ_HET_CHAIN_PHASE).  The same input runs once sample by sample
// through operator() and once in blocks of BSIZE through process().  Writes the configuration,
// the input and both outputs into argv[1]; tests/test_cpp_phasebank_gpu.py compares them with the
// restatement (tests/oracle_chains.py).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/harmbank.h"

using namespace soundmath;

#define BSIZE 32

// a quiet first block (the latches arm), then a tone inside the bank's two octaves (77 Hz) with a
// deterministic rattle on top
static double input(int t) {
    const double v = 0.4 * std::sin(0.0105 * t) + 0.2 * (((t * 7919) % 13) - 6) / 6.0;
    return t < BSIZE ? 1e-4 * v : v;
}

static void dump(const std::string& dir, const char* name, const std::vector<double>& v) {
    FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
    std::fwrite(v.data(), sizeof(double), v.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    constexpr int octaves = 2, division = 12, parities = 2, n = parities * division * octaves;
    constexpr int kBlocks = 12, kSamples = kBlocks * BSIZE;
    const int multiplicity = 1;
    const double frequency = mtof(28), detune = 0.125, wavelengths = 25, cutoff = 0.999, transp = 12;

    std::vector<std::complex<double>> radii(n);
    std::vector<double> fa(n), fs(n), rad(2 * n);
    for (int i = 0; i < division * octaves; i++)
        for (int l = 0; l < parities; l++) {
            const double midi = (i + detune * std::pow(2 * (0 + 0.5) / 1.0 - 1, 1)) / division;
            const double partial = frequency * std::pow(2, midi) * 1 * std::pow(-1, l);
            const int idx = parities * i + l;
            fa[idx] = partial;
            fs[idx] = -1 * partial * std::pow(2, transp / 12);
            radii[idx] = std::min(cutoff, std::exp((std::log(0.5) - multiplicity - 1) /
                                                   (wavelengths * SR / std::abs(partial))));
            rad[2 * idx] = radii[idx].real();
            rad[2 * idx + 1] = radii[idx].imag();
        }

    std::vector<double> x(kSamples), y_op(kSamples), y_blk(kSamples);
    for (int t = 0; t < kSamples; t++) x[t] = input(t);

    // Latchbank(0.0005), RMSbank(SR / 20), Stickbank(1, -0.9), dry 0, gain 3 (phasebank.cpp:56-69)
    Heterodyne<n> a(multiplicity, radii, 0.0005, 0.2, SR / 20, 1, -0.9, 0, 3, 0, HZ_HET_CHAIN_PHASE);
    Heterodyne<n> b(multiplicity, radii, 0.0005, 0.2, SR / 20, 1, -0.9, 0, 3, 0, HZ_HET_CHAIN_PHASE);
    for (Heterodyne<n>* h : {&a, &b}) {
        for (int i = 0; i < n; i++) {
            h->analysis().freqmod(i, fa[i]);
            h->synthesis().freqmod(i, fs[i]);
        }
        h->analysis().open();
        h->synthesis().open();
    }
    int chain = -1;
    if (hz_het_chain(a.native(), &chain) != HZ_OK || chain != HZ_HET_CHAIN_PHASE) return 3;

    for (int t = 0; t < kSamples; t++) y_op[t] = a(x[t]);
    for (int t0 = 0; t0 < kSamples; t0 += BSIZE) b.process(x.data() + t0, y_blk.data() + t0, BSIZE);

    // the +-partial pairs of this instrument cancel in the mix for a real input (conjugate
    // Slidebank outputs, opposite angles), so the smoothbank taps are dumped as well
    std::vector<double> stick(2 * n);
    if (hz_het_state(b.native(), HZ_HET_STATE_STICK, stick.data()) != HZ_OK) return 4;
    dump(dir, "phase_stick", stick);
    dump(dir, "phase_fa", fa);
    dump(dir, "phase_fs", fs);
    dump(dir, "phase_radii", rad);
    dump(dir, "phase_x", x);
    dump(dir, "phase_y_op", y_op);
    dump(dir, "phase_y_blk", y_blk);
    std::printf("phasebank_dropin ok\n");
    return 0;
}
