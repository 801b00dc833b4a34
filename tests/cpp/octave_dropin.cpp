// octave_dropin.cpp -- long frames through the drop-in headers, in the shape of the reference's
// spectral programs: a Fourier with a host gate that keeps the bins above 10 x the squared mean
// magnitude, N = 16384 and 4 laps, driven with write() / read() per sample; and a Cosine of
// 32768 points, forward then backward on its own buffers.  The input is deterministic.  Writes
// the input and the outputs into argv[1]; tests/test_cpp_long_stft_gpu.py compares them with
// the numpy spec and scipy.
#include <cmath>
#include <complex>
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/fourier.h"

using namespace soundmath;

static const int kN = 16384, kLaps = 4, kSamples = 2 * kN + 40, kDct = 32768;

// zero every bin whose squared magnitude is below 10 x (mean magnitude)^2
static int host_gate10(const std::complex<double>* in, std::complex<double>* out) {
    long double sum = 0;
    for (int k = 0; k < kN; ++k) sum += std::hypot(in[k].real(), in[k].imag());
    const long double mean = sum / kN, floor2 = 10 * mean * mean;
    for (int k = 0; k < kN; ++k) {
        const long double n2 = (long double)(in[k].real() * in[k].real() + in[k].imag() * in[k].imag());
        out[k] = n2 < floor2 ? std::complex<double>(0, 0) : in[k];
    }
    return 0;
}

static double hiss(int t) { return ((t * 7919L + 13) % 1009) / 1009.0 - 0.5; }

static void dump(const std::string& dir, const char* name, const std::vector<double>& v) {
    FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
    std::fwrite(v.data(), sizeof(double), v.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const double pi = std::acos(-1.0);

    Fourier fourier(host_gate10, kN, kLaps);
    std::vector<double> x(kSamples), yr(kSamples), yi(kSamples);
    for (int t = 0; t < kSamples; ++t) {
        // a tone that steps from bin N/8 to bin 3N/8 half way, over a hiss floor
        const int bin = t < kSamples / 2 ? kN / 8 : 3 * kN / 8;
        x[t] = 0.5 * std::sin(2 * pi * ((long)bin * t % kN) / kN) + 1e-3 * hiss(t);
        fourier.write(x[t]);
        fourier.read(&yr[t], &yi[t]);
    }
    dump(dir, "octave_x", x);
    dump(dir, "octave_yr", yr);
    dump(dir, "octave_yi", yi);

    double *in = nullptr, *out = nullptr;
    Cosine cosine(kDct, &in, &out);
    std::vector<double> c(kDct), fwd(kDct), back(kDct);
    for (int k = 0; k < kDct; ++k) in[k] = c[k] = std::sin(0.001 * k) + hiss(k);
    cosine.forward();
    for (int k = 0; k < kDct; ++k) fwd[k] = out[k];
    cosine.backward();
    for (int k = 0; k < kDct; ++k) back[k] = in[k];
    dump(dir, "cosine_x", c);
    dump(dir, "cosine_fwd", fwd);
    dump(dir, "cosine_back", back);
    std::printf("octave_dropin ok\n");
    return 0;
}
