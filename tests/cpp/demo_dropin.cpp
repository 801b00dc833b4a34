// demo_dropin.cpp -- the reference's tests/demo.cpp audio callback over the drop-in header: a
// Fourier of 32768 points and 2 laps whose processor is the pitch transposer, fed one sample at a
// time from an interleaved stereo float buffer with write() and read back with read().  The one
// change against the program is the constructor: the transposer is the built-in device processor
// (HZ_PROC_TRANSPOSE with the program's transp = 2), not a host callback.  The input is
// deterministic.  Writes the input and both output parts into argv[1];
// tests/test_cpp_transpose_gpu.py compares them with the numpy spec.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/fourier.h"

using namespace soundmath;

#define BSIZE 256
#define N 32768
#define LAPS 2

static const int kSamples = 3 * N + 5;
static double transp = 2;

static Fourier* F1 = nullptr;
static std::vector<double> g_x, g_yr, g_yi;

// one audio block: left input channel in, the real part out on both channels
static int process(const float* in, float* out, int frames) {
    for (int i = 0; i < frames; i++) {
        F1->write(in[2 * i]);

        double real, imag;
        F1->read(&real, &imag);
        out[2 * i] = out[2 * i + 1] = (float)real;

        g_x.push_back(in[2 * i]);
        g_yr.push_back(real);
        g_yi.push_back(imag);
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

    Fourier fourier(HZ_PROC_TRANSPOSE, N, LAPS, transp, 0);
    F1 = &fourier;

    std::vector<float> in(2 * BSIZE), out(2 * BSIZE);
    for (int t0 = 0; t0 < kSamples; t0 += BSIZE) {
        const int frames = kSamples - t0 < BSIZE ? kSamples - t0 : BSIZE;
        for (int i = 0; i < frames; ++i) {
            // two tones (bins 300 and 1001.5 of the frame) over a hiss floor; the right channel is unused
            const int t = t0 + i;
            const double v = 0.4 * std::sin(2 * pi * ((300L * t) % N) / N) +
                             0.3 * std::sin(2 * pi * ((2003L * t) % (2 * N)) / (2.0 * N)) + 0.05 * hiss(t);
            in[2 * i] = (float)v;
            in[2 * i + 1] = 0.0f;
        }
        process(in.data(), out.data(), frames);
    }
    dump(dir, "demo_x", g_x);
    dump(dir, "demo_yr", g_yr);
    dump(dir, "demo_yi", g_yi);
    std::printf("demo_dropin ok\n");
    return 0;
}
