// ambi_dropin.cpp -- the reference's ambisonic demo (tests/ambi.cpp) over the drop-in headers: six
// sources circling two ears, one Delay<double>(1, SR) per source and ear, every line's single
// forward tap {sqrt(d2) / SPEED, DIFFUSION / d2} recomputed for every sample (the moving delay
// times are the Doppler).  The twelve lines are one Delaybank<double, 12>; the taps of a block go
// in as one stream through process_stream() instead of coefficients() before every sample.
// The LFO runs at an audible rate so the taps move within a short run, and the sources play a
// deterministic signal.  Writes the inputs, the tap stream it used and the outputs into argv[1];
// tests/test_cpp_delay_tv_gpu.py replays the dumped stream through the oracle.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/delay.h"

using namespace soundmath;

#define BSIZE 32
#define DISTANCE 10
#define RADIUS 5
#define DIFFUSION 1.0
#define SPEED 0.01

struct Point {
    double x, y, z;
};

static double sqdist(const Point& a, const Point& b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}

static double source(int i, int t) {
    const int u = t + 131 * i;
    return 0.5 * std::sin(0.02 * (i + 1) * t) + 0.25 * (((u * 7919) % 13) - 6) / 6.0;
}

template <typename T>
static void dump(const std::string& dir, const char* name, const std::vector<T>& v) {
    FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
    std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    constexpr int kLines = 12, kSamples = 2048;
    const double lfo_hz = 37.0;   // the reference's 0.1 Hz would not move a tap in 2048 samples

    Delaybank<double, kLines> bank(1, SR);   // lines 0-5: left ear, 6-11: right ear
    const Point ears[2] = {{1, 1, 1}, {-1, -1, -1}};
    Point positions[6];

    // whole-run arrays [line][sample] for the dump; the blocks below are cut out of them
    std::vector<double> x((size_t)kLines * kSamples), y((size_t)kLines * kSamples), fg((size_t)kLines * kSamples);
    std::vector<unsigned> ft((size_t)kLines * kSamples);
    std::vector<double> blk_x(kLines * BSIZE), blk_y(kLines * BSIZE), blk_g(kLines * BSIZE);
    std::vector<unsigned> blk_t(kLines * BSIZE);

    double phase = 0.0;
    for (int t0 = 0; t0 < kSamples; t0 += BSIZE) {
        for (int j = 0; j < BSIZE; j++) {
            const int t = t0 + j;
            const double a = 2 * PI * phase;
            positions[0] = {DISTANCE, RADIUS * std::cos(a), RADIUS * std::sin(a)};
            positions[1] = {-DISTANCE, RADIUS * std::cos(-a), RADIUS * std::sin(-a)};
            positions[2] = {RADIUS * std::sin(a), DISTANCE, RADIUS * std::cos(a)};
            positions[3] = {RADIUS * std::sin(-a), -DISTANCE, RADIUS * std::cos(-a)};
            positions[4] = {RADIUS * std::cos(a), RADIUS * std::sin(a), DISTANCE};
            positions[5] = {RADIUS * std::cos(-a), RADIUS * std::sin(-a), -DISTANCE};
            for (int i = 0; i < 6; i++)
                for (int ear = 0; ear < 2; ear++) {
                    const int line = 6 * ear + i;
                    const double distance = sqdist(ears[ear], positions[i]);
                    const std::pair<uint, double> tap(sqrt(distance) / SPEED, DIFFUSION / distance);
                    blk_t[line * BSIZE + j] = ft[(size_t)line * kSamples + t] = tap.first;
                    blk_g[line * BSIZE + j] = fg[(size_t)line * kSamples + t] = tap.second;
                    blk_x[line * BSIZE + j] = x[(size_t)line * kSamples + t] = source(i, t);
                }
            phase += lfo_hz / SR;
            phase -= (int)phase;
        }
        bank.process_stream(blk_x.data(), blk_y.data(), BSIZE, false, true, blk_t.data(), blk_g.data());
        for (int line = 0; line < kLines; line++)
            for (int j = 0; j < BSIZE; j++) y[(size_t)line * kSamples + t0 + j] = blk_y[line * BSIZE + j];
    }
    dump(dir, "ambi_x", x);
    dump(dir, "ambi_ft", ft);
    dump(dir, "ambi_fg", fg);
    dump(dir, "ambi_y", y);
    std::printf("ambi_dropin ok\n");
    return 0;
}
