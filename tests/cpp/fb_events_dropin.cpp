// The MIDI instrument of the reference's tests/filterbank.cpp (process_midi, 217-252) as events of
// block calls: Filterbank<double>(2, 36) and FFilterbank<double, 36, 2> -- 9 keys x 4 courses --
// play a short score of note-ons and note-offs through process(in, out, n, ev, nev), block by
// block as the audio callback would.  Dumps the input, the events (at counted from the score's
// start) and both outputs; tests/test_cpp_fb_events_gpu.py replays them through the oracle.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/filterbank.h"

using namespace soundmath;

namespace {

constexpr int kKeys = 9, kCourses = 4, kBands = kKeys * kCourses, kBlock = 1024, kBlocks = 6;
constexpr double kPi = 3.14159265359;

struct Note {
    long at;
    int key;
    int velocity;   // 0: note-off
};

void dump(const std::string& dir, const char* name, const std::vector<double>& v) {
    std::FILE* f = std::fopen((dir + "/" + name + ".bin").c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
}

template <class Bank>
std::vector<double> play(Bank& F, const std::vector<double>& x, const std::vector<Note>& score,
                         const std::vector<double>& gains, std::vector<double>* flat) {
    for (int i = 0; i < kBands; ++i) {
        const double g = 0.01 * (i % 7 + 1), R = 0.995, th = 2 * kPi * (i + 1) / 90.0;
        F.coefficients(i, {g, 0, -g}, {-2 * R * std::cos(th), R * R});
    }
    std::vector<double> y(x.size());
    size_t next = 0;
    for (int b = 0; b < kBlocks; ++b) {
        const long t0 = (long)b * kBlock;
        std::vector<hz_fb_event> ev;   // what process_midi would have queued during this block
        for (; next < score.size() && score[next].at < t0 + kBlock; ++next) {
            const Note& m = score[next];
            const long at = m.at - t0;
            for (int j = 0; j < kCourses; ++j) {
                const int band = kCourses * m.key + j;
                ev.push_back({at, band, HZ_FB_EV_BOOST, m.velocity ? 1.0 : 0.0});
                ev.push_back({at, band, HZ_FB_EV_MIX, m.velocity ? gains[band] : 0.0});
            }
        }
        F.process(x.data() + t0, y.data() + t0, kBlock, ev.data(), (int)ev.size(), HZ_DIST_SOFTCLIP);
        if (flat)
            for (const hz_fb_event& e : ev) {
                const double row[4] = {(double)(e.at + t0), (double)e.band, (double)e.kind, e.value};
                flat->insert(flat->end(), row, row + 4);
            }
    }
    return y;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const long n = (long)kBlock * kBlocks;
    std::vector<double> x(n), gains(kBands);
    for (long t = 0; t < n; ++t) x[t] = 0.4 * std::sin(0.01 * t) + 0.2 * (double)(((t * 7919) % 13) - 6) / 6.0;
    for (int i = 0; i < kBands; ++i) gains[i] = 0.5 + 0.05 * (i % 9);
    // chords, a note-off in the block of its note-on, notes on block boundaries and one sample off them
    const std::vector<Note> score = {{0, 2, 100},    {37, 5, 90},    {37, 7, 64},   {700, 2, 0},   {1023, 0, 80},
                                     {1024, 8, 127}, {1025, 5, 0},   {2500, 7, 0},  {2501, 3, 70}, {3000, 0, 0},
                                     {4095, 8, 0},   {4096, 4, 110}, {5000, 3, 0},  {6143, 4, 0}};
    std::vector<double> flat;
    Filterbank<double> F(2, kBands, 0.05, 0.3);
    const std::vector<double> y1 = play(F, x, score, gains, &flat);
    FFilterbank<double, kBands, 2> FF(0.05, 0.3);
    const std::vector<double> y2 = play(FF, x, score, gains, nullptr);
    dump(dir, "fbev_x", x);
    dump(dir, "fbev_events", flat);
    dump(dir, "fbev_y", y1);
    dump(dir, "fbev_yf", y2);
    std::printf("fb_events_dropin ok: %zu events\n", flat.size() / 4);
    return 0;
}
