// tests/filterbanks.cpp:191-211's multi-channel loop one callback block at a time: the frames of the
// audio callback's interleaved float buffers go through soundmath::process_many_frames (one
// hz_fb_process_many call per block, the channels' launches in one sequence), and the same program
// runs per sample through soundmath::sample_many on a second set of banks.
// argv: <dir> -- reads coef.bin ([864] x {3 forward, 2 back}) and x.bin ([T][8]), writes
// y_block.bin ([T][8], the float outputs as doubles) and y_sample.bin ([T][8]).
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/filterbank.h"

constexpr int CHANELS = 8, N = 864, BSIZE = 512;
constexpr int INPUT_OFFSET = 2, OUTPUT_OFFSET = 1;   // device channels ahead of ours in a frame
constexpr float GAP = -77.25f;

using Bank = soundmath::FFilterbank<double, N, 2>;

static std::vector<double> slurp(const std::string& path) {
    std::vector<double> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    double d;
    while (std::fread(&d, sizeof d, 1, f) == 1) v.push_back(d);
    std::fclose(f);
    return v;
}

static void dump(const std::string& path, const std::vector<double>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    std::fwrite(v.data(), sizeof(double), v.size(), f);
    std::fclose(f);
}

static void build(Bank** Fs, const std::vector<double>& coef) {
    for (int j = 0; j < CHANELS; ++j) {
        Fs[j] = new Bank();
        for (int n = 0; n < N; ++n)
            Fs[j]->coefficients(n, {coef[5 * n], coef[5 * n + 1], coef[5 * n + 2]}, {coef[5 * n + 3], coef[5 * n + 4]});
        Fs[j]->boost(std::vector<double>(N, 1.0 + 0.1 * j));
        Fs[j]->open();
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::vector<double> coef = slurp(dir + "/coef.bin"), x = slurp(dir + "/x.bin");
    if (coef.size() != 5 * N || x.size() % CHANELS) return 3;
    const int T = (int)(x.size() / CHANELS);
    const int in_frame = CHANELS + INPUT_OFFSET, out_frame = CHANELS + OUTPUT_OFFSET;
    std::vector<float> in((size_t)T * in_frame, GAP), out((size_t)T * out_frame, GAP);
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < CHANELS; ++j) in[(size_t)in_frame * i + INPUT_OFFSET + j] = (float)x[(size_t)i * CHANELS + j];

    Bank *Fb[CHANELS], *Fs[CHANELS];
    build(Fb, coef);
    build(Fs, coef);
    // the callback, BSIZE frames at a time (the last block ragged)
    for (int i0 = 0; i0 < T; i0 += BSIZE) {
        const int len = T - i0 < BSIZE ? T - i0 : BSIZE;
        soundmath::process_many_frames(Fb, CHANELS, &in[(size_t)in_frame * i0], in_frame, INPUT_OFFSET,
                                       &out[(size_t)out_frame * i0], out_frame, OUTPUT_OFFSET, (size_t)len,
                                       HZ_DIST_SOFTCLIP);
    }
    // the same frames per sample
    std::vector<double> yb((size_t)T * CHANELS), ys((size_t)T * CHANELS);
    for (int i = 0; i < T; ++i) {
        double xs[CHANELS];
        for (int j = 0; j < CHANELS; ++j) xs[j] = in[(size_t)in_frame * i + INPUT_OFFSET + j];
        soundmath::sample_many(Fs, CHANELS, xs, &ys[(size_t)i * CHANELS], HZ_DIST_SOFTCLIP);
        for (int j = 0; j < CHANELS; ++j) Fs[j]->tick();
    }
    for (int i = 0; i < T; ++i) {
        for (int j = 0; j < OUTPUT_OFFSET; ++j)
            if (out[(size_t)out_frame * i + j] != GAP) return 4;   // the other device channels stay untouched
        for (int j = 0; j < CHANELS; ++j) yb[(size_t)i * CHANELS + j] = out[(size_t)out_frame * i + OUTPUT_OFFSET + j];
    }
    dump(dir + "/y_block.bin", yb);
    dump(dir + "/y_sample.bin", ys);
    for (int j = 0; j < CHANELS; ++j) {
        delete Fb[j];
        delete Fs[j];
    }
    std::printf("multichannel block ok\n");
    return 0;
}
