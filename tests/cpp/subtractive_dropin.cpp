// The reference programs' Subtractive loop (tests/subtractive.cpp, bop.cpp) over
// include/soundmath/subtractive.h: Subtractive<double, 2> sub(7, 7, 0.7, 0.999995, 1, 1), a physics
// step every 32 samples, 128-sample blocks, three notes of which one is released half way.
// Rendered once through process() and once through the per-sample operator() / physics() / tick().
//   subtractive_dropin DIR   reads DIR/sub_in.bin ([2][1024] doubles), writes DIR/sub_block.bin and
//                            DIR/sub_sample.bin ([2][1024] doubles each)
#include <cstdio>
#include <string>
#include <vector>

#include "soundmath/subtractive.h"

using namespace soundmath;

namespace {
constexpr std::size_t kN = 1024, kBlock = 128, kPeriod = 32, kRelease = 512;

void notes(Subtractive<double, 2>& sub) {
    sub.makenote(48, 1.0);
    sub.makenote(55.3, 0.6);
    sub.makenote(60.1, 0.8);
}

bool write(const std::string& path, const std::vector<double>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    std::vector<double> in(2 * kN), block(2 * kN), sample(2 * kN);
    FILE* f = std::fopen((dir + "/sub_in.bin").c_str(), "rb");
    if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 3;
    std::fclose(f);
    try {
        {   // block path
            Subtractive<double, 2> sub(7, 7, 0.7, 0.999995, 1, 1);
            sub.physics_every(kPeriod, HZ_GRAV_TRUNC);
            notes(sub);
            std::vector<double> bi(2 * kBlock), bo(2 * kBlock);
            for (std::size_t t0 = 0; t0 < kN; t0 += kBlock) {
                if (t0 == kRelease) sub.endnote(55.3);
                for (std::size_t k = 0; k < 2; ++k)
                    for (std::size_t j = 0; j < kBlock; ++j) bi[k * kBlock + j] = in[k * kN + t0 + j];
                sub.process(bi.data(), bo.data(), kBlock);
                for (std::size_t k = 0; k < 2; ++k)
                    for (std::size_t j = 0; j < kBlock; ++j) block[k * kN + t0 + j] = bo[k * kBlock + j];
            }
        }
        {   // the loop as the reference writes it
            Subtractive<double, 2> sub(7, 7, 0.7, 0.999995, 1, 1);
            sub.enable_physics(HZ_GRAV_TRUNC);
            notes(sub);
            for (std::size_t T = 0; T < kN; ++T) {
                if (T == kRelease) sub.endnote(55.3);
                const std::array<double, 2> out = sub({in[T], in[kN + T]});
                sample[T] = out[0];
                sample[kN + T] = out[1];
                if (T >= kPeriod && T % kPeriod == 0) sub.physics();
                sub.tick();
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "subtractive_dropin: %s\n", e.what());
        return 1;
    }
    if (!write(dir + "/sub_block.bin", block) || !write(dir + "/sub_sample.bin", sample)) return 4;
    std::puts("subtractive dropin ok");
    return 0;
}
