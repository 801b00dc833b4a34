// hz::mix_plan_batch (huygens_amd/csrc/hz_mixplan.h), the segment plan of one hz_fb_process_many
// launch sequence, on the host: a batch's plan is the plan of its total group count, its segments
// cover n with none empty, and every member's buffers -- a slab of groups[j] rows of n_pad, segment
// start states [N_j][nseg][O] -- hold every element the kernels address (the writes are made here,
// element by element, into vectors of exactly the size the launch reserves: a sanitized build
// sees any index past them).
#include <cstdio>
#include <vector>

#include "../../huygens_amd/csrc/hz_mixplan.h"

constexpr int kTile = 1024;

static int fail(const char* what, int a, long b) {
    std::printf("FAIL %s (%d, %ld)\n", what, a, b);
    return 1;
}

// one batch: members of N[j] bands at `waves` waves, one band per wave
static int check_batch(const std::vector<int>& N, int waves, long n, int target, long want_nseg) {
    const int cnt = (int)N.size(), O = 2;
    std::vector<int> groups(cnt);
    long total = 0;
    for (int j = 0; j < cnt; ++j) total += groups[j] = (N[j] + waves - 1) / waves;
    const hz::MixPlan mp = hz::mix_plan_batch(groups.data(), cnt, n, kTile, target);
    const hz::MixPlan whole = hz::mix_plan(total, n, kTile, target);
    if (mp.nseg != whole.nseg || mp.seg_tiles != whole.seg_tiles || mp.n_pad != whole.n_pad) return fail("total", cnt, n);
    if (want_nseg && mp.nseg != want_nseg) return fail("nseg", (int)mp.nseg, want_nseg);
    if (mp.n_pad < n || mp.n_pad % kTile || mp.seg_len != mp.seg_tiles * kTile) return fail("n_pad", cnt, mp.n_pad);
    if (mp.nseg * mp.seg_len < n || (mp.nseg - 1) * mp.seg_len >= n) return fail("cover", (int)mp.nseg, mp.seg_len);
    for (int j = 0; j < cnt; ++j) {
        std::vector<char> slab((size_t)groups[j] * mp.n_pad, 0), seg((size_t)N[j] * mp.nseg * O, 0);
        for (long s = 0; s < mp.nseg; ++s) {   // the mix kernel's stores of segment s, workgroup g
            const long t0 = s * mp.seg_len, t1 = std::min(t0 + mp.seg_len, n);
            for (int g = 0; g < groups[j]; ++g)
                for (long t = t0; t < t1; ++t) slab[(size_t)g * mp.n_pad + t] += 1;
            if (s + 1 < mp.nseg)   // the pre-pass: end state of segment s -> slot s + 1
                for (int b = 0; b < N[j]; ++b)
                    for (int k = 0; k < O; ++k) seg[((size_t)b * mp.nseg + s + 1) * O + k] += 1;
        }
        for (int g = 0; g < groups[j]; ++g)   // every sample of every row written once
            for (long t = 0; t < n; ++t)
                if (slab[(size_t)g * mp.n_pad + t] != 1) return fail("slab", j, t);
    }
    return 0;
}

int main() {
    int bad = 0, plans = 0;
    // the program's shape, 8 x 864 bands at 16 waves on 256 CUs: 432 groups need no segments where
    // a member's 54 groups alone are cut in 4 at 4096 samples
    bad += check_batch(std::vector<int>(8, 864), 16, 4096, 256, 1), ++plans;
    if (hz::mix_plan(54, 4096, kTile, 256).nseg != 4) bad += fail("alone", 54, 4096);
    bad += check_batch(std::vector<int>(8, 864), 16, 1024, 256, 1), ++plans;
    bad += check_batch(std::vector<int>(8, 864), 16, 48000, 256, 1), ++plans;
    // two 7-band members at 4 waves, 4096 groups wanted: one segment per tile
    bad += check_batch({7, 7}, 4, 9000, 4096, 9), ++plans;
    bad += check_batch({37, 5, 130}, 8, 1500, 1, 1), ++plans;
    // a grid: ragged lengths, members of unequal size, targets below and above the group count
    const long lens[] = {1, 15, 1023, 1024, 1025, 2500, 9000};
    const int targets[] = {1, 64, 256, 4096};
    const int waves[] = {4, 8, 16};
    const std::vector<int> shapes[] = {{37, 5, 130}, {1, 1}, {864, 7, 200, 300}, {5, 5, 5, 5, 5, 5, 5}};
    for (long n : lens)
        for (int t : targets)
            for (int w : waves)
                for (const auto& s : shapes) bad += check_batch(s, w, n, t, 0), ++plans;
    if (bad) return 1;
    std::printf("many plan ok: %d plans\n", plans);
    return 0;
}
