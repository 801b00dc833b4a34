// hz_mixplan.h -- the time-segment plan of every "partials x time -> mixdown" launch (host-only;
// the device half is hz_mix.h).  A bank with `groups` workgroups of partials covers n samples in
// tiles; when the groups alone do not reach target_groups workgroups, time is cut into nseg
// segments of seg_tiles whole tiles (blockIdx.y), none of them empty.  A plain C++ compiler can
// include it (tests/cpp/mix_host.cpp).
#pragma once

#include <algorithm>

namespace hz {

struct MixPlan {
    long ntiles;     // ceil(n / tile)
    long nseg;       // time segments (grid.y)
    long seg_tiles;  // tiles per segment (the last segment may hold fewer)
    long n_pad;      // ntiles * tile: the row stride of the groups' slab
    long seg_len;    // seg_tiles * tile
};

inline MixPlan mix_plan(long groups, long n, int tile, int target_groups) {
    MixPlan p;
    p.ntiles = (n + tile - 1) / tile;
    p.nseg = std::max<long>(1, std::min<long>(p.ntiles, (target_groups + groups - 1) / groups));
    p.seg_tiles = (p.ntiles + p.nseg - 1) / p.nseg;
    p.nseg = (p.ntiles + p.seg_tiles - 1) / p.seg_tiles;   // drops segments the rounding left empty
    p.n_pad = p.ntiles * tile;
    p.seg_len = p.seg_tiles * tile;
    return p;
}

// One launch over several banks side by side (hz_fb_process_many): the members bring their own
// groups of partials and share n, so the plan is the one of their total group count -- a batch
// that covers the chip with groups runs unsegmented where its members alone would not.  Every
// member's slab is groups[j] rows of n_pad.
inline MixPlan mix_plan_batch(const int* groups, int count, long n, int tile, int target_groups) {
    long total = 0;
    for (int j = 0; j < count; ++j) total += groups[j];
    return mix_plan(std::max<long>(1, total), n, tile, target_groups);
}

}  // namespace hz
