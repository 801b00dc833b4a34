// hz_transpose.h -- source runs of the spectral transposer (HZ_PROC_TRANSPOSE), host and device.
//
// The reference's processor (tests/demo.cpp:49-81) scatters: bin i < N/2 is added into bin
// ix(i) = int(i * ratio), then bins above N/2 are filled as out[N - i].  ix is non-decreasing in i,
// so the sources of a bin t <= N/2 are one contiguous run [first, first + count) of i < N/2, and a
// bin k > N/2 takes the run of N - k.  The kernels gather: each output bin adds its run in
// ascending i, starting from +0.0 -- the order of the reference's loop, with no atomics.
//
// The run's ends come from the very predicate the scatter evaluates, (int)((double)i * ratio) (one
// FP64 product, truncated), by bisection: a division would round differently next to a bin edge.
// ratio is finite and in [0, 8192] (checked at creation), so i * ratio < 2^30 for i < 2^17.
#pragma once

#include <hip/hip_runtime.h>

namespace hz {

constexpr double kTransposeMaxRatio = 8192.0;

__host__ __device__ inline bool transpose_ratio_ok(double r) { return r >= 0.0 && r <= kTransposeMaxRatio; }

// the reference's int(i * transp)
__host__ __device__ __forceinline__ int transpose_ix(int i, double ratio) { return (int)((double)i * ratio); }

// the first i in [from, H] with ix(i) >= t (H when there is none)
__host__ __device__ __forceinline__ int transpose_lower(int from, int H, double ratio, int t) {
    int lo = from, hi = H;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (transpose_ix(mid, ratio) >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the source run of output bin k, 0 <= k < N (N a power of two): bins above N/2 mirror N - k
__host__ __device__ __forceinline__ void transpose_run(int N, double ratio, int k, int* first, int* count) {
    const int H = N >> 1, t = k <= H ? k : N - k;
    const int lo = transpose_lower(0, H, ratio, t);
    *first = lo;
    *count = transpose_lower(lo, H, ratio, t + 1) - lo;
}

}  // namespace hz
