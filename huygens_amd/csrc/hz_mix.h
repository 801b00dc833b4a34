// hz_mix.h -- the device half of the "partials x time -> mixdown" skeleton shared by the bank
// engines (Oscbank, Additive/Sinusoids, Bowl, Subtractive, the general Filterbank engine); the
// host half, the segment plan, is hz_mixplan.h.  A workgroup of kWaves waves owns one group of
// partials and walks a time segment in tiles of 64 kL samples: lane c of a wave holds the kL
// samples [kL c, kL c + kL) of its partials' mix.  At the end of a tile every wave has its mix in
// LDS rows [kL][kPad] (put_rows, or accumulated there directly), tile_reduce sums the waves in
// ascending order and stores one slab row per group, and slab_reduce_kernel sums the groups' rows
// in a fixed order (deterministic: no atomics).
#pragma once

#include <hip/hip_runtime.h>

namespace hz::mix {

constexpr int kWaves = 8;          // waves per workgroup
constexpr int kMaxPerWave = 64;    // partials per wave per tile (upper bound)
constexpr int kPad = 66;           // LDS row pad (conflict-free transposed reads)

constexpr int tile_len(int kL) { return 64 * kL; }
constexpr int plane_len(int kL) { return kWaves * kL * kPad; }   // doubles of the waves' mix rows [kWaves][kL][kPad]

__device__ __forceinline__ void cmul(double ar, double ai, double br, double bi, double& cr, double& ci) {
    const double r = fma(ar, br, -ai * bi);
    const double i = fma(ar, bi, ai * br);
    cr = r;
    ci = i;
}

// lane q's double (q wave-uniform)
__device__ __forceinline__ double lane_d(double v, int q) {
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffff), q);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), q);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// a wave's kL accumulators into its rows of one plane (my = plane + wave kL kPad)
template <int kL>
__device__ __forceinline__ void put_rows(double* my, int lane, const double (&acc)[kL]) {
#pragma unroll
    for (int j = 0; j < kL; ++j) my[j * kPad + lane] = acc[j];
}

// End of a tile: barrier, sample tl of the tile = the waves' sums w = 0..7 from 0.0 of row
// j = tl % kL, column tl / kL, per plane (planes lie plane_len(kL) doubles apart: Oscbank's re, im);
// store(t, s) for the samples t = t0 + tl < n; barrier (the rows are free for the next tile).
template <int kL, int PLANES, class Store>
__device__ __forceinline__ void tile_reduce(const double* part, long t0, long n, Store store) {
    __syncthreads();
    for (int tl = threadIdx.x; tl < tile_len(kL); tl += blockDim.x) {
        const int src = tl / kL, j = tl % kL;
        double s[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) s[p] = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w)
#pragma unroll
            for (int p = 0; p < PLANES; ++p) s[p] += part[p * plane_len(kL) + w * (kL * kPad) + j * kPad + src];
        const long t = t0 + tl;
        if (t < n) store(t, s);
    }
    __syncthreads();
}

// ---- the slab reduce: out[t] = sum_g slab[row(g) + t] ----------------------------------------
// 64 samples per workgroup, slice ty sums rows g = ty, ty + 4, ...; the slices add as
// (r0 + r1) + (r2 + r3).  The epilogue is a compile-time policy: where group g's row starts and
// how the sum is stored.
__device__ __forceinline__ double slab_add(double a, double b) { return a + b; }
__device__ __forceinline__ double2 slab_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

template <class OutT>
struct SlabStore {   // out[t] = (OutT)sum
    OutT* out;
    __device__ long row(int g, long stride) const { return (long)g * stride; }
    template <class T>
    __device__ void store(long t, T v) const { out[t] = (OutT)v; }
};
struct SlabScale {   // out[t] = sum * scale
    double scale;
    double* out;
    __device__ long row(int g, long stride) const { return (long)g * stride; }
    __device__ void store(long t, double v) const { out[t] = v * scale; }
};
struct SlabChannel { // rows [G][N] of a slab, channel blockIdx.y: out[ch][t] = sum
    int N;
    double* out;
    long ostride;
    __device__ size_t row(int g, long stride) const { return ((size_t)g * N + blockIdx.y) * stride; }
    __device__ void store(long t, double v) const { out[(size_t)blockIdx.y * ostride + t] = v; }
};

namespace {   // (a kernel per translation unit, as the engines' own kernels)
template <class T, class Ep>
__global__ __launch_bounds__(256) void slab_reduce_kernel(const T* __restrict__ slab, long stride, int G, long n,
                                                          Ep ep) {
    __shared__ T red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long t = (long)blockIdx.x * 64 + tx;
    T s = T();
    if (t < n)
        for (int g = ty; g < G; g += 4) s = slab_add(s, slab[ep.row(g, stride) + t]);
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && t < n) ep.store(t, slab_add(slab_add(red[0][tx], red[1][tx]), slab_add(red[2][tx], red[3][tx])));
}

}  // namespace

// grid (ceil(n / 64), channels), 256 threads, on `stream`; the launch error is the caller's to read
template <class T, class Ep>
inline void slab_reduce(hipStream_t stream, const T* slab, long stride, int G, long n, Ep ep, unsigned channels = 1) {
    hipLaunchKernelGGL((slab_reduce_kernel<T, Ep>), dim3((unsigned)((n + 63) / 64), channels), dim3(256), 0, stream,
                       slab, stride, G, n, ep);
}

}  // namespace hz::mix
