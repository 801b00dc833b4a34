// hz_fb_mac.h -- the stationary engine's MAC launch, Y_b = sum_{p < Q} H_p Z_{b+Q-1-p} per bin
// (included by hz_fb_resp.hip; tests/cpp/mac_bits.cpp launches the kernels on their own).
//
//   resp_mac_kernel<R, QP>     operands in registers: the streaming engine's response tail
//   resp_mac_kernel_lds<QP, S> operands staged in LDS, Qp = 8, 16, 24: the stationary step
//   resp_mac_kernel_ldsc       the same in chunks of 24 partitions: long horizons
// All three run the same FMAs in the same order per accumulator, so the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "hz_lds.h"

namespace hz_mac {

constexpr int kH = 2048;   // bins stored per spectrum row (hz_fb_resp.hip: kH)
constexpr int kMacR = 8;   // output blocks per MAC thread (partitions padded to it)

// 16-byte stores of what the next launch (Z, Y) or the caller (out) reads, through one helper with
// a policy per buffer.  kStThrough: write-through (sc1) buffer stores -- the bytes leave the
// producer's L2 while other workgroups still compute, instead of in the write-back after the
// launch's last workgroup.  The descriptor's base is the workgroup's own row / block (wave-uniform:
// kernel arguments and blockIdx only), so offsets and the record count stay far below 2^31 for any
// call length, and a store past `bytes` is dropped by the range check.  Narrow (8-byte) stores stay
// plain: write-through is one fabric write per store whatever its width.  The macros are the A/B
// hooks (one build per policy set); DESIGN.md 3.6 has the measurements behind the defaults.
enum StorePolicy { kStPlain = 0, kStThrough = 1 };
#ifndef HZ_ST_Y
#define HZ_ST_Y kStThrough
#endif
constexpr int kStY = HZ_ST_Y;       // output spectra: the LDS-staged MACs
typedef unsigned int hz_u32x4 __attribute__((ext_vector_type(4)));
template <int POL>
struct Store16 {
    double2* base;
    __amdgpu_buffer_rsrc_t rs;
    __device__ __forceinline__ Store16(double2* b, unsigned bytes) : base(b) {
        if constexpr (POL == kStThrough) rs = __builtin_amdgcn_make_buffer_rsrc(b, 0, bytes, 0x00020000);
    }
    __device__ __forceinline__ void operator()(unsigned i, double2 v) const {   // base[i] = v
        if constexpr (POL == kStThrough) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(hz_u32x4, v), rs, 16u * i, 0, 16);
        else base[i] = v;
    }
};

#ifdef HZ_DIAG_STAMPS
// (diagnostic builds) per-workgroup stamps of the forward [0], MAC [1] and inverse [2] kernels.
// Forward and inverse: start, operands arrived, transform done, end.  MAC (resp_mac_kernel_lds):
// start, the first stage's operands landed, all operands landed, MAC steps done, end.
constexpr int kDiagStamps = 5;
__device__ long long g_diag[3][1024][kDiagStamps];
__device__ __forceinline__ void diag_stamp(int k, int i) {
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_diag[k][blockIdx.x][i] = __builtin_amdgcn_s_memrealtime();
}
#define HZ_DIAG_AT(k, i) hz_mac::diag_stamp(k, i)
#define HZ_DIAG_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#else
#define HZ_DIAG_AT(k, i) ((void)0)
#define HZ_DIAG_VMCNT(n) ((void)0)
#endif

// Y_b[q] = sum_{p < Q} H_p[q] Z_{b+Q-1-p}[q] for b in [b0, b0 + R): thread = bin q x R output
// blocks.  The R Z values of step p sit in a register ring (element r in slot (r - p) mod R): each
// step brings one new Z value and one H value for R complex MACs.  Partitions are padded to a
// multiple of R with zero spectra (Qp), so every block of R steps loads unguarded.
// QP > 0 (Qp == QP, a compile-time count): every H and Z operand of the thread is loaded before
// the first MAC -- one memory latency per launch (a lone workgroup per CU hides none of it);
// QP == 0: any Qp, the next block's 2R loads issued before this block's MACs.
template <int R, int QP>
__global__ __launch_bounds__(256) void resp_mac_kernel(const double2* __restrict__ H, const double2* __restrict__ Z,
                                                       double2* __restrict__ Y, int Q, int Qp, int B) {
    constexpr int kBinGroups = kH / 256;
    const int q = (blockIdx.x % kBinGroups) * blockDim.x + threadIdx.x;   // bin
    const int b0 = (blockIdx.x / kBinGroups) * R;
    double ar[R], ai[R], zr[R], zi[R];
    const long base = (long)b0 + Q - 1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        ar[r] = ai[r] = 0.0;
        const double2 z = Z[(base + r) * kH + q];
        zr[r] = z.x;
        zi[r] = z.y;
    }
    auto zrow = [&](int p) {   // Z row of step p + 1's new element; < 0 only past Q (zero H rows)
        const long zi_ = base - p - 1;
        return (zi_ > 0 ? zi_ : 0) * kH + q;
    };
    auto step = [&](int u, const double2& hc, const double2& zc) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int sl = ((r - u) % R + R) % R;
            ar[r] = fma(hc.x, zr[sl], ar[r]);
            ar[r] = fma(-hc.y, zi[sl], ar[r]);
            ai[r] = fma(hc.x, zi[sl], ai[r]);
            ai[r] = fma(hc.y, zr[sl], ai[r]);
        }
        // element 0 of step p + 1 = Z[base - p - 1] into the slot element R - 1 leaves
        const int sl = ((-(u + 1)) % R + R) % R;
        zr[sl] = zc.x;
        zi[sl] = zc.y;
    };
    if constexpr (QP > 0) {
        double2 hv[QP], zv[QP];
#pragma unroll
        for (int p = 0; p < QP; ++p) {
            hv[p] = H[(long)p * kH + q];
            zv[p] = Z[zrow(p)];
        }
#pragma unroll
        for (int p = 0; p < QP; ++p) step(p % R, hv[p], zv[p]);
    } else {
        double2 hb[R], zb[R];
        auto fetch = [&](int p0) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                hb[u] = H[(long)(p0 + u) * kH + q];
                zb[u] = Z[zrow(p0 + u)];
            }
        };
        fetch(0);
        for (int p0 = 0; p0 < Qp; p0 += R) {
            double2 hc[R], zc[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                hc[u] = hb[u];
                zc[u] = zb[u];
            }
            if (p0 + R < Qp) fetch(p0 + R);
#pragma unroll
            for (int u = 0; u < R; ++u) step(u, hc[u], zc[u]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (b0 + r < B) Y[(long)(b0 + r) * kH + q] = make_double2(ar[r], ai[r]);
}

// The MAC with its operands staged in LDS: a workgroup owns 64 bins x 32 output blocks (a wave per
// 8 blocks), loads the QP partition spectra and the 32 + QP - 1 window-spectrum rows those blocks
// read once (80 KB at QP = 24), and each thread runs resp_mac_kernel's register ring (the same
// FMAs in the same order, so the same bits) from LDS.  The register-only kernel loads every H row
// once per 8 blocks and every Z row about four times: 55 MB through the L2s per C2 call, which its
// operand phase waits 3.4 us for (stamps, profiles/r5/diag); here 20 MB.
// (Of those 20 MB only 10 are fetched: the 8 block groups of a bin group run on one XCD, so their
// re-reads hit its L2.  Tiles of 16 bins x 128 blocks and 8 x 256, which load every row once per
// workgroup, measured level and 0.5 us slower per C2 launch: DESIGN.md 3.6.)
constexpr int kMacBins = 64;
// kMacBpw output blocks per wave, 4 waves: 32 blocks per workgroup (4 per wave -- 16 per workgroup,
// twice the workgroups -- measured slower: 8.25 against 6.07 us per C2 launch,
// profiles/r5/bpw/summary.txt)
constexpr int kMacBpw = 8;
template <int QP>
constexpr size_t mac_lds_bytes() { return sizeof(double2) * kMacBins * (QP + 4 * kMacBpw + QP - 1); }

// Stages of S steps (S divides QP, a multiple of 4; S == QP: one stage, what is built).  Step p reads
// H row p and the Z rows QP - 1 - p .. QP + 30 - p of the tile, so the order of use is known: stage
// 0 (steps < S) needs H rows < S and Z rows >= QP - S, stage s > 0 the H rows [s S, s S + S) and
// the Z rows [QP - s S - S, QP - s S).  A thread issues all its loads up front in that order (row r
// is wave r mod 4's), and each stage stores only its own rows to LDS from the registers that held
// them, behind its own barrier, so that the first stage's MACs could run while the later rows
// arrive (the stage's stores wait on vmcnt for its own loads only; tests/test_mac_stage_cpu.py is
// the index model).  A stage writes rows no earlier stage reads, so one barrier per stage is enough.
// Measured and not built: a wave's last operand lands 0.2 us after those of its
// first 8 steps, at C2 and on a time shard alike, so there is nothing to overlap; stages of 8 or 12
// steps cost the C2 step 0.3-0.4 us (two more barriers, the sums kept from sinking into the guarded
// stores) and gain a time shard 0.2-0.35 us.  HZ_MAC_STAGE is the A/B hook (one build per value).
#ifndef HZ_MAC_STAGE
#define HZ_MAC_STAGE 0
#endif
constexpr int mac_stage_of(int qp, int steps) { return steps > 0 && qp > 8 && qp % steps == 0 ? steps : qp; }
template <int QP>
constexpr int mac_stage() { return mac_stage_of(QP, HZ_MAC_STAGE); }

// f(std::integral_constant<int, i>) for i = I0 .. I1 - 1 (static_for) or I1 - 1 .. I0 (static_for_down)
template <int I0, int I1, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I0>());
        static_for<I0 + 1, I1>(f);
    }
}
template <int I1, int I0, class F>
__device__ __forceinline__ void static_for_down(F&& f) {
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I1 - 1>());
        static_for_down<I1 - 1, I0>(f);
    }
}
// the Z rows of stage s, stages of L steps, as a thread's k range [mac_zlo, mac_zhi) (row = wave + 4 k)
constexpr int mac_zlo(int QP, int s, int L) { return (QP - (s + 1) * L) / 4; }
constexpr int mac_zhi(int QP, int kZL, int s, int L) { return s == 0 ? kZL : (QP - s * L) / 4; }

template <int QP, int S>
__global__ __launch_bounds__(256) void resp_mac_kernel_lds(const double2* __restrict__ H, const double2* __restrict__ Z,
                                                           double2* __restrict__ Y, int Q, int B) {
    constexpr int BPW = kMacBpw, kMacBlk = 4 * BPW, kZr = kMacBlk + QP - 1, kHL = QP / 4, kZL = (kZr + 3) / 4;
    constexpr int NS = QP / S;
    static_assert(QP % S == 0 && S % 4 == 0, "stages of whole steps, rows four at a time");
    extern __shared__ double2 mac_lds[];
    double2(*hs)[kMacBins] = (double2(*)[kMacBins])mac_lds;
    double2(*zs)[kMacBins] = (double2(*)[kMacBins])(mac_lds + QP * kMacBins);
    const int t = threadIdx.x, lq = t & (kMacBins - 1), sl = t >> 6;
    const int q0 = (blockIdx.x % (kH / kMacBins)) * kMacBins, q = q0 + lq;
    const int b0 = (blockIdx.x / (kH / kMacBins)) * kMacBlk;
    HZ_DIAG_AT(1, 0);
    // Z row of block b, partition p: b + Q - 1 - p = row_lo + (b - b0) + QP - 1 - p; rows < 0 only
    // for p >= Q (zero H rows), read as row 0
    const long row_lo = (long)b0 + Q - QP;
    double2 hv[kHL], zv[kZL];
    // the thread's rows of stage s, stages of L steps: H k in [s L / 4, (s + 1) L / 4), Z k in
    // [zlo(s, L), zhi(s, L)); every index below is a compile-time constant (static_for), so hv / zv
    // are registers (hv[k] = H[...] itself is a 16-byte memcpy into the array, which stayed in
    // scratch once the array lived across a barrier: the element is rebuilt from its halves)
    auto hload = [&](auto k_) {
        constexpr int k = decltype(k_)::value;
        const double2 v = H[(long)(sl + 4 * k) * kH + q];
        hv[k] = make_double2(v.x, v.y);
    };
    auto zload = [&](auto k_) {   // (only the tile's last four rows can lie past kZr)
        constexpr int k = decltype(k_)::value;
        const int r = sl + 4 * k;
        const long row = row_lo + r;
        zv[k] = 4 * k + 3 < kZr || r < kZr ? Z[(row > 0 ? row : 0) * kH + q] : make_double2(0.0, 0.0);
    };
    // issued in order of use, H ascending and Z descending, S steps at a time (a single stage: 8 at
    // a time, so a diagnostic build times the same arrival order with and without the staging).
    // Only the tile's last four Z rows are guarded, by a wave-uniform test: with every row k >= 10
    // behind a branch on threadIdx (the compiler does not know that the wave index is < 4) the
    // loads were issued in five groups; the C2 step's median is 0.35 us lower without them
    constexpr int OS = S < QP ? S : (QP > 8 ? 8 : QP);
    static_for<0, QP / OS>([&](auto s_) {
        constexpr int s = decltype(s_)::value;
        static_for<s * OS / 4, (s + 1) * OS / 4>(hload);
        static_for_down<mac_zhi(QP, kZL, s, OS), mac_zlo(QP, s, OS)>(zload);
    });
    HZ_DIAG_VMCNT(kHL - OS / 4 + (QP - OS) / 4);   // the loads issued after the first OS steps' rows
    HZ_DIAG_AT(1, 1);
    double ar[BPW], ai[BPW], zr[BPW], zi[BPW];
    static_for<0, NS>([&](auto s_) {
        constexpr int s = decltype(s_)::value;
        if constexpr (s == NS - 1) {
            HZ_DIAG_VMCNT(0);
            HZ_DIAG_AT(1, 2);
        }
        static_for<s * S / 4, (s + 1) * S / 4>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            hs[sl + 4 * k][lq] = hv[k];
        });
        static_for_down<mac_zhi(QP, kZL, s, S), mac_zlo(QP, s, S)>([&](auto k_) {
            constexpr int k = decltype(k_)::value;
            if (4 * k + 3 < kZr || sl + 4 * k < kZr) zs[sl + 4 * k][lq] = zv[k];
        });
        __syncthreads();
        if constexpr (s == 0) {
#pragma unroll
            for (int r = 0; r < BPW; ++r) {
                ar[r] = ai[r] = 0.0;
                const double2 z = zs[BPW * sl + r + QP - 1][lq];
                zr[r] = z.x;
                zi[r] = z.y;
            }
        }
#pragma unroll
        for (int p = s * S; p < (s + 1) * S; ++p) {
            if (p > 0) {   // step p reads step p - 1's rows one block down, and one new row
#pragma unroll
                for (int r = BPW - 1; r > 0; --r) {
                    zr[r] = zr[r - 1];
                    zi[r] = zi[r - 1];
                }
                const double2 z = zs[BPW * sl + QP - 1 - p][lq];
                zr[0] = z.x;
                zi[0] = z.y;
            }
            const double2 hc = hs[p][lq];
#pragma unroll
            for (int r = 0; r < BPW; ++r) {   // resp_mac_kernel's step: the same FMA order
                ar[r] = fma(hc.x, zr[r], ar[r]);
                ar[r] = fma(-hc.y, zi[r], ar[r]);
                ai[r] = fma(hc.x, zi[r], ai[r]);
                ai[r] = fma(hc.y, zr[r], ai[r]);
            }
        }
        // The next stage's LDS stores, and the vmcnt wait in front of them, stay behind this stage's
        // MACs: left alone the compiler sinks every accumulator's whole chain into the guarded Y
        // store at the end (the last stage's still go there: a wave past B skips them), so the
        // sums are pinned here, and the scheduler may not move the stores up either.
        // (Diagnostic builds pin the last stage too: the stamp after it is the end of the MACs.)
#ifndef HZ_DIAG_STAMPS
        if constexpr (s + 1 < NS)
#endif
        {
#pragma unroll
            for (int r = 0; r < BPW; ++r) asm volatile("" : "+v"(ar[r]), "+v"(ai[r]));
            __builtin_amdgcn_sched_barrier(0);
        }
    });
    HZ_DIAG_AT(1, 3);
    // the workgroup's tile of Y: rows b0 .. min(B, b0 + 32) - 1, bins q0 .. q0 + 63
    const int nb = min(B - b0, kMacBlk);
    const Store16<kStY> yst(Y + (long)b0 * kH + q0, (unsigned)sizeof(double2) * ((nb - 1) * kH + kMacBins));
#pragma unroll
    for (int r = 0; r < BPW; ++r) {
        const int lb = BPW * sl + r;
        if (lb < nb) yst(lb * kH + lq, make_double2(ar[r], ai[r]));
    }
    HZ_DIAG_AT(1, 4);
}

// The LDS-staged MAC for long horizons (Qp > 24 partitions, e.g. R = 0.9999: K = 507,904, Q = 248):
// the partitions in chunks of 24 -- per chunk the 24 H rows and the 24 + 31 Z rows of the
// workgroup's 32 blocks go through LDS as in resp_mac_kernel_lds<24> (the next chunk's operands
// loaded into registers while this chunk's MACs run), the accumulators carried across chunks.  The
// partitions are visited in order with the same FMAs, so the result is the register kernel's bit
// for bit.  The register kernel it replaces pulled every H row once per 8 blocks and every Z row
// ~4 times through the L2s: ~0.5 GB per R = 0.9999 call.
constexpr int kMacChunk = 24;
// kMaccBins bins x (256 / kMaccBins) slices of kMacBpw blocks per workgroup: 16 x 16 x 8 = 128 blocks
// (the H rows re-read by 2 instead of 8 block rows, the Z rows re-read less per block): 35.5 us per
// R = 0.9999 call against 37.4 (32 x 8 x 8 = 64 blocks) and 46.2 (64 x 4 x 8 = 32 blocks, the C2
// kernel's tile), alternating on one box (profiles/r6/highq)
constexpr int kMaccBins = 16;
constexpr size_t kMaccLdsBytes = sizeof(double2) * kMaccBins * (kMacChunk + (256 / kMaccBins) * kMacBpw + kMacChunk - 1);
__global__ __launch_bounds__(256) void resp_mac_kernel_ldsc(const double2* __restrict__ H, const double2* __restrict__ Z,
                                                            double2* __restrict__ Y, int Q, int B, int nch, int cps,
                                                            long ystride) {
    constexpr int BINS = kMaccBins, BPW = kMacBpw;
    constexpr int QP = kMacChunk, SL = 256 / BINS, kMacBlk = SL * BPW, kZr = kMacBlk + QP - 1;
    constexpr int kHL = (QP + SL - 1) / SL, kZL = (kZr + SL - 1) / SL;
    extern __shared__ double2 mac_lds[];
    double2(*hs)[BINS] = (double2(*)[BINS])mac_lds;
    double2(*zs)[BINS] = (double2(*)[BINS])(mac_lds + QP * BINS);
    const int t = threadIdx.x, lq = t & (BINS - 1), sl = t / BINS;
    const int q0 = (blockIdx.x % (kH / BINS)) * BINS, q = q0 + lq;
    const int b0 = (blockIdx.x / (kH / BINS)) * kMacBlk;
    double2 hv[kHL], zv[kZL];
    auto fetch = [&](int c) {   // chunk c: partitions [24 c, 24 c + 24)
#pragma unroll
        for (int k = 0; k < kHL; ++k)
            hv[k] = sl + SL * k < QP ? H[(long)(QP * c + sl + SL * k) * kH + q] : make_double2(0.0, 0.0);
        const long row_lo = (long)b0 + Q - (long)QP * (c + 1);
#pragma unroll
        for (int k = 0; k < kZL; ++k) {
            const int r = sl + SL * k;
            const long row = row_lo + r;
            zv[k] = r < kZr ? Z[(row > 0 ? row : 0) * kH + q] : make_double2(0.0, 0.0);
        }
    };
    double ar[BPW], ai[BPW];
#pragma unroll
    for (int r = 0; r < BPW; ++r) ar[r] = ai[r] = 0.0;
    // split blockIdx.y: chunks [c0, c1) into its own partial-sum plane of Y
    const int c0 = blockIdx.y * cps, c1 = min(nch, c0 + cps);
    Y += blockIdx.y * ystride;
    if (c0 < c1) fetch(c0);
    for (int c = c0; c < c1; ++c) {
#pragma unroll
        for (int k = 0; k < kHL; ++k)
            if (sl + SL * k < QP) hs[sl + SL * k][lq] = hv[k];
#pragma unroll
        for (int k = 0; k < kZL; ++k)
            if (sl + SL * k < kZr) zs[sl + SL * k][lq] = zv[k];
        __syncthreads();
        if (c + 1 < c1) fetch(c + 1);   // in flight under this chunk's MACs
        double zr[BPW], zi[BPW];
#pragma unroll
        for (int r = 0; r < BPW; ++r) {
            const double2 z = zs[BPW * sl + r + QP - 1][lq];
            zr[r] = z.x;
            zi[r] = z.y;
        }
#pragma unroll
        for (int p = 0; p < QP; ++p) {
            const double2 hc = hs[p][lq];
#pragma unroll
            for (int r = 0; r < BPW; ++r) {
                ar[r] = fma(hc.x, zr[r], ar[r]);
                ar[r] = fma(-hc.y, zi[r], ar[r]);
                ai[r] = fma(hc.x, zi[r], ai[r]);
                ai[r] = fma(hc.y, zr[r], ai[r]);
            }
            if (p + 1 < QP) {
#pragma unroll
                for (int r = BPW - 1; r > 0; --r) {
                    zr[r] = zr[r - 1];
                    zi[r] = zi[r - 1];
                }
                const double2 z = zs[BPW * sl + QP - 2 - p][lq];
                zr[0] = z.x;
                zi[0] = z.y;
            }
        }
        __syncthreads();   // the next chunk's stores overwrite hs / zs
    }
    const int nb = min(B - b0, kMacBlk);
    const Store16<kStY> yst(Y + (long)b0 * kH + q0, (unsigned)sizeof(double2) * ((nb - 1) * kH + BINS));
#pragma unroll
    for (int r = 0; r < BPW; ++r) {
        const int lb = BPW * sl + r;
        if (lb < nb) yst(lb * kH + lq, make_double2(ar[r], ai[r]));
    }
}
// The long-horizon MAC is latency-bound per chunk (each chunk's operands are fetched one chunk ahead,
// and a 10 s call gives (kH / kMaccBins) x ceil(B / blk) = 128 workgroups whatever the tile: twice as
// many, 4 blocks per thread, measured the same 35 us), so the chunks are split over two workgroup
// planes whose partial sums the inverse launch adds.  The gain is small (R = 0.9999, alternating: 1
// plane 0.0645 / 0.0644, 2: 0.0632 / 0.0628, 4: 0.0640 / 0.0639 ms per call; MAC 35.0 -> 32.5 us, the
// inverse's sums +1 us), so chunk latency is not what bounds it either
inline int macc_splits(int Qp) { return std::min(2, Qp / kMacChunk); }

// the LDS-staged MAC: Qp = 8, 16, 24 or whole chunks of 24 (q_padded) (C2: 6.1 against 7.4 us per
// launch of the register-only kernel, step 29.4 against 30.6 us, alternating runs on one box,
// profiles/r5/mac/summary.txt)
inline unsigned mac_lds_grid(int B) { return (unsigned)((kH / kMacBins) * ((B + 4 * kMacBpw - 1) / (4 * kMacBpw))); }
template <int QP, int S = mac_stage<QP>()>
int launch_mac_lds_qp(int device, int B, const double2* H, const double2* Z, double2* Y, int Q, hipStream_t s) {
    if (int r = hz::allow_lds(device, (const void*)resp_mac_kernel_lds<QP, S>, mac_lds_bytes<QP>())) return r;
    hipLaunchKernelGGL((resp_mac_kernel_lds<QP, S>), dim3(mac_lds_grid(B)), dim3(256), (mac_lds_bytes<QP>()), s, H, Z, Y, Q, B);
    return HZ_OK;
}
inline int launch_mac_lds(int device, int Qp, int B, const double2* H, const double2* Z, double2* Y, int Q, hipStream_t s) {
    if (Qp > kMacChunk) {   // long horizons: partitions in chunks of 24
        constexpr int blk = (256 / kMaccBins) * kMacBpw;
        const int ns = macc_splits(Qp), nch = Qp / kMacChunk, cps = (nch + ns - 1) / ns;
        const dim3 grid((unsigned)((kH / kMaccBins) * ((B + blk - 1) / blk)), (unsigned)ns);
        if (int r = hz::allow_lds(device, (const void*)resp_mac_kernel_ldsc, kMaccLdsBytes)) return r;
        hipLaunchKernelGGL(resp_mac_kernel_ldsc, grid, dim3(256), kMaccLdsBytes, s, H, Z, Y, Q, B, nch, cps, (long)B * kH);
        return HZ_OK;
    }
    if (Qp == 8) return launch_mac_lds_qp<8>(device, B, H, Z, Y, Q, s);
    if (Qp == 16) return launch_mac_lds_qp<16>(device, B, H, Z, Y, Q, s);
    return launch_mac_lds_qp<24>(device, B, H, Z, Y, Q, s);
}

// the register-only MAC: the streaming engine's response tail (fb_resp_tail_conv)
typedef void (*MacKernel)(const double2*, const double2*, double2*, int, int, int);
inline MacKernel pick_mac(int Qp) {
    switch (Qp) {
    case 8: return resp_mac_kernel<kMacR, 8>;
    case 16: return resp_mac_kernel<kMacR, 16>;
    case 24: return resp_mac_kernel<kMacR, 24>;
    default: return resp_mac_kernel<kMacR, 0>;
    }
}

}  // namespace hz_mac
