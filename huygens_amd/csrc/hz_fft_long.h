// hz_fft_long.h -- multi-pass FP64 complex FFT for frames of 2^14 .. 2^18 points (gfx950).
//
// A frame above 8192 points no longer fits in LDS, so the transform is split four-step
// (Bailey): N = N1 N2, lg1 = floor(lg / 2), lg2 = lg - lg1 (128 x 128 ... 512 x 512; 2^15 is
// 128 x 256).  With n = N2 n1 + n2 and k = k1 + N1 k2,
//
//     X[k1 + N1 k2] = sum_n2 W_N2^(n2 k2) * W_N^(n2 k1) * sum_n1 x[N2 n1 + n2] W_N1^(n1 k1)
//
// and the inverse is the mirror: sum over k2 first, times conj W_N^(n2 k1), then over k1.
//
//   column pass  one workgroup owns kTile = 16 adjacent columns n2 (every global access is a
//                128-byte line per row or more), runs their N1-point transforms in LDS with the
//                register-blocked passes of hz_fft.h (dif_regs / dit_regs, pad16), multiplies by
//                the inter-pass twiddle and stores to the device workspace ws[frame][p1][n2];
//   row pass     one workgroup owns kRows = 4 adjacent rows p1 of the workspace, runs their
//                N2-point transforms, the processor, and (where the processor allows) the
//                inverse N2-point transforms in the same launch, in place.
//
// Forward passes are decimation in frequency (natural in, bit-reversed out), inverse passes
// decimation in time (bit-reversed in, natural out), so nothing is transposed or re-ordered
// on the fused paths.  THE BIN-INDEX MAP: the value stored in workspace row p1 (p1 < N1), column
// p2 (p2 < N2) after the forward row pass is bin
//
//     k(p1, p2) = bitrev_lg1(p1) + N1 * bitrev_lg2(p2)
//
// (tests/test_long_stft_cpu.py checks it against numpy.fft for lg 14..18).  The Hilbert half
// band k < N/2 is therefore "p2 even"; forward-only launches scatter to k(p1, p2) (FFTW order)
// and inverse-only launches gather from it.
//
// Twiddles: the sub-transforms use the compact tables of W_N1 and W_N2 (hz::twc); the inter-pass
// factor W_N^e, e = n2 k1 < N, comes from one table of N/2 entries built on the host in long
// double (W^e = -W^(e - N/2) above the middle: exact).
//
// Gates reduce over the whole frame, which spans N1 / 4 row workgroups: the forward row launch
// writes one partial sum per workgroup (double-double for the keep gate), and every workgroup
// of the next launch adds the frame's partials in index order -- no floating-point atomics,
// the same bits on every run.
#pragma once

#include "hz_common.h"
#include "hz_fft.h"
#include "hz_transpose.h"

namespace hzl {

constexpr int kTile = 16, kTileLg = 4;   // columns per column-pass workgroup
constexpr int kRows = 4, kRowsLg = 2;    // rows per row-pass workgroup
constexpr int kColThreads = 512, kRowThreads = 256;
constexpr int kMaxLg = 18, kMinLg = 14;

// where a column pass reads (forward) or writes (inverse) its frame
enum { kIoStft = 0, kIoComplex = 1, kIoDct = 2 };
// row launches
enum { kRowFused = 0, kRowFwdGate = 1, kRowGateInv = 2, kRowFwdOut = 3, kRowInInv = 4 };

struct Args {
    // STFT frames: [history (N-1) | block input], as StftArgs
    const double* hr;
    const double* hi;
    const double* inr;
    const double* ini;
    const double* win;
    double* fo;             // frame ring, planar Re [R][N] then Im [R][N]
    const double2* csrc;    // natural-order complex frames (slot forward; inverse-only spectra)
    double2* cdst;          // natural-order complex frames (slot inverse; forward-only spectra)
    const double* rsrc;     // Cosine input  [batch][N]
    double* rdst;           // Cosine output [batch][N]
    double2* ws;            // workspace [frames][N1][N2]
    double* part;           // gate partial sums [frames][2 N1 / kRows]
    const double2* tw1;     // W_N1^k (compact prefix used)
    const double2* tw2;     // W_N2^k
    const double2* twN;     // W_N^k, k < N/2
    const double2* rot;     // Cosine: e^(-i pi k / 2N), k < N
    long f_lo, T0;
    int lg, lg1, lg2, laps, stride, R;
    double p0, p1;
};

__host__ __device__ constexpr int col_stride(int lgs) { return hz::padded_len(1 << lgs) + 1; }

inline size_t col_lds(int lg1) {
    return sizeof(double) * 2 * (size_t)kTile * col_stride(lg1) + sizeof(double2) * (size_t)hz::twc_len(lg1);
}
inline size_t row_lds(int lg2) {
    return sizeof(double) * 2 * (size_t)kRows * col_stride(lg2) + sizeof(double2) * (size_t)hz::twc_len(lg2);
}

// W_N^e for e in [0, N)
__device__ __forceinline__ double2 tw_full(const double2* __restrict__ twN, int e, int lg) {
    const int H = 1 << (lg - 1);
    if (e < H) return twN[e];
    const double2 t = twN[e - H];
    return make_double2(-t.x, -t.y);
}

// one pass of 2^lb transforms side by side (transform c at re + c cs): hz::dif_pass / dit_pass
template <int R, bool INV>
__device__ __forceinline__ void bpass(double* re, double* im, int lg, int lh, const double2* T, int lb, int cs) {
    constexpr int M = 1 << R;
    const int step = INV ? lh : lh - (R - 1);
    for (int g = threadIdx.x; g < (1 << (lg - R + lb)); g += blockDim.x) {
        const int c = g & ((1 << lb) - 1), b = g >> lb;
        double* cr = re + c * cs;
        double* ci = im + c * cs;
        const int p = b & ((1 << step) - 1);
        const int base = INV ? ((b >> lh) << (lh + R)) + p : ((b >> step) << (lh + 1)) + p;
        double xr[M], xi[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int e = hz::pad16(base + (j << step));
            xr[j] = cr[e];
            xi[j] = ci[e];
        }
        if constexpr (INV) hz::dit_regs<R, true>(xr, xi, lg, lh, p, T);
        else hz::dif_regs<R, true>(xr, xi, lg, lh, p, T);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int e = hz::pad16(base + (j << step));
            cr[e] = xr[j];
            ci[e] = xi[j];
        }
    }
}

template <bool INV>
__device__ __forceinline__ void bpass_r(int R, double* re, double* im, int lg, int lh, const double2* T, int lb,
                                        int cs) {
    switch (R) {
    case 3: bpass<3, INV>(re, im, lg, lh, T, lb, cs); break;
    case 2: bpass<2, INV>(re, im, lg, lh, T, lb, cs); break;
    default: bpass<1, INV>(re, im, lg, lh, T, lb, cs); break;
    }
    __syncthreads();
}

// hz::fft_fwd_lead<3> / fft_inv_tail<3> (all passes) over 2^lb transforms; lg >= 3
__device__ __forceinline__ void bfft_fwd(double* re, double* im, int lg, const double2* T, int lb, int cs) {
    int lh = lg - 1, left = lg;
    const int rem = lg % 3;
    if (rem) {
        bpass_r<false>(rem, re, im, lg, lh, T, lb, cs);
        lh -= rem;
        left -= rem;
    }
    for (; left > 0; left -= 3, lh -= 3) bpass_r<false>(3, re, im, lg, lh, T, lb, cs);
}

__device__ __forceinline__ void bfft_inv(double* re, double* im, int lg, const double2* T, int lb, int cs) {
    int lh = 0, left = lg;
    while (left > 0) {
        const int R = left >= 3 ? 3 : left;   // the remainder pass comes last
        bpass_r<true>(R, re, im, lg, lh, T, lb, cs);
        lh += R;
        left -= R;
    }
}

__device__ __forceinline__ long frame_start(long f, int laps, int stride, long N) {
    const long c = f / (2 * laps);
    const int i = (int)(f - c * 2 * laps);
    return (long)stride * i + c * (2 * N - 1);
}

// ---- forward column pass: source -> N1-point DIF per column -> x W_N^(n2 k1) -> workspace --------
template <int SRC>
__global__ __launch_bounds__(kColThreads) void long_col_fwd_kernel(Args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lg1 = a.lg1, lg2 = a.lg2, N1 = 1 << lg1, N2 = 1 << lg2, cs = col_stride(lg1);
    const long N = 1L << a.lg;
    double* re = lds;
    double* im = lds + kTile * cs;
    double2* T = (double2*)(im + kTile * cs);
    for (int k = threadIdx.x; k < hz::twc_len(lg1); k += blockDim.x) T[k] = a.tw1[k];
    const int tiles = N2 >> kTileLg;
    const long fl = blockIdx.x / tiles;
    const int c0 = (int)(blockIdx.x - fl * tiles) << kTileLg;
    long off = 0;
    if constexpr (SRC == kIoStft) off = frame_start(a.f_lo + fl, a.laps, a.stride, N) - a.T0 + (N - 1);
    for (int i = threadIdx.x; i < (N1 << kTileLg); i += blockDim.x) {
        const int c = i & (kTile - 1), n1 = i >> kTileLg;
        const long n = ((long)n1 << lg2) + c0 + c;
        double vr, vi = 0.0;
        if constexpr (SRC == kIoStft) {
            const long u = off + n;   // position in [history (N-1) | block input]
            if (u < N - 1) {
                vr = a.hr[u];
                if (a.hi) vi = a.hi[u];
            } else {
                vr = a.inr[u - (N - 1)];
                if (a.hi && a.ini) vi = a.ini[u - (N - 1)];
            }
            const double w = a.win[n];
            vr = w * vr;   // fourier.h:110-112: window * real, window * imag
            vi = w * vi;
        } else if constexpr (SRC == kIoComplex) {
            const double2 v = a.csrc[fl * N + n];
            vr = v.x;
            vi = v.y;
        } else {   // Makhoul: v[n] = x[2n], v[N-1-n] = x[2n+1]
            const long s = n < N / 2 ? 2 * n : 2 * (N - 1 - n) + 1;
            vr = a.rsrc[fl * N + s];
        }
        const int e = c * cs + hz::pad16(n1);
        re[e] = vr;
        im[e] = vi;
    }
    __syncthreads();
    bfft_fwd(re, im, lg1, T, kTileLg, cs);
    double2* ws = a.ws + fl * N;
    for (int i = threadIdx.x; i < (N1 << kTileLg); i += blockDim.x) {
        const int c = i & (kTile - 1), p1 = i >> kTileLg;
        const int n2 = c0 + c, k1 = hz::bitrev(p1, lg1);
        const int e = c * cs + hz::pad16(p1);
        double xr = re[e], xi = im[e];
        hz::cmul_tw(xr, xi, tw_full(a.twN, n2 * k1, a.lg), false);
        ws[((long)p1 << lg2) + n2] = make_double2(xr, xi);
    }
}

// ---- inverse column pass: workspace -> N1-point DIT per column -> destination ---------------------
template <int DST>
__global__ __launch_bounds__(kColThreads) void long_col_inv_kernel(Args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lg1 = a.lg1, lg2 = a.lg2, N1 = 1 << lg1, N2 = 1 << lg2, cs = col_stride(lg1);
    const long N = 1L << a.lg;
    double* re = lds;
    double* im = lds + kTile * cs;
    double2* T = (double2*)(im + kTile * cs);
    for (int k = threadIdx.x; k < hz::twc_len(lg1); k += blockDim.x) T[k] = a.tw1[k];
    const int tiles = N2 >> kTileLg;
    const long fl = blockIdx.x / tiles;
    const int c0 = (int)(blockIdx.x - fl * tiles) << kTileLg;
    const double2* ws = a.ws + fl * N;
    for (int i = threadIdx.x; i < (N1 << kTileLg); i += blockDim.x) {
        const int c = i & (kTile - 1), p1 = i >> kTileLg;
        const double2 v = ws[((long)p1 << lg2) + c0 + c];
        const int e = c * cs + hz::pad16(p1);
        re[e] = v.x;
        im[e] = v.y;
    }
    __syncthreads();
    bfft_inv(re, im, lg1, T, kTileLg, cs);
    long row = 0;
    if constexpr (DST == kIoStft) row = (a.f_lo + fl) % a.R;
    const long plane = (long)a.R * N;
    for (int i = threadIdx.x; i < (N1 << kTileLg); i += blockDim.x) {
        const int c = i & (kTile - 1), n1 = i >> kTileLg;
        const long n = ((long)n1 << lg2) + c0 + c;
        const int e = c * cs + hz::pad16(n1);
        if constexpr (DST == kIoStft) {
            a.fo[row * N + n] = re[e];
            a.fo[plane + row * N + n] = im[e];
        } else if constexpr (DST == kIoComplex) {
            a.cdst[fl * N + n] = make_double2(re[e], im[e]);
        } else {   // y[2n] = v[n], y[2n+1] = v[N-1-n]
            const long s = n < N / 2 ? 2 * n : 2 * (N - 1 - n) + 1;
            a.rdst[fl * N + s] = re[e];
        }
    }
}

// workgroup sums in one fixed order (wave shuffles, then the waves in index order)
__device__ __forceinline__ double wg_sum(double v, double* scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += scratch[w];
    return s;
}

__device__ __forceinline__ void wg_sum_dd(double& hi, double& lo, double* scratch) {
    for (int o = 32; o > 0; o >>= 1) {
        const double oh = __shfl_xor(hi, o, 64), ol = __shfl_xor(lo, o, 64);
        hz::dd_add(hi, lo, oh);
        hz::dd_add(hi, lo, ol);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) {
        scratch[2 * wave] = hi;
        scratch[2 * wave + 1] = lo;
    }
    __syncthreads();
    double h = 0.0, l = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
        hz::dd_add(h, l, scratch[2 * w]);
        hz::dd_add(h, l, scratch[2 * w + 1]);
    }
    hi = h;
    lo = l;
}

// ---- row pass ---------------------------------------------------------------------------------------
// kRowFused    workspace -> N2-point DIF -> PROC (identity / Hilbert) -> N2-point DIT -> x conj W -> workspace
// kRowFwdGate  workspace -> DIF -> spectrum back in place + this workgroup's partial magnitude sum
// kRowGateInv  the frame's partials in index order -> threshold -> gate -> DIT -> x conj W -> workspace
// kRowFwdOut   workspace -> DIF -> cdst in FFTW order (DCT: the REDFT10 rotation -> rdst)
// kRowInInv    csrc in FFTW order (DCT: the REDFT01 rotation of rsrc) -> DIT -> x conj W -> workspace;
//              PROC = HZ_PROC_TRANSPOSE: each bin gathered from csrc as the sum of its source run
template <int PROC, int MODE, bool DCT>
__global__ __launch_bounds__(kRowThreads) void long_row_kernel(Args a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double scratch[2 * (kRowThreads / 64)];
    __shared__ double thr_s;
    const int lg1 = a.lg1, lg2 = a.lg2, N1 = 1 << lg1, N2 = 1 << lg2, cs = col_stride(lg2);
    const long N = 1L << a.lg;
    double* re = lds;
    double* im = lds + kRows * cs;
    double2* T = (double2*)(im + kRows * cs);
    for (int k = threadIdx.x; k < hz::twc_len(lg2); k += blockDim.x) T[k] = a.tw2[k];
    const int wpf = N1 >> kRowsLg;   // workgroups per frame
    const long fl = blockIdx.x / wpf;
    const int wg = (int)(blockIdx.x - fl * wpf), r0 = wg << kRowsLg;
    double2* ws = a.ws + fl * N + ((long)r0 << lg2);
    const int cnt = kRows << lg2;

    double thr = 0.0;
    if constexpr (MODE == kRowGateInv) {
        if (threadIdx.x == 0) {
            const double* part = a.part + fl * 2 * wpf;
            if constexpr (PROC == HZ_PROC_STATIC_GATE) {   // staticSTFT.h:99-128
                double average = 0.0;
                for (int w = 0; w < wpf; ++w) average += part[2 * w];
                thr_s = a.p0 * average * average;
            } else {   // tests/spectral.cpp:32-72: sum / N in long double
                double hi = 0.0, lo = 0.0;
                for (int w = 0; w < wpf; ++w) {
                    hz::dd_add(hi, lo, part[2 * w]);
                    hz::dd_add(hi, lo, part[2 * w + 1]);
                }
                const double q = hi / (double)N;
                const double avg = q + (fma(-q, (double)N, hi) + lo) / (double)N;
                thr_s = a.p0 * avg * avg;
            }
        }
        __syncthreads();
        thr = thr_s;
    }

    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int r = i >> lg2, p2 = i & (N2 - 1);
        double vr, vi;
        if constexpr (MODE == kRowInInv) {
            const long k = hz::bitrev(r0 + r, lg1) + ((long)hz::bitrev(p2, lg2) << lg1);
            if constexpr (DCT) {   // V_k = e^(i pi k / 2N) (x_k - i x_(N-k))
                const double* xb = a.rsrc + fl * N;
                const double x0 = xb[k], x1 = k ? xb[N - k] : 0.0;
                const double2 w = a.rot[k];
                vr = x0 * w.x + x1 * (-w.y);
                vi = -x0 * w.y - x1 * w.x;
            } else if constexpr (PROC == HZ_PROC_TRANSPOSE) {
                // tests/demo.cpp:49-81 (p0 the ratio) as a gather from the spectrum in csrc: bin k
                // adds its run of source bins in ascending order from +0.0 (hz_transpose.h)
                int first, count;
                hz::transpose_run((int)N, a.p0, (int)k, &first, &count);
                const double2* sp = a.csrc + fl * N;
                vr = 0.0;
                vi = 0.0;
                for (int s = first; s < first + count; ++s) {
                    const double2 v = sp[s];
                    vr += v.x;
                    vi += v.y;
                }
            } else {
                const double2 v = a.csrc[fl * N + k];
                vr = v.x;
                vi = v.y;
            }
        } else {
            const double2 v = ws[i];
            vr = v.x;
            vi = v.y;
            if constexpr (MODE == kRowGateInv) {
                if constexpr (PROC == HZ_PROC_STATIC_GATE) {
                    if (vr * vr + vi * vi < thr) {
                        vr = vr * a.p1;
                        vi = vi * a.p1;
                    }
                } else {
                    if (!(vr * vr + vi * vi > thr)) vr = vi = 0.0;
                }
            }
        }
        const int e = r * cs + hz::pad16(p2);
        re[e] = vr;
        im[e] = vi;
    }
    __syncthreads();

    if constexpr (MODE == kRowFused || MODE == kRowFwdGate || MODE == kRowFwdOut) {
        bfft_fwd(re, im, lg2, T, kRowsLg, cs);
        if constexpr (MODE == kRowFwdGate) {
            double hi = 0.0, lo = 0.0;
            const double inv_n = 1.0 / (double)N;   // exact: N = 2^lg
            for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
                const int e = (i >> lg2) * cs + hz::pad16(i & (N2 - 1));
                const double xr = re[e], xi = im[e];
                if constexpr (PROC == HZ_PROC_STATIC_GATE) hi += sqrt(xr * xr + xi * xi) * inv_n;
                else hz::dd_add(hi, lo, hypot(xr, xi));
                ws[i] = make_double2(xr, xi);
            }
            if constexpr (PROC == HZ_PROC_STATIC_GATE) hi = wg_sum(hi, scratch);
            else wg_sum_dd(hi, lo, scratch);
            if (threadIdx.x == 0) {
                a.part[(fl * wpf + wg) * 2] = hi;
                a.part[(fl * wpf + wg) * 2 + 1] = lo;
            }
            return;
        } else if constexpr (MODE == kRowFwdOut) {
            for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
                const int r = i >> lg2, p2 = i & (N2 - 1);
                const int e = r * cs + hz::pad16(p2);
                const long k = hz::bitrev(r0 + r, lg1) + ((long)hz::bitrev(p2, lg2) << lg1);
                if constexpr (DCT) {   // Y_k = 2 Re(V_k e^(-i pi k / 2N))
                    const double2 w = a.rot[k];
                    a.rdst[fl * N + k] = 2.0 * (re[e] * w.x - im[e] * w.y);
                } else {
                    a.cdst[fl * N + k] = make_double2(re[e], im[e]);
                }
            }
            return;
        } else if constexpr (PROC == HZ_PROC_HILBERT) {   // bins k < N/2 kept: even p2
            for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
                const int p2 = i & (N2 - 1);
                if (p2 & 1) {
                    const int e = (i >> lg2) * cs + hz::pad16(p2);
                    re[e] = 0.0;
                    im[e] = 0.0;
                }
            }
            __syncthreads();
        }
    }
    bfft_inv(re, im, lg2, T, kRowsLg, cs);
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int r = i >> lg2, n2 = i & (N2 - 1);
        const int e = r * cs + hz::pad16(n2);
        double xr = re[e], xi = im[e];
        hz::cmul_tw(xr, xi, tw_full(a.twN, n2 * hz::bitrev(r0 + r, lg1), a.lg), true);
        ws[i] = make_double2(xr, xi);
    }
}

// ---- host side -----------------------------------------------------------------------------------
inline void split_lg(int lg, int& lg1, int& lg2) {
    lg1 = lg / 2;
    lg2 = lg - lg1;
}

// the column kernels' dynamic-LDS limit, at the longest frame's size
inline int init_attrs(int device) {
    return hz::allow_lds(device,
                         {(const void*)long_col_fwd_kernel<kIoStft>, (const void*)long_col_fwd_kernel<kIoComplex>,
                          (const void*)long_col_fwd_kernel<kIoDct>, (const void*)long_col_inv_kernel<kIoStft>,
                          (const void*)long_col_inv_kernel<kIoComplex>, (const void*)long_col_inv_kernel<kIoDct>},
                         col_lds(kMaxLg / 2));
}

template <int IO>
inline void col_fwd(const Args& a, long frames, hipStream_t s) {
    hipLaunchKernelGGL(long_col_fwd_kernel<IO>, dim3((unsigned)(frames << (a.lg2 - kTileLg))), dim3(kColThreads),
                       col_lds(a.lg1), s, a);
}
template <int IO>
inline void col_inv(const Args& a, long frames, hipStream_t s) {
    hipLaunchKernelGGL(long_col_inv_kernel<IO>, dim3((unsigned)(frames << (a.lg2 - kTileLg))), dim3(kColThreads),
                       col_lds(a.lg1), s, a);
}
template <int PROC, int MODE, bool DCT>
inline void row(const Args& a, long frames, hipStream_t s) {
    hipLaunchKernelGGL((long_row_kernel<PROC, MODE, DCT>), dim3((unsigned)(frames << (a.lg1 - kRowsLg))),
                       dim3(kRowThreads), row_lds(a.lg2), s, a);
}

}  // namespace hzl
