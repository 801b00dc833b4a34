// hz_resonant.h -- device code of Filter<T>::resonant() / Subtractive::resonant()
// (src/filter.h:123-138, src/subtractive.h:240-249): the gain of the two-pole, two-zero resonator
// {g, 0, -g}, {-2 R cos(2 PI f / SR), R^2}.  One copy for the per-sample coefficient stream of
// hz_fb_tv.hip and the per-physics-step coefficient rows of hz_subtractive.hip.
// Every function switches FMA contraction off in its own body, so the arithmetic does not depend
// on the including file's setting.
#pragma once

#include "hz_common.h"
#include "hz_rt.h"

namespace hz_res {

// x / SR correctly rounded without the IEEE divide sequence: q = x RN(1/SR), then one FMA
// residual step (Markstein; x >= 0 normal here).  Equal to x / 48000.0 -- checked on the
// host (tests/cpp/divcheck.c: random exponents, no mismatch).
__device__ __forceinline__ double div_sr(double x) {
#pragma clang fp contract(off)
    constexpr double inv = 1.0 / hz::kSR;
    const double q = x * inv;
    return __builtin_fma(__builtin_fma(-q, (double)hz::kSR, x), inv, q);
}

// cdiv(1, 0, c, d) of libgcc's __divdc3 (Smith's algorithm): both quotients share the denominator,
// so one IEEE reciprocal r = RN(1/den) serves both: -1/den = -r exactly, and ratio/den is taken as
// RN(q0 + RN(ratio - den q0) r), q0 = RN(ratio r) (one FMA residual step).  Markstein's exactness
// theorem needs q0 within 1 ulp, which RN(ratio r) does not guarantee (up to ~1.5 ulp), so
// exactness is checked, not proven: tests/cpp/divcheck.c compares it bit for bit with the Smith
// quotient on random resonant() operands, generic operands and targeted hard cases (quotient
// mantissa near 2, reciprocal error near 1/2 ulp) -- no mismatch in ~1e9 trials.  The sign of a
// zero may differ; nothing sees it.
__device__ __forceinline__ void cdiv_one(double c, double d, double& x, double& y) {
#pragma clang fp contract(off)
    const bool lt = fabs(c) < fabs(d);
    const double ratio = lt ? c / d : d / c;
    const double den = lt ? (c * ratio) + d : (d * ratio) + c;
    const double r = 1.0 / den;
    const double q0 = ratio * r;
    const double q = __builtin_fma(__builtin_fma(-q0, den, ratio), r, q0);   // RN(ratio / den)
    x = lt ? q : r;
    y = lt ? -r : -q;
}

// cos / sincos of an angle: the bounded-range kernels (< 1 ulp, hz_rt.h) for 0 <= x <= 2 PI -- every
// audio frequency's 2 PI f / SR and 4 PI f / SR -- else libm
__device__ __forceinline__ double tv_cos(double x) {
    return (x >= 0.0 && x <= 6.2831853072) ? hz_rt::cos_0_2pi(x) : cos(x);
}
__device__ __forceinline__ void tv_sincos(double x, double* s, double* c) {
    if (x >= 0.0 && x <= 6.2831853072) hz_rt::sincos_0_2pi(x, s, c);
    else sincos(x, s, c);
}

// subtractive.h:240-249, filter.h:129-133
__device__ __forceinline__ double resonant(double frequency, double Q) {
#pragma clang fp contract(off)
    double s2, c2;
    tv_sincos(div_sr(4 * hz::kPI * frequency), &s2, &c2);
    const double ir = 0.0 * s2 - 1.0 * 0.0, ii = 0.0 * 0.0 + 1.0 * s2;   // 1.0i * sine2
    const double dr = (Q - c2) - ir, di = -0.0 - ii;
    double qr, qi;
    cdiv_one(dr, di, qr, qi);
    const double mr = 1.0 / (Q - 1) - qr, mi = 0.0 - qi;
    return 1 / sqrt(hypot(mr, mi));
}

}  // namespace hz_res
