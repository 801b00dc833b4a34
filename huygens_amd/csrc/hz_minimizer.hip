// hz_minimizer.hip -- Minimizer<T>::physics() on the device (src/minimizer.h:61-108,
// src/particle.h) and the Additive render that follows the moving particles (src/additive.h:38-62).
//
// One physics step over the voices with active[i] != 0:
//   prepare   acceleration = 0, mass = active[i]
//   springs   (i, 0) guide -> particle 0, k = 0.1 FORCE; (i, j) particle j-1 -> j, k = FORCE;
//             first->pull(k disp), second->pull(-k disp), pull(f): acceleration += f / mass
//   gravity   every pair of particles of two different active voices (particle.h:116-125)
//   tick      v += a / SR; v *= drag; x += v / SR
// The reference scatters forces pair by pair.  The order in which one particle's `acceleration`
// receives its terms is: its own spring, the next overtone's spring, then gravity from the other
// active voices in ascending voice and overtone order (as `second` of the pair when the other
// voice's index is smaller, as `first` when it is larger).  One thread per particle walks the other
// particles in that order -- a gather, no scatter and no atomic -- and so reproduces the reference's
// positions bit for bit: every expression below keeps the reference's association, divisions stay
// divisions (IEEE: v_div_scale / v_div_fmas / v_div_fixup), and the whole file is compiled with
// contraction off.
//
// particle.h:119,121 call an unqualified abs on doubles, which binds ::abs(int) or the double
// overload depending on the platform's headers: HZ_GRAV_TRUNC and HZ_GRAV_FABS (huygens_hip.h).
// Beyond the cutoff the force is 0 and the pull adds +-0 to an acceleration that starts at +0 and
// can never be -0 (x + (-x) = +0 in round-to-nearest), so those pairs are skipped before the division.
#include "hz_minimizer.h"

#pragma clang fp contract(off)

namespace {

constexpr double kSRd = (double)hz::kSR;

// one Gravity::tick (particle.h:116-125): d = second->position - first->position,
// gmm = (G first->mass) second->mass.  grav_cut: the cutoff zeroes the force.
template <int LAW>
__device__ __forceinline__ bool grav_cut(double d) {
    // TRUNC: abs(int(d)) >= 0.5 <=> |int(d)| >= 1 <=> |d| >= 1 (conversion truncates toward zero)
    return fabs(d) >= (LAW == HZ_GRAV_TRUNC ? 1.0 : 0.5);
}

template <int LAW>
__device__ __forceinline__ double grav_force(double d, double gmm, double eps) {
    double cubed;
    if constexpr (LAW == HZ_GRAV_TRUNC)
        cubed = (double)abs((int)(d * d * d));
    else
        cubed = fabs(d * d * d);
    return gmm * d / (eps + cubed);
}

// four pairs at once: their forces and pulls (force / mass) are independent and overlap; only the
// additions into the acceleration are ordered, so the serial chain per pair is one add instead of
// two divisions.  SECOND: this particle is the pair's `second` (distance = xme - other,
// pull(-force)), else its `first`.
template <int LAW, bool SECOND>
__device__ __forceinline__ void gravity_quad(double& a, double xme, double m, double gmm, double eps,
                                             const double* xs) {
    double d[4];
    bool on = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        d[k] = SECOND ? xme - xs[k] : xs[k] - xme;
        on |= !grav_cut<LAW>(d[k]);
    }
    if (!on) return;
    double pull[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double force = grav_force<LAW>(d[k], gmm, eps);
        pull[k] = (SECOND ? -force : force) / m;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a += grav_cut<LAW>(d[k]) ? 0.0 : pull[k];   // a is never -0: a + 0 == a
}

// gravity from one other voice's particles xs[0 .. n) in index order.  (Testing 16 pairs against
// the cutoff before the quads was measured slower: 64 x 256 at 677 ms per block against 590.)
template <int LAW, bool SECOND>
__device__ __forceinline__ void gravity_voice(double& a, double xme, double m, double gmm, double eps,
                                              const double* xs, int n) {
    int q = 0;
    for (; q + 4 <= n; q += 4) gravity_quad<LAW, SECOND>(a, xme, m, gmm, eps, xs + q);
    for (; q < n; ++q) {
        const double d = SECOND ? xme - xs[q] : xs[q] - xme;
        if (grav_cut<LAW>(d)) continue;
        const double force = grav_force<LAW>(d, gmm, eps);
        a += (SECOND ? -force : force) / m;
    }
}

// gravity on the particle at xme (voice i, mass m) from particles [base, base + count), whose
// positions are xs[0 .. count); ascending index = ascending voice, ascending overtone
template <int LAW>
__device__ __forceinline__ void gravity_range(double& a, double xme, double m, int i, const double* act, int O,
                                              const double* xs, int base, int count, double G, double eps) {
    int q = base;
    const int end = base + count;
    while (q < end) {
        const int u = q / O;
        const int uend = min(end, (u + 1) * O);
        const double mo = act[u];
        if (u != i && mo != 0.0) {
            if (u < i)   // this particle is `second`: gmm = (G first->mass) second->mass
                gravity_voice<LAW, true>(a, xme, m, G * mo * m, eps, xs + (q - base), uend - q);
            else
                gravity_voice<LAW, false>(a, xme, m, G * m * mo, eps, xs + (q - base), uend - q);
        }
        q = uend;
    }
}

// the particle's own spring, then the next overtone's (Spring::tick, particle.h:85-91)
__device__ __forceinline__ double spring_accel(double xme, double first, double eq_me, double k_me, bool has_next,
                                               double xnext, double eq_next, double k_next, double m) {
    double a = 0.0;
    double disp = (xme - first) - eq_me;
    a += -k_me * disp / m;
    if (has_next) {
        disp = (xnext - xme) - eq_next;
        a += k_next * disp / m;
    }
    return a;
}

// Small banks: one workgroup, one thread per particle, every step of the call in one launch.
// Positions sit in two LDS rows; a step reads one and writes the other, so one barrier per step
// separates a step's force reads from the next step's.  LDS: [2][P] positions, [V] active.
template <int LAW>
__global__ __launch_bounds__(1024) void min_steps_kernel(hz::MinParams prm, int steps, double* __restrict__ rows,
                                                         double* __restrict__ v, const double* __restrict__ eq,
                                                         const double* __restrict__ act,
                                                         const double* __restrict__ guide) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int P = prm.V * prm.O, O = prm.O;
    double* xs0 = lds;
    double* xs1 = lds + P;
    double* acts = lds + 2 * P;
    const int tid = threadIdx.x;
    const bool valid = tid < P;
    const int i = valid ? tid / O : 0, j = valid ? tid - i * O : 0;
    for (int q = tid; q < prm.V; q += blockDim.x) acts[q] = act[q];
    double vel = 0.0, eq_me = 0.0, eq_next = 0.0, first0 = 0.0;
    const bool has_next = valid && j + 1 < O;
    if (valid) {
        xs0[tid] = rows[tid];
        vel = v[tid];
        eq_me = eq[tid];
        if (has_next) eq_next = eq[tid + 1];
        first0 = guide[i];
    }
    __syncthreads();
    const double m = valid ? acts[i] : 0.0;
    const double k_me = j == 0 ? prm.k0 : prm.k1;
    for (int s = 0; s < steps; ++s) {
        const double* cur = (s & 1) ? xs1 : xs0;
        double* nxt = (s & 1) ? xs0 : xs1;
        if (valid) {
            const double xme = cur[tid];
            double xn = xme;
            if (m != 0.0) {
                double a = spring_accel(xme, j == 0 ? first0 : cur[tid - 1], eq_me, k_me, has_next,
                                        has_next ? cur[tid + 1] : 0.0, eq_next, prm.k1, m);
                gravity_range<LAW>(a, xme, m, i, acts, O, cur, 0, P, prm.G, prm.eps);
                vel += a / kSRd;
                vel *= prm.drag;
                xn = xme + vel / kSRd;
            }
            nxt[tid] = xn;
            rows[(size_t)(s + 1) * P + tid] = xn;
        }
        __syncthreads();
    }
    if (valid) v[tid] = vel;
}

// Larger banks: one launch per step, one thread per particle; the other particles' positions pass
// through LDS in tiles of blockDim.x.  Reads row `xin`, writes row `xout`: stream order is the only
// dependency between steps.  LDS: [blockDim.x] positions, [V] active.
template <int LAW>
__global__ __launch_bounds__(1024) void min_step_kernel(hz::MinParams prm, const double* __restrict__ xin,
                                                        double* __restrict__ xout, double* __restrict__ v,
                                                        const double* __restrict__ eq,
                                                        const double* __restrict__ act,
                                                        const double* __restrict__ guide) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int P = prm.V * prm.O, O = prm.O, tile = blockDim.x;
    double* chunk = lds;
    double* acts = lds + tile;
    const int tid = threadIdx.x;
    const int p = blockIdx.x * tile + tid;
    const bool valid = p < P;
    const int i = valid ? p / O : 0, j = valid ? p - i * O : 0;
    for (int q = tid; q < prm.V; q += tile) acts[q] = act[q];
    __syncthreads();
    const double m = valid ? acts[i] : 0.0;
    const bool moving = valid && m != 0.0;
    double xme = 0.0, a = 0.0;
    if (valid) xme = xin[p];
    if (moving) {
        const bool has_next = j + 1 < O;
        a = spring_accel(xme, j == 0 ? guide[i] : xin[p - 1], eq[p], j == 0 ? prm.k0 : prm.k1, has_next,
                         has_next ? xin[p + 1] : 0.0, has_next ? eq[p + 1] : 0.0, prm.k1, m);
    }
    for (int base = 0; base < P; base += tile) {
        const int count = min(tile, P - base);
        if (tid < count) chunk[tid] = xin[base + tid];
        __syncthreads();
        if (moving) gravity_range<LAW>(a, xme, m, i, acts, O, chunk, base, count, prm.G, prm.eps);
        __syncthreads();
    }
    if (valid) {
        double xn = xme;
        if (moving) {
            double vel = v[p];
            vel += a / kSRd;
            vel *= prm.drag;
            v[p] = vel;
            xn = xme + vel / kSRd;
        }
        xout[p] = xn;
    }
}

constexpr int kTT = 64;         // samples per transposed tile
constexpr int kTPad = kTT + 1;  // tile row stride: lane-major writes and time-major reads both conflict-free

// Audio with moving particles.  Lanes are partials, time is sequential: per sample the Oscillator
// recurrence (oscillator.h:27-38 with phase == target_phase: the pull term is the identity)
//   phi += f / SR;  f <- ft (1 - s) + f s;  phi -= int(phi)
// with ft = mtof(position in effect), recomputed only when a step happened.  A wave's 64 partials x
// 64 samples are transposed through a padded LDS tile; lanes then become time and sum the partials
// in index order, so a sample's sum does not depend on how a call is split.  One wave per workgroup
// (a 64 x 256 bank is 256 workgroups, one per CU); each writes one group row for hz_mix.h's slab reduce.
__global__ __launch_bounds__(64) void add_track_kernel(hz::TrackArgs a) {
    __shared__ double tile[64 * kTPad];
    const int lane = threadIdx.x;
    const int p = blockIdx.x * 64 + lane;
    const bool valid = p < a.P;
    const int vo = valid ? p / a.O : 0;
    double phi = 0.0, f = 0.0, ft = 0.0, c = 0.0;
    const double act = a.act[vo];
    if (valid) {
        phi = a.phi[p];
        f = a.f[p];
        c = a.c[p];
        ft = 440.0 * exp2((a.rows[p] - 69) / 12);
    }
    long row = 0;
    double* grow = a.partial + (size_t)blockIdx.x * a.n_pad;
    for (long t0 = 0; t0 < a.n; t0 += kTT) {
        const int cnt = (int)min((long)kTT, a.n - t0);
        for (int tt = 0; tt < cnt; ++tt) {
            const long t = t0 + tt;
            const double amp = a.amp[t * a.V + vo];
            tile[lane * kTPad + tt] = (valid && amp != 0.0) ? amp * (c * sinpi(2.0 * phi)) : 0.0;
            const long T = a.T0 + t;
            if (a.period > 0 && T >= a.period && T % a.period == 0) {   // physics() between operator() and tick()
                ++row;
                if (valid) ft = 440.0 * exp2((a.rows[(size_t)row * a.P + p] - 69) / 12);
            }
            const double amp_next = a.amp[(t + 1) * a.V + vo];
            if (valid && (act != 0.0 || amp_next != 0.0)) {
                phi += f / kSRd;
                f = ft * (1 - a.s) + f * a.s;
                phi -= (double)(int)phi;
            }
        }
        __syncthreads();
        if (lane < cnt) {
            double sum = 0.0;
#pragma unroll 8
            for (int q = 0; q < 64; ++q) sum += tile[q * kTPad + lane];
            grow[t0 + lane] = sum;
        }
        __syncthreads();
    }
    if (a.advance && valid) {
        a.phi[p] = phi;
        a.f[p] = f;
    }
}

}  // namespace

namespace hz {

int min_run(hipStream_t stream, const MinParams& prm, int law, int steps, bool single_group, int tile, double* rows,
            double* v, const double* eq, const double* act, const double* guide) {
    const int P = prm.V * prm.O;
    if (steps <= 0) return HZ_OK;
    const bool trunc = law == HZ_GRAV_TRUNC;
    if (single_group) {
        const int threads = (P + 63) / 64 * 64;
        const size_t lds = sizeof(double) * (2 * (size_t)P + prm.V);
        if (trunc)
            hipLaunchKernelGGL(min_steps_kernel<HZ_GRAV_TRUNC>, dim3(1), dim3(threads), lds, stream, prm, steps, rows,
                               v, eq, act, guide);
        else
            hipLaunchKernelGGL(min_steps_kernel<HZ_GRAV_FABS>, dim3(1), dim3(threads), lds, stream, prm, steps, rows,
                               v, eq, act, guide);
        HZ_TRY_HIP(hipGetLastError());
        return HZ_OK;
    }
    const int groups = (P + tile - 1) / tile;
    const size_t lds = sizeof(double) * ((size_t)tile + prm.V);
    for (int s = 0; s < steps; ++s) {
        const double* xin = rows + (size_t)s * P;
        double* xout = rows + (size_t)(s + 1) * P;
        if (trunc)
            hipLaunchKernelGGL(min_step_kernel<HZ_GRAV_TRUNC>, dim3(groups), dim3(tile), lds, stream, prm, xin, xout,
                               v, eq, act, guide);
        else
            hipLaunchKernelGGL(min_step_kernel<HZ_GRAV_FABS>, dim3(groups), dim3(tile), lds, stream, prm, xin, xout,
                               v, eq, act, guide);
    }
    HZ_TRY_HIP(hipGetLastError());
    return HZ_OK;
}

int add_track_groups(int P) { return (P + 63) / 64; }

int add_track(hipStream_t stream, const TrackArgs& a) {
    hipLaunchKernelGGL(add_track_kernel, dim3(add_track_groups(a.P)), dim3(64), 0, stream, a);
    HZ_TRY_HIP(hipGetLastError());
    return HZ_OK;
}

}  // namespace hz
