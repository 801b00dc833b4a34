// hz_additive.hip -- Additive<double> and Sinusoids<double> banks for MI355X (gfx950).
//
// Both are banks of Oscillator<T> phase accumulators (src/oscillator.h:27-38) mixed
// through cycle(p) = sin(2 PI p) (src/wave.h:147):
//   Additive  (src/additive.h:38-62):  out = sum_v [amp_v != 0] sum_j amp_v decay^j
//             sin(2 PI phi_vj) / (V norm);  tick: amp_v <- (1-a) active_v + a amp_v, then
//             for voices with active_v || amp_v: freqmod(mtof(position_vj)); Oscillator::tick()
//   Sinusoids (src/sinusoids.h:34-57): out = sum_i decay^i sin(2 PI phi_i) / norm
//
// Oscillator::tick advances phase by f/SR and relaxes f toward its target with stiffness s:
//   phi(t) = phi0 + A t + D (1 - s^t),   A = f_target/SR,  D = (f0 - f_target)/((1-s) SR)
// (phase and target_phase stay equal without phasemod, so the pull term is the identity).
// The engine evaluates that closed form:
//   * lanes are TIME (16-sample chunks of a 1024-sample tile); a wave owns a slice of one
//     voice's overtones, accumulates sum_j c_j sin(...) per sample in registers, then
//     multiplies by the voice envelope amp(t) = act + a^t (amp0 - act) (closed-form seed,
//     one-pole recurrence inside the chunk);
//   * chunks where the frequency transient still moves the phase (|D| s^t > 2^-60) are
//     evaluated per sample (sincospi); all others seed a phasor by w = e^{2 pi i A} per
//     16-sample chunk (seed = z(t0) (w^16)^p (w^256)^r from per-partial tables,
//     z(t0+1024) = z(t0) w^1024) and run the two-term sine recurrence inside the chunk;
//   * time segments need no carry (closed form), so small banks still fill the chip;
//   * a wave takes tpw tasks in turn (the envelope applied per task); the waves' mixes are summed
//     through LDS and written once per workgroup: straight to the output when one group of
//     workgroups covers every task (long calls), else as group rows a second kernel sums.
// PI: the reference's truncated PI enters only through sin(2 PI frac(phi)); using 2 pi
// changes the argument by <= 4.2e-13 rad.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "hz_common.h"
#include "hz_minimizer.h"
#include "hz_mix.h"
#include "hz_mixplan.h"

namespace {

using namespace hz::mix;   // kWaves, kMaxPerWave, kPad, cmul, lane_d and the end-of-tile / slab reductions

constexpr int kL = 32;   // samples per lane chunk (16: 1.28 ms per C3 launch; 32 halves the per-chunk
                         // seed / table / transient-check work per sample)
constexpr int kTile = tile_len(kL);

// per-partial record (depends only on the target frequency and the output weight):
// A = f_target/SR (cycles/sample), c (output weight), W1 = e^{2 pi i A},
// T1[p] = W1^(kL p) (p < 16), T2[r] = W1^(16 kL r) (r < 4), WT = W1^(64 kL)
struct PRec {
    static constexpr int A = 0, C = 1;
    static constexpr int W1 = 2;
    static constexpr int T1 = 4;
    static constexpr int T2 = T1 + 32;
    static constexpr int WT = T2 + 8;
    static constexpr int SIZE = 48;
};

// one wave task: a slice of one voice's partials
struct Task {
    int first;   // first partial (local index)
    int count;   // partials in the slice
    int voice;   // voice slot (amp arrays)
    int pad;
};

struct AddArgs {
    const Task* tasks;
    const double* phi;     // [P] oscillator phase at call start
    const double* f;       // [P] oscillator frequency at call start
    const double* ft;      // [P] target frequency
    const double* amp0;    // [V] envelope value at call start
    const double* act;     // [V] envelope target (Minimizer::active)
    const double* c0;      // [P] output weights of the call's first sample, or null when
                           // equal to the records' (Sinusoids::operator() runs before tick()
                           // applies a decaymod, sinusoids.h:34-57)
    double* partial;       // [G][n_pad]: one row per group (G > 1), or the output itself (G == 1)
    double scale;          // (G == 1) the output scale, applied here
    long n, n_pad, seg_len;
    int ntasks, nseg;
    int tpw;               // tasks per wave: workgroup g's wave w takes tasks (g tpw + k) kWaves + w
    double a;              // attack smoothing coefficient
    double s;              // oscillator stiffness
};

// frac(phi0 + A t + D (1 - s^t)) with the A t product kept exact (fma residual)
__device__ __forceinline__ double phase_at(double phi0, double A, double D, double s, double t, double st) {
    const double p = A * t;
    const double e = fma(A, t, -p);
    double q = p - floor(p);
    q += phi0 + e + D * (1.0 - st);
    return q - floor(q);
}

// kL samples of one partial in its frequency transient, exact closed form per sample, added to
// the LDS column `col` (stride kPad); out of line so sinpi's registers stay out of the main loop
// (scaled by the voice envelope amp(t), advanced per sample as in the mix)
__device__ __attribute__((noinline)) void add_transient(double* col, double phi0, double A, double c, double D,
                                                        double s, long tc, double st, double amp, double ea,
                                                        double act) {
    for (int j = 0; j < kL; ++j) {
        const double ph = phase_at(phi0, A, D, s, (double)(tc + j), st);
        col[j * kPad] = fma(amp, c * sinpi(2.0 * ph), col[j * kPad]);
        st *= s;
        amp = fma(ea, amp, (1.0 - ea) * act);
    }
}

__global__ __launch_bounds__(64 * kWaves) void add_mix_kernel(const double* __restrict__ rec, AddArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* part = lds;                           // [W][kL][kPad] the waves' mix rows
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p16 = lane & 15, r4 = lane >> 4;
    const int seg = blockIdx.y;
    const long seg_t0 = (long)seg * a.seg_len;
    const long seg_end = min(seg_t0 + a.seg_len, a.n);
    const int ntiles = (int)((seg_end - seg_t0 + kTile - 1) / kTile);
    const double a_lane = pow(a.a, (double)(kL * lane));
    double a_t = seg_t0 ? pow(a.a, (double)seg_t0) : 1.0;
    const double inv_trans = 1.0 / ((1.0 - a.s) * hz::kSR);
    double* my = part + wave * (kL * kPad);

    for (int tile = 0; tile < ntiles; ++tile) {
        const long t0 = seg_t0 + (long)tile * kTile;
        const long tc = t0 + (long)kL * lane;
        const double s_tc = pow(a.s, (double)tc);  // transient decay at this chunk
        // the wave's mix of the tile accumulates in its LDS rows (registers hold one task's)
#pragma unroll
        for (int j = 0; j < kL; ++j) my[j * kPad + lane] = 0.0;
        for (int k = 0; k < a.tpw; ++k) {
            const int task = (blockIdx.x * a.tpw + k) * kWaves + wave;
            if (task >= a.ntasks) break;
            const Task tk = a.tasks[task];
            const double amp0 = a.amp0[tk.voice], act = a.act[tk.voice];
            // tile-start phasor of partial `lane` of the task (lanes in parallel; read below with
            // readlane; transient taken as complete -- chunks where it is not are evaluated per sample)
            double zr0 = 0.0, zi0 = 0.0;
            if (lane < tk.count) {
                const int pi = tk.first + lane;
                const double* rr = rec + (long)pi * PRec::SIZE;
                const double D = (a.f[pi] - a.ft[pi]) * inv_trans;
                const double ph = phase_at(a.phi[pi], rr[PRec::A], D, a.s, (double)t0, 0.0);
                sincospi(2.0 * ph, &zi0, &zr0);
            }
            double acc[kL];
#pragma unroll
            for (int j = 0; j < kL; ++j) acc[j] = 0.0;
            bool trans = false;
            // the next partial's record and frequency pair are fetched one iteration ahead (their
            // global latency runs under this partial's recurrence)
            struct Fetch {
                double c, D, t1r, t1i, t2r, t2i, w1r, w1i;
            };
            auto fetch = [&](int q, Fetch& p) {
                const int pi = tk.first + q;
                const double* rr = rec + (long)pi * PRec::SIZE;
                p.c = rr[PRec::C];
                p.D = (a.f[pi] - a.ft[pi]) * inv_trans;
                p.t1r = rr[PRec::T1 + 2 * p16];
                p.t1i = rr[PRec::T1 + 2 * p16 + 1];
                p.t2r = rr[PRec::T2 + 2 * r4];
                p.t2i = rr[PRec::T2 + 2 * r4 + 1];
                p.w1r = rr[PRec::W1];
                p.w1i = rr[PRec::W1 + 1];
            };
            Fetch cur;
            if (tk.count) fetch(0, cur);
            for (int q = 0; q < tk.count; ++q) {
                const int pi = tk.first + q;
                Fetch nxt;
                if (q + 1 < tk.count) fetch(q + 1, nxt);
                const double c = cur.c, D = cur.D;
                const double sr = lane_d(zr0, q), si = lane_d(zi0, q);
                if (a.c0 && tc == 0) acc[0] = fma(a.c0[pi] - c, sinpi(2.0 * a.phi[pi]), acc[0]);
                if (fabs(D) * s_tc > 0x1p-60) {
                    trans = true;   // frequency transient: the second pass below
                } else {
                    // seed z(tc) = z(t0) w^(kL p) w^(16 kL r); inside the chunk the sines follow the
                    // two-term recurrence sin((k+1) th) = 2 cos th sin(k th) - sin((k-1) th): one
                    // FMA per sample instead of a complex multiply (4), re-seeded every kL samples
                    // (error <= kL eps / |sin th| of the partial's amplitude)
                    double ur, ui, zr, zi;
                    cmul(cur.t1r, cur.t1i, cur.t2r, cur.t2i, ur, ui);
                    cmul(sr, si, ur, ui, zr, zi);
                    const double w1r = cur.w1r, w1i = cur.w1i;
                    const double c2 = 2.0 * w1r;
                    double s0 = zi, s1 = fma(zr, w1i, zi * w1r);
                    acc[0] = fma(c, s0, acc[0]);
                    acc[1] = fma(c, s1, acc[1]);
#pragma unroll
                    for (int j = 2; j < kL; ++j) {
                        const double s2 = fma(c2, s1, -s0);
                        acc[j] = fma(c, s2, acc[j]);
                        s0 = s1;
                        s1 = s2;
                    }
                }
                cur = nxt;
            }
            // voice envelope amp(t) = act + a^t (amp0 - act), advanced per sample
            double amp = act + (a_lane * a_t) * (amp0 - act);
            // the settled partials, then (chunks still inside a frequency transient: the first tiles
            // of a retune) the exact closed form per sample, out of line so sinpi's registers do not
            // spill the accumulators
            const double amp_c = amp;
#pragma unroll
            for (int j = 0; j < kL; ++j) {
                my[j * kPad + lane] = fma(amp, acc[j], my[j * kPad + lane]);
                amp = fma(a.a, amp, (1.0 - a.a) * act);
            }
            if (__builtin_amdgcn_ballot_w64(trans) != 0) {
                for (int q = 0; q < tk.count; ++q) {
                    const int pi = tk.first + q;
                    const double* rr = rec + (long)pi * PRec::SIZE;
                    const double D = (a.f[pi] - a.ft[pi]) * inv_trans;
                    if (fabs(D) * s_tc > 0x1p-60)
                        add_transient(my + lane, a.phi[pi], rr[PRec::A], rr[PRec::C], D, a.s, tc, s_tc, amp_c, a.a, act);
                }
            }
        }
        const bool direct = gridDim.x == 1;   // one group: the output itself, scaled
        tile_reduce<kL, 1>(part, t0, a.n, [&](long t, const double (&s0)[1]) {
            if (direct) a.partial[t] = s0[0] * a.scale;
            else a.partial[(long)blockIdx.x * a.n_pad + t] = s0[0];
        });
        a_t *= pow(a.a, (double)kTile);
    }
}

// end-of-call oscillator state for the partials of alive voices:
//   phi <- phi(n), f <- ft + s^n (f0 - ft)
__global__ __launch_bounds__(64) void add_advance_kernel(const double* __restrict__ rec, const Task* tasks,
                                                         int ntasks, long n, double s, double s_n,
                                                         const double* __restrict__ ft, double* phi, double* f) {
    const int task = blockIdx.x;
    if (task >= ntasks) return;
    const Task tk = tasks[task];
    const double inv_trans = 1.0 / ((1.0 - s) * hz::kSR);
    for (int q = threadIdx.x; q < tk.count; q += blockDim.x) {
        const int p = tk.first + q;
        const double* rr = rec + (long)p * PRec::SIZE;
        const double D = (f[p] - ft[p]) * inv_trans;
        phi[p] = phase_at(phi[p], rr[PRec::A], D, s, (double)n, s_n);
        f[p] = ft[p] + s_n * (f[p] - ft[p]);
    }
}

void fill_tables(double A, double* rec) {
    using C = std::complex<long double>;
    const long double th = 2.0L * 3.141592653589793238462643383279502884L * (long double)A;
    const C w(std::cos(th), std::sin(th));
    rec[PRec::W1] = (double)w.real();
    rec[PRec::W1 + 1] = (double)w.imag();
    C wl(1, 0);
    for (int k = 0; k < kL; ++k) wl *= w;
    C acc(1, 0);
    for (int p = 0; p < 16; ++p) {
        rec[PRec::T1 + 2 * p] = (double)acc.real();
        rec[PRec::T1 + 2 * p + 1] = (double)acc.imag();
        acc *= wl;
    }
    const C w256 = acc;   // W1^(16 kL)
    acc = C(1, 0);
    for (int r = 0; r < 4; ++r) {
        rec[PRec::T2 + 2 * r] = (double)acc.real();
        rec[PRec::T2 + 2 * r + 1] = (double)acc.imag();
        acc *= w256;
    }
    rec[PRec::WT] = (double)acc.real();
    rec[PRec::WT + 1] = (double)acc.imag();
}

long double mtofl(long double m) { return 440.0L * powl(2.0L, (m - 69) / 12); }

}  // namespace

// ---------------------------------------------------------------------------
// shared engine: V voices x OL local overtones (overtones [o0, o0 + OL) of O)
// ---------------------------------------------------------------------------
struct PhaseBank {
    hz::Stream stream;
    int V = 1, O = 1, o0 = 0, OL = 1, device = 0;
    double s = 0;      // oscillator stiffness
    double a = 0;      // envelope smoothing (Additive attack); 0 for Sinusoids
    std::vector<double> ft;      // [V*OL] target frequency (Hz)
    std::vector<double> c;       // [V*OL] output weight
    std::vector<double> c_first; // weights of the next call's first sample
    hz::DevBuf<double> d_c0;
    std::vector<double> amp, act;
    std::vector<char> alive;
    double scale = 1.0;
    // device
    hz::DevBuf<double> d_rec, d_phi, d_f, d_ft, d_amp, d_act, d_partial, d_out;
    hz::DevBuf<Task> d_tasks;
    std::vector<double> h_rec;
    std::vector<char> dirty;     // per voice: records need rebuilding
    std::vector<Task> tasks;
    int target_groups = 256;
    bool prof = false;
    hz::ProfEvents ev;
    long launches = 0;
    // Per-sample calls (operator() / tick(): fills shorter than kLookMin) are served from a
    // speculative block: the next kLook samples rendered at once from a snapshot of the state
    // (the outputs need no input: src/additive.h:38-62, src/sinusoids.h:34-57), consumed one by
    // one; a setter or a longer fill first rolls the engine back to the consumed position
    // (snapshot restored, exactly that many samples re-rendered), so every sample is the one the
    // per-sample sequence produces.
    static constexpr long kLook = 1024, kLookMin = 64;
    hz::PinBuf<double> la_buf;         // pinned [kLook] rendered outputs
    long la_n = 0, la_pos = 0;         // rendered / consumed samples of the speculative block
    hz::DevBuf<double> d_phi_snap, d_f_snap;
    std::vector<double> amp_snap, c_first_snap;
    std::vector<char> alive_snap;
    long la_blocks = 0, la_rollbacks = 0;

    int init(int V_, int O_, int o0_, int OL_, double s_, double a_, int dev) {
        V = V_;
        O = O_;
        o0 = o0_;
        OL = OL_;
        s = s_;
        a = a_;
        device = dev;
        const size_t P = (size_t)V * OL;
        ft.assign(P, 0.0);
        c.assign(P, 0.0);
        c_first.assign(P, 0.0);
        amp.assign(V, 0.0);
        act.assign(V, 0.0);
        alive.assign(V, 0);
        dirty.assign(V, 1);
        h_rec.assign(P * PRec::SIZE, 0.0);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            target_groups = prop.multiProcessorCount;
        HZ_TRY(stream.create());
        HZ_TRY(d_rec.reserve(P * PRec::SIZE));
        HZ_TRY(d_phi.reserve(P));
        HZ_TRY(d_f.reserve(P));
        HZ_TRY(d_ft.reserve(P));
        HZ_TRY(d_amp.reserve(V));
        HZ_TRY(d_act.reserve(V));
        HZ_TRY(d_c0.reserve(P));
        HZ_TRY_HIP(hipMemset(d_phi, 0, sizeof(double) * P));
        HZ_TRY_HIP(hipMemset(d_f, 0, sizeof(double) * P));
        return HZ_OK;
    }

    void release() {   // quiet, before the handle is deleted
        (void)hipSetDevice(device);
        (void)stream.sync();
    }

    // render n samples into d_out (device), then advance all state
    int render(double* d_dst, long n) {
        if (n <= 0) return HZ_OK;
        HZ_TRY_HIP(hipSetDevice(device));
        const size_t P = (size_t)V * OL;
        // records of voices whose targets changed (note events); state stays on the device
        tasks.clear();
        const int per_wave = std::min(kMaxPerWave, std::max(1, OL));
        bool any_dirty = false;
        for (int v = 0; v < V; ++v) {
            if (dirty[v]) {
                for (int j = 0; j < OL; ++j) {
                    const size_t p = (size_t)v * OL + j;
                    double* r = &h_rec[p * PRec::SIZE];
                    r[PRec::A] = ft[p] / hz::kSR;
                    r[PRec::C] = c[p];
                    fill_tables(r[PRec::A], r);
                }
                HZ_TRY_HIP(hipMemcpyAsync(d_rec + (size_t)v * OL * PRec::SIZE, &h_rec[(size_t)v * OL * PRec::SIZE],
                                          sizeof(double) * OL * PRec::SIZE, hipMemcpyHostToDevice, stream));
                dirty[v] = 0;
                any_dirty = true;
            }
            if (!(alive[v] || act[v] != 0.0)) continue;  // never-sounded voices are skipped and frozen
            for (int j0 = 0; j0 < OL; j0 += per_wave)
                tasks.push_back(Task{v * OL + j0, std::min(per_wave, OL - j0), v, 0});
        }
        if (any_dirty)
            HZ_TRY_HIP(hipMemcpyAsync(d_ft, ft.data(), sizeof(double) * P, hipMemcpyHostToDevice, stream));
        HZ_TRY_HIP(hipMemcpyAsync(d_amp, amp.data(), sizeof(double) * V, hipMemcpyHostToDevice, stream));
        HZ_TRY_HIP(hipMemcpyAsync(d_act, act.data(), sizeof(double) * V, hipMemcpyHostToDevice, stream));
        const int ntasks = (int)tasks.size();
        if (ntasks > 0) {
            HZ_TRY(d_tasks.reserve(ntasks));
            HZ_TRY_HIP(hipMemcpyAsync(d_tasks, tasks.data(), sizeof(Task) * ntasks, hipMemcpyHostToDevice, stream));
        }
        const bool c0_differs = c_first != c;
        if (c0_differs)
            HZ_TRY_HIP(hipMemcpyAsync(d_c0, c_first.data(), sizeof(double) * P, hipMemcpyHostToDevice, stream));
        HZ_TRY_HIP(hipStreamSynchronize(stream));  // pageable host sources above are reused

        hipEvent_t* e = nullptr;
        if (prof) {
            HZ_TRY(ev.take(2, &e));
            HZ_TRY_HIP(hipEventRecord(e[0], stream));
        }
        if (ntasks == 0) {
            HZ_TRY_HIP(hipMemsetAsync(d_dst, 0, sizeof(double) * n, stream));
        } else {
            // groups: one task per wave by default.  Fewer groups (a wave taking several tasks in turn)
            // cut the partial rows -- one group writes the output directly, 146 -> 67 MB counted per
            // C3 step -- but measured slower (C3: 19 groups 1.19 ms, 4: 1.46, 2: 1.86; one group for the
            // long call 1.47 ms: every workgroup then streams all 3.7 MB of partial records per tile)
            // (tpw is fixed at 1 here; the kernel's loop over a wave's tasks stays as it is)
            const int G = (ntasks + kWaves - 1) / kWaves, tpw = 1;
            const hz::MixPlan mp = hz::mix_plan(G, n, kTile, target_groups);
            const size_t need = G > 1 ? (size_t)G * mp.n_pad : 1;
            HZ_TRY(d_partial.reserve(need));
            const size_t lds = sizeof(double) * plane_len(kL);
            HZ_TRY(hz::allow_lds(device, (const void*)add_mix_kernel, lds));
            AddArgs args;
            args.tasks = d_tasks;
            args.phi = d_phi;
            args.f = d_f;
            args.ft = d_ft;
            args.amp0 = d_amp;
            args.act = d_act;
            args.c0 = c0_differs ? d_c0 : nullptr;
            args.partial = G > 1 ? d_partial : d_dst;
            args.scale = scale;
            args.tpw = tpw;
            args.n = n;
            args.n_pad = mp.n_pad;
            args.seg_len = mp.seg_len;
            args.ntasks = ntasks;
            args.nseg = (int)mp.nseg;
            args.a = a;
            args.s = s;
            hipLaunchKernelGGL(add_mix_kernel, dim3(G, (unsigned)mp.nseg), dim3(64 * kWaves), lds, stream,
                               (const double*)d_rec, args);
            HZ_TRY_HIP(hipGetLastError());
            if (G > 1) {
                slab_reduce(stream, (const double*)d_partial, mp.n_pad, G, n, SlabScale{scale, d_dst});
                HZ_TRY_HIP(hipGetLastError());
            }
            const double s_n = (double)powl((long double)s, (long double)n);
            hipLaunchKernelGGL(add_advance_kernel, dim3(ntasks), dim3(64), 0, stream, (const double*)d_rec,
                               (const Task*)d_tasks, ntasks, n, s, s_n, (const double*)d_ft, d_phi, d_f);
            HZ_TRY_HIP(hipGetLastError());
        }
        if (e) HZ_TRY_HIP(hipEventRecord(e[1], stream));
        launches += prof ? 1 : 0;
        c_first = c;
        // envelopes (V scalars): closed form, alive is sticky (a released envelope decays
        // to a denormal fixed point > 0 in the reference and never reaches 0)
        const long double an = powl((long double)a, (long double)n);
        for (int v = 0; v < V; ++v) {
            if (act[v] != 0.0) alive[v] = 1;
            if (!alive[v]) continue;
            amp[v] = (double)((long double)act[v] + an * ((long double)amp[v] - (long double)act[v]));
        }
        return HZ_OK;
    }

    // roll the engine back to the consumed position of the speculative block (before any setter,
    // any longer fill or a device fill)
    int settle() {
        if (la_pos < la_n) {
            const size_t P = (size_t)V * OL;
            HZ_TRY_HIP(hipMemcpyAsync(d_phi, d_phi_snap, sizeof(double) * P, hipMemcpyDeviceToDevice, stream));
            HZ_TRY_HIP(hipMemcpyAsync(d_f, d_f_snap, sizeof(double) * P, hipMemcpyDeviceToDevice, stream));
            amp = amp_snap;
            alive = alive_snap;
            c_first = c_first_snap;
            const long m = la_pos;
            la_n = la_pos = 0;
            ++la_rollbacks;
            if (m > 0) HZ_TRY(render_scratch(m));
        }
        la_n = la_pos = 0;
        return HZ_OK;
    }

    int render_scratch(long n) {
        HZ_TRY(d_out.reserve(n));
        return render(d_out, n);
    }

    // a new speculative block: snapshot, render kLook samples, outputs to pinned memory
    int look_ahead() {
        const size_t P = (size_t)V * OL;
        if (!la_buf) {
            HZ_TRY(la_buf.reserve(kLook));
            HZ_TRY(d_phi_snap.reserve(P));
            HZ_TRY(d_f_snap.reserve(P));
        }
        HZ_TRY_HIP(hipMemcpyAsync(d_phi_snap, d_phi, sizeof(double) * P, hipMemcpyDeviceToDevice, stream));
        HZ_TRY_HIP(hipMemcpyAsync(d_f_snap, d_f, sizeof(double) * P, hipMemcpyDeviceToDevice, stream));
        amp_snap = amp;
        alive_snap = alive;
        c_first_snap = c_first;
        HZ_TRY(d_out.reserve(kLook));
        HZ_TRY(render(d_out, kLook));
        HZ_TRY_HIP(hipMemcpyAsync(la_buf, d_out, sizeof(double) * kLook, hipMemcpyDeviceToHost, stream));
        HZ_TRY_HIP(hipStreamSynchronize(stream));
        la_n = kLook;
        la_pos = 0;
        ++la_blocks;
        return HZ_OK;
    }

    int fill_host(double* out, long n) {
        if (n <= 0) return HZ_OK;
        if (n < kLookMin) {   // per-sample calls: from the speculative block
            for (long i = 0; i < n; ++i) {
                if (la_pos == la_n) HZ_TRY(look_ahead());
                out[i] = la_buf[la_pos++];
            }
            return HZ_OK;
        }
        HZ_TRY(settle());
        HZ_TRY(d_out.reserve(n));
        HZ_TRY(render(d_out, n));
        HZ_TRY_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
        HZ_TRY_HIP(hipStreamSynchronize(stream));
        return HZ_OK;
    }
};

// ---------------------------------------------------------------------------
// Additive<double>  (src/additive.h:11-71 + Minimizer note API, src/minimizer.h:111-181)
// ---------------------------------------------------------------------------
struct hz_add : hz::MinNotes {   // the note layer: position covers all overtones; with physics on, the
                                 // device copy (phys.d_x) is the one that moves
    PhaseBank bank;
    double decay = 0, norm = 1;
    // Minimizer::physics() (hz_minimizer.hip).  The device state exists from the first physics call
    // on; before it no particle has moved (velocity 0) and the host mirrors above are complete.
    struct Physics {
        enum { OFF, MANUAL, PERIODIC };
        int mode = OFF;          // MANUAL: hz_add_physics() steps, PERIODIC: hz_add_physics_every(period > 0)
        int law = 0, period = 0;
        long T = 0;              // samples since the period was set
        bool ready = false;
        int single_max = kSingleMax, tile = kStepTile;
        static constexpr int kSingleLimit = 1024, kSingleMax = 256, kStepTile = 256;
        // a call is rendered in pieces of at most kMaxSamples samples whose position rows
        // ([steps + 1][V O] doubles) fit kMaxRowBytes
        static constexpr long kMaxSamples = 4096;
        static constexpr size_t kMaxRowBytes = (size_t)32 << 20;
        hz::DevBuf<double> d_x, d_v, d_eq, d_guide, d_c, d_rows, d_amp, d_partial;
        std::vector<double> amp;   // [n + 1][V] envelope rows of the piece being rendered
        hz::ProfEvents ev;   // profile: 3 per piece (start, physics done, audio done)
    } phys;
};

namespace {

int add_check(hz_add* h) {
    return hz::check_handle(h ? &h->bank : nullptr, "hz_add");   // (the bank has the device)
}

// Additive::tick's freqmod(mtof(particle position)) for the local overtones of voice v
void add_retarget(hz_add* h, int v) {
    PhaseBank& b = h->bank;
    b.dirty[v] = 1;
    for (int jl = 0; jl < b.OL; ++jl) {
        const int j = b.o0 + jl;
        b.ft[(size_t)v * b.OL + jl] = (double)mtofl((long double)h->position[(size_t)v * h->O + j]);
    }
}

// ---- Minimizer::physics() (kernels in hz_minimizer.hip) ----------------------------------

int phys_law_check(hz_add* h, int law) {
    if (!h) {
        hz::set_error("null hz_add handle");
        return HZ_E_INVALID;
    }
    if (law != HZ_GRAV_TRUNC && law != HZ_GRAV_FABS) {
        hz::set_error("gravity law %d: HZ_GRAV_TRUNC or HZ_GRAV_FABS (there is no default)", law);
        return HZ_E_INVALID;
    }
    if (h->bank.OL != h->O) {
        hz::set_error("physics on an overtone shard: every partial is needed");
        return HZ_E_UNSUPPORTED;
    }
    return HZ_OK;
}

hz::MinParams phys_params(const hz_add* h) {
    return hz::min_params(h->V, h->O, 0.1 * 50000, 1 * 50000);   // minimizer.h:40, 45
}

// device rows of one voice after request(): position, equilibrium, velocity 0
int phys_upload_voice(hz_add* h, int v) {
    hz_add::Physics& ph = h->phys;
    const size_t O = h->O, at = (size_t)v * O;
    hipStream_t st = h->bank.stream;
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_x + at, &h->position[at], sizeof(double) * O, hipMemcpyHostToDevice, st));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_eq + at, &h->equilibrium[at], sizeof(double) * O, hipMemcpyHostToDevice, st));
    HZ_TRY_HIP(hipMemsetAsync(ph.d_v + at, 0, sizeof(double) * O, st));
    HZ_TRY_HIP(hipStreamSynchronize(st));   // pageable sources
    return HZ_OK;
}

// the device state, from the host mirrors (nothing has moved before the first physics call)
int phys_ensure(hz_add* h) {
    hz_add::Physics& ph = h->phys;
    if (ph.ready) return HZ_OK;
    const size_t P = (size_t)h->V * h->O;
    hipStream_t st = h->bank.stream;
    HZ_TRY(ph.d_x.reserve(P));
    HZ_TRY(ph.d_v.reserve(P));
    HZ_TRY(ph.d_eq.reserve(P));
    HZ_TRY(ph.d_c.reserve(P));
    HZ_TRY(ph.d_guide.reserve(h->V));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_x, h->position.data(), sizeof(double) * P, hipMemcpyHostToDevice, st));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_eq, h->equilibrium.data(), sizeof(double) * P, hipMemcpyHostToDevice, st));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_c, h->bank.c.data(), sizeof(double) * P, hipMemcpyHostToDevice, st));
    HZ_TRY_HIP(hipMemsetAsync(ph.d_v, 0, sizeof(double) * P, st));
    HZ_TRY_HIP(hipStreamSynchronize(st));
    ph.ready = true;
    return HZ_OK;
}

// `steps` physics steps on the device state: rows[0] <- x, kernels write rows 1..steps, x <- rows[steps]
int phys_steps(hz_add* h, int steps) {
    hz_add::Physics& ph = h->phys;
    const size_t P = (size_t)h->V * h->O;
    hipStream_t st = h->bank.stream;
    HZ_TRY(ph.d_rows.reserve((size_t)(steps + 1) * P));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_rows, ph.d_x, sizeof(double) * P, hipMemcpyDeviceToDevice, st));
    if (steps <= 0) return HZ_OK;
    HZ_TRY(hz::min_run(st, phys_params(h), ph.law, steps, (long)P <= ph.single_max, ph.tile, ph.d_rows, ph.d_v,
                       ph.d_eq, h->bank.d_act, ph.d_guide));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_x, ph.d_rows + (size_t)steps * P, sizeof(double) * P, hipMemcpyDeviceToDevice, st));
    return HZ_OK;
}

// envelope rows of n samples, op for op (additive.h:40-41): row 0 = amplitudes now, row t + 1 after
// sample t's tick
void phys_envelope(const PhaseBank& b, long n, std::vector<double>& rows) {
#pragma clang fp contract(off)
    const int V = b.V;
    rows.resize((size_t)(n + 1) * V);
    for (int v = 0; v < V; ++v) rows[v] = b.amp[v];
    for (long t = 0; t < n; ++t)
        for (int v = 0; v < V; ++v)
            rows[(size_t)(t + 1) * V + v] = (1 - b.a) * b.act[v] + b.a * rows[(size_t)t * V + v];
}

// active / guide / envelope rows to the device (pageable sources: synchronised)
int phys_upload_call(hz_add* h, long n_rows) {
    hz_add::Physics& ph = h->phys;
    PhaseBank& b = h->bank;
    HZ_TRY(ph.d_amp.reserve((size_t)n_rows * b.V));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_amp, ph.amp.data(), sizeof(double) * n_rows * b.V, hipMemcpyHostToDevice, b.stream));
    HZ_TRY_HIP(hipMemcpyAsync(b.d_act, b.act.data(), sizeof(double) * b.V, hipMemcpyHostToDevice, b.stream));
    HZ_TRY_HIP(hipMemcpyAsync(ph.d_guide, h->guide.data(), sizeof(double) * b.V, hipMemcpyHostToDevice, b.stream));
    HZ_TRY_HIP(hipStreamSynchronize(b.stream));
    return HZ_OK;
}

// the audio of n samples over position rows already on the device; d_dst [n]
int phys_audio(hz_add* h, double* d_dst, long n, const double* rows, int period, long T0, int advance) {
    hz_add::Physics& ph = h->phys;
    PhaseBank& b = h->bank;
    const int P = h->V * h->O, G = hz::add_track_groups(P);
    HZ_TRY(ph.d_partial.reserve((size_t)G * n));
    hz::TrackArgs a;
    a.rows = rows;
    a.amp = ph.d_amp;
    a.act = b.d_act;
    a.c = ph.d_c;
    a.phi = b.d_phi;
    a.f = b.d_f;
    a.partial = ph.d_partial;
    a.n = n;
    a.n_pad = n;
    a.T0 = T0;
    a.period = period;
    a.P = P;
    a.V = h->V;
    a.O = h->O;
    a.s = b.s;
    a.advance = advance;
    HZ_TRY(hz::add_track(b.stream, a));
    slab_reduce(b.stream, (const double*)ph.d_partial, n, G, n, SlabScale{b.scale, d_dst});
    HZ_TRY_HIP(hipGetLastError());
    return HZ_OK;
}

// n x { out[t] = operator()(); if (T >= period && T % period == 0) physics(); tick(); T++; } into
// d_dst (device), in pieces whose position rows stay within Physics::kMaxRowBytes
int phys_render(hz_add* h, double* d_dst, long n) {
    hz_add::Physics& ph = h->phys;
    PhaseBank& b = h->bank;
    if (n <= 0) return HZ_OK;
    HZ_TRY(b.settle());
    HZ_TRY(phys_ensure(h));
    const size_t P = (size_t)h->V * h->O;
    const int period = ph.mode == hz_add::Physics::PERIODIC ? ph.period : 0;
    const long max_steps = std::max<long>(1, (long)(hz_add::Physics::kMaxRowBytes / (sizeof(double) * P)) - 1);
    for (long done = 0; done < n;) {
        long m = std::min(n - done, hz_add::Physics::kMaxSamples);
        if (period > 0) m = std::min(m, max_steps * period);
        int steps = 0;
        for (long t = 0; t < m && period > 0; ++t)
            steps += (ph.T + t >= period && (ph.T + t) % period == 0) ? 1 : 0;
        phys_envelope(b, m, ph.amp);
        HZ_TRY(phys_upload_call(h, m + 1));
        hipEvent_t* e = nullptr;
        if (b.prof) {
            HZ_TRY(ph.ev.take(3, &e));
            HZ_TRY_HIP(hipEventRecord(e[0], b.stream));
        }
        HZ_TRY(phys_steps(h, steps));
        if (e) HZ_TRY_HIP(hipEventRecord(e[1], b.stream));
        HZ_TRY(phys_audio(h, d_dst + done, m, ph.d_rows, period, ph.T, 1));
        if (e) HZ_TRY_HIP(hipEventRecord(e[2], b.stream));
        for (int v = 0; v < b.V; ++v) {
            b.amp[v] = ph.amp[(size_t)m * b.V + v];
            if (b.act[v] != 0.0 || b.amp[v] != 0.0) b.alive[v] = 1;
        }
        if (period > 0) ph.T += m;
        done += m;
    }
    return HZ_OK;
}

}  // namespace

extern "C" {

int hz_add_create_shard(int voices, int overtones, int o_begin, int o_count, double decay, double harmonicity,
                        double k, int device, hz_add** out) {
    if (!out || voices <= 0 || overtones <= 0 || o_begin < 0 || o_count <= 0 || o_begin + o_count > overtones) {
        hz::set_error("hz_add_create: invalid arguments");
        return HZ_E_INVALID;
    }
    *out = nullptr;
    HZ_TRY(hz::select_device(device));
    hz_add* h = new (std::nothrow) hz_add();
    if (!h) return HZ_E_ALLOC;
    h->notes_init(voices, overtones, harmonicity);
    h->decay = decay;
    // additive.h:27 normalization; oscillators are Oscillator(0, 0, 0.0001) (35)
    h->norm = decay != 1 ? (1 - std::pow(decay, overtones)) / (1 - decay) : overtones;
    int rc = h->bank.init(voices, overtones, o_begin, o_count, hz::relaxation(0.0001), hz::relaxation(k), device);
    if (rc != HZ_OK) {
        hz_add_destroy(h);
        return rc;
    }
    for (int v = 0; v < voices; ++v)
        for (int jl = 0; jl < o_count; ++jl)
            h->bank.c[(size_t)v * o_count + jl] = std::pow(decay, o_begin + jl);
    h->bank.c_first = h->bank.c;
    h->bank.scale = 1.0 / (voices * h->norm);
    *out = h;
    return HZ_OK;
}

int hz_add_create(int voices, int overtones, double decay, double harmonicity, double k, int device, hz_add** out) {
    return hz_add_create_shard(voices, overtones, 0, overtones, decay, harmonicity, k, device, out);
}

int hz_add_destroy(hz_add* h) {
    if (!h) return HZ_OK;
    h->bank.release();
    delete h;
    return HZ_OK;
}

// request(fundamental, amplitude)  minimizer.h:111-158: the voice's particles (mass 1, v = a = 0) and
// spring equilibria are re-initialised; with physics on, on the device too.
int hz_add_request(hz_add* h, double fundamental, double amplitude, int* voice_out) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY(add_check(h));
    HZ_TRY(h->bank.settle());   // a speculative block rolls back to the consumed sample first
    const int voice = h->request(fundamental, amplitude);
    h->bank.act[voice] = amplitude;
    add_retarget(h, voice);
    if (h->phys.ready) HZ_TRY(phys_upload_voice(h, voice));   // particles re-initialised: v = 0
    if (voice_out) *voice_out = voice;
    return HZ_OK;
}

// release(voice) minimizer.h:161-172 (voice < 0: all)
int hz_add_release(hz_add* h, int voice) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY(add_check(h));
    HZ_TRY(h->bank.settle());
    h->release(voice);
    for (int i = 0; i < h->V; ++i)
        if (voice < 0 || i == voice) h->bank.act[i] = 0;
    return HZ_OK;
}

int hz_add_makenote(hz_add* h, double pitch, double amplitude, int* voice_out) {   // minimizer.h:174-179
    if (!h) return HZ_E_INVALID;
    int v = -1;
    HZ_TRY(hz_add_request(h, hz::MinNotes::mtof(pitch), amplitude, &v));
    if (v >= 0) h->pitches[v] = pitch;
    if (voice_out) *voice_out = v;
    return HZ_OK;
}

int hz_add_endnote(hz_add* h, double pitch) {   // minimizer.h:182-187
    if (!h) return HZ_E_INVALID;
    for (int j = 0; j < h->V; ++j)
        if (h->pitches[j] == pitch) hz_add_release(h, j);
    return HZ_OK;
}

// n x { out[t] = operator()(); tick(); }   additive.h:38-62
int hz_add_fill(hz_add* h, double* out, size_t n) {
    HZ_TRY(add_check(h));
    if (n && !out) return HZ_E_INVALID;
    if (h->phys.mode != hz_add::Physics::OFF) {   // served directly, whatever the length
        if (!n) return HZ_OK;
        PhaseBank& b = h->bank;
        HZ_TRY(b.d_out.reserve(n));
        HZ_TRY(phys_render(h, b.d_out, (long)n));
        HZ_TRY_HIP(hipMemcpyAsync(out, b.d_out, sizeof(double) * n, hipMemcpyDeviceToHost, b.stream));
        HZ_TRY_HIP(hipStreamSynchronize(b.stream));
        return HZ_OK;
    }
    return h->bank.fill_host(out, (long)n);
}

int hz_add_fill_device(hz_add* h, double* d_out, size_t n) {
    HZ_TRY(add_check(h));
    if (n && !d_out) return HZ_E_INVALID;
    if (h->phys.mode != hz_add::Physics::OFF) return phys_render(h, d_out, (long)n);
    HZ_TRY(h->bank.settle());
    return h->bank.render(d_out, (long)n);
}

// per-sample service statistics: speculative blocks rendered, rollbacks (setters inside a block)
int hz_add_lookahead_info(hz_add* h, long* blocks, long* rollbacks, long* block_len) {
    if (!h) return HZ_E_INVALID;
    if (blocks) *blocks = h->bank.la_blocks;
    if (rollbacks) *rollbacks = h->bank.la_rollbacks;
    if (block_len) *block_len = PhaseBank::kLook;
    return HZ_OK;
}

int hz_add_set_stream(hz_add* h, void* s) {
    HZ_TRY(add_check(h));
    HZ_TRY(h->bank.settle());
    return h->bank.stream.rebind(s, hz::NullMeans::Private);
}

int hz_add_set_target_groups(hz_add* h, int groups) {
    if (!h || groups < 1) return HZ_E_INVALID;
    h->bank.target_groups = groups;
    return HZ_OK;
}

int hz_add_profile(hz_add* h, int enable) {
    HZ_TRY(add_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->bank.stream));
    h->bank.prof = enable != 0;
    h->bank.ev.rewind();
    h->bank.launches = 0;
    h->phys.ev.rewind();
    return HZ_OK;
}

int hz_add_profile_read(hz_add* h, double* ms, long* launches) {
    HZ_TRY(add_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->bank.stream));
    double m = 0;
    HZ_TRY(h->bank.ev.elapsed(2, 0, 1, &m));   // (no rewind: a read keeps the counters)
    if (ms) *ms = m;
    if (launches) *launches = h->bank.launches;
    return HZ_OK;
}

int hz_add_physics_every(hz_add* h, int period, int law) {
    HZ_TRY(phys_law_check(h, law));
    if (period < 0) {
        hz::set_error("hz_add_physics_every: period %d", period);
        return HZ_E_INVALID;
    }
    HZ_TRY(add_check(h));
    HZ_TRY(h->bank.settle());
    hz_add::Physics& ph = h->phys;
    if (period > 0) {
        HZ_TRY(phys_ensure(h));
        ph.mode = hz_add::Physics::PERIODIC;
        ph.law = law;
        ph.period = period;
        ph.T = 0;
        return HZ_OK;
    }
    if (ph.mode != hz_add::Physics::OFF) {   // the static engine renders from the positions as moved
        const size_t P = (size_t)h->V * h->O;
        HZ_TRY_HIP(hipMemcpyAsync(h->position.data(), ph.d_x, sizeof(double) * P, hipMemcpyDeviceToHost,
                                  h->bank.stream));
        HZ_TRY_HIP(hipStreamSynchronize(h->bank.stream));
        for (int v = 0; v < h->V; ++v) add_retarget(h, v);
    }
    ph.mode = hz_add::Physics::OFF;
    ph.period = 0;
    return HZ_OK;
}

int hz_add_physics(hz_add* h, int law) {
    HZ_TRY(phys_law_check(h, law));
    HZ_TRY(add_check(h));
    HZ_TRY(h->bank.settle());
    HZ_TRY(phys_ensure(h));
    hz_add::Physics& ph = h->phys;
    if (ph.mode == hz_add::Physics::OFF) ph.mode = hz_add::Physics::MANUAL;
    ph.law = law;
    ph.amp.assign(h->bank.amp.begin(), h->bank.amp.end());
    HZ_TRY(phys_upload_call(h, 1));   // active and guides
    return phys_steps(h, 1);
}

int hz_add_peek(hz_add* h, double* y) {
    HZ_TRY(add_check(h));
    if (!y) return HZ_E_INVALID;
    if (h->bank.OL != h->O) {
        hz::set_error("hz_add_peek on an overtone shard");
        return HZ_E_UNSUPPORTED;
    }
    PhaseBank& b = h->bank;
    HZ_TRY(b.settle());
    HZ_TRY(phys_ensure(h));
    // the per-sample path: the ticks that follow are served directly, not from a speculative block
    if (h->phys.mode == hz_add::Physics::OFF) h->phys.mode = hz_add::Physics::MANUAL;
    phys_envelope(b, 1, h->phys.amp);
    HZ_TRY(phys_upload_call(h, 2));
    HZ_TRY(b.d_out.reserve(1));
    HZ_TRY(phys_audio(h, b.d_out, 1, h->phys.d_x, 0, 0, 0));
    HZ_TRY_HIP(hipMemcpyAsync(y, b.d_out, sizeof(double), hipMemcpyDeviceToHost, b.stream));
    HZ_TRY_HIP(hipStreamSynchronize(b.stream));
    return HZ_OK;
}

int hz_add_positions(hz_add* h, double* out) {
    HZ_TRY(add_check(h));
    if (!out) return HZ_E_INVALID;
    const size_t P = (size_t)h->V * h->O;
    if (!h->phys.ready) {   // nothing has moved yet
        std::memcpy(out, h->position.data(), sizeof(double) * P);
        return HZ_OK;
    }
    HZ_TRY_HIP(hipMemcpyAsync(out, h->phys.d_x, sizeof(double) * P, hipMemcpyDeviceToHost, h->bank.stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->bank.stream));
    return HZ_OK;
}

int hz_add_tune_physics(hz_add* h, int single_group_max, int tile) {
    if (!h || single_group_max < 0 || single_group_max > hz_add::Physics::kSingleLimit || tile < 0 || tile > 1024 ||
        tile % 64 != 0) {
        hz::set_error("hz_add_tune_physics: single_group_max in [0, 1024], tile a multiple of 64 up to 1024");
        return HZ_E_INVALID;
    }
    // (a request of 0 particles for the single-workgroup path cannot be told from "default": 1 does it)
    h->phys.single_max = single_group_max ? single_group_max : hz_add::Physics::kSingleMax;
    h->phys.tile = tile ? tile : hz_add::Physics::kStepTile;
    return HZ_OK;
}

int hz_add_physics_profile_read(hz_add* h, double* physics_ms, double* audio_ms) {
    HZ_TRY(add_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->bank.stream));
    double p = 0, a = 0;
    HZ_TRY(h->phys.ev.elapsed(3, 0, 1, &p));   // (no rewind here either)
    HZ_TRY(h->phys.ev.elapsed(3, 1, 2, &a));
    if (physics_ms) *physics_ms = p;
    if (audio_ms) *audio_ms = a;
    return HZ_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Sinusoids<double>  (src/sinusoids.h:10-79): one voice, amp = 1, partial i at
// fundamental (i+1)^harmonicity, weight decay^i / normalization.  tick() relaxes fundamental /
// decay / harmonicity toward their targets with stiffness relaxation(k) (sinusoids.h:46-48) and
// retargets every synth.  While one of the three still moves, the host steps that recurrence
// exactly as the reference writes it and renders one sample per launch (operator() before
// tick(): the sample takes the previous weights, c_first; the tick the new targets); the
// recurrence reaches its floating-point fixed point after about k SR samples (3 at the default
// k = 2/SR), and from there on the closed-form block engine is exact.
// ---------------------------------------------------------------------------
struct hz_sin {
    PhaseBank bank;
    int O = 0;
    double fundamental = 0, decay = 0, harmonicity = 1;
    double target_fundamental = 0, target_decay = 0, target_harmonicity = 1;
    double stiffness = 0;
    bool moving = true;   // the smoothed parameters may not be at their fixed point yet
};

namespace {
void sin_retarget(hz_sin* h) {
    PhaseBank& b = h->bank;
    b.dirty[0] = 1;
    const double norm = h->decay != 1 ? (1 - std::pow(h->decay, h->O)) / (1 - h->decay) : h->O;
    for (int i = 0; i < h->O; ++i) {
        b.ft[i] = h->fundamental * std::pow(i + 1, h->harmonicity);
        b.c[i] = std::pow(h->decay, i) / norm;
    }
}

// one tick of the smoothed parameters (sinusoids.h:46-48); false once none of them moves
bool sin_step(hz_sin* h) {
    const double k = h->stiffness;
    const double f = h->target_fundamental * (1 - k) + h->fundamental * k;
    const double d = h->target_decay * (1 - k) + h->decay * k;
    const double m = h->target_harmonicity * (1 - k) + h->harmonicity * k;
    if (f == h->fundamental && d == h->decay && m == h->harmonicity) return false;
    h->fundamental = f;
    h->decay = d;
    h->harmonicity = m;
    sin_retarget(h);
    return true;
}

// the first samples of a call, while the parameters still move: one launch each; *done of n rendered
int sin_transient(hz_sin* h, double* d_dst, long n, long* done) {
    *done = 0;
    while (h->moving && *done < n) {
        if (!sin_step(h)) {
            h->moving = false;
            break;
        }
        HZ_TRY(h->bank.render(d_dst + *done, 1));
        ++*done;
    }
    return HZ_OK;
}
}  // namespace

extern "C" {

int hz_sin_create(double fundamental, int overtones, double decay, double harmonicity, double k, int device,
                  hz_sin** out) {
    if (!out || overtones <= 0) {
        hz::set_error("hz_sin_create: invalid arguments");
        return HZ_E_INVALID;
    }
    *out = nullptr;
    HZ_TRY(hz::select_device(device));
    hz_sin* h = new (std::nothrow) hz_sin();
    if (!h) return HZ_E_ALLOC;
    h->O = overtones;
    h->fundamental = h->target_fundamental = fundamental;
    h->decay = h->target_decay = decay;
    h->harmonicity = h->target_harmonicity = harmonicity;
    h->stiffness = hz::relaxation(k);
    // Synth(form, fundamental * pow(i+1, harmonicity)) with the default k = 2/SR (sinusoids.h:23-27)
    int rc = h->bank.init(1, overtones, 0, overtones, hz::relaxation(2.0 / hz::kSR), 0.0, device);
    if (rc != HZ_OK) {
        hz_sin_destroy(h);
        return rc;
    }
    h->bank.act[0] = 1.0;
    h->bank.amp[0] = 1.0;
    h->bank.alive[0] = 1;
    h->bank.scale = 1.0;
    sin_retarget(h);
    h->bank.c_first = h->bank.c;
    // oscillators start at their target frequency, phase 0 (oscillator.h:16-24)
    std::vector<double> f0(h->bank.ft);
    if (hipMemcpy(h->bank.d_f, f0.data(), sizeof(double) * overtones, hipMemcpyHostToDevice) != hipSuccess) {
        hz::set_error("hz_sin_create: hipMemcpy failed");
        hz_sin_destroy(h);
        return HZ_E_HIP;
    }
    *out = h;
    return HZ_OK;
}

int hz_sin_destroy(hz_sin* h) {
    if (!h) return HZ_OK;
    h->bank.release();
    delete h;
    return HZ_OK;
}

int hz_sin_fundmod(hz_sin* h, double target) {   // sinusoids.h:67-68
    if (!h) return HZ_E_INVALID;
    HZ_TRY_HIP(hipSetDevice(h->bank.device));
    HZ_TRY(h->bank.settle());
    h->target_fundamental = target;
    h->moving = true;
    return HZ_OK;
}

int hz_sin_decaymod(hz_sin* h, double target) {   // sinusoids.h:61-62
    if (!h) return HZ_E_INVALID;
    HZ_TRY_HIP(hipSetDevice(h->bank.device));
    HZ_TRY(h->bank.settle());
    h->target_decay = target;
    h->moving = true;
    return HZ_OK;
}

int hz_sin_harmmod(hz_sin* h, double target) {    // sinusoids.h:64-65
    if (!h) return HZ_E_INVALID;
    HZ_TRY_HIP(hipSetDevice(h->bank.device));
    HZ_TRY(h->bank.settle());
    h->target_harmonicity = target;
    h->moving = true;
    return HZ_OK;
}

// n x { out[t] = operator()(); tick(); }   sinusoids.h:34-57
int hz_sin_fill(hz_sin* h, double* out, size_t n) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY_HIP(hipSetDevice(h->bank.device));
    if (n && !out) return HZ_E_INVALID;
    long done = 0;
    if (h->moving && n) {
        PhaseBank& b = h->bank;
        HZ_TRY(b.settle());
        HZ_TRY(b.d_out.reserve(n));
        HZ_TRY(sin_transient(h, b.d_out, (long)n, &done));
        if (done) {
            HZ_TRY_HIP(hipMemcpyAsync(out, b.d_out, sizeof(double) * done, hipMemcpyDeviceToHost, b.stream));
            HZ_TRY_HIP(hipStreamSynchronize(b.stream));
        }
    }
    return h->bank.fill_host(out + done, (long)n - done);
}

int hz_sin_fill_device(hz_sin* h, double* d_out, size_t n) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY_HIP(hipSetDevice(h->bank.device));
    if (n && !d_out) return HZ_E_INVALID;
    HZ_TRY(h->bank.settle());
    long done = 0;
    HZ_TRY(sin_transient(h, d_out, (long)n, &done));
    return h->bank.render(d_out + done, (long)n - done);
}

}  // extern "C"
