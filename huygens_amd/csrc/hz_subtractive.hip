// hz_subtractive.hip -- Subtractive<double, N> (src/subtractive.h:15-101, the MIMO variant the
// reference compiles) for MI355X (gfx950): a Minimizer whose particles tune voices x overtones x N
// two-pole Filter<T> resonators (src/filter.h).
//
//   tick():      amp_v <- (1 - a) active_v + a amp_v; then, for voices with amp_v != 0 only,
//                every partial: f = mtof(position); while (f > SR/2) f /= 2;
//                resonant(f, R): forward {g, 0, -g}, back {0, -2 R cos(2 PI f / SR), R^2};
//                Filter::tick()
//   operator():  out[k] += amp_v decay^j filter_{k,v,j}(x[k]) / (V norm), voices with amp_v != 0
//   block loop:  n x { out[:, t] = operator()(x[:, t]); if (T >= p && T % p == 0) physics(); tick(); T++ }
//
// A voice whose amplitude is zero is neither computed nor ticked: its filters are frozen.  A
// Filter's ring (size 4) then reduces to four registers per filter, shifted when a sample is
// computed: y = (g x - b1 y1) + ((-g) x2 - b2 y2) in the sum order of filter.h:108-114 (the i = 0
// term's back[0] output[origin] is 0 times a finite stale value).
//
// Device engine, per piece of a call:
//   1. hz::min_run (hz_minimizer.hip) writes the position rows [steps + 1][P], P = V O;
//   2. sub_coef_kernel turns each row into [row][P]{g, b1, b2}: the positions move once per
//      physics period, so mtof / fold / resonant() run per step, not per sample;
//   3. the host writes the envelope rows amp[n + 1][V] op for op (V scalars per sample);
//   4. sub_res_kernel: one lane per filter, grid (ceil(P / 64), N) so a channel's lanes are
//      contiguous in partial order; time is serial per lane, the four history values and three
//      coefficients in registers, coefficients reloaded at the first gated tick after a step;
//      the output weight is amp_v (decay^j / (V norm)), the quotient taken once per lane (the
//      reference divides per sample: a difference of an ulp or two of each term);
//      every round (up to 16 samples, cut at a physics step so the positions change only at a
//      round's last tick; a round's input, envelope and coefficients are fetched one round ahead)
//      the lanes' weighted outputs are summed through LDS (hz_fb_tv.hip's rounds: 16-value runs,
//      an xor tree over 4 lanes) into partial rows [groups][N][n];
//   5. hz_mix.h's slab reduce sums the group rows (one group: the resonator writes the output itself).
// Filter state and the coefficients last set persist in the handle across calls, note events and
// a stolen voice (the reference never calls forget()).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "hz_common.h"
#include "hz_minimizer.h"
#include "hz_mix.h"
#include "hz_resonant.h"

namespace {

constexpr int kThreads = 64;              // filters per workgroup: one wave
constexpr int kCH = 16;                   // samples per LDS mix round
constexpr int kLanes = kThreads / kCH;    // lanes summing one sample
constexpr int kRunLen = kThreads / kLanes;
constexpr int kRun = kRunLen + 1;
constexpr int kRow = kLanes * kRun + 1;
constexpr int kMaxChannels = 8;

// which voices sound and tick (subtractive.h:54, 73).  Polyres / Polyphon gate differently; the
// launchers take the rule so they can follow.
enum Gate { kGateAmplitude = 0 };   // amplitudes[v] != 0

struct Coef {
    double g, b1, b2;
};

// position rows -> coefficient rows (subtractive.h:57-63, filter.h:123-138)
__global__ __launch_bounds__(256) void sub_coef_kernel(const double* __restrict__ rows, Coef* __restrict__ coef,
                                                       long count, double R) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double f = 440.0 * exp2((rows[i] - 69) / 12);
    // (bounded: a position that has left the doubles' range must not spin the lane)
    for (int q = 0; q < 1100 && f > hz::kSR / 2; ++q) f /= 2;
    const double cosine = hz_res::tv_cos(hz_res::div_sr(2 * hz::kPI * f));
    Coef c;
    c.g = hz_res::resonant(f, R);
    c.b1 = -2 * R * cosine;
    c.b2 = R * R;
    coef[i] = c;
}

struct ResArgs {
    const double* x;       // [N][xstride] input
    const double* amp;     // [n + 1][V] envelope: row t at sample t's output, row t + 1 after its tick
    const Coef* coef;      // [steps + 1][P]: row k in effect after the call's k-th step
    const double* dec;     // [O] decay^j
    double* state;         // [N P][4] y1, y2, x1, x2 per filter
    Coef* cur;             // [N P] coefficients last set, per filter
    double* part;          // [G][N][pstride] group rows; with one group the output [N][pstride]
    long n, xstride, pstride;
    long T0;               // samples since the period was set, at the call's first sample
    int period;            // 0: no step inside the call
    int P, V, O, N;
    int advance;           // 0: operator() only (hz_sub_peek; coef may be null)
    double den;            // V norm
};

__global__ __launch_bounds__(kThreads) void sub_res_kernel(ResArgs a) {
#pragma clang fp contract(off)
    __shared__ double buf[kCH * kRow];
    const int tid = threadIdx.x;
    const int p = blockIdx.x * kThreads + tid;
    const int ch = blockIdx.y;
    const bool live = p < a.P;
    const int pp = live ? p : 0;
    const int vo = pp / a.O;
    const double w = a.dec[pp - vo * a.O] / a.den;   // decay^j / (V norm)
    const size_t fi = (size_t)ch * a.P + pp;
    double* st = a.state + fi * 4;
    double y1 = st[0], y2 = st[1], x1 = st[2], x2 = st[3];
    Coef c = a.cur[fi];
    const double* x = a.x + (size_t)ch * a.xstride;
    double* prow = a.part + ((size_t)blockIdx.x * a.N + ch) * a.pstride;
    double* bcol = buf + (tid / kRunLen) * kRun + tid % kRunLen;
    // A round is up to kCH samples and ends with the call or with the next physics step, so the
    // positions change at most once in it, at its last tick.  plan: the round starting at call
    // sample t0 (T samples since the period was set): its length and whether a step ends it.
    auto plan = [&](long t0, long T, int& m, bool& step) {
        long len = min((long)kCH, a.n - t0);
        step = false;
        if (a.period > 0) {
            long d = (a.period - T % a.period) % a.period;   // samples before the next multiple of the period
            if (T + d < a.period) d += a.period;             // no step before sample `period`
            if (d < len) {
                len = d + 1;
                step = true;
            }
        }
        m = (int)len;
    };
    // A round's input, its envelope values after each tick and the coefficients of its two position
    // rows are fetched together, one round ahead: their latency runs under the previous round's
    // recurrence, and the sample loop holds no global load.
    // (every lane holds the round's inputs: one address per sample for the whole wave)
    double am_next[kCH], x_next[kCH];
    Coef ca_next = c, cb_next = c;
    auto fetch = [&](long t0, int row, int m, bool step) {
#pragma unroll
        for (int j = 0; j < kCH; ++j) {
            x_next[j] = j < m ? x[t0 + j] : 0.0;
            am_next[j] = j < m ? a.amp[(t0 + j + 1) * a.V + vo] : 0.0;
        }
        if (a.advance && m > 0) {
            ca_next = a.coef[(size_t)row * a.P + pp];
            cb_next = step ? a.coef[(size_t)(row + 1) * a.P + pp] : ca_next;
        }
    };
    long T = a.T0;
    int row = 0, loaded = -1;
    double amp = a.amp[vo];
    int m, m_next;
    bool step, step_next;
    plan(0, T, m, step);
    fetch(0, row, m, step);
    for (long t0 = 0; t0 < a.n;) {
        double am[kCH], xr[kCH];
#pragma unroll
        for (int j = 0; j < kCH; ++j) {
            am[j] = am_next[j];
            xr[j] = x_next[j];
        }
        const Coef ca = ca_next, cb = cb_next;   // of the row in effect, and of the row after the round's step
        const int row_next = row + (step ? 1 : 0);
        plan(t0 + m, T + m, m_next, step_next);
        fetch(t0 + m, row_next, m_next, step_next);
        __syncthreads();   // the previous round's sums have left buf
        auto sample = [&](int j, double xt, double amp_next, bool stepped) {
            double v = 0.0;
            if (amp != 0.0) {   // operator(): filter.h:102-121
                double out = c.g * xt;
                out += 0.0 * x1 - c.b1 * y1;
                out += -c.g * x2 - c.b2 * y2;
                y2 = y1;
                y1 = out;
                x2 = x1;
                x1 = xt;
                v = amp * w * out;
            }
            bcol[j * kRow] = live ? v : 0.0;
            const int r = stepped ? row_next : row;   // stepped: physics() between operator() and tick()
            amp = amp_next;
            if (a.advance && amp != 0.0 && loaded != r) {   // tick(): resonant() from the positions in effect
                c = stepped ? cb : ca;
                loaded = r;
            }
        };
        if (m == kCH) {   // a full round: unrolled, the inputs in fixed registers
#pragma unroll
            for (int j = 0; j < kCH; ++j) sample(j, xr[j], am[j], step && j == kCH - 1);
        } else {
            for (int j = 0; j < m; ++j) sample(j, xr[j], am[j], step && j == m - 1);
        }
        __syncthreads();
        {
            const int j = tid / kLanes, q = tid % kLanes;
            double s = 0.0;
            if (j < m) {
                const double* r = buf + j * kRow + q * kRun;
#pragma unroll
                for (int k = 0; k < kRunLen; ++k) s += r[k];
            }
#pragma unroll
            for (int w = 1; w < kLanes; w <<= 1) s += __shfl_xor(s, w);
            if (q == 0 && j < m) prow[t0 + j] = s;
        }
        t0 += m;
        T += m;
        row = row_next;
        m = m_next;
        step = step_next;
    }
    if (a.advance && live) {
        st[0] = y1;
        st[1] = y2;
        st[2] = x1;
        st[3] = x2;
        a.cur[fi] = c;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Subtractive<double, N>
// ---------------------------------------------------------------------------
struct hz_sub : hz::MinNotes {
    hz::Stream stream;
    int N = 1, device = 0;
    double decay = 0, resonance = 0, norm = 1, attack = 0;
    std::vector<double> amp;   // amplitudes[v]
    // Minimizer::physics()
    int law = 0, period = 0;
    long T = 0;                // samples since the period was set
    int single_max = kSingleMax, tile = kStepTile;
    static constexpr int kSingleLimit = 1024, kSingleMax = 256, kStepTile = 256;
    // a call is rendered in pieces of at most kMaxSamples samples whose position rows fit kMaxRowBytes
    static constexpr long kMaxSamples = 4096;
    static constexpr size_t kMaxRowBytes = (size_t)32 << 20;
    hz::DevBuf<double> d_x, d_v, d_eq, d_guide, d_act, d_rows, d_amp, d_dec, d_state, d_part, d_in, d_out;
    hz::DevBuf<Coef> d_coef, d_cur;
    std::vector<double> amp_rows;   // [n + 1][V] envelope rows of the piece being rendered
    bool prof = false;
    hz::ProfEvents ev;     // profile: 5 per piece (start, physics, coefficients, resonators, reduce)
};

namespace {

int sub_check(hz_sub* h) {
    return hz::check_handle(h, "hz_sub");
}

int sub_law_check(int law) {
    if (law != HZ_GRAV_TRUNC && law != HZ_GRAV_FABS) {
        hz::set_error("gravity law %d: HZ_GRAV_TRUNC or HZ_GRAV_FABS (there is no default)", law);
        return HZ_E_INVALID;
    }
    return HZ_OK;
}

// device rows of one voice after request(): position, equilibrium, velocity 0
int sub_upload_voice(hz_sub* h, int v) {
    const size_t O = h->O, at = (size_t)v * O;
    HZ_TRY_HIP(hipMemcpyAsync(h->d_x + at, &h->position[at], sizeof(double) * O, hipMemcpyHostToDevice, h->stream));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_eq + at, &h->equilibrium[at], sizeof(double) * O, hipMemcpyHostToDevice, h->stream));
    HZ_TRY_HIP(hipMemsetAsync(h->d_v + at, 0, sizeof(double) * O, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));   // pageable sources
    return HZ_OK;
}

// active / guide and n_rows envelope rows to the device (pageable sources: synchronised)
int sub_upload_call(hz_sub* h, long n_rows) {
    if (n_rows > 0) {
        HZ_TRY(h->d_amp.reserve((size_t)n_rows * h->V));
        HZ_TRY_HIP(hipMemcpyAsync(h->d_amp, h->amp_rows.data(), sizeof(double) * n_rows * h->V, hipMemcpyHostToDevice,
                                  h->stream));
    }
    HZ_TRY_HIP(hipMemcpyAsync(h->d_act, h->active.data(), sizeof(double) * h->V, hipMemcpyHostToDevice, h->stream));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_guide, h->guide.data(), sizeof(double) * h->V, hipMemcpyHostToDevice, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

// `steps` physics steps on the device state: rows[0] <- x, kernels write rows 1..steps, x <- rows[steps]
int sub_steps(hz_sub* h, int steps) {
    const size_t P = (size_t)h->V * h->O;
    HZ_TRY(h->d_rows.reserve((size_t)(steps + 1) * P));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_rows, h->d_x, sizeof(double) * P, hipMemcpyDeviceToDevice, h->stream));
    if (steps <= 0) return HZ_OK;
    // subtractive.h inherits Minimizer's springs: k0 = 0.1 FORCE, k1 = FORCE (minimizer.h:40, 45)
    HZ_TRY(hz::min_run(h->stream, hz::min_params(h->V, h->O, 0.1 * 50000, 1 * 50000), h->law, steps,
                       (long)P <= h->single_max, h->tile, h->d_rows, h->d_v, h->d_eq, h->d_act, h->d_guide));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_x, h->d_rows + (size_t)steps * P, sizeof(double) * P, hipMemcpyDeviceToDevice,
                              h->stream));
    return HZ_OK;
}

// envelope rows of n samples, op for op (subtractive.h:49-50): row 0 = amplitudes now, row t + 1
// after sample t's tick
void sub_envelope(const hz_sub* h, long n, std::vector<double>& rows) {
#pragma clang fp contract(off)
    const int V = h->V;
    rows.resize((size_t)(n + 1) * V);
    for (int v = 0; v < V; ++v) rows[v] = h->amp[v];
    for (long t = 0; t < n; ++t)
        for (int v = 0; v < V; ++v)
            rows[(size_t)(t + 1) * V + v] = (1 - h->attack) * h->active[v] + h->attack * rows[(size_t)t * V + v];
}

int sub_coefs(hz_sub* h, int n_rows) {
    const long count = (long)n_rows * h->V * h->O;
    HZ_TRY(h->d_coef.reserve((size_t)count));
    hipLaunchKernelGGL(sub_coef_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)h->d_rows, h->d_coef.get(), count, h->resonance);
    HZ_TRY_HIP(hipGetLastError());
    return HZ_OK;
}

// the resonators over n samples (n <= kMaxSamples), coefficient and envelope rows on the device;
// d_x [N][xstride], d_dst [N][ostride]
int sub_audio(hz_sub* h, const double* d_x, long xstride, double* d_dst, long ostride, long n, int period, long T0,
              int gate, int advance) {
    const int P = h->V * h->O, G = (P + kThreads - 1) / kThreads;
    if (gate != kGateAmplitude) {
        hz::set_error("resonator gate rule %d is not implemented", gate);
        return HZ_E_UNSUPPORTED;
    }
    ResArgs a;
    a.x = d_x;
    a.amp = h->d_amp;
    a.coef = h->d_coef;
    a.dec = h->d_dec;
    a.state = h->d_state;
    a.cur = h->d_cur;
    a.n = n;
    a.xstride = xstride;
    a.T0 = T0;
    a.period = period;
    a.P = P;
    a.V = h->V;
    a.O = h->O;
    a.N = h->N;
    a.advance = advance;
    a.den = h->V * h->norm;
    if (G > 1) {
        HZ_TRY(h->d_part.reserve((size_t)G * h->N * n));
        a.part = h->d_part;
        a.pstride = n;
    } else {   // one group: its rows are the output
        a.part = d_dst;
        a.pstride = ostride;
    }
    hipLaunchKernelGGL(sub_res_kernel, dim3(G, h->N), dim3(kThreads), 0, h->stream, a);
    HZ_TRY_HIP(hipGetLastError());
    return HZ_OK;
}

int sub_reduce(hz_sub* h, double* d_dst, long ostride, long n) {
    const int P = h->V * h->O, G = (P + kThreads - 1) / kThreads;
    if (G <= 1) return HZ_OK;
    // out[k][t] = sum of the group rows, a channel per blockIdx.y
    hz::mix::slab_reduce(h->stream, (const double*)h->d_part, n, G, n, hz::mix::SlabChannel{h->N, d_dst, ostride},
                         (unsigned)h->N);
    HZ_TRY_HIP(hipGetLastError());
    return HZ_OK;
}

// n x { out[:, t] = operator()(x[:, t]); if (T >= period && T % period == 0) physics(); tick(); T++; }
// d_in, d_dst [N][n] on the device, in pieces whose position rows stay within kMaxRowBytes
int sub_render(hz_sub* h, const double* d_in, double* d_dst, long n) {
    const size_t P = (size_t)h->V * h->O;
    const int period = h->period;
    const long max_steps = std::max<long>(1, (long)(hz_sub::kMaxRowBytes / (sizeof(double) * P)) - 1);
    for (long done = 0; done < n;) {
        long m = std::min(n - done, hz_sub::kMaxSamples);
        if (period > 0) m = std::min(m, max_steps * period);
        int steps = 0;
        for (long t = 0; t < m && period > 0; ++t) steps += (h->T + t >= period && (h->T + t) % period == 0) ? 1 : 0;
        sub_envelope(h, m, h->amp_rows);
        HZ_TRY(sub_upload_call(h, m + 1));
        hipEvent_t* e = nullptr;
        if (h->prof) {
            HZ_TRY(h->ev.take(5, &e));
            HZ_TRY_HIP(hipEventRecord(e[0], h->stream));
        }
        HZ_TRY(sub_steps(h, steps));
        if (e) HZ_TRY_HIP(hipEventRecord(e[1], h->stream));
        HZ_TRY(sub_coefs(h, steps + 1));
        if (e) HZ_TRY_HIP(hipEventRecord(e[2], h->stream));
        HZ_TRY(sub_audio(h, d_in + done, n, d_dst + done, n, m, period, h->T, kGateAmplitude, 1));
        if (e) HZ_TRY_HIP(hipEventRecord(e[3], h->stream));
        HZ_TRY(sub_reduce(h, d_dst + done, n, m));
        if (e) HZ_TRY_HIP(hipEventRecord(e[4], h->stream));
        for (int v = 0; v < h->V; ++v) h->amp[v] = h->amp_rows[(size_t)m * h->V + v];
        if (period > 0) h->T += m;
        done += m;
    }
    return HZ_OK;
}

}  // namespace

extern "C" {

int hz_sub_create(int voices, int overtones, int channels, double decay, double resonance, double harmonicity,
                  double k, int device, hz_sub** out) {
    // Minimizer::request divides by overtones - 1 (minimizer.h:146)
    if (!out || voices < 1 || overtones < 2 || channels < 1) {
        hz::set_error("hz_sub_create: voices >= 1, overtones >= 2, channels >= 1");
        return HZ_E_INVALID;
    }
    *out = nullptr;
    if (channels > kMaxChannels) {
        hz::set_error("hz_sub_create: %d channels (at most %d)", channels, kMaxChannels);
        return HZ_E_UNSUPPORTED;
    }
    HZ_TRY(hz::select_device(device));
    hz_sub* h = new (std::nothrow) hz_sub();
    if (!h) return HZ_E_ALLOC;
    h->notes_init(voices, overtones, harmonicity);
    h->N = channels;
    h->device = device;
    h->decay = decay;
    h->resonance = resonance;
    h->attack = hz::relaxation(k);
    h->norm = decay != 1 ? (1 - std::pow(decay, overtones)) / (1 - decay) : overtones;   // subtractive.h:38
    h->amp.assign(voices, 0.0);
    const size_t P = (size_t)voices * overtones;
    std::vector<double> dec(overtones);
    for (int j = 0; j < overtones; ++j) dec[j] = std::pow(decay, j);
    auto init = [&]() -> int {
        HZ_TRY(h->stream.create());
        HZ_TRY(h->d_x.reserve(P));
        HZ_TRY(h->d_v.reserve(P));
        HZ_TRY(h->d_eq.reserve(P));
        HZ_TRY(h->d_guide.reserve(voices));
        HZ_TRY(h->d_act.reserve(voices));
        HZ_TRY(h->d_dec.reserve(overtones));
        HZ_TRY(h->d_state.reserve(P * channels * 4));
        HZ_TRY(h->d_cur.reserve(P * channels));
        // particles at 0, filters Filter({1,0,0},{0}) with zero history (subtractive.h:42-44); the
        // identity coefficients never run: a voice's first gated tick sets resonant() first
        HZ_TRY_HIP(hipMemset(h->d_x, 0, sizeof(double) * P));
        HZ_TRY_HIP(hipMemset(h->d_v, 0, sizeof(double) * P));
        HZ_TRY_HIP(hipMemset(h->d_eq, 0, sizeof(double) * P));
        HZ_TRY_HIP(hipMemset(h->d_state, 0, sizeof(double) * P * channels * 4));
        std::vector<Coef> id(P * channels, Coef{1.0, 0.0, 0.0});
        HZ_TRY_HIP(hipMemcpy(h->d_cur, id.data(), sizeof(Coef) * id.size(), hipMemcpyHostToDevice));
        HZ_TRY_HIP(hipMemcpy(h->d_dec, dec.data(), sizeof(double) * overtones, hipMemcpyHostToDevice));
        return HZ_OK;
    };
    const int rc = init();
    if (rc != HZ_OK) {
        hz_sub_destroy(h);
        return rc;
    }
    *out = h;
    return HZ_OK;
}

int hz_sub_destroy(hz_sub* h) {
    if (!h) return HZ_OK;
    (void)hipSetDevice(h->device);
    (void)h->stream.sync();
    delete h;
    return HZ_OK;
}

int hz_sub_request(hz_sub* h, double fundamental, double amplitude, int* voice_out) {
    HZ_TRY(sub_check(h));
    const int voice = h->request(fundamental, amplitude);
    HZ_TRY(sub_upload_voice(h, voice));   // particles re-initialised: v = 0
    if (voice_out) *voice_out = voice;
    return HZ_OK;
}

int hz_sub_release(hz_sub* h, int voice) {
    HZ_TRY(sub_check(h));
    h->release(voice);
    return HZ_OK;
}

int hz_sub_makenote(hz_sub* h, double pitch, double amplitude, int* voice_out) {   // minimizer.h:174-179
    int v = -1;
    HZ_TRY(hz_sub_request(h, hz::MinNotes::mtof(pitch), amplitude, &v));
    if (v >= 0) h->pitches[v] = pitch;
    if (voice_out) *voice_out = v;
    return HZ_OK;
}

int hz_sub_endnote(hz_sub* h, double pitch) {   // minimizer.h:182-187
    HZ_TRY(sub_check(h));
    for (int j = 0; j < h->V; ++j)
        if (h->pitches[j] == pitch) h->release(j);
    return HZ_OK;
}

int hz_sub_physics_every(hz_sub* h, int period, int law) {
    if (!h) {
        hz::set_error("null hz_sub handle");
        return HZ_E_INVALID;
    }
    HZ_TRY(sub_law_check(law));
    if (period < 0) {
        hz::set_error("hz_sub_physics_every: period %d", period);
        return HZ_E_INVALID;
    }
    h->period = period;
    h->law = law;
    h->T = 0;
    return HZ_OK;
}

int hz_sub_physics(hz_sub* h, int law) {
    if (!h) {
        hz::set_error("null hz_sub handle");
        return HZ_E_INVALID;
    }
    HZ_TRY(sub_law_check(law));
    HZ_TRY(sub_check(h));
    h->law = law;
    HZ_TRY(sub_upload_call(h, 0));   // active and guides
    return sub_steps(h, 1);
}

int hz_sub_process_device(hz_sub* h, const double* d_in, double* d_out, size_t n) {
    HZ_TRY(sub_check(h));
    if (n == 0) return HZ_OK;
    if (!d_in || !d_out) {
        hz::set_error("hz_sub_process: null buffer");
        return HZ_E_INVALID;
    }
    return sub_render(h, d_in, d_out, (long)n);
}

int hz_sub_process(hz_sub* h, const double* in, double* out, size_t n) {
    HZ_TRY(sub_check(h));
    if (n == 0) return HZ_OK;
    if (!in || !out) {
        hz::set_error("hz_sub_process: null buffer");
        return HZ_E_INVALID;
    }
    const size_t count = n * h->N;
    HZ_TRY(h->d_in.reserve(count));
    HZ_TRY(h->d_out.reserve(count));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_in, in, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));   // pageable source
    HZ_TRY(sub_render(h, h->d_in, h->d_out, (long)n));
    HZ_TRY_HIP(hipMemcpyAsync(out, h->d_out, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

// operator()(in[N]) without tick(): nothing advances
int hz_sub_peek(hz_sub* h, const double* in, double* out) {
    HZ_TRY(sub_check(h));
    if (!in || !out) {
        hz::set_error("hz_sub_peek: null buffer");
        return HZ_E_INVALID;
    }
    HZ_TRY(h->d_in.reserve(h->N));
    HZ_TRY(h->d_out.reserve(h->N));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_in, in, sizeof(double) * h->N, hipMemcpyHostToDevice, h->stream));
    sub_envelope(h, 1, h->amp_rows);
    HZ_TRY(sub_upload_call(h, 2));
    HZ_TRY(sub_audio(h, h->d_in, 1, h->d_out, 1, 1, 0, 0, kGateAmplitude, 0));
    HZ_TRY(sub_reduce(h, h->d_out, 1, 1));
    HZ_TRY_HIP(hipMemcpyAsync(out, h->d_out, sizeof(double) * h->N, hipMemcpyDeviceToHost, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

int hz_sub_positions(hz_sub* h, double* out) {
    HZ_TRY(sub_check(h));
    if (!out) return HZ_E_INVALID;
    HZ_TRY_HIP(hipMemcpyAsync(out, h->d_x, sizeof(double) * h->V * h->O, hipMemcpyDeviceToHost, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

int hz_sub_amplitudes(hz_sub* h, double* out) {
    if (!h || !out) return HZ_E_INVALID;
    std::memcpy(out, h->amp.data(), sizeof(double) * h->V);
    return HZ_OK;
}

int hz_sub_set_stream(hz_sub* h, void* s) {
    HZ_TRY(sub_check(h));
    return h->stream.rebind(s, hz::NullMeans::Private);
}

int hz_sub_tune_physics(hz_sub* h, int single_group_max, int tile) {
    if (!h || single_group_max < 0 || single_group_max > hz_sub::kSingleLimit || tile < 0 || tile > 1024 ||
        tile % 64 != 0) {
        hz::set_error("hz_sub_tune_physics: single_group_max in [0, 1024], tile a multiple of 64 up to 1024");
        return HZ_E_INVALID;
    }
    h->single_max = single_group_max ? single_group_max : hz_sub::kSingleMax;
    h->tile = tile ? tile : hz_sub::kStepTile;
    return HZ_OK;
}

int hz_sub_profile(hz_sub* h, int enable) {
    HZ_TRY(sub_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    h->prof = enable != 0;
    h->ev.rewind();
    return HZ_OK;
}

int hz_sub_profile_read(hz_sub* h, double* physics_ms, double* coef_ms, double* resonator_ms, double* reduce_ms) {
    HZ_TRY(sub_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    double ms[4] = {0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) HZ_TRY(h->ev.elapsed(5, q, q + 1, &ms[q]));   // (no rewind: a read keeps the counters)
    if (physics_ms) *physics_ms = ms[0];
    if (coef_ms) *coef_ms = ms[1];
    if (resonator_ms) *resonator_ms = ms[2];
    if (reduce_ms) *reduce_ms = ms[3];
    return HZ_OK;
}

}  // extern "C"
