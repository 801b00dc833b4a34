// hz_oscbank.hip -- Oscbank<double,N> engine for MI355X (gfx950).
//
// Replaces src/oscbank.h:15-97 (+ the active-set protocol of src/multichannel.h:16-159):
//   freqmod(i, hz): w_i = (cos(2 PI hz/SR), sin(2 PI hz/SR))              (49-56)
//   tick():         z_i <- z_i w_i ; z_i <- z_i / ((1 + |z_i|^2)/2)  for active i   (59-63)
//   mixdown():      sum_{active i} z_i                                      (81-90)
//   operator()():   all N phasors                                            (65-68)
//
// z and w are unit phasors, so the renormalisation is the identity to O(eps) and the
// trajectory is the closed form z_i(t) = z_i(0) w_i^t.  The kernels therefore rotate
// exactly-seeded phasors (no transcendental in the hot loop):
//   * lanes are TIME: lane c of a wave owns samples [16c, 16c+16) of a 1024-sample tile;
//     each wave walks up to 64 active partials per tile and accumulates the complex mix
//     of its 16 samples in registers (no cross-lane reduction);
//   * chunk seed = z(t0) * (w^16)^p * (w^256)^r  (p = lane & 15, r = lane >> 4) from a
//     per-partial table built on the host in long double; z(t0 + 1024) = z(t0) w^1024;
//   * time segments cost nothing (closed form): z(t_seg) = z(0) (w^1024)^(t_seg/1024);
//   * waves' 1024-sample mixes are summed through LDS into one partial row per group,
//     and a second kernel sums the rows (deterministic).
// Error vs the reference's renormalised recurrence: O(t eps) in phase (1e-10 after 1e6
// samples), far inside the 1e-5 bound.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <new>
#include <vector>

#include "hz_common.h"
#include "hz_mix.h"
#include "hz_mixplan.h"

namespace {

using namespace hz::mix;   // kWaves, kMaxPerWave, kPad, cmul and the end-of-tile / slab reductions

constexpr int kL = 16;
constexpr int kTile = tile_len(kL);

// per-partial record (doubles): w, T1[16] = (w^16)^p, T2[4] = (w^256)^r, W = w^1024
struct ORec {
    static constexpr int W1 = 0;
    static constexpr int T1 = 2;
    static constexpr int T2 = T1 + 32;
    static constexpr int WT = T2 + 8;
    static constexpr int SIZE = 48;
};

struct OscArgs {
    const int* act;        // [A] active local indices, ascending
    const double* z0;      // [N][2] phasors at call start
    double* partial;       // [G][n_pad][2]
    long n, n_pad, seg_len;
    int A, nseg, per_wave;
};

__global__ __launch_bounds__(64 * kWaves) void osc_mix_kernel(const double* __restrict__ rec, OscArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* part_re = lds;                                   // [W][16][66]
    double* part_im = lds + kWaves * kL * kPad;              // [W][16][66]
    double* zt = lds + 2 * kWaves * kL * kPad;               // [W][64][2] tile-start phasors
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = lane & 15, r = lane >> 4;
    const int seg = blockIdx.y;
    const long seg_t0 = (long)seg * a.seg_len;
    const long seg_end = min(seg_t0 + a.seg_len, a.n);
    const int ntiles = (int)((seg_end - seg_t0 + kTile - 1) / kTile);
    const int first = (blockIdx.x * kWaves + wave) * a.per_wave;
    const int count = max(0, min(a.per_wave, a.A - first));
    double* myzt = zt + wave * (2 * kMaxPerWave);

    // tile-start phasors at the segment start: z(0) (w^1024)^(seg_t0 / 1024)
    for (int q = 0; q < count; ++q) {
        const int i = a.act[first + q];
        const double* rr = rec + (long)i * ORec::SIZE;
        double zr = a.z0[2 * i], zi = a.z0[2 * i + 1];
        double br = rr[ORec::WT], bi = rr[ORec::WT + 1];
        for (long e = seg_t0 / kTile; e > 0; e >>= 1) {
            if (e & 1) cmul(zr, zi, br, bi, zr, zi);
            cmul(br, bi, br, bi, br, bi);
        }
        if (lane == 0) {  // wave-private slot; DS ops of one wave complete in order
            myzt[2 * q] = zr;
            myzt[2 * q + 1] = zi;
        }
    }
    __builtin_amdgcn_wave_barrier();

    for (int tile = 0; tile < ntiles; ++tile) {
        const long t0 = seg_t0 + (long)tile * kTile;
        double accr[kL], acci[kL];
#pragma unroll
        for (int j = 0; j < kL; ++j) accr[j] = acci[j] = 0.0;
        for (int q = 0; q < count; ++q) {
            const int i = a.act[first + q];
            const double* rr = rec + (long)i * ORec::SIZE;
            const double wr = rr[ORec::W1], wi = rr[ORec::W1 + 1];
            double sr = myzt[2 * q], si = myzt[2 * q + 1];
            // advance the tile-start phasor for the next tile (all lanes, same value)
            double nr, ni;
            cmul(sr, si, rr[ORec::WT], rr[ORec::WT + 1], nr, ni);
            if (lane == 0) {
                myzt[2 * q] = nr;
                myzt[2 * q + 1] = ni;
            }
            __builtin_amdgcn_wave_barrier();
            // lane seed z(t0 + 16 lane) = z(t0) T1[p] T2[r]
            double ur, ui;
            cmul(rr[ORec::T1 + 2 * p], rr[ORec::T1 + 2 * p + 1], rr[ORec::T2 + 2 * r], rr[ORec::T2 + 2 * r + 1],
                 ur, ui);
            cmul(sr, si, ur, ui, sr, si);
#pragma unroll
            for (int j = 0; j < kL; ++j) {
                accr[j] += sr;
                acci[j] += si;
                cmul(sr, si, wr, wi, sr, si);
            }
        }
        // ---- workgroup reduction over waves (hz_mix.h) ----------------------------
        put_rows<kL>(part_re + wave * (kL * kPad), lane, accr);
        put_rows<kL>(part_im + wave * (kL * kPad), lane, acci);
        tile_reduce<kL, 2>(part_re, t0, a.n, [&](long t, const double (&s)[2]) {
            reinterpret_cast<double2*>(a.partial)[(long)blockIdx.x * a.n_pad + t] = make_double2(s[0], s[1]);
        });
    }
}

// per-band output (operator()() at every sample): per_band[t][i] = z_i(t); inactive
// partials are frozen.  Lane = partial, 256-sample chunks; HBM-write bound.
constexpr int kPbChunk = 256;
__global__ __launch_bounds__(256) void osc_per_band_kernel(const double* __restrict__ rec, const double* z0,
                                                           const unsigned char* __restrict__ active, int N,
                                                           long n, double2* __restrict__ per_band) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const long tb = (long)blockIdx.y * kPbChunk;
    if (i >= N) return;
    const double* rr = rec + (long)i * ORec::SIZE;
    double zr = z0[2 * i], zi = z0[2 * i + 1];
    const bool on = active[i] != 0;
    const double wr = on ? rr[ORec::W1] : 1.0, wi = on ? rr[ORec::W1 + 1] : 0.0;
    double br = wr, bi = wi;
    for (long e = tb; e > 0; e >>= 1) {  // z(0) w^tb
        if (e & 1) cmul(zr, zi, br, bi, zr, zi);
        cmul(br, bi, br, bi, br, bi);
    }
    const long te = min(tb + kPbChunk, n);
    for (long t = tb; t < te; ++t) {
        double2 v;
        v.x = zr;
        v.y = zi;
        per_band[t * N + i] = v;
        cmul(zr, zi, wr, wi, zr, zi);
    }
}

// end-of-call state: z_i <- z_i w_i^n / |.|  for active i (the reference keeps |z| = 1
// by its first-order renormalisation, oscbank.h:62)
__global__ __launch_bounds__(256) void osc_advance_kernel(const double* __restrict__ rec, const int* __restrict__ act,
                                                          int A, long n, double* z) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A) return;
    const int i = act[q];
    const double* rr = rec + (long)i * ORec::SIZE;
    double zr = z[2 * i], zi = z[2 * i + 1];
    double br = rr[ORec::W1], bi = rr[ORec::W1 + 1];
    for (long e = n; e > 0; e >>= 1) {
        if (e & 1) cmul(zr, zi, br, bi, zr, zi);
        cmul(br, bi, br, bi, br, bi);
    }
    const double m = 1.0 / sqrt(zr * zr + zi * zi);
    z[2 * i] = zr * m;
    z[2 * i + 1] = zi * m;
}

void build_orec(double wr, double wi, double* rec) {
    using C = std::complex<long double>;
    std::memset(rec, 0, sizeof(double) * ORec::SIZE);
    const C w((long double)wr, (long double)wi);
    rec[ORec::W1] = wr;
    rec[ORec::W1 + 1] = wi;
    C w16(1, 0);
    for (int k = 0; k < 16; ++k) w16 *= w;
    C acc(1, 0);
    for (int p = 0; p < 16; ++p) {
        rec[ORec::T1 + 2 * p] = (double)acc.real();
        rec[ORec::T1 + 2 * p + 1] = (double)acc.imag();
        acc *= w16;
    }
    const C w256 = acc;  // (w^16)^16
    acc = C(1, 0);
    for (int r = 0; r < 4; ++r) {
        rec[ORec::T2 + 2 * r] = (double)acc.real();
        rec[ORec::T2 + 2 * r + 1] = (double)acc.imag();
        acc *= w256;
    }
    rec[ORec::WT] = (double)acc.real();  // (w^256)^4 = w^1024
    rec[ORec::WT + 1] = (double)acc.imag();
}

}  // namespace

struct hz_osc {
    hz::Stream stream;
    int N = 0, N_total = 0, begin = 0, device = 0;
    std::vector<double> wr, wi;               // staged frequencies (local)
    std::vector<unsigned char> active;        // local active flags
    std::vector<double> h_rec;
    bool dirty_rec = true, dirty_act = true;
    std::vector<int> act;                     // ascending active local indices
    hz::DevBuf<double> d_rec, d_z, d_partial, d_mix, d_pb;
    hz::DevBuf<int> d_act;
    hz::DevBuf<unsigned char> d_active;
    int target_groups = 256;
    bool prof = false;
    hz::ProfEvents ev;
    long launches = 0;
    // per-sample calls (operator() / mixdown() / tick() of the drop-in) are served from a
    // speculative block: the phasors and mixes of the next la_L samples rendered at once from a
    // snapshot (an Oscbank has no input); setters roll the phasors back to the consumed sample
    // (huygens_hip.h, hz_add_fill)
    long la_L = 0, la_n = 0, la_pos = 0;
    hz::DevBuf<double> d_la_pb, d_la_mix, d_z_snap;
    hz::PinBuf<double> la_mix;         // pinned [la_L][2]
    hz::PinBuf<double> la_pb;          // pinned [la_L][N][2] per-band rows (small banks: N la_L <= 2^18)
};

namespace {

int osc_check(hz_osc* h) {
    return hz::check_handle(h, "hz_osc");
}

int osc_local(const hz_osc* h, int i) {
    if (i < h->begin || i >= h->begin + h->N) return -1;
    return i - h->begin;
}

int osc_upload(hz_osc* h) {
    if (h->dirty_rec) {
        h->h_rec.assign((size_t)h->N * ORec::SIZE, 0.0);
        for (int i = 0; i < h->N; ++i) build_orec(h->wr[i], h->wi[i], &h->h_rec[(size_t)i * ORec::SIZE]);
        HZ_TRY_HIP(hipMemcpyAsync(h->d_rec, h->h_rec.data(), sizeof(double) * h->h_rec.size(),
                                  hipMemcpyHostToDevice, h->stream));
        h->dirty_rec = false;
    }
    if (h->dirty_act) {
        h->act.clear();
        for (int i = 0; i < h->N; ++i)
            if (h->active[i]) h->act.push_back(i);
        if (!h->act.empty())
            HZ_TRY_HIP(hipMemcpyAsync(h->d_act, h->act.data(), sizeof(int) * h->act.size(), hipMemcpyHostToDevice,
                                      h->stream));
        HZ_TRY_HIP(hipMemcpyAsync(h->d_active, h->active.data(), h->N, hipMemcpyHostToDevice, h->stream));
        h->dirty_act = false;
    }
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

int osc_launch(hz_osc* h, double* d_mix, double* d_per_band, long n) {
    if (n <= 0) return HZ_OK;
    const int A = (int)h->act.size();
    hipEvent_t* e = nullptr;
    if (h->prof) {
        HZ_TRY(h->ev.take(2, &e));
        HZ_TRY_HIP(hipEventRecord(e[0], h->stream));
    }
    if (d_per_band) {
        dim3 grid((unsigned)((h->N + 255) / 256), (unsigned)((n + kPbChunk - 1) / kPbChunk));
        hipLaunchKernelGGL(osc_per_band_kernel, grid, dim3(256), 0, h->stream, (const double*)h->d_rec,
                           (const double*)h->d_z, (const unsigned char*)h->d_active, h->N, n, (double2*)d_per_band);
        HZ_TRY_HIP(hipGetLastError());
    }
    if (d_mix && A == 0) HZ_TRY_HIP(hipMemsetAsync(d_mix, 0, sizeof(double) * 2 * n, h->stream));
    if (d_mix && A > 0) {
        // partials per wave and groups: few partial rows, then time segments to fill the CUs
        int per_wave = std::min(kMaxPerWave, std::max(1, (A + kWaves * 32 - 1) / (kWaves * 32)));
        const int G = (A + kWaves * per_wave - 1) / (kWaves * per_wave);
        const hz::MixPlan mp = hz::mix_plan(G, n, kTile, h->target_groups);
        const size_t need = (size_t)G * mp.n_pad * 2;
        HZ_TRY(h->d_partial.reserve(need));
        const size_t lds = sizeof(double) * (2 * plane_len(kL) + kWaves * 2 * kMaxPerWave);
        HZ_TRY(hz::allow_lds(h->device, (const void*)osc_mix_kernel, lds));
        OscArgs a;
        a.act = h->d_act;
        a.z0 = h->d_z;
        a.partial = h->d_partial;
        a.n = n;
        a.n_pad = mp.n_pad;
        a.seg_len = mp.seg_len;
        a.A = A;
        a.nseg = (int)mp.nseg;
        a.per_wave = per_wave;
        hipLaunchKernelGGL(osc_mix_kernel, dim3(G, (unsigned)mp.nseg), dim3(64 * kWaves), lds, h->stream,
                           (const double*)h->d_rec, a);
        HZ_TRY_HIP(hipGetLastError());
        // mix[t] = sum_g partial[g][t]   (complex, interleaved)
        slab_reduce(h->stream, (const double2*)h->d_partial.get(), mp.n_pad, G, n, SlabStore<double2>{(double2*)d_mix});
        HZ_TRY_HIP(hipGetLastError());
    }
    if (e) HZ_TRY_HIP(hipEventRecord(e[1], h->stream));
    if (A > 0) {
        hipLaunchKernelGGL(osc_advance_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, h->stream,
                           (const double*)h->d_rec, (const int*)h->d_act, A, n, h->d_z);
        HZ_TRY_HIP(hipGetLastError());
    }
    h->launches += h->prof ? 1 : 0;
    return HZ_OK;
}

int osc_settle(hz_osc* h) {
    if (h->la_pos < h->la_n) {
        HZ_TRY_HIP(hipMemcpyAsync(h->d_z, h->d_z_snap, sizeof(double) * 2 * h->N, hipMemcpyDeviceToDevice, h->stream));
        const long m = h->la_pos;
        h->la_n = h->la_pos = 0;
        if (m > 0) HZ_TRY(osc_launch(h, nullptr, nullptr, m));   // the consumed ticks again
    }
    h->la_n = h->la_pos = 0;
    return HZ_OK;
}

int osc_look_ahead(hz_osc* h) {
    if (!h->la_L) {
        h->la_L = std::min<long>(1024, std::max<long>(16, (1L << 21) / std::max(1, h->N)));
        HZ_TRY(h->d_la_pb.reserve((size_t)2 * h->la_L * h->N));
        HZ_TRY(h->d_la_mix.reserve((size_t)2 * h->la_L));
        HZ_TRY(h->d_z_snap.reserve((size_t)2 * h->N));
        HZ_TRY(h->la_mix.reserve((size_t)2 * h->la_L));
        if ((long)h->N * h->la_L <= (1L << 18))   // small banks: operator() reads host memory
            HZ_TRY(h->la_pb.reserve((size_t)2 * h->la_L * h->N));
    }
    HZ_TRY(osc_upload(h));
    HZ_TRY_HIP(hipMemcpyAsync(h->d_z_snap, h->d_z, sizeof(double) * 2 * h->N, hipMemcpyDeviceToDevice, h->stream));
    HZ_TRY(osc_launch(h, h->d_la_mix, h->d_la_pb, h->la_L));
    HZ_TRY_HIP(hipMemcpyAsync(h->la_mix, h->d_la_mix, sizeof(double) * 2 * h->la_L, hipMemcpyDeviceToHost, h->stream));
    if (h->la_pb)
        HZ_TRY_HIP(hipMemcpyAsync(h->la_pb, h->d_la_pb, sizeof(double) * 2 * h->la_L * h->N, hipMemcpyDeviceToHost,
                                  h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    h->la_n = h->la_L;
    h->la_pos = 0;
    return HZ_OK;
}

}  // namespace

extern "C" {

int hz_osc_create_shard(int N_total, int begin, int count, double k, int device, hz_osc** out) {
    (void)k;  // Oscbank(double k): stiffness = relaxation(k) is never used (oscbank.h:37,96)
    if (!out || N_total <= 0 || begin < 0 || count <= 0 || begin + count > N_total) {
        hz::set_error("hz_osc_create: invalid arguments");
        return HZ_E_INVALID;
    }
    *out = nullptr;
    HZ_TRY(hz::select_device(device));
    hz_osc* h = new (std::nothrow) hz_osc();
    if (!h) return HZ_E_ALLOC;
    h->N = count;
    h->N_total = N_total;
    h->begin = begin;
    h->device = device;
    h->wr.assign(count, 1.0);  // setOnes (oscbank.h:45-46)
    h->wi.assign(count, 0.0);
    h->active.assign(count, 0);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        h->target_groups = prop.multiProcessorCount;
    auto fail = [&](int code) {
        hz_osc_destroy(h);
        return code;
    };
    if (h->stream.create() != HZ_OK) return fail(HZ_E_HIP);
    if (h->d_rec.reserve((size_t)count * ORec::SIZE) || h->d_z.reserve((size_t)2 * count) ||
        h->d_act.reserve(count) || h->d_active.reserve(count)) {
        hz::set_error("hipMalloc failed for oscbank state");
        return fail(HZ_E_ALLOC);
    }
    std::vector<double> ones(2 * (size_t)count, 0.0);
    for (int i = 0; i < count; ++i) ones[2 * i] = 1.0;  // phases setOnes (oscbank.h:45)
    if (hipMemcpy(h->d_z, ones.data(), sizeof(double) * 2 * count, hipMemcpyHostToDevice) != hipSuccess)
        return fail(HZ_E_HIP);
    *out = h;
    return HZ_OK;
}

int hz_osc_create(int N, double k, int device, hz_osc** out) { return hz_osc_create_shard(N, 0, N, k, device, out); }

int hz_osc_destroy(hz_osc* h) {
    if (!h) return HZ_OK;
    (void)hipSetDevice(h->device);
    (void)h->stream.sync();
    delete h;
    return HZ_OK;
}

int hz_osc_freqmod(hz_osc* h, int index, double hz) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY(osc_check(h));
    HZ_TRY(osc_settle(h));
    const int l = osc_local(h, index);  // out of range: ignored, as oscbank.h:51
    if (l < 0) return HZ_OK;
    h->wr[l] = std::cos(2 * hz::kPI * hz / hz::kSR);
    h->wi[l] = std::sin(2 * hz::kPI * hz / hz::kSR);
    h->dirty_rec = true;
    return HZ_OK;
}

int hz_osc_activate(hz_osc* h, const int* idx, int count) {
    if (!h || (count > 0 && !idx) || count < 0) return HZ_E_INVALID;
    HZ_TRY(osc_check(h));
    HZ_TRY(osc_settle(h));
    for (int c = 0; c < count; ++c) {
        const int l = osc_local(h, idx[c]);  // out of range: ignored (multichannel.h:90)
        if (l >= 0 && !h->active[l]) {
            h->active[l] = 1;
            h->dirty_act = true;
        }
    }
    return HZ_OK;
}

int hz_osc_deactivate(hz_osc* h, const int* idx, int count) {
    if (!h || (count > 0 && !idx) || count < 0) return HZ_E_INVALID;
    HZ_TRY(osc_check(h));
    HZ_TRY(osc_settle(h));
    for (int c = 0; c < count; ++c) {
        const int l = osc_local(h, idx[c]);
        if (l >= 0 && h->active[l]) {
            h->active[l] = 0;
            h->dirty_act = true;
        }
    }
    return HZ_OK;
}

int hz_osc_open(hz_osc* h) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY(osc_check(h));
    HZ_TRY(osc_settle(h));
    std::fill(h->active.begin(), h->active.end(), 1);
    h->dirty_act = true;
    return HZ_OK;
}

int hz_osc_close(hz_osc* h) {
    if (!h) return HZ_E_INVALID;
    HZ_TRY(osc_check(h));
    HZ_TRY(osc_settle(h));
    std::fill(h->active.begin(), h->active.end(), 0);
    h->dirty_act = true;
    return HZ_OK;
}

int hz_osc_active_count(hz_osc* h, int* count) {
    if (!h || !count) return HZ_E_INVALID;
    int c = 0;
    for (unsigned char a : h->active) c += a ? 1 : 0;
    *count = c;
    return HZ_OK;
}

int hz_osc_fill_device(hz_osc* h, double* d_mix, double* d_per_band, size_t n) {
    HZ_TRY(osc_check(h));
    if (n == 0) return HZ_OK;
    HZ_TRY(osc_settle(h));
    HZ_TRY(osc_upload(h));
    return osc_launch(h, d_mix, d_per_band, (long)n);
}

int hz_osc_fill(hz_osc* h, double* mix, double* per_band, size_t n) {
    HZ_TRY(osc_check(h));
    if (n == 0) return HZ_OK;
    if (n == 1 && !mix && !per_band) {   // tick(): from the speculative block
        if (h->la_pos == h->la_n) HZ_TRY(osc_look_ahead(h));
        ++h->la_pos;
        return HZ_OK;
    }
    HZ_TRY(osc_settle(h));
    if (mix) HZ_TRY(h->d_mix.reserve(2 * n));
    const size_t pbn = 2 * n * (size_t)h->N;
    if (per_band) HZ_TRY(h->d_pb.reserve(pbn));
    HZ_TRY(osc_upload(h));
    HZ_TRY(osc_launch(h, mix ? h->d_mix : nullptr, per_band ? h->d_pb : nullptr, (long)n));
    if (mix) HZ_TRY_HIP(hipMemcpyAsync(mix, h->d_mix, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, h->stream));
    if (per_band)
        HZ_TRY_HIP(hipMemcpyAsync(per_band, h->d_pb, sizeof(double) * pbn, hipMemcpyDeviceToHost, h->stream));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

int hz_osc_phases(hz_osc* h, double* z) {
    HZ_TRY(osc_check(h));
    if (!z) return HZ_E_INVALID;
    if (h->la_L) {   // per-sample use: the row of the speculative block
        if (h->la_pos == h->la_n) HZ_TRY(osc_look_ahead(h));
        if (h->la_pb) {
            std::memcpy(z, h->la_pb + 2 * (size_t)h->la_pos * h->N, sizeof(double) * 2 * h->N);
            return HZ_OK;
        }
        HZ_TRY_HIP(hipMemcpyAsync(z, h->d_la_pb + 2 * (size_t)h->la_pos * h->N, sizeof(double) * 2 * h->N,
                                  hipMemcpyDeviceToHost, h->stream));
        HZ_TRY_HIP(hipStreamSynchronize(h->stream));
        return HZ_OK;
    }
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    HZ_TRY_HIP(hipMemcpy(z, h->d_z, sizeof(double) * 2 * h->N, hipMemcpyDeviceToHost));
    return HZ_OK;
}

int hz_osc_mixdown(hz_osc* h, double* mix) {   // oscbank.h:81-90, without advancing
    HZ_TRY(osc_check(h));
    if (!mix) return HZ_E_INVALID;
    if (h->la_L) {   // per-sample use: the speculative block's mix (the engine's summation order)
        if (h->la_pos == h->la_n) HZ_TRY(osc_look_ahead(h));
        mix[0] = h->la_mix[2 * h->la_pos];
        mix[1] = h->la_mix[2 * h->la_pos + 1];
        return HZ_OK;
    }
    std::vector<double> z(2 * (size_t)h->N);
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    HZ_TRY_HIP(hipMemcpy(z.data(), h->d_z, sizeof(double) * z.size(), hipMemcpyDeviceToHost));
    double re = 0.0, im = 0.0;
    for (int i = 0; i < h->N; ++i)   // ascending active indices, as `where`
        if (h->active[i]) {
            re += z[2 * i];
            im += z[2 * i + 1];
        }
    mix[0] = re;
    mix[1] = im;
    return HZ_OK;
}

int hz_osc_set_phases(hz_osc* h, const double* z) {
    HZ_TRY(osc_check(h));
    if (!z) return HZ_E_INVALID;
    HZ_TRY(osc_settle(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    HZ_TRY_HIP(hipMemcpy(h->d_z, z, sizeof(double) * 2 * h->N, hipMemcpyHostToDevice));
    return HZ_OK;
}

int hz_osc_set_stream(hz_osc* h, void* s) {
    HZ_TRY(osc_check(h));
    return h->stream.rebind(s, hz::NullMeans::Private);
}

int hz_osc_synchronize(hz_osc* h) {
    HZ_TRY(osc_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    return HZ_OK;
}

int hz_osc_set_target_groups(hz_osc* h, int groups) {
    if (!h || groups < 1) return HZ_E_INVALID;
    h->target_groups = groups;
    return HZ_OK;
}

int hz_osc_profile(hz_osc* h, int enable) {
    HZ_TRY(osc_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    h->prof = enable != 0;
    h->ev.rewind();
    h->launches = 0;
    return HZ_OK;
}

int hz_osc_profile_read(hz_osc* h, double* ms, long* launches) {
    HZ_TRY(osc_check(h));
    HZ_TRY_HIP(hipStreamSynchronize(h->stream));
    double m = 0;
    HZ_TRY(h->ev.elapsed(2, 0, 1, &m));   // (no rewind: a read keeps the counters)
    if (ms) *ms = m;
    if (launches) *launches = h->launches;
    return HZ_OK;
}

}  // extern "C"
