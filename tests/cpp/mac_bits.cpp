// The stationary engine's MAC kernels against each other, bit for bit (tests/test_mac_bits_gpu.py):
// resp_mac_kernel<8, QP> (operands in registers) and resp_mac_kernel_lds<QP> as the library builds
// it (operands staged through LDS) on the same seeded H and Z, for QP in {8, 16, 24}, Q in {QP - 7,
// QP - 1, QP} (zero-padded partitions, and Z rows below 0 read as row 0) and B in {1, 8, 31, 32,
// 33, 65} output blocks.  Every byte of Y must agree, the rows past B must stay untouched, and a
// sample of bins is checked against the same FMAs on the host.  The stage splits behind the
// HZ_MAC_STAGE hook (8 steps at QP = 16 and 24, 12 at 24) are held to the same bytes.
// Compiled as HIP for gfx950.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../huygens_amd/csrc/hz_fb_mac.h"

namespace hz {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}
}  // namespace hz

#define CHECK_HIP(expr)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            std::fprintf(stderr, "%s: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__); \
            return 2;                                                                        \
        }                                                                                    \
    } while (0)

namespace {

using hz_mac::kH;
constexpr int kGuard = 8;          // Y rows past B: never written
constexpr int kMaxB = 65, kMaxQp = 24;
constexpr int kZRows = (kMaxB + 127) / 128 * 128 + kMaxQp;   // the engine's own row count (run_resp: zrows)

uint64_t g_seed = 0x243F6A8885A308D3ull;
double rnd() {   // splitmix64 -> (-1, 1), every mantissa bit in play
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(int64_t)z * (1.0 / 9223372036854775808.0);
}

template <int QP, int S = hz_mac::mac_stage<QP>()>
int launch_lds(int B, const double2* H, const double2* Z, double2* Y, int Q) {
    return hz_mac::launch_mac_lds_qp<QP, S>(0, B, H, Z, Y, Q, nullptr);
}

// the same FMAs in the same order as the kernels' step, on the host
void host_bin(const std::vector<double2>& H, const std::vector<double2>& Z, int Qp, int Q, int b, int q, double* yr, double* yi) {
    double ar = 0.0, ai = 0.0;
    for (int p = 0; p < Qp; ++p) {
        const long row = (long)b + Q - 1 - p;
        const double2 h = H[(size_t)p * kH + q], z = Z[(size_t)(row > 0 ? row : 0) * kH + q];
        ar = std::fma(h.x, z.x, ar);
        ar = std::fma(-h.y, z.y, ar);
        ai = std::fma(h.x, z.y, ai);
        ai = std::fma(h.y, z.x, ai);
    }
    *yr = ar;
    *yi = ai;
}

}  // namespace

int main() {
    CHECK_HIP(hipSetDevice(0));
    const size_t hn = (size_t)kMaxQp * kH, zn = (size_t)kZRows * kH, yn = (size_t)(kMaxB + kGuard) * kH;
    std::vector<double2> H(hn), Z(zn), Ya(yn), Yb(yn);
    for (auto& v : Z) v = make_double2(rnd(), rnd());
    double2 *dH = nullptr, *dZ = nullptr, *dYa = nullptr, *dYb = nullptr;
    CHECK_HIP(hipMalloc(&dH, hn * sizeof(double2)));
    CHECK_HIP(hipMalloc(&dZ, zn * sizeof(double2)));
    CHECK_HIP(hipMalloc(&dYa, yn * sizeof(double2)));
    CHECK_HIP(hipMalloc(&dYb, yn * sizeof(double2)));
    CHECK_HIP(hipMemcpy(dZ, Z.data(), zn * sizeof(double2), hipMemcpyHostToDevice));
    int cases = 0, bad = 0;
    for (int Qp : {8, 16, 24})
        for (int Q : {Qp - 7, Qp - 1, Qp}) {
            for (size_t i = 0; i < hn; ++i)   // rows >= Q: the zero spectra the partitions are padded with
                H[i] = i < (size_t)Q * kH ? make_double2(rnd(), rnd()) : make_double2(0.0, 0.0);
            CHECK_HIP(hipMemcpy(dH, H.data(), hn * sizeof(double2), hipMemcpyHostToDevice));
            for (int B : {1, 8, 31, 32, 33, 65}) {
                CHECK_HIP(hipMemset(dYa, 0xFF, yn * sizeof(double2)));
                CHECK_HIP(hipMemset(dYb, 0xFF, yn * sizeof(double2)));
                const unsigned nreg = (unsigned)((kH / 256) * ((B + hz_mac::kMacR - 1) / hz_mac::kMacR));
                hipLaunchKernelGGL(hz_mac::pick_mac(Qp), dim3(nreg), dim3(256), 0, nullptr, dH, dZ, dYa, Q, Qp, B);
                CHECK_HIP(hipGetLastError());
                const int r = Qp == 8 ? launch_lds<8>(B, dH, dZ, dYb, Q)
                              : Qp == 16 ? launch_lds<16>(B, dH, dZ, dYb, Q) : launch_lds<24>(B, dH, dZ, dYb, Q);
                if (r != HZ_OK) return 2;
                CHECK_HIP(hipGetLastError());
                CHECK_HIP(hipDeviceSynchronize());
                CHECK_HIP(hipMemcpy(Ya.data(), dYa, yn * sizeof(double2), hipMemcpyDeviceToHost));
                CHECK_HIP(hipMemcpy(Yb.data(), dYb, yn * sizeof(double2), hipMemcpyDeviceToHost));
                ++cases;
                size_t diff = 0, guard = 0, host = 0;
                const unsigned char *pa = (const unsigned char*)Ya.data(), *pb = (const unsigned char*)Yb.data();
                const size_t used = (size_t)B * kH * sizeof(double2);
                for (size_t i = 0; i < used; i += sizeof(double2)) diff += std::memcmp(pa + i, pb + i, sizeof(double2)) != 0;
                for (size_t i = used; i < yn * sizeof(double2); ++i) guard += (pa[i] != 0xFF) + (pb[i] != 0xFF);
                for (int b = 0; b < B; ++b)
                    for (int q = (b * 5) % 37; q < kH; q += 37) {
                        double yr, yi;
                        host_bin(H, Z, Qp, Q, b, q, &yr, &yi);
                        const double2 y = Ya[(size_t)b * kH + q];
                        host += std::memcmp(&yr, &y.x, 8) != 0 || std::memcmp(&yi, &y.y, 8) != 0;
                    }
                // the staged splits: the same bytes, the same untouched rows
                for (int S : {8, 12}) {
                    if (Qp == 8 || Qp % S) continue;
                    CHECK_HIP(hipMemset(dYb, 0xFF, yn * sizeof(double2)));
                    const int rs = Qp == 16 ? launch_lds<16, 8>(B, dH, dZ, dYb, Q)
                                   : S == 8 ? launch_lds<24, 8>(B, dH, dZ, dYb, Q) : launch_lds<24, 12>(B, dH, dZ, dYb, Q);
                    if (rs != HZ_OK) return 2;
                    CHECK_HIP(hipGetLastError());
                    CHECK_HIP(hipMemcpy(Yb.data(), dYb, yn * sizeof(double2), hipMemcpyDeviceToHost));
                    for (size_t i = 0; i < used; i += sizeof(double2)) diff += std::memcmp(pa + i, pb + i, sizeof(double2)) != 0;
                    for (size_t i = used; i < yn * sizeof(double2); ++i) guard += pb[i] != 0xFF;
                }
                if (diff || guard || host) {
                    ++bad;
                    std::printf("Qp %d Q %d B %d: %zu elements differ, %zu guard bytes written, %zu host mismatches\n",
                                Qp, Q, B, diff, guard, host);
                }
            }
        }
    std::printf("mac_bits: %d cases, %d bad; the library's stages: %d (Qp 16) and %d (Qp 24) steps\n", cases, bad,
                hz_mac::mac_stage<16>(), hz_mac::mac_stage<24>());
    if (cases == 54 && bad == 0) std::printf("mac_bits ok\n");
    return bad ? 1 : 0;
}
