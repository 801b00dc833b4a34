// Host check of the event compiler of hz_fb_process_events (huygens_amd/csrc/hz_fb_events.h): a
// stand-alone program, plain g++, no HIP runtime.  Every compiled table is compared with a plain
// per-sample loop of the two one-pole smoothers (src/filterbank.h:172-173) driven by the same
// events applied as setters before their sample: row times, the targets in force, the smoother
// values entering each row (1e-12 relative) and the end state; plus band -1 expansion, shard
// filtering, equal-`at` collapse, the CSR offsets, and every error code with nothing written.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../huygens_amd/csrc/hz_fb_events.h"

namespace {

int g_cases = 0;

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// 1e-12 relative to the smoother's scale, the larger of the value and the target it moves toward:
// a gain on its way from -0.4 to 0.8 passes through zero, where an error relative to the value
// itself would have no bound
bool close(double a, double b, double scale) {
    return std::fabs(a - b) <= 1e-12 * std::fmax(std::fmax(std::fabs(a), std::fabs(b)), std::fabs(scale));
}

hz_fb_event E(long at, int band, int kind, double v) {
    hz_fb_event e;
    e.at = at, e.band = band, e.kind = kind, e.value = v;
    return e;
}

struct Bank {
    int N_total, begin, N;
    double sp, sg;
    std::vector<double> pin, gin, pg;
};

Bank make_bank(int N_total, int begin, int N, double sp, double sg) {
    Bank b{N_total, begin, N, sp, sg, {}, {}, {}};
    for (int i = 0; i < N; ++i) {
        b.pin.push_back(0.5 + 0.01 * i);
        b.gin.push_back(1.0 - 0.003 * i);
        b.pg.push_back(0.2 + 0.02 * i);    // pre
        b.pg.push_back(-0.4 + 0.01 * i);   // gain
    }
    return b;
}

// the split sequence of one local band, sample by sample: pre[t], gain[t] ENTERING sample t for
// t in [0, n], and the targets in force at each t (setters with at == t applied before it)
struct Track {
    std::vector<double> pre, gain, pin, gin;
};

Track per_sample(const Bank& B, int local, const std::vector<hz_fb_event>& ev, long t_base, long n) {
    Track T;
    double pin = B.pin[local], gin = B.gin[local], p = B.pg[2 * local], g = B.pg[2 * local + 1];
    size_t i = 0;
    for (long t = 0; t <= n; ++t) {
        while (i < ev.size() && ev[i].at - t_base <= t) {
            const bool mine = ev[i].band == -1 || ev[i].band == B.begin + local;
            if (mine) (ev[i].kind == HZ_FB_EV_BOOST ? pin : gin) = ev[i].value;
            ++i;
        }
        T.pre.push_back(p), T.gain.push_back(g), T.pin.push_back(pin), T.gin.push_back(gin);
        p = (1.0 - B.sp) * pin + B.sp * p;
        g = (1.0 - B.sg) * gin + B.sg * g;
    }
    return T;
}

// compiles and checks every row of every band against the per-sample loop; -> rows in the table
int check_case(const Bank& B, const std::vector<hz_fb_event>& ev, long t_base, long n) {
    hz_fbev::Plan P;
    const int rc = hz_fbev::compile(ev.data(), (int)ev.size(), t_base, n, B.N_total, B.begin, B.N, B.sp, B.sg,
                                    B.pin.data(), B.gin.data(), B.pg.data(), &P);
    REQUIRE(rc == HZ_OK);
    REQUIRE((int)P.seg_off.size() == B.N + 1);
    REQUIRE(P.seg_off[0] == 0);
    REQUIRE((size_t)P.seg_off[B.N] * hz_fbev::kRow == P.rows.size());
    size_t nb = 0;
    for (int b = 0; b < B.N; ++b) {
        bool has = false;
        for (const hz_fb_event& e : ev) has = has || e.band == -1 || e.band == B.begin + b;
        const int r0 = P.seg_off[b], r1 = P.seg_off[b + 1];
        REQUIRE(r1 >= r0);
        if (!has) {
            REQUIRE(r1 == r0);   // out-of-shard and untouched bands get no rows
            continue;
        }
        REQUIRE(nb < P.bands.size() && P.bands[nb] == b);
        ++nb;
        REQUIRE(r1 - r0 >= 2);
        const Track T = per_sample(B, b, ev, t_base, n);
        const double* rw = &P.rows[(size_t)r0 * hz_fbev::kRow];
        REQUIRE(rw[hz_fbev::kT] == 0.0);
        REQUIRE(P.rows[(size_t)(r1 - 1) * hz_fbev::kRow + hz_fbev::kT] == (double)n);
        for (int k = r0; k < r1; ++k, rw += hz_fbev::kRow) {
            const long t = (long)rw[hz_fbev::kT];
            if (k > r0 && n > 0) REQUIRE(rw[hz_fbev::kT] > rw[hz_fbev::kT - hz_fbev::kRow]);   // collapsed: distinct times
            REQUIRE(t >= 0 && t <= n);
            REQUIRE(rw[hz_fbev::kPin] == T.pin[t] && rw[hz_fbev::kGin] == T.gin[t]);
            REQUIRE(close(rw[hz_fbev::kP], T.pre[t], t ? T.pin[t - 1] : 0.0));
            REQUIRE(close(rw[hz_fbev::kG], T.gain[t], t ? T.gin[t - 1] : 0.0));
            // inside the row, the kernel's seed: target + s^(t - t_k) (value - target)
            const long t_end = k + 1 < r1 ? (long)rw[hz_fbev::kRow + hz_fbev::kT] : n;
            for (long u = t; u <= t_end; u += 1 + (t_end - t) / 7) {
                REQUIRE(close(hz_fbev::advance(rw[hz_fbev::kP], rw[hz_fbev::kPin], B.sp, u - t), T.pre[u], rw[hz_fbev::kPin]));
                REQUIRE(close(hz_fbev::advance(rw[hz_fbev::kG], rw[hz_fbev::kGin], B.sg, u - t), T.gain[u], rw[hz_fbev::kGin]));
            }
        }
    }
    REQUIRE(nb == P.bands.size());
    ++g_cases;
    return P.seg_off[B.N];
}

void check_error(const Bank& B, const std::vector<hz_fb_event>& ev, int nev, long n, int want) {
    hz_fbev::Plan P;
    P.seg_off.assign(3, 77);
    P.rows.assign(4, -5.0);
    P.bands.assign(2, 9);
    int bad = -2;
    REQUIRE(hz_fbev::validate(ev.data(), nev, n, B.N_total, &bad) == want);
    REQUIRE(hz_fbev::compile(ev.data(), nev, 0, n, B.N_total, B.begin, B.N, B.sp, B.sg, B.pin.data(), B.gin.data(),
                             B.pg.data(), &P) == want);
    REQUIRE(P.seg_off == std::vector<int>(3, 77) && P.rows == std::vector<double>(4, -5.0) &&
            P.bands == std::vector<int>(2, 9));   // nothing written
    ++g_cases;
}

}  // namespace

int main() {
    const int BO = HZ_FB_EV_BOOST, MI = HZ_FB_EV_MIX;
    // positions around the 16-sample chunk and the 1024-sample tile, two events inside one chunk,
    // equal `at` on one band and kind (the last wins), BOOST and MIX at one `at`, the last band
    const std::vector<hz_fb_event> pos = {
        E(0, 3, BO, 1.5),    E(0, -1, MI, 0.8),  E(1, 3, MI, 0.2),     E(15, 4, BO, 2.0),   E(16, 4, MI, 0.1),
        E(17, 4, BO, 0.3),   E(20, 4, BO, 0.9),  E(500, 7, BO, 1.0),   E(500, 7, BO, 3.0),  E(500, 7, MI, 0.4),
        E(1023, 36, BO, 2.5), E(1024, 36, MI, 0.0), E(1025, 0, BO, 0.7), E(2999, 5, MI, 1.2), E(3000, 5, BO, 4.0),
        E(3000, -1, MI, 0.5)};
    for (double sp : {0.95122942450071402, 0.0}) {
        for (double sg : {0.74081822068171788, 0.99004983374916811}) {
            const Bank B = make_bank(37, 0, 37, sp, sg);
            const int rows = check_case(B, pos, 0, 3000);
            // band 7: rows at 0, 500, 3000 -- the three events at 500 collapse into one row
            hz_fbev::Plan P;
            REQUIRE(hz_fbev::compile(pos.data(), (int)pos.size(), 0, 3000, 37, 0, 37, sp, sg, B.pin.data(),
                                     B.gin.data(), B.pg.data(), &P) == HZ_OK);
            REQUIRE(P.seg_off[8] - P.seg_off[7] == 3);
            REQUIRE(P.rows[(size_t)(P.seg_off[7] + 1) * hz_fbev::kRow + hz_fbev::kPin] == 3.0);
            // band 4: 0, 15, 16, 17, 20, 3000; a band only the -1 events touch: 0 and 3000
            REQUIRE(P.seg_off[5] - P.seg_off[4] == 6);
            REQUIRE(P.seg_off[21] - P.seg_off[20] == 2);
            REQUIRE(rows == P.seg_off[37]);
            if (sp == 0.0) {   // an instant pre-amp: pre == pin from the event's own sample on
                const double* rw = &P.rows[(size_t)(P.seg_off[4] + 2) * hz_fbev::kRow];   // t = 16 (after BOOST at 15)
                REQUIRE(rw[hz_fbev::kT] == 16.0 && rw[hz_fbev::kP] == 2.0);
            }
        }
    }
    // shards: global indices, out-of-shard bands dropped, -1 is every band of the shard
    const std::vector<hz_fb_event> sh = {E(3, 5, BO, 2.0),   E(3, 128, BO, 1.1), E(9, 227, MI, 0.3),
                                         E(9, 228, MI, 0.6), E(40, -1, BO, 0.9), E(77, 299, MI, 0.2)};
    REQUIRE(check_case(make_bank(300, 0, 128, 0.9, 0.8), sh, 0, 100) == 3 * 128 + 1);      // band 5: one more row
    REQUIRE(check_case(make_bank(300, 128, 100, 0.9, 0.8), sh, 0, 100) == 3 * 100 + 2);    // bands 128, 227
    REQUIRE(check_case(make_bank(300, 228, 72, 0.9, 0.8), sh, 0, 100) == 3 * 72 + 2);      // bands 228, 299
    // no band of the shard: an empty table
    REQUIRE(check_case(make_bank(300, 128, 100, 0.9, 0.8), {E(3, 5, BO, 2.0)}, 0, 100) == 0);
    // dense: 300 events on one band of nine, -1 events interleaved
    {
        std::vector<hz_fb_event> d;
        for (int i = 0; i < 300; ++i) {
            d.push_back(E(8 * i + (i % 3), 4, i % 2 ? MI : BO, 0.1 * (i % 17)));
            if (i % 50 == 0) d.push_back(E(8 * i + (i % 3), -1, MI, 0.01 * i));
        }
        check_case(make_bank(9, 0, 9, 0.97, 0.5), d, 0, 2500);
    }
    // tiny calls
    check_case(make_bank(5, 0, 5, 0.9, 0.8), {E(0, 1, BO, 2.0), E(1, 1, MI, 0.3)}, 0, 1);
    check_case(make_bank(5, 0, 5, 0.9, 0.8), {E(0, 1, BO, 2.0), E(0, -1, MI, 0.3)}, 0, 0);
    check_case(make_bank(5, 0, 5, 0.0, 0.0), {E(2, 1, BO, 2.0), E(5, -1, MI, 0.3)}, 0, 5);
    check_case(make_bank(5, 0, 5, 0.9, 0.8), {}, 0, 64);
    // a piece of a longer call: times count from t_base; an event before it counts as one at it
    check_case(make_bank(37, 0, 37, 0.95, 0.7), {E(1000, 2, BO, 2.0), E(1024, 2, MI, 0.5), E(1500, -1, BO, 1.0)}, 1000,
               500);
    check_case(make_bank(37, 0, 37, 0.95, 0.7), {E(0, 2, BO, 2.0), E(1, 3, MI, 0.5), E(9, 3, BO, 1.0)}, 1, 20);
    // errors: the stated code, nothing written
    const Bank B = make_bank(37, 0, 37, 0.9, 0.8);
    check_error(B, {E(5, 1, BO, 1.0), E(4, 1, BO, 1.0)}, 2, 100, HZ_E_INVALID);   // descending at
    check_error(B, {E(101, 1, BO, 1.0)}, 1, 100, HZ_E_INVALID);                   // at = n + 1
    check_error(B, {E(-1, 1, BO, 1.0)}, 1, 100, HZ_E_INVALID);                    // at < 0
    check_error(B, {E(5, 1, 2, 1.0)}, 1, 100, HZ_E_INVALID);                      // kind = 2
    check_error(B, {E(5, 37, BO, 1.0)}, 1, 100, HZ_E_RANGE);                      // band = N
    check_error(B, {E(5, -2, MI, 1.0)}, 1, 100, HZ_E_RANGE);                      // band = -2
    check_error(B, {E(5, 1, BO, 1.0)}, -1, 100, HZ_E_INVALID);                    // nev < 0
    check_error(B, {E(5, 1, BO, 1.0), E(6, 36, MI, 1.0), E(7, 40, MI, 1.0)}, 3, 100, HZ_E_RANGE);   // the last one bad
    std::printf("fb_events ok: %d cases\n", g_cases);
    return 0;
}
