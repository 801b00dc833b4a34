// hz_fb_events.h -- host side of hz_fb_process_events: validates an hz_fb_event array and compiles
// it, per band, into the table the general engine's event form reads (hz_filterbank.hip,
// fb_mix_kernel<.., EV>).  Self-contained host code without a HIP dependency: a plain C++ compiler
// can include it (tests/cpp/fb_events_host.cpp).
//
// A band's smoothers are one-pole (src/filterbank.h:172-173): pre[t] = (1 - sp) pin + sp pre[t-1].
// With a target that changes at samples t_1 < t_2 < ... the closed form the kernel seeds its lanes
// with becomes piecewise: row k of a band holds
//     { t_k, pin_k, gin_k, P_k, G_k }
// the targets in force from sample t_k on and the smoother values ENTERING sample t_k (pre[t_k - 1],
// gain[t_k - 1]), so for t_k <= t < t_{k+1}
//     pre entering t = pin_k + sp^(t - t_k) (P_k - pin_k).
// Row 0 of a band sits at t = 0 with the call's start values; the last row sits at t = n: its
// targets are the ones staged for the next call (events with at == n included) and its P, G the
// end-of-call smoother state.  Only bands that have events get rows (CSR offsets seg_off).
#pragma once

#include <cmath>
#include <vector>

#include "../../include/huygens_hip.h"

namespace hz_fbev {

constexpr int kRow = 5;   // doubles per row
enum { kT = 0, kPin = 1, kGin = 2, kP = 3, kG = 4 };

struct Plan {
    std::vector<int> seg_off;    // [N_local + 1]: rows of local band b are [seg_off[b], seg_off[b + 1])
    std::vector<double> rows;    // [seg_off[N_local]][kRow]
    std::vector<int> bands;      // local bands that have rows, ascending
};

// s^d for an integer distance d >= 0; s = 0 (k = 0: an instant smoother) gives 1 at d = 0
inline double pow_steps(double s, long d) { return d == 0 ? 1.0 : std::pow(s, (double)d); }

// the smoother value v after d samples toward `target`
inline double advance(double v, double target, double s, long d) { return target + pow_steps(s, d) * (v - target); }

// HZ_OK, or the code of the first offending event (nothing is written on an error); *bad gets its
// index (-1: the array itself)
inline int validate(const hz_fb_event* ev, int nev, long n, int N_total, int* bad = nullptr) {
    if (bad) *bad = -1;
    if (nev < 0 || (nev > 0 && !ev) || n < 0) return HZ_E_INVALID;
    long prev = 0;
    for (int i = 0; i < nev; ++i) {
        if (bad) *bad = i;
        if (ev[i].kind != HZ_FB_EV_BOOST && ev[i].kind != HZ_FB_EV_MIX) return HZ_E_INVALID;
        if (ev[i].at < prev || ev[i].at > n) return HZ_E_INVALID;
        if (ev[i].band < -1 || ev[i].band >= N_total) return HZ_E_RANGE;
        prev = ev[i].at;
    }
    if (bad) *bad = -1;
    return HZ_OK;
}

// Compiles ev[0 .. nev) for the n samples that start at sample t_base of the caller's array (event
// times are at - t_base, at most n; an event before t_base counts as one at it: a setter made
// before a sample that was already computed) for the shard [band_begin, band_begin + N_local) of an
// N_total-band bank.  pin / gin [N_local]: the targets in force before the first event; pg
// [N_local][2]: pre, gain entering sample 0.  The events are validated first (against t_base + n).
inline int compile(const hz_fb_event* ev, int nev, long t_base, long n, int N_total, int band_begin, int N_local,
                   double sp, double sg, const double* pin, const double* gin, const double* pg, Plan* out) {
    const int rc = validate(ev, nev, t_base + n, N_total);
    if (rc != HZ_OK) return rc;
    // events per local band (band -1: every band), then their indices in array order
    std::vector<int> cnt((size_t)N_local + 1, 0);
    int all = 0;
    for (int i = 0; i < nev; ++i) {
        if (ev[i].band < 0) ++all;
        else if (ev[i].band >= band_begin && ev[i].band < band_begin + N_local) ++cnt[ev[i].band - band_begin];
    }
    std::vector<int> eoff((size_t)N_local + 1, 0);
    for (int b = 0; b < N_local; ++b) eoff[b + 1] = eoff[b] + cnt[b] + all;
    std::vector<int> eidx((size_t)eoff[N_local]);
    std::vector<int> fill(eoff.begin(), eoff.end() - 1);
    for (int i = 0; i < nev; ++i) {
        if (ev[i].band < 0) {
            for (int b = 0; b < N_local; ++b) eidx[fill[b]++] = i;
        } else if (ev[i].band >= band_begin && ev[i].band < band_begin + N_local) {
            eidx[fill[ev[i].band - band_begin]++] = i;
        }
    }
    out->seg_off.assign((size_t)N_local + 1, 0);
    out->rows.clear();
    out->bands.clear();
    for (int b = 0; b < N_local; ++b) {
        out->seg_off[b] = (int)(out->rows.size() / kRow);
        if (eoff[b + 1] == eoff[b]) continue;
        out->bands.push_back(b);
        double row[kRow] = {0.0, pin[b], gin[b], pg[2 * (size_t)b], pg[2 * (size_t)b + 1]};
        const size_t first = out->rows.size();
        auto push = [&]() { out->rows.insert(out->rows.end(), row, row + kRow); };
        auto move_to = [&](long t) {   // close the row in force and open one at t > its t_k
            const long d = t - (long)row[kT];
            row[kP] = advance(row[kP], row[kPin], sp, d);
            row[kG] = advance(row[kG], row[kGin], sg, d);
            row[kT] = (double)t;
        };
        for (int e = eoff[b]; e < eoff[b + 1]; ++e) {
            const hz_fb_event& v = ev[eidx[e]];
            const long t = v.at > t_base ? v.at - t_base : 0;
            if (t > (long)row[kT]) {   // equal `at`: the same row, the last value on a kind wins
                push();
                move_to(t);
            }
            row[v.kind == HZ_FB_EV_BOOST ? kPin : kGin] = v.value;
        }
        // the end row at t = n (already open when an event sat at n; a call of no samples gets
        // a second row all the same: first and last row, both at 0)
        if ((long)row[kT] < n || out->rows.size() == first) {
            push();
            move_to(n);
        }
        push();
    }
    out->seg_off[N_local] = (int)(out->rows.size() / kRow);
    return HZ_OK;
}

}  // namespace hz_fbev
