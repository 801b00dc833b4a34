"""numpy twin of the Filterbank event form (TEST INFRASTRUCTURE).

hz_fb_process_events compiles its events per band into rows {t_k, pin_k, gin_k, P_k, G_k}
(huygens_amd/csrc/hz_fb_events.h) and the general engine's event form (hz_filterbank.hip,
fb_mix_kernel<.., EV>) turns them into the per-sample pre-amp and gain of every lane:

    seed at the lane's chunk start tc:  v = target_k + s^(tc - t_k) (V_k - target_k),  k the row in force at tc
    then per sample t = tc .. tc + 15:  the target switches to the next row's when t reaches its t_k;
                                        v = s v + (1 - s) target

compile_rows restates the host compiler, lane_track the kernel's per-lane arithmetic, and
run_events_split drives any Filterbank-like object (oracle or GPU) through the same events as
setter calls between process() pieces -- the reference of every events test.
"""
from __future__ import annotations

import numpy as np

EV_BOOST, EV_MIX = 0, 1
CHUNK, TILE = 16, 1024
T, PIN, GIN, P, G = range(5)


def run_events_split(fb, x, events):
    """n x {setters with at == t; out[t] = F(x[t]); F.tick()}: process() on the pieces between
    distinct `at` values, boost / mix between them (band -1: every band, as a vector setter)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(len(x))
    pos = 0
    N = fb.N
    for at, band, kind, value in events:
        at = int(at)
        if at > pos:
            out[pos:at] = fb.process(x[pos:at])
            pos = at
        setter = fb.boost if kind == EV_BOOST else fb.mix
        if band < 0:
            setter(np.full(N, float(value)))
        else:
            setter(int(band), float(value))
    if pos < len(x):
        out[pos:] = fb.process(x[pos:])
    return out


def positions_events(N, n):
    """the positions case of the CPU and GPU tests: around the 16-sample chunk and the 1024-sample tile, the call's
    first and last sample and its end; two events in one chunk; equal `at` on one band and kind;
    BOOST and MIX at one `at`; the last band"""
    return [(0, 3, EV_BOOST, 1.5), (0, -1, EV_MIX, 0.8), (1, 3, EV_MIX, 0.2), (15, 4, EV_BOOST, 2.0),
            (16, 4, EV_MIX, 0.1), (17, 4, EV_BOOST, 0.3), (20, 4, EV_BOOST, 0.9), (500, 7, EV_BOOST, 1.0),
            (500, 7, EV_BOOST, 3.0), (500, 7, EV_MIX, 0.4), (1023, N - 1, EV_BOOST, 2.5), (1024, N - 1, EV_MIX, 0.0),
            (1025, 0, EV_BOOST, 0.7), (n - 1, 5, EV_MIX, 1.2), (n, 5, EV_BOOST, 4.0), (n, -1, EV_MIX, 0.5)]


def compile_rows(events, n, band_begin, N_local, sp, sg, pin, gin, pg):
    """-> {local band: rows [K][5]} for the bands that have events (hz_fbev::compile)."""
    def adv(v, target, s, d):
        return target + (1.0 if d == 0 else s ** d) * (v - target)

    table = {}
    for b in range(N_local):
        mine = [e for e in events if e[1] < 0 or e[1] == band_begin + b]
        if not mine:
            continue
        row = [0.0, float(pin[b]), float(gin[b]), float(pg[b][0]), float(pg[b][1])]
        rows = []

        def move_to(t):
            d = t - int(row[T])
            row[P] = adv(row[P], row[PIN], sp, d)
            row[G] = adv(row[G], row[GIN], sg, d)
            row[T] = float(t)

        for at, _, kind, value in mine:
            if at > row[T]:
                rows.append(list(row))
                move_to(int(at))
            row[PIN if kind == EV_BOOST else GIN] = float(value)
        if row[T] < n or not rows:
            rows.append(list(row))
            move_to(n)
        rows.append(list(row))
        table[b] = np.array(rows)
    return table


def lane_track(rows, which, s, n):
    """The smoother (which = 0 pre, 1 gain) of one band at every sample t < n as the kernel's lanes
    compute it: per 16-sample chunk the closed-form seed from the row in force at the chunk start,
    then the recurrence with the targets switching inside the chunk."""
    out = np.zeros(n)
    t_rows = rows[:, T]
    for tc in range(0, n, CHUNK):
        k = int(np.searchsorted(t_rows, tc, side="right")) - 1   # largest k with t_k <= tc
        target = rows[k, PIN + which]
        d = tc - t_rows[k]
        w = 1.0 if d == 0 else s ** d
        v = target + w * (rows[k, P + which] - target)
        for t in range(tc, min(tc + CHUNK, n)):
            while k + 1 < len(rows) and t >= t_rows[k + 1]:
                k += 1
                target = rows[k, PIN + which]
            v = s * v + (1.0 - s) * target
            out[t] = v
    return out
