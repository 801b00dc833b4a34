"""numpy restatement of src/fourier.h:236-562 (FFrame, IFrame, DFrame, Freezer), independent of
oracle/hz_oracle_frz.c (numpy's FFT against the oracle's long double DFT).  TEST INFRASTRUCTURE.

PyFreezer.sample() is the reference's operator() line by line.  process() runs the same
statements over stretches in which no frame reaches spot 0 (no FFT, no draw), as array slices: the
per-sample order of every sum is kept, so both give the same bits (tests/test_freezer_cases_cpu.py
asserts it).  rand() comes from libc like the reference.

A Trace, when asked for, records which branches a schedule reaches; split_schedule() tells dry
samples from frozen periods from the events alone.
"""
import ctypes as C

import numpy as np

PI = 3.14159265359
_libc = C.CDLL(None)


def halfhann(p):
    return np.sqrt(0.5 * (1 - np.cos(2 * PI * p)))


class Trace:
    """What a run of PyFreezer reached.

    frozen[t], period[t]: the state that produced sample t (period -1 while dry; a period starts at
    every dry -> frozen transition, a re-freeze while frozen stays in its period).
    freezes: (t, transition, excluded, readhead before the call) per freeze() call.
    populates: one dict per IFrame draw --
        t, slot (the slot i at spot 0), next, excluded, period,
        refreshed: DFrame `next` was written by this period's freeze(), (next - excluded) mod M in
                   [1, M-2]; otherwise it is excluded - 1, stale from an earlier freeze (or zero),
        midread:   the slot iindex that received `next` stood at a spot in (0, N),
        reread:    IFrame `next` held another period's frame while a slot was reading it.
    """

    def __init__(self):
        self.freezes, self.populates, self._runs = [], [], []
        self.frozen = np.zeros(0, bool)
        self.period = np.zeros(0, np.int64)

    def mark(self, n, frozen, period):
        self._runs.append((n, frozen, period if frozen else -1))

    def finish(self):
        self.frozen = np.concatenate([np.full(n, f, bool) for n, f, _ in self._runs] or [np.zeros(0, bool)])
        self.period = np.concatenate([np.full(n, p, np.int64) for n, _, p in self._runs] or [np.zeros(0, np.int64)])
        return self


class PyFreezer:
    def __init__(self, N, laps, width, trace=False):
        width, laps = max(width, 1.0), max(laps, 2)
        self.N, self.stride = N, N // laps
        self.M = int(width * laps) + 1
        self.size = self.M * self.stride
        M = self.M
        self.data = np.zeros((M, N), complex)
        self.norms = np.zeros((M, N))
        self.phases = np.zeros((M, N))
        self.dn = np.zeros((M, N))
        self.dp = np.zeros((M, N))
        self.idata = np.zeros((M, N), complex)
        self.iqueue = [0] * M
        self.iindex = self.origin = self.readhead = self.excluded = 0
        self.frozen = False
        self.din = np.zeros(N + 1)
        self.dorigin = 0
        self.win = halfhann(np.arange(N) / N)
        self.t = 0
        self.nperiod = -1                     # index of the latest period
        self.iperiod = [-1] * M               # the period whose frame each IFrame holds
        self.trace = Trace() if trace else None

    def write(self, x):
        for i in range(self.M):
            spot = (self.origin - i * self.stride) % self.size
            if spot < self.N:
                self.data[i, spot] = complex(self.win[spot] * x, self.win[spot] * 0.0)
            if spot == 0:
                j = (i - 1) % self.M
                X = np.fft.fft(self.data[j])
                self.norms[j] = X.real ** 2 + X.imag ** 2
                self.phases[j] = np.arctan2(X.imag, X.real)
        self.origin = (self.origin + 1) % self.size

    def freeze(self):
        transition = not self.frozen
        if not self.frozen:
            self.nperiod += 1
            self.excluded = self.origin // self.stride
            for i in range(1, self.M - 1):
                d = (self.excluded + i) % self.M
                s = (d + 1) % self.M
                self.dn[d] = self.norms[s]
                self.dp[d] = self.phases[s] - self.phases[d]
        if self.trace is not None:
            self.trace.freezes.append((self.t, transition, self.excluded, self.readhead))
        self.readhead = 0
        self.frozen = True

    def unfreeze(self):
        self.frozen = False

    def _populate(self, i):
        nxt = _libc.rand() % (self.M - 2)
        if nxt >= self.excluded:
            nxt += 2
        self.iindex = (self.iindex + 1) % self.M
        if self.trace is not None:
            spots = [(self.readhead - q * self.stride) % self.size for q in range(self.M)]
            self.trace.populates.append(dict(
                t=self.t, slot=i, next=nxt, excluded=self.excluded, period=self.nperiod,
                refreshed=1 <= (nxt - self.excluded) % self.M <= self.M - 2,
                midread=0 < spots[self.iindex] < self.N,
                reread=self.iperiod[nxt] != self.nperiod and any(
                    self.iqueue[q] == nxt and 0 < spots[q] < self.N for q in range(self.M) if q != self.iindex)))
        self.iqueue[self.iindex] = nxt
        self.iperiod[nxt] = self.nperiod
        voc = np.fmod(self.dp[nxt], 2 * PI)
        r = np.sqrt(self.dn[nxt])
        self.idata[nxt] = np.fft.ifft(r * np.cos(voc) + 1j * r * np.sin(voc)) * self.N

    def sample(self, x):
        self.write(x)
        out = 0.0
        if self.frozen:
            for i in range(self.M):
                spot = (self.readhead - i * self.stride) % self.size
                if spot < self.N:
                    out += self.idata[self.iqueue[i], spot].real * self.win[spot]
                if spot == 0:
                    self._populate(i)
            self.readhead = (self.readhead + 1) % self.size
            out /= self.N
        else:
            o = self.dorigin
            self.din[o] = x
            out = self.din[(o + 1) % (self.N + 1)]
        self.dorigin = (self.dorigin + 1) % (self.N + 1)
        self.t += 1
        return out

    def _stretch(self, xs):
        """len(xs) samples in which no write spot and no read spot is 0: sample()'s statements as
        slices (each frame's spots are consecutive and stay inside one stride)."""
        L, N = len(xs), self.N
        for i in range(self.M):
            s0 = (self.origin - i * self.stride) % self.size
            if s0 < N:
                m = min(L, N - s0)
                self.data[i, s0:s0 + m] = self.win[s0:s0 + m] * xs[:m]
        self.origin = (self.origin + L) % self.size
        if self.frozen:
            out = np.zeros(L)
            for i in range(self.M):
                s0 = (self.readhead - i * self.stride) % self.size
                if s0 < N:
                    m = min(L, N - s0)
                    out[:m] += self.idata[self.iqueue[i], s0:s0 + m].real * self.win[s0:s0 + m]
            self.readhead = (self.readhead + L) % self.size
            out /= N
        else:   # L <= stride <= N / 2: no slot is read after its write within the stretch
            idx = (self.dorigin + np.arange(L)) % (N + 1)
            out = self.din[(idx + 1) % (N + 1)].copy()
            self.din[idx] = xs
        self.dorigin = (self.dorigin + L) % (N + 1)
        self.t += L
        return out

    def process(self, x, events=(), per_sample=False):
        """events (at, kind), kind 1 freeze / 0 unfreeze, applied before sample `at`; an event at
        len(x) is not applied (as orc_frz_process)."""
        ev = list(events)
        x = np.asarray(x, dtype=float)
        n = len(x)
        y, k, i = np.zeros(n), 0, 0
        while i < n:
            while k < len(ev) and ev[k][0] == i:
                self.freeze() if ev[k][1] else self.unfreeze()
                k += 1
            frozen, period = self.frozen, self.nperiod
            wr, rd = self.origin % self.stride, self.readhead % self.stride
            if per_sample or wr == 0 or (frozen and rd == 0):
                y[i] = self.sample(x[i])
                L = 1
            else:
                L = min((ev[k][0] if k < len(ev) else n) - i, self.stride - wr)
                if frozen:
                    L = min(L, self.stride - rd)
                y[i:i + L] = self._stretch(x[i:i + L])
            if self.trace is not None:
                self.trace.mark(L, frozen, period)
            i += L
        if self.trace is not None:
            self.trace.finish()
        return y


def split_schedule(n, events, frozen=False):
    """From the schedule alone: (dry, periods) of a run of n samples.  dry[t] is True where sample t
    is a dry (Delay) sample; periods lists (start, end) of every frozen period that holds a sample,
    in order -- a period begins at each dry -> frozen transition and ends at the next unfreeze."""
    state = np.zeros(n, np.int64)   # 0 dry, p + 1 in period p
    ev = sorted(events, key=lambda e: e[0])   # stable: events on one sample keep their order
    p, k, cur = 0, 0, 0
    bounds = []
    t = 0
    while t < n:
        while k < len(ev) and ev[k][0] == t:
            if ev[k][1]:
                if not frozen:
                    p += 1
                    cur = p
                frozen = True
            else:
                frozen, cur = False, 0
            k += 1
        t1 = min(ev[k][0], n) if k < len(ev) else n
        state[t:t1] = cur if frozen else 0
        if frozen:
            if bounds and bounds[-1][2] == cur:
                bounds[-1][1] = t1
            else:
                bounds.append([t, t1, cur])
        t = t1
    return state == 0, [(a, b) for a, b, _ in bounds]
