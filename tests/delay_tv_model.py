"""Numpy model of the Delaybank stream kernels (TEST INFRASTRUCTURE).

Mirrors huygens_amd/csrc/hz_delay.hip (dly_tv_scan_kernel, dly_tv_line_kernel, the commit): the
32-bit slot index and its age per read, tv_rem's divide-free remainder, the scan's sub-block
length Lc, evaluation sub-block by sub-block with every sample of a sub-block computed from the
state before it, the choice between the call's arrays and the rings, and the commit of the last
min(n, size) samples.  The CPU tests hold it against the per-sample oracle before the kernel runs
on a GPU; it is not the product and not the oracle.  Also the scenario both test files share.
"""
from __future__ import annotations

import functools

import numpy as np

M32 = 0xFFFFFFFF


def max_time(dtype):
    """The largest time (int)(T)t holds: set_tap's limit."""
    return 2147483520 if np.dtype(dtype) == np.float32 else 2147483647


def rem(w, size):
    """tv_rem: w % size through the reciprocal, one conditional subtraction (w: uint32 values)."""
    w = np.asarray(w, dtype=np.uint64)
    rcp = np.uint64(min((1 << 32) // size, M32))
    r = (w - ((w * rcp) >> np.uint64(32)) * np.uint64(size)) & np.uint64(M32)
    return np.where(r >= size, r - np.uint64(size), r).astype(np.int64)


def slot_age(times, o, size, dtype):
    """buffer.h:42-46 for a vector of reads: c = (int)(T)time, idx = (uint32)(o - c + size) % size,
    age = o - idx mod size."""
    c = np.asarray(times, dtype=np.uint32).astype(dtype).astype(np.int32).astype(np.int64)
    idx = rem((o - c + size) & M32, size)
    return idx, np.where(o >= idx, o - idx, o + size - idx)


class DelayTvModel:
    def __init__(self, lines, sparsity, time, dtype=np.float64):
        self.N, self.S, self.size, self.dtype = lines, sparsity, time + 1, np.dtype(dtype)
        self.rx = np.zeros((lines, self.size), dtype=self.dtype)
        self.ry = np.zeros((lines, self.size), dtype=self.dtype)
        self.o0 = 0
        self.bt = np.zeros((lines, sparsity), dtype=np.uint32)   # staged feedback taps
        self.bg = np.zeros((lines, sparsity), dtype=self.dtype)
        self.last_Lc = None

    def origin(self):
        return self.o0

    def scan(self, n, bt, bg):
        """Lc: the smallest age >= 1 of a live feedback read of the call, each sample at its own
        origin; n when there is none."""
        o = rem(self.o0 + np.arange(n, dtype=np.int64), self.size)
        live = (bt != 0) & (bg != 0)
        _, age = slot_age(bt, o[None, None, :], self.size, self.dtype)
        ages = age[live & (age > 0)]
        return int(min(ages.min(), n)) if ages.size else n

    def process_tv(self, x, ft, fg, bt=None, bg=None):
        dt, size = self.dtype, self.size
        x = np.ascontiguousarray(x, dtype=dt)
        n = x.shape[-1]
        if n == 0:
            return np.zeros((self.N, 0), dtype=dt)
        xl = x if x.ndim == 2 else np.broadcast_to(x, (self.N, n))
        ft, fg = np.asarray(ft, dtype=np.uint32), np.asarray(fg, dtype=dt)
        assert int(ft.max()) <= max_time(dt)
        if bt is None:
            sbt = np.broadcast_to(self.bt[:, :, None], (self.N, self.S, n))
            sbg = np.broadcast_to(self.bg[:, :, None], (self.N, self.S, n))
        else:
            sbt, sbg = np.asarray(bt, dtype=np.uint32), np.asarray(bg, dtype=dt)
            assert int(sbt.max()) <= max_time(dt)
        Lc = self.last_Lc = self.scan(n, sbt, sbg)
        y = np.zeros((self.N, n), dtype=dt)
        for s0 in range(0, n, Lc):
            j = np.arange(s0, min(n, s0 + Lc), dtype=np.int64)
            o = rem(self.o0 + j, size)
            for l in range(self.N):
                acc = np.zeros(j.size, dtype=dt)
                for i in range(self.S):
                    xi, af = slot_age(ft[l, i, j], o, size, dt)
                    own = af <= j
                    xv = np.where(own, xl[l][np.where(own, j - af, 0)], self.rx[l][xi])
                    tb = sbt[l, i, j]
                    b = np.where(tb == 0, dt.type(0), sbg[l, i, j]).astype(dt)   # zero time -> {0, 0}
                    live = b != 0
                    yi, ab = slot_age(tb, o, size, dt)
                    own = live & (ab <= j) & (ab > 0)
                    # no sample of a sub-block reads an output of the same sub-block
                    assert np.all((j - ab)[own] < s0), "feedback read inside its own sub-block"
                    yv = np.where(own, y[l][np.where(own, j - ab, 0)], self.ry[l][yi])
                    yv = np.where(ab == 0, acc, yv)          # age 0: the partial sum
                    yv = np.where(live, yv, dt.type(0)).astype(dt)
                    fx = fg[l, i, j] * xv.astype(dt)
                    acc = acc + (fx - b * yv)
                y[l, j] = acc
        j = np.arange(max(0, n - size), n, dtype=np.int64)   # commit
        slots = rem(self.o0 + j, size)
        self.rx[:, slots] = xl[:, j]
        self.ry[:, slots] = y[:, j]
        self.o0 = int((self.o0 + n) % size)
        if bt is not None:                                   # the staged taps: the last row
            self.bt = sbt[:, :, -1].copy()
            self.bg = np.where(self.bt == 0, dt.type(0), sbg[:, :, -1]).astype(dt)
        return y


# ---- the scenario of tests/test_delay_tv_cpu.py and tests/test_delay_tv_gpu.py -----------------
LINES, SPARSITY, TIME = 3, 2, 96           # ring 97 (prime)
CALLS = (1, 127, 1, 171, 300)


def make_streams(rng, n, dtype, lines=LINES, sparsity=SPARSITY, size=TIME + 1):
    """Forward times in [0, 3 size) with ~15 % edge values, back times in [5, 40] with ~10 % edge
    values, back gains in +-0.4 with 20 % exactly zero."""
    shape = (lines, sparsity, n)
    ft = rng.integers(0, 3 * size, shape)
    edge = np.array([0, size - 1, size, size + 5, 2 * size, 200, max_time(dtype)])
    ft = np.where(rng.random(shape) < 0.15, edge[rng.integers(0, edge.size, shape)], ft).astype(np.uint32)
    fg = rng.uniform(-1, 1, shape).astype(dtype)
    bt = rng.integers(5, 41, shape)
    edge = np.array([0, size, size + 7, 2 * size + 9])
    bt = np.where(rng.random(shape) < 0.10, edge[rng.integers(0, edge.size, shape)], bt).astype(np.uint32)
    bg = np.where(rng.random(shape) < 0.20, 0.0, rng.uniform(-0.4, 0.4, shape)).astype(dtype)
    return ft, fg, bt, bg


@functools.lru_cache(maxsize=None)
def scenario(dtype_name):
    """The calls [(x, ft, fg, bt, bg)]: 1, 127, 1, 171, 300 samples, mono and per-line input in
    turn.  |x| <= 0.5 and sum |bg| <= 0.8 per line bound every output by 2 * 0.5 / (1 - 0.8) = 5."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng(2024)
    calls = []
    for k, n in enumerate(CALLS):
        x = rng.uniform(-0.5, 0.5, (LINES, n) if k % 2 else n).astype(dtype)
        calls.append((x,) + make_streams(rng, n, dtype))
    for c in calls:
        for a in c:
            a.setflags(write=False)
    return tuple(calls)


def oracle_tv(o, x, ft, fg, bt=None, bg=None):
    """The contract's loop on an OracleDelaybank: modulate_* every tap, then one sample."""
    x = np.asarray(x)
    n = x.shape[-1]
    y = np.zeros((o.lines, n), dtype=o.dtype)
    for t in range(n):
        for l in range(ft.shape[0]):
            for i in range(ft.shape[1]):
                o.modulate_forward(l, i, (ft[l, i, t], fg[l, i, t]))
                if bt is not None:
                    o.modulate_back(l, i, (bt[l, i, t], bg[l, i, t]))
        y[:, t] = o.process(x[..., t:t + 1])[:, 0]
    return y


@functools.lru_cache(maxsize=None)
def scenario_reference(dtype_name):
    """The oracle's outputs of scenario() and its origin after each call (computed once)."""
    from oracle_delay import OracleDelaybank
    o = OracleDelaybank(LINES, SPARSITY, TIME, np.dtype(dtype_name))
    ys, origins = [], []
    for c in scenario(dtype_name):
        y = oracle_tv(o, *c)
        y.setflags(write=False)
        ys.append(y)
        origins.append(o.origin())
    return tuple(ys), tuple(origins)
