"""numpy restatements of the PHASE and STICKS chains and the output stage.  TEST INFRASTRUCTURE.

OraclePhase  tests/phasebank.cpp:77-101 (src/oscbank.h, modbank.h, slidebank.h, rmsbank.h,
             latchbank.h, distbank.h, stickbank.h, mixer.h)
OracleSticks tests/oscbank.cpp:106-110
output_stage tests/slidebank.cpp:81-95 / harmbank.cpp:78 / oscbank.cpp:106

Vectorised over channels on real arrays, one time step per loop iteration; every product and
sum is its own numpy operation in the reference's order (no fused multiply-add, no complex128
kernels).  Both classes mirror huygens_amd.Heterodyne's interface (freqmod, activate, open,
setup, process, state)."""
from __future__ import annotations

import math

import numpy as np

PI = 3.14159265359   # src/includes.h
SR = 48000
OUT_LIMITER, OUT_RAW = 0, 1


def softclip(v, width):
    """tests/slidebank.cpp:81-89 (abs taken as fabs)."""
    v = np.asarray(v, dtype=np.float64)
    sign = np.sign(v)
    gap = v - sign * width
    tail = sign * width + (1 - width) * 2.0 / PI * np.arctan(PI * gap / (2 * (1 - width)))
    return np.where(np.abs(v) < width, v, tail)


def output_stage(x, mix, dry, gain, shaper=OUT_LIMITER, drive=0.0, clip=0.0):
    """shaper(dry x + gain v); v = mix, or softclip(drive mix, clip) when drive != 0."""
    v = mix if drive == 0.0 else softclip(drive * mix, clip)
    u = dry * x + gain * v
    return u if shaper == OUT_RAW else 2.0 / PI * np.arctan(u)


def _tick(z, w, act):
    """oscbank.h:61-62: z *= w; z /= (1 + |z|^2) / 2, active channels only."""
    zr, zi = z
    wr, wi = w
    r, m = zr * wr - zi * wi, zr * wi + zi * wr
    nrm = (1.0 + (r * r + m * m)) / 2
    return [np.where(act, r / nrm, zr), np.where(act, m / nrm, zi)]


def _stick(y, back, sgain, lr, li):
    """stickbank.h:189: (1 + rad)^order l - block * back (back real, as complex b + 0i)."""
    accr, acci = np.zeros_like(lr), np.zeros_like(lr)
    for k in range(len(y)):
        accr = accr + (y[k][0] * back[k] - y[k][1] * 0.0)
        acci = acci + (y[k][0] * 0.0 + y[k][1] * back[k])
    return sgain * lr - accr, sgain * li - acci


def _stick_back(order, rad):
    """stickbank.h:197-217: coefficients of the monic polynomial with `order` roots at rad,
    ascending, without the leading 1 (the recursion's own products and sums)."""
    c = [rad, 1.0]
    for deg in range(2, order + 1):
        t = [0.0] * (deg + 1)
        for i in range(deg):
            t[i] += rad * c[i]
            t[i + 1] += c[i]
        c = t
    return c[:order]


class _Banks:
    """The two Oscbanks and their controls."""

    def __init__(self, N):
        self.N = N
        self.z = {b: [np.ones(N), np.zeros(N)] for b in (0, 1)}
        self.w = {b: [np.ones(N), np.zeros(N)] for b in (0, 1)}
        self.act = {b: np.zeros(N, bool) for b in (0, 1)}

    def freqmod(self, bank, index, hz):
        for i, f in zip(np.atleast_1d(index), np.atleast_1d(hz)):
            if 0 <= i < self.N:
                self.w[bank][0][i] = math.cos(2 * PI * float(f) / SR)   # libm, like the engine's host code
                self.w[bank][1][i] = math.sin(2 * PI * float(f) / SR)

    def activate(self, bank, index, on=True):
        self.act[bank][np.atleast_1d(index)] = on

    def open(self, bank, on=True):
        self.act[bank][:] = on

    def process(self, x):
        return np.array([self.sample(float(v)) for v in np.asarray(x, dtype=np.float64)])


class OraclePhase(_Banks):
    def __init__(self, channels, order, radii, thresh=0.0005, ratio=0.2, width=2400, stick_order=1, stick_rad=-0.9,
                 dry=0.0, gain=3.0, record=False):
        super().__init__(channels)
        N = channels
        self.W, self.S = width, max(1, stick_order)
        self.thresh, self.ratio, self.dry, self.gain = thresh, ratio, dry, gain
        self.hist = np.zeros((width + 1, N))   # |s|^2, row = time mod (width + 1)
        self.t = 0
        self.rsum = np.zeros(N)
        self.armed, self.engaged = np.zeros(N, bool), np.zeros(N, bool)
        self.back = _stick_back(self.S, stick_rad)
        self.sgain = math.pow(1 + stick_rad, self.S)
        self.y = [[np.zeros(N), np.zeros(N)] for _ in range(self.S)]
        self.shaper, self.drive, self.clip = OUT_LIMITER, 0.0, 0.0
        self.record = record
        # per sample: P, engaged after the first and after the second update, |y|, the mix
        self.trace = {"P": [], "engaged1": [], "engaged": [], "y": [], "mix": []}
        self.setup(order, radii)

    def setup(self, order, radii):
        radii = np.asarray(radii, dtype=np.float64)
        self.O = max(1, order)
        self.rr, self.ri = radii[0::2].copy(), radii[1::2].copy()
        self.sl = [[np.zeros(self.N), np.zeros(self.N)] for _ in range(self.O)]

    def set_output(self, shaper=OUT_LIMITER, drive=0.0, clip_width=0.0):
        self.shaper, self.drive, self.clip = shaper, drive, clip_width

    def _latch(self, rms):
        """latchbank.h:83-93, one call."""
        lo, hi = self.thresh * self.ratio, self.thresh * (1 - self.ratio)
        armed = self.armed | (rms < lo)
        t1 = self.engaged & (rms < lo)
        t2 = ~self.engaged & (rms > hi) & armed
        self.engaged = (self.engaged & ~t1) | t2
        self.armed = armed & ~t1

    def _middle(self, sr, si, r1):
        """From the Slidebank output and the first RMS to the demodulators' input."""
        # absbank(latchbank(&rmsbank, slidebank())): first argument first (clang)
        self._latch(r1)
        e1 = self.engaged.astype(float)
        A = np.hypot(sr * e1, si * e1)
        # second call: `computed` is set, so only *out = sqrt(*out / width) runs again
        with np.errstate(invalid="ignore"):
            r2 = np.sqrt(r1 / self.W)
        self._latch(r2)
        e2 = self.engaged.astype(float)
        P = np.arctan2(si * e2, sr * e2)   # (+-0, -0) -> +-pi on a silent channel
        # smoothbank on (P, 0)
        yr, yi = _stick(self.y, self.back, self.sgain, P, np.zeros(self.N))
        self.y = [[yr, yi]] + self.y[:-1]
        # phase_combiners((A, 0), y); demodulators(synthesis(), .); Mixer takes the real part
        cre, cim = A * yr - 0.0 * yi, A * yi + 0.0 * yr
        if self.record:
            self.trace["P"].append(P)
            self.trace["engaged1"].append(e1 != 0)
            self.trace["engaged"].append(self.engaged.copy())
            self.trace["y"].append(np.hypot(yr, yi))
        return cre, cim

    def sample(self, x):
        # modulators(x, analysis()); slidebank (sparse product: (1 - r) in_q, then r old_q)
        zr, zi = self.z[0]
        ir, ii = x * zr, x * zi
        cr, ci = 1.0 - self.rr, 0.0 - self.ri
        for q in range(self.O):
            o_r, o_i = self.sl[q]
            nr = (cr * ir - ci * ii) + (self.rr * o_r - self.ri * o_i)
            ni = (cr * ii + ci * ir) + (self.rr * o_i + self.ri * o_r)
            ir, ii = o_r, o_i
            self.sl[q] = [nr, ni]
        sr, si = self.sl[-1]
        # rmsbank, first call: the running sum, then *out = sqrt(*out / width)
        a2 = sr * sr + si * si
        W1 = self.W + 1
        old = self.hist[(self.t - self.W) % W1]
        self.hist[self.t % W1] = a2
        self.rsum = (a2 - old) + self.rsum
        with np.errstate(invalid="ignore"):   # a running sum rounded below zero gives NaN, as in the reference
            r1 = np.sqrt(self.rsum / self.W)
        cre, cim = self._middle(sr, si, r1)
        szr, szi = self.z[1]
        d = szr * cre - szi * cim
        mix = 0.0
        for v in d:   # Mixer: channel order
            mix += v
        out = output_stage(x, mix, self.dry, self.gain, self.shaper, self.drive, self.clip)
        if self.record:
            self.trace["mix"].append(mix)
        for b in (0, 1):
            self.z[b] = _tick(self.z[b], self.w[b], self.act[b])
        self.t += 1
        return float(out)

    def state(self, what):
        N = self.N
        if what in (0, 1):
            return np.stack(self.z[what], 1).ravel()
        if what == 2:
            return np.stack([np.stack(s, 1) for s in self.sl], 1).ravel()
        if what == 3:
            return self.rsum.copy()
        if what == 4:
            return np.stack([self.armed, self.engaged], 1).astype(float).ravel()
        if what == 5:
            return np.stack([np.stack(s, 1) for s in self.y], 1).ravel()
        W1 = self.W + 1   # history, newest first
        return np.stack([self.hist[(self.t - 1 - k) % W1] for k in range(self.W)], 1).reshape(N * self.W)


class OracleHarm(OraclePhase):
    """tests/harmbank.cpp:77-101 and tests/slidebank.cpp:91-112 (one latch update, the Stickbank on
    the latched signal): the existing chain with the output stage, for set_output's parity."""

    def _middle(self, sr, si, r1):
        self._latch(r1)
        eg = self.engaged.astype(float)
        yr, yi = _stick(self.y, self.back, self.sgain, sr * eg, si * eg)
        self.y = [[yr, yi]] + self.y[:-1]
        return yr, yi


class OracleSticks(_Banks):
    def __init__(self, channels, pre=3, post=1, rad=-0.999, gate=0.001, dry=0.0, gain=1.0, record=False):
        super().__init__(channels)
        self.pre, self.post, self.gate, self.dry, self.gain = pre, post, gate, dry, gain
        self.back, self.sgain = [rad], math.pow(1 + rad, 1)
        self.y = [[np.zeros(channels), np.zeros(channels)] for _ in range(pre + post)]
        self.shaper, self.drive, self.clip = OUT_RAW, 0.0, 0.0
        self.record = record
        self.trace = {"mag": [], "gated": []}   # per sample: |x| at the gate, the gate's decision

    def set_output(self, shaper=OUT_LIMITER, drive=0.0, clip_width=0.0):
        self.shaper, self.drive, self.clip = shaper, drive, clip_width

    def sample(self, x):
        zr, zi = self.z[0]
        vr, vi = x * zr, x * zi
        for k in range(self.pre + self.post):
            if k == self.pre and self.gate > 0:   # gate(x) = abs(x) < gate ? 0 : x
                mag = np.hypot(vr, vi)
                shut = mag < self.gate
                vr, vi = np.where(shut, 0.0, vr), np.where(shut, 0.0, vi)
                if self.record:
                    self.trace["mag"].append(mag)
                    self.trace["gated"].append(shut)
            vr, vi = _stick([self.y[k]], self.back, self.sgain, vr, vi)
            self.y[k] = [vr, vi]
        if self.post == 0 and self.gate > 0:
            mag = np.hypot(vr, vi)
            shut = mag < self.gate
            vr, vi = np.where(shut, 0.0, vr), np.where(shut, 0.0, vi)
            if self.record:
                self.trace["mag"].append(mag)
                self.trace["gated"].append(shut)
        szr, szi = self.z[1]
        d = szr * vr - szi * vi
        mix = 0.0
        for v in d:
            mix += v
        out = output_stage(x, mix, self.dry, self.gain, self.shaper, self.drive, self.clip)
        for b in (0, 1):
            self.z[b] = _tick(self.z[b], self.w[b], self.act[b])
        return float(out)

    def state(self, what):
        if what in (0, 1):
            return np.stack(self.z[what], 1).ravel()
        if what == 5:
            return np.stack([np.stack(s, 1) for s in self.y], 1).ravel()
        raise ValueError("the STICKS chain has no such state")
