"""Scalar, op-for-op restatement of the reference's Subtractive<double, N> (TEST INFRASTRUCTURE;
src/subtractive.h:15-101, the MIMO variant it compiles by default, and src/filter.h).

This is a restatement, not the compiled reference: the MIMO Subtractive includes filterbank.h and
with it Eigen, which the frozen compiled oracle (oracle/) does not build, so the class is pinned the
way the other Eigen / FFTW classes are -- by restating its text.  Python floats are IEEE doubles and
every expression keeps the reference's association.  The note layer and Minimizer::physics() are
tests/oracle_phys.py's (bit-exact against the reference's recorded positions); this file adds
Filter<T> as written -- the ring of size order + 2, `origin`, the `computed` flag, the stale
back[0] * output[origin] term -- Filter::resonant(), the octave fold and the amplitude gating of
Subtractive::tick() / operator().
"""
from __future__ import annotations

import math

import numpy as np

from oracle_phys import PI, SR, PhysAdditive, ftom, mtof, relaxation  # noqa: F401


def _divdc3(a, b, c, d):
    """libgcc's __divdc3 for finite operands (Smith's algorithm): (a + ib) / (c + id)"""
    if abs(c) < abs(d):
        ratio = c / d
        denom = (c * ratio) + d
        return ((a * ratio) + b) / denom, ((b * ratio) - a) / denom
    ratio = d / c
    denom = (d * ratio) + c
    return ((b * ratio) + a) / denom, (b - (a * ratio)) / denom


class Filter:
    """Filter<double> (src/filter.h)"""

    def __init__(self, feedforward, feedback):          # filter.h:16-27
        self.forward = list(map(float, feedforward))
        self.back = list(map(float, feedback))
        self.back[0] = 0.0
        self.order = max(len(self.forward), len(self.back)) - 1
        self.forward += [0.0] * (self.order + 1 - len(self.forward))
        self.back += [0.0] * (self.order + 1 - len(self.back))
        self.reset()

    def reset(self):                                    # 57-64
        self.buffsize = self.order + 2
        self.output = [0.0] * self.buffsize
        self.history = [0.0] * self.buffsize
        self.origin = 0
        self.computed = False

    def tick(self):                                     # 95-100
        self.origin += 1
        self.origin %= self.buffsize
        self.computed = False

    def __call__(self, sample):                         # 102-121
        if not self.computed:
            self.history[self.origin] = sample
            out = 0.0
            for i in range(self.order + 1):
                index = (self.origin - i + self.buffsize) % self.buffsize
                out += self.forward[i] * self.history[index] - self.back[i] * self.output[index]
            self.output[self.origin] = out
            self.computed = True
        return self.output[self.origin]

    def resonant(self, frequency, Q):                   # 123-138
        cosine = math.cos(2 * PI * frequency / SR)
        c2 = math.cos(4 * PI * frequency / SR)
        s2 = math.sin(4 * PI * frequency / SR)
        # 1.0i * sine2: (0 + 1i)(s2 + 0i)
        ir, ii = 0.0 * s2 - 1.0 * 0.0, 0.0 * 0.0 + 1.0 * s2
        # Q - cosine2 - 1.0i * sine2
        dr, di = (Q - c2) - ir, -0.0 - ii
        qr, qi = _divdc3(1.0, 0.0, dr, di)
        # 1.0 / (Q - 1) - q
        mr, mi = 1.0 / (Q - 1) - qr, 0.0 - qi
        amplitude = 1 / math.sqrt(math.hypot(mr, mi))
        self.forward = [amplitude, 0.0, -amplitude]
        self.back = [0.0, -2 * Q * cosine, Q * Q]
        self.order = 2


def fold(frequency):
    """subtractive.h:58-59 (SR / 2 is the integer 24000)"""
    while frequency > SR // 2:
        frequency /= 2
    return frequency


class SubOracle(PhysAdditive):
    """Subtractive<double, N>(V, O, decay, resonance, harm, k); `law` is required."""

    def __init__(self, V, O, decay, resonance=0.99999, harm=1.0, k=0.1, N=2, *, law):
        super().__init__(V, O, decay, harm, k, law=law)   # attack, normalization, Minimizer state
        self.N = N
        self.resonance = resonance
        self.filters = [Filter([1, 0, 0], [0]) for _ in range(V * O * N)]

    def tick(self):                                     # subtractive.h:47-67
        V, O = self.V, self.O
        for i in range(V):
            self.amps[i] = (1 - self.attack) * self.active[i] + self.attack * self.amps[i]
        for i in range(V):
            if self.amps[i]:
                for j in range(O):
                    frequency = fold(mtof(self.x[i * O + j]))
                    for k in range(self.N):
                        f = self.filters[k * O * V + i * O + j]
                        f.resonant(frequency, self.resonance)
                        f.tick()

    def __call__(self, sample):                         # 69-79
        V, O = self.V, self.O
        out = [0.0] * self.N
        for i in range(V):
            if self.amps[i]:
                for j in range(O):
                    for k in range(self.N):
                        out[k] += (self.amps[i] * math.pow(self.decay, j) * self.filters[k * O * V + i * O + j](sample[k])
                                   / (V * self.norm))
        return out

    def process(self, x, track=None):
        """n x { out[:, t] = operator()(x[:, t]); if (T >= p && T % p == 0) physics(); tick(); T++ };
        x [N][n]; positions after every step are appended to `track`"""
        x = np.asarray(x, dtype=np.float64).reshape(self.N, -1)
        n = x.shape[1]
        out = np.zeros((self.N, n))
        p = self.period
        for t in range(n):
            out[:, t] = self([float(x[k, t]) for k in range(self.N)])
            if p > 0 and self.T >= p and self.T % p == 0:
                self.physics()
                if track is not None:
                    track.append(list(self.x))
            self.tick()
            self.T += 1
        return out

    def amplitudes(self):
        return np.array(self.amps, dtype=np.float64)


def run_sub_scenario(sc, x, obj):
    """Drive a SubOracle or a huygens_amd.Subtractive (same makenote / endnote / process members)
    through an oracle_phys scenario dict with the input x [N][n]; events at their sample times.
    Returns the audio [N][n]."""
    x = np.asarray(x, dtype=np.float64)
    n, pos, chunks = sc["n"], 0, []
    for t in sorted({t for t, *_ in sc["events"]} | {n}):
        if t > pos:
            chunks.append(obj.process(np.ascontiguousarray(x[:, pos:t])))
            pos = t
        for et, kind, a, b in sc["events"]:
            if et == t and t < n:
                if kind == 0:
                    obj.makenote(a, b)
                else:
                    obj.endnote(a)
    return np.concatenate(chunks, axis=1)
