"""Scalar, op-for-op restatement of the reference's Additive with Minimizer::physics()
(TEST INFRASTRUCTURE; src/minimizer.h:61-187, src/particle.h, src/additive.h:38-62,
src/oscillator.h:27-38).  Python floats are IEEE doubles and every expression below keeps the
reference's association, so positions are comparable bit for bit.

The physics step is written as the gather loop the device engine runs: per particle its own
spring, the next overtone's spring, then gravity from every other active voice in ascending
voice and overtone order -- the order in which the reference's scatter loop reaches that
particle's `acceleration`.

Two gravity laws (particle.h:119,121 call an unqualified abs on doubles):
  GRAV_TRUNC  abs binds ::abs(int) (the reference as oracle/Makefile compiles it)
  GRAV_FABS   abs binds the double overload (the text as written)
"""
from __future__ import annotations

import math

import numpy as np

GRAV_TRUNC, GRAV_FABS = 1, 2

PI = 3.14159265359
SR = 48000
FORCE = 50000
A4 = 440.0
ORDER = math.log2(np.finfo(np.float64).eps)


def relaxation(k):
    if k == 0:
        return 0.0
    return math.pow(2.0, ORDER / (max(0.0, k) * SR))


def mtof(m):
    return A4 * math.pow(2, (m - 69) / 12)


def ftom(f):
    return 69 + math.log2(f / A4) * 12


def _trunc(x):
    return float(int(x))   # (int) conversion: toward zero


class PhysAdditive:
    """Additive<double>(&cycle, V, O, decay, harm, k) with physics(); `law` is required."""

    def __init__(self, V, O, decay, harm=1.0, k=0.1, *, law):
        if law not in (GRAV_TRUNC, GRAV_FABS):
            raise ValueError("law must be GRAV_TRUNC or GRAV_FABS")
        self.V, self.O, self.decay, self.harm, self.law = V, O, decay, harm, law
        P = V * O
        self.attack = relaxation(k)
        self.norm = (1 - math.pow(decay, O)) / (1 - decay) if decay != 1 else float(O)
        self.active = [0.0] * V
        self.pitches = [0.0] * V
        self.amps = [0.0] * V
        self.guide = [0.0] * V
        self.x = [0.0] * P
        self.v = [0.0] * P
        self.mass = [0.0] * P
        self.eq = [0.0] * P
        self.kspring = [(0.1 * FORCE) if j == 0 else float(1 * FORCE) for _ in range(V) for j in range(O)]
        self.G = float(1 * FORCE)
        self.eps = 0.0001
        self.drag = relaxation(0.01)
        # Oscillator(0, 0, 0.0001)
        self.s = relaxation(0.0001)
        self.phase = [0.0] * P
        self.tphase = [0.0] * P
        self.freq = [0.0] * P
        self.tfreq = [0.0] * P
        self.period = 0
        self.T = 0
        self.dec = [math.pow(decay, j) for j in range(O)]

    # ---- Minimizer note API -------------------------------------------------------------
    def request(self, fundamental, amplitude=0.0):
        V, O = self.V, self.O
        voice = -1
        for i in range(V):
            if not self.active[i]:
                voice = i
                break
        if voice < 0:
            pitch = ftom(fundamental)
            distance, nearest = 0.0, -1
            for i in range(V):
                offset = pitch - self.guide[i]
                offset *= offset
                if nearest < 0 or offset < distance:
                    nearest, distance = i, offset
            voice = nearest
        frequency = fundamental
        self.active[voice] = amplitude
        self.guide[voice] = ftom(fundamental)
        for j in range(O):
            previous = frequency
            frequency = fundamental * (1 + math.pow(j / (O - 1), self.harm) * (O - 1))
            p = voice * O + j
            self.mass[p], self.x[p], self.v[p] = 1.0, ftom(frequency), 0.0
            self.eq[p] = ftom(frequency) - ftom(previous)
        return voice

    def release(self, voice):
        if voice >= 0:
            self.active[voice] = 0.0
        else:
            self.active = [0.0] * self.V

    def makenote(self, pitch, amplitude):
        voice = self.request(mtof(pitch), amplitude)
        if voice >= 0:
            self.pitches[voice] = pitch
        return voice

    def endnote(self, pitch):
        for j in range(self.V):
            if self.pitches[j] == pitch:
                self.release(j)

    # ---- Minimizer::physics(), gather order ------------------------------------------------
    def _gravity(self, d, gmm):
        """force of one Gravity::tick with distance d = second - first; gmm = (G m_first) m_second"""
        if self.law == GRAV_TRUNC:
            cubed = abs(_trunc(d * d * d))
            cut = abs(int(d)) >= 0.5
        else:
            cubed = abs(d * d * d)
            cut = abs(d) >= 0.5
        force = gmm * d / (self.eps + cubed)
        return 0.0 if cut else force

    def physics(self):
        V, O, x, act = self.V, self.O, self.x, self.active
        newx = list(x)
        for i in range(V):
            if not act[i]:
                continue
            m = act[i]
            for j in range(O):
                p = i * O + j
                self.mass[p] = m
                a = 0.0
                first = self.guide[i] if j == 0 else x[p - 1]
                disp = (x[p] - first) - self.eq[p]
                a += (-self.kspring[p] * disp) / m
                if j + 1 < O:
                    disp = (x[p + 1] - x[p]) - self.eq[p + 1]
                    a += (self.kspring[p + 1] * disp) / m
                for u in range(V):
                    if u == i or not act[u]:
                        continue
                    mo = act[u]
                    for q in range(u * O, (u + 1) * O):
                        if u < i:     # this particle is `second`
                            a += (-self._gravity(x[p] - x[q], self.G * mo * m)) / m
                        else:         # this particle is `first`
                            a += self._gravity(x[q] - x[p], self.G * m * mo) / m
                vel = self.v[p] + a / SR
                vel *= self.drag
                self.v[p] = vel
                newx[p] = x[p] + vel / SR
        self.x = newx

    # ---- Additive ----------------------------------------------------------------------
    def peek(self):
        sample = 0.0
        scale = self.V * self.norm
        for i in range(self.V):
            if self.amps[i]:
                for j in range(self.O):
                    sample += self.amps[i] * self.dec[j] * math.sin(2 * PI * self.phase[i * self.O + j]) / scale
        return sample

    def tick(self):
        V, O, s = self.V, self.O, self.s
        for i in range(V):
            self.amps[i] = (1 - self.attack) * self.active[i] + self.attack * self.amps[i]
        for i in range(V):
            if self.active[i] or self.amps[i]:
                for p in range(i * O, (i + 1) * O):
                    self.tfreq[p] = mtof(self.x[p])
                    self.phase[p] += self.freq[p] / SR
                    self.tphase[p] += self.freq[p] / SR
                    self.freq[p] = self.tfreq[p] * (1 - s) + self.freq[p] * s
                    w = (1 - s) * math.sin(2 * PI * (2 * abs(self.tphase[p] - self.phase[p]) + 0.25))
                    self.phase[p] = w * self.tphase[p] + (1 - w) * self.phase[p]
                    self.phase[p] -= _trunc(self.phase[p])
                    self.tphase[p] -= _trunc(self.tphase[p])

    def physics_every(self, period):
        self.period = period
        self.T = 0

    def fill(self, n, track=None):
        """n x { out = operator()(); if (T >= p && T % p == 0) physics(); tick(); T++ };
        positions after every step are appended to `track`"""
        out = np.zeros(n)
        p = self.period
        for t in range(n):
            out[t] = self.peek()
            if p > 0 and self.T >= p and self.T % p == 0:
                self.physics()
                if track is not None:
                    track.append(list(self.x))
            self.tick()
            self.T += 1
        return out

    def positions(self):
        return np.array(self.x, dtype=np.float64)


def run_scenario(sc, law, obj=None):
    """Drive a PhysAdditive (or an object with the same makenote / endnote / physics_every / fill
    members) through a scenario dict: V, O, decay, harm, k, period, n, events [(t, kind, a, b)] with
    kind 0 makenote, 1 endnote.  Returns (audio, track [steps][V*O] or None, object)."""
    track = None
    if obj is None:
        obj = PhysAdditive(sc["V"], sc["O"], sc["decay"], sc["harm"], sc["k"], law=law)
        track = []
        obj.physics_every(sc["period"])
    n, pos, chunks = sc["n"], 0, []
    times = sorted({t for t, *_ in sc["events"]} | {n})
    for t in times:
        if t > pos:
            chunks.append(obj.fill(t - pos, track) if track is not None else obj.fill(t - pos))
            pos = t
        for et, kind, a, b in sc["events"]:
            if et == t and t < n:
                if kind == 0:
                    obj.makenote(a, b)
                else:
                    obj.endnote(a)
    audio = np.concatenate(chunks) if chunks else np.zeros(0)
    return audio, (np.array(track, dtype=np.float64).reshape(-1, sc["V"] * sc["O"]) if track is not None else None), obj


# the scenarios of tests/golden/physics_ref.npz (make_golden_physics.py) and of the GPU tests
SCENARIOS = {
    # three voices, two of them 0.3 semitone apart (inside the cutoff), one released mid-run
    "v3o4": dict(V=3, O=4, decay=0.75, harm=1.0, k=0.1, period=2, n=512,
                 events=[(0, 0, 60.0, 1.0), (0, 0, 60.3, 0.5), (0, 0, 67.2, 0.8), (200, 1, 60.3, 0.0)]),
    # two voices, a third note steals the nearest: its particles and velocities are re-initialised
    "steal": dict(V=2, O=3, decay=0.75, harm=1.0, k=0.1, period=2, n=256,
                  events=[(0, 0, 60.0, 1.0), (0, 0, 60.4, 0.7), (100, 0, 60.2, 0.9)]),
    # period 3: no step before sample 3 (T >= p), then every third
    "p3": dict(V=2, O=3, decay=0.75, harm=1.0, k=0.1, period=3, n=128,
               events=[(0, 0, 57.0, 1.0), (0, 0, 57.25, 0.6)]),
}
