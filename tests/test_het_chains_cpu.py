"""CPU: the PHASE and STICKS restatements (tests/oracle_chains.py) against the existing chain's
restatement, scalar state machines and closed forms, and the conditions under which the GPU
parity cases (tests/het_chain_cases.py) can see what they are meant to see."""
import math

import numpy as np
import pytest

from het_chain_cases import (PHASE_CASES, STICKS_CASES, STICKS_GATE, TOTAL, configure, phase_args, phase_oracle,
                             signal, sticks_oracle)
from huygens_amd._lib import header_symbols
from huygens_amd.heterodyne import phasebank
from oracle_chains import (OUT_LIMITER, OUT_RAW, PI, OracleHarm, OraclePhase, OracleSticks, output_stage,
                           softclip)
from oracle_het import OracleHet


@pytest.mark.parametrize("case", PHASE_CASES[1:3])
def test_shared_front_end(case):
    """Nothing downstream of the RMSbank feeds back: analysis, synthesis, Slidebank, RMS sums and
    history of the PHASE restatement equal the existing chain's restatement bit for bit."""
    N, order, sorder, width, seed = case
    args = phase_args(N, order, sorder, width, seed)
    p, o = configure(OraclePhase(*args), N, seed), configure(OracleHet(*args), N, seed)
    x = signal(TOTAL, seed)
    p.process(x)
    o.process(x)
    for what in (0, 1, 2, 3, 6):
        assert np.array_equal(p.state(what), o.state(what)), f"state {what}"


def test_harm_restatement_equals_the_c_restatement():
    """OracleHarm (the numpy chain that carries the output stage) against oracle/hz_oracle_het.c."""
    N, order, sorder, width, seed = PHASE_CASES[2]
    args = phase_args(N, order, sorder, width, seed)
    p, o = configure(OracleHarm(*args), N, seed), configure(OracleHet(*args), N, seed)
    x = signal(TOTAL, seed)
    assert np.max(np.abs(p.process(x) - o.process(x))) <= 1e-13
    for what in range(7):
        assert np.array_equal(p.state(what), o.state(what)), f"state {what}"


class ScalarLatch:
    """latchbank.h:83-93 for one channel."""

    def __init__(self, lo, hi):
        self.lo, self.hi, self.armed, self.engaged = lo, hi, False, False

    def update(self, r):
        self.armed = self.armed or r < self.lo
        if self.engaged and r < self.lo:
            self.engaged = self.armed = False
        elif not self.engaged and r > self.hi and self.armed:
            self.engaged = True
        return self.engaged


def latch_run(x, width=2400, thresh=5e-4, ratio=0.2):
    """One channel whose Slidebank passes x through (radius 0, closed oscillators), so the RMS sum
    is the running sum of x^2: the oracle's two-updates-per-sample trace and the scalar machine's."""
    o = OraclePhase(1, 1, np.zeros(2), thresh, ratio, width, record=True)
    o.process(x)
    m = ScalarLatch(thresh * ratio, thresh * (1 - ratio))
    rs, a2s, want, r1s = 0.0, [], [], []
    for t, v in enumerate(x):
        a2s.append(v * v)
        rs = (a2s[t] - (a2s[t - width] if t >= width else 0.0)) + rs
        r1 = math.sqrt(rs / width)
        e1 = m.update(r1)
        e2 = m.update(math.sqrt(r1 / width))
        want.append((e1, e2, m.armed))
        r1s.append(r1)
    got = list(zip((bool(e[0]) for e in o.trace["engaged1"]), (bool(e[0]) for e in o.trace["engaged"])))
    assert got == [(w[0], w[1]) for w in want]
    assert (bool(o.armed[0]), bool(o.engaged[0])) == (want[-1][2], want[-1][1])
    return np.array(r1s), want


def ramp_input(r1, width=2400):
    """x whose running sum of squares follows width r1^2 (r1 rising)."""
    rsum = width * np.asarray(r1) ** 2
    return np.sqrt(np.diff(rsum, prepend=0.0))


def test_latch_trace_two_updates_per_sample():
    """width 2400, lo 1e-4, hi 4e-4.  The second update sees r2 = sqrt(r1 / 2400), which exceeds
    r1 for r1 < 1 / 2400: for r1 in (3.84e-4, 4e-4) on an armed, disengaged channel r1 does not
    engage (r1 <= hi) but r2 > hi does -- the magnitude path stays shut for that sample while
    the phase path opens.  For r1 in (4e-4, 0.384) r1 engages at the first update (there r2 lies in
    (4.08e-4, 0.0127), above hi as well).  Both kinds of sample are in the traces."""
    # a slow rising ramp through the disagreement window
    r1, want = latch_run(ramp_input(np.geomspace(1e-5, 1.0, 400)))
    split = [t for t, w in enumerate(want) if w[0] != w[1]]
    assert split and all(3.84e-4 < r1[t] <= 4e-4 and not want[t][0] and want[t][1] for t in split)
    assert want[-1][1] and not want[0][1]
    # an armed channel jumping into (4e-4, 0.384): the first update engages
    r1, want = latch_run(ramp_input([5e-5, 6e-5, 1e-3, 2e-3, 0.3]))
    assert [w[0] for w in want] == [False, False, True, True, True] and 4e-4 < r1[2] < 0.384
    # a burst, then silence: the sum falls once the burst leaves the window; the latch releases
    # at the first update and disarms, then re-arms one sample later
    # (squares that sum without rounding: the sum returns to exactly 0, never below)
    x = np.concatenate([[2.0 ** -20], np.full(50, 0.25), np.zeros(2500)])
    r1, want = latch_run(x)
    eng = np.array([w[1] for w in want])
    assert eng[1:2400].all() and not eng[-1] and want[-1][2]


@pytest.mark.parametrize("case", PHASE_CASES)
def test_signed_zeros_are_live(case):
    """Every PHASE parity case has samples with P = +-pi on disengaged channels and a channel
    that engages afterwards while its smoothbank still holds more than 1e-3 of it: a kernel that
    shortcut silent channels to P = 0 would fail the case."""
    o = phase_oracle(case, record=True)
    y = o.process(signal(TOTAL, case[-1]))
    assert np.max(np.abs(y)) > 1e-2
    P, E, Y = (np.array(o.trace[k]) for k in ("P", "engaged", "y"))
    silent_pi = (np.abs(P) == np.pi) & ~E
    assert silent_pi.any()
    rise = E[1:] & ~E[:-1] & (Y[:-1] > 1e-3)
    seen = [c for c in range(case[0]) for t in np.flatnonzero(rise[:, c])[:1] if silent_pi[:t + 1, c].any()]
    assert seen
    if case[3] <= 7:   # short windows also release
        assert (~E[1:] & E[:-1]).any()


@pytest.mark.parametrize("pre,rad", [(1, -0.9), (3, -0.999), (4, -0.5)])
def test_sticks_impulse_closed_form(pre, rad):
    """`pre` cascaded one-pole sticks: (1 + rad)^pre C(t + pre - 1, pre - 1) (-rad)^t."""
    o = OracleSticks(1, pre, 0, rad, 0.0, 0.0, 1.0)
    n = 200
    x = np.zeros(n)
    x[0] = 1.0
    y = o.process(x)
    want = np.array([(1 + rad) ** pre * math.comb(t + pre - 1, pre - 1) * (-rad) ** t for t in range(n)])
    assert np.max(np.abs(y - want) / np.abs(want)) <= 1e-12


def test_gate_zeroes_exactly_the_samples_below_threshold():
    case = STICKS_CASES[1]   # one Stickbank, the gate behind it: the state does not depend on the gate
    g, u = sticks_oracle(case, record=True), sticks_oracle(case, gate=0.0)
    x = signal(TOTAL, case[-1])
    yg, yu = g.process(x), u.process(x)
    shut = np.array(g.trace["gated"])[:, 0]
    assert shut.any() and not shut.all()
    assert np.array_equal(shut, np.array(g.trace["mag"])[:, 0] < STICKS_GATE)
    assert np.array_equal(yg, np.where(shut, 0.1 * x, yu))   # dry 0.1, RAW: only the dry part is left


@pytest.mark.parametrize("case", STICKS_CASES)
def test_gate_margin(case):
    """A condition on the case, not a measurement: no |x| lies within 1e-9 (relative) of the gate,
    so a device hypot one ulp from libm's cannot flip a decision."""
    o = sticks_oracle(case, record=True)
    o.process(signal(TOTAL, case[-1]))
    mag, shut = np.array(o.trace["mag"]), np.array(o.trace["gated"])
    assert np.min(np.abs(mag / STICKS_GATE - 1)) > 1e-9
    assert 0.05 < shut.mean() < 0.95   # both decisions occur


def test_output_stage():
    rng = np.random.default_rng(5)
    x, mix = rng.standard_normal(500), 0.5 * rng.standard_normal(500)
    # drive 0: today's expression
    assert np.array_equal(output_stage(x, mix, 0.3, 3.0), 2.0 / PI * np.arctan(0.3 * x + 3.0 * mix))
    assert np.array_equal(output_stage(x, mix, 0.3, 3.0, OUT_RAW), 0.3 * x + 3.0 * mix)

    def scalar(xv, m, dry=0.0, gain=1.0, drive=4.0, width=0.9):   # tests/slidebank.cpp:81-95
        s = drive * m
        if abs(s) >= width:
            sign = 1 if s > 0 else -1
            gap = s - sign * width
            s = sign * width + (1 - width) * 2.0 / PI * math.atan(PI * gap / (2 * (1 - width)))
        return 2.0 / PI * math.atan(dry * xv + gain * s)
    got = output_stage(x, mix, 0.0, 1.0, OUT_LIMITER, 4.0, 0.9)
    want = np.array([scalar(float(a), float(b)) for a, b in zip(x, mix)])
    assert (np.abs(4.0 * mix) < 0.9).any() and (np.abs(4.0 * mix) > 0.9).any()
    assert np.max(np.abs(got - want)) <= 4 * np.finfo(float).eps
    assert np.array_equal(softclip(np.array([0.5, -0.5]), 0.9), [0.5, -0.5])


def test_phasebank_config():
    """tests/phasebank.cpp: 48 channels from mtof(28), +-partials, synthesis an octave up, reversed."""
    n, fa, fs, radii = phasebank()
    assert n == 48
    assert np.allclose(fs, -2 * fa)
    assert math.isclose(fa[0], 440.0 * 2 ** ((28 - 69) / 12), rel_tol=1e-12)
    assert np.all(fa[0::2] > 0) and np.all(fa[1::2] < 0)
    assert np.all((radii[0::2] > 0.9) & (radii[0::2] <= 0.999)) and not radii[1::2].any()


def test_abi_declares_the_chains():
    syms = header_symbols()
    for s in ("hz_het_create_phase", "hz_het_create_sticks", "hz_het_set_output", "hz_het_chain"):
        assert s in syms
