"""The PHASE and STICKS parity cases shared by tests/test_het_chains_{cpu,gpu}.py.  TEST INFRASTRUCTURE.

The GPU tests run these configurations against the restatement; the CPU tests assert that each
case can see what it is meant to see (live signed zeros, latch traffic, gate decisions with a
margin), so a passing GPU case means something."""
import numpy as np

from oracle_chains import OraclePhase, OracleSticks

CALLS = [1, 15, 16, 17, 300]   # ragged mix rounds (kCH = 16), state carried across calls
TOTAL = sum(CALLS)

# channels, order, stick_order, width, seed
#   channels: 1; the reference's own 48; 65 and 130 cross the 64-lane boundary with dead lanes
#   order: phasebank's multiplicity 1 and harmbank's 4; width <= 4 takes the non-prefetch path
PHASE_CASES = [(1, 1, 1, 3, 1), (48, 1, 1, 2400, 2), (65, 4, 2, 7, 3), (130, 4, 1, 2400, 4), (130, 1, 2, 3, 5)]
STICK_RAD = {1: -0.9, 2: -0.2}   # stable Stickbanks (the feedback is (z + rad)^order)
THRESH = 0.004

# channels, pre, post, seed
STICKS_CASES = [(48, 3, 1, 11), (1, 1, 0, 12), (65, 2, 2, 13), (130, 3, 1, 14)]
STICKS_RAD, STICKS_GATE = -0.9, 0.02


def signal(n, seed, amp=0.5):
    """A quiet lead-in (the latches arm), then noise plus a tone under an on/off envelope (they
    engage and release)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    env = np.where(t < 8, 1e-4, (np.sin(2 * np.pi * (t - 8) / 90.0) > -0.2).astype(float))
    return amp * env * (np.sin(2 * np.pi * 1900.0 * t / 48000) + 0.5 * rng.standard_normal(n))


def pieces(x):
    a = 0
    for n in CALLS:
        yield x[a:a + n]
        a += n


def configure(h, N, seed, active=0.8):
    """Frequencies of both banks; some channels inactive in each bank."""
    rng = np.random.default_rng(1000 + seed)
    fa = rng.uniform(200, 6000, N) * np.where(rng.random(N) < 0.5, -1, 1)
    fs = -2 * fa
    idx = np.arange(N)
    h.freqmod(0, idx, fa)
    h.freqmod(1, idx, fs)
    for b in (0, 1):
        on = idx[rng.random(N) < active] if N > 1 else idx
        h.activate(b, on)
    return h


def phase_args(N, order, sorder, width, seed):
    rng = np.random.default_rng(seed)
    radii = np.zeros(2 * N)
    radii[0::2] = rng.uniform(0.5, 0.9, N)
    radii[1::2] = 0.05 * rng.standard_normal(N)   # complex radii
    return (N, order, radii, THRESH, 0.2, width, sorder, STICK_RAD[sorder], 0.1, 3.0)


def phase_oracle(case, record=False):
    N, order, sorder, width, seed = case
    return configure(OraclePhase(*phase_args(N, order, sorder, width, seed), record=record), N, seed)


def sticks_oracle(case, gate=STICKS_GATE, record=False):
    N, pre, post, seed = case
    return configure(OracleSticks(N, pre, post, STICKS_RAD, gate, 0.1, 1.0, record=record), N, seed)
