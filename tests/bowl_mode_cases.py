"""The cases of tests/test_bowl_modes_gpu.py, shared with their CPU proofs
(tests/test_bowl_float_model_cpu.py).  TEST INFRASTRUCTURE; numpy only.

A case is a Bowl<float> bank, a start counter and a list of call lengths.  One-hot cases give
every mode but one the amplitude 0: the float restatement of such a bank is OracleBowl(1, ...) of
the hot mode, bit for bit (a term of amplitude 0 adds +-0 to the float running sum), so a bank of
thousands of modes has a single-mode reference and the bound is relative to that mode's own
amplitude.  Everything below is data; the helpers only expand it.
"""
import numpy as np

import bowl_float_model as bm

SR = 48000
STUCK = bm.STUCK

# ---- fill(): one-hot banks ------------------------------------------------------------------------
FILL_M = [1, 303, 2048, 2049, 16400]
FILL_GROUPS = [1, 8, 256]
# from trigger(): short reduce with a ragged tail; slab reduce, several time segments; then calls
# that carry the counter (one sample, less than a chunk, a ragged tile, the look-ahead threshold)
FILL_CALLS = [3 * 1024 + 517, 17000, 1, 15, 1021, 64]
FILL_WINDOWS = [(0, 3589), (3589, 20589), (20589, 21690)]   # the compared windows (first two calls, the rest)
# bowl_launch's plan of the calls whose plan is distinct, restated as literals:
# (M, target_groups) -> {n: (per_wave, G, nseg, reduce)}.  tests/test_bowl_float_model_cpu.py
# recomputes them; a changed plan fails there instead of silently moving the edges.
FILL_PLANS = {
    (1, 1): {3589: (1, 1, 1, "short"), 17000: (1, 1, 1, "slab"), 1021: (1, 1, 1, "short")},
    (1, 8): {3589: (1, 1, 4, "short"), 17000: (1, 1, 6, "slab"), 1021: (1, 1, 1, "short")},
    (1, 256): {3589: (1, 1, 4, "short"), 17000: (1, 1, 17, "slab"), 1021: (1, 1, 1, "short")},
    (303, 1): {3589: (2, 19, 1, "short"), 17000: (2, 19, 1, "slab"), 1021: (2, 19, 1, "short")},
    (303, 8): {3589: (2, 19, 1, "short"), 17000: (2, 19, 1, "slab"), 1021: (2, 19, 1, "short")},
    (303, 256): {3589: (1, 38, 4, "short"), 17000: (1, 38, 6, "slab"), 1021: (1, 38, 1, "short")},
    (2048, 1): {3589: (8, 32, 1, "short"), 17000: (8, 32, 1, "slab"), 1021: (8, 32, 1, "short")},
    (2048, 8): {3589: (8, 32, 1, "short"), 17000: (8, 32, 1, "slab"), 1021: (8, 32, 1, "short")},
    (2048, 256): {3589: (2, 128, 2, "short"), 17000: (8, 32, 6, "slab"), 1021: (1, 256, 1, "short")},
    (2049, 1): {3589: (9, 29, 1, "short"), 17000: (9, 29, 1, "slab"), 1021: (9, 29, 1, "short")},
    (2049, 8): {3589: (9, 29, 1, "short"), 17000: (9, 29, 1, "slab"), 1021: (9, 29, 1, "short")},
    (2049, 256): {3589: (2, 129, 2, "short"), 17000: (8, 33, 6, "slab"), 1021: (1, 257, 1, "short")},
    (16400, 1): {3589: (64, 33, 1, "short"), 17000: (64, 33, 1, "slab"), 1021: (64, 33, 1, "short")},
    (16400, 8): {3589: (64, 33, 1, "short"), 17000: (64, 33, 1, "slab"), 1021: (64, 33, 1, "short")},
    (16400, 256): {3589: (16, 129, 2, "short"), 17000: (64, 33, 6, "slab"), 1021: (4, 513, 1, "short")},
}
PLAN_CALLS = [3589, 17000, 1021]


def fill_hot(M, groups):
    """the plan's edge modes of every distinct plan of the case's calls"""
    hot = set()
    for n in PLAN_CALLS:
        hot |= set(bm.hot_modes(M, n, groups))
    return sorted(hot)


def mode_of(M, i):
    """mode i's (f, a, d) of the one-hot cases: log-uniform 50 Hz .. 16 kHz, a in [1e-4, 5e-2],
    d in [0.05, 15] (test_c5_shape's ranges; f from 50 Hz so that the 1101-sample window of the
    carried calls holds a full cycle)"""
    rng = np.random.default_rng([M, i])
    return (float(np.exp(rng.uniform(np.log(50.0), np.log(16000.0)))), float(rng.uniform(1e-4, 5e-2)),
            float(rng.uniform(0.05, 15.0)))


def one_hot(M, i, fad):
    """full-length coefficient vectors with mode i alone sounding.  The silent modes keep a
    frequency and a decay of their own (drawn once per M): only their amplitude is 0"""
    rng = np.random.default_rng(M)
    f = np.exp(rng.uniform(np.log(20.0), np.log(16000.0), M))
    d = rng.uniform(0.05, 15.0, M)
    a = np.zeros(M)
    f[i], a[i], d[i] = fad
    return f, a, d


# ---- multi-mode banks against the model -----------------------------------------------------------
def c5_shape_model(M):
    """test_bowl_gpu.py::test_c5_shape's model"""
    rng = np.random.default_rng(M)
    return (np.exp(rng.uniform(np.log(20.0), np.log(16000.0), M)), rng.uniform(1e-4, 5e-2, M),
            rng.uniform(0.05, 15.0, M))


MULTI = [("shape", 2048, 5000, 256), ("shape", 303, 30000, 256), ("shape", 5, 7000, 1), ("bench", 2048, 5000, 256)]
SUM_SLACK = 1e-12   # x sum of a_i: the mode sum's order and the last bits of exp, in float64


def multi_calls(n):
    return [n // 3, 1, n - n // 3 - 1]


# ---- late counters and the saturation at 2^24 -----------------------------------------------------
LATE_WINDOW = 6000
LATE_STARTS = [479_000, 4_000_000, STUCK - 3000]   # the last sticks at sample 3000: 3000 % 16 = 8
LATE_STEP = 2 ** 20                                # fill_device calls that only advance the counter
# (f, a, d).  At 2^24 the phase p = f n / SR has a float spacing of 0.5 cycles from 12 kHz up, where
# every wave value is sin(k pi) ~ 0: the reference is silent there, so the 16 kHz mode is only
# compared at the first two starts.  d in {0, 0.003, 0.02} keeps e^(-d n / SR) >= 3e-4 at 2^24.
LATE_MODES = [(440.0, 0.03, 0.003), (3001.7, 0.02, 0.02), (7000.3, 0.05, 0.0), (16000.0, 0.01, 0.003)]
LATE_M = [1, 65]
LATE_HOT = {1: [0], 65: [0, 64]}


def late_modes(start):
    return [m for m in LATE_MODES if not (start > 4_000_000 and m[0] >= 12000.0)]


def late_bank(M):
    """the all-hot bank of the late cases: the late modes' ranges, d small enough for 2^24"""
    rng = np.random.default_rng(1000 + M)
    return (np.exp(rng.uniform(np.log(20.0), np.log(11000.0), M)), rng.uniform(1e-3, 5e-2, M),
            rng.choice([0.0, 0.003, 0.02], M))


def advance_calls(start):
    """call lengths that take a triggered Bowl to counter `start`"""
    return [LATE_STEP] * (start // LATE_STEP) + ([start % LATE_STEP] if start % LATE_STEP else [])


# ---- the fused Bowl -> Delaybank block ------------------------------------------------------------
CHAIN_M = [300, 512, 513, 2048, 2049, 4100]
CHAIN_HOT = [0, 511, 512, 2047, 2048]        # and M - 1: the thread's four table entries, the second pass
CHAIN_BLOCKS = [1024, 1021, 64, 3, 1]
CHAIN_LINES = 5
CHAIN_LATE_M = CHAIN_M                       # every M also from 479,000 and across 2^24
CHAIN_LATE = 479_000
CHAIN_STUCK_START = STUCK - 2050             # blocks of 1024: the third starts at 2^24 - 2, so the counter
CHAIN_STUCK_BLOCKS = [1024, 1024, 1024, 1021, 64, 3, 1]   # sticks at the third sample of its first workgroup


def chain_hot(M):
    return sorted({i for i in CHAIN_HOT + [M - 1] if i < M})


def chain_taps(k):
    """test_chain_gpu.py's C5 taps: every feedback tap is longer than a block, so the block fuses"""
    return [(0, 1.0)], [(10000 + 37 * k, 0.5), (20000 + 53 * k, 0.5)]


def chain_mode(M, i, late):
    """a hot mode of the chain cases; late: d from the late cases' set"""
    f, a, d = mode_of(M, i)
    if late:
        d = [0.0, 0.003, 0.02][i % 3]
        f = min(f, 11000.0)
    return f, a, d


RENDER_DEVICE_N = [1, 63, 64, 1025, 17000]
