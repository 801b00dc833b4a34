"""CPU: what tests/test_long_stft_gpu.py relies on, proved without a GPU.

1. The bin-index map of DESIGN.md 4.10 / hz_fft_long.h -- workspace row p1, column p2 holds bin
   bitrev_lg1(p1) + N1 bitrev_lg2(p2) -- against numpy.fft for every lg in 14..18, with a pure
   numpy model of the two passes (tests/long_stft_cases.py), and what follows from it: the inverse
   mirror needs no re-ordering, and the Hilbert half band is "p2 even".
2. The conditions on the gate inputs: every bin at least MARGIN_MIN from its threshold, at least 16
   frames (sp.gate_cuts), every gate passes bins, and the kept set changes between consecutive
   frames.
"""
import numpy as np
import pytest
import scipy.fft

import long_stft_cases as lc
import stft_spec as sp


@pytest.mark.parametrize("lg", lc.LONG_LGS)
def test_bin_index_map(lg):
    N = 1 << lg
    lg1, lg2 = lc.split(lg)
    assert lg1 + lg2 == lg and max(lg1, lg2) <= 9 and min(lg1, lg2) >= 7
    x = sp.noise(N, 900 + lg)
    X = np.fft.fft(x)
    c = lc.two_pass_forward(x, lg)
    p1, p2 = np.meshgrid(np.arange(1 << lg1), np.arange(1 << lg2), indexing="ij")
    k = lc.bin_of(p1, p2, lg)
    assert np.array_equal(np.sort(k.ravel()), np.arange(N))   # a permutation of the bins
    assert np.max(np.abs(c - X[k])) < 1e-11 * np.max(np.abs(X))
    # the Hilbert half band k < N/2 is the even columns
    assert np.array_equal(k < N // 2, (p2 & 1) == 0)
    # the mirror: stored positions straight into the inverse passes
    y = lc.two_pass_inverse(c, lg)
    assert np.max(np.abs(y - N * x)) < 1e-11 * N * np.max(np.abs(x))
    # a position-dependent processor through the map: gains g[k] applied at k(p1, p2)
    g = sp.bin_gains(N)
    y = lc.two_pass_inverse(c * g[k], lg)
    assert np.max(np.abs(y - np.fft.ifft(g * X) * N)) < 1e-11 * N * np.max(np.abs(x))


@pytest.mark.parametrize("lg", [14, 15])
def test_makhoul_through_two_passes(lg):
    """REDFT10 as the engine computes it above 8192: even/odd reorder, the two passes, the rotation
    e^(-i pi k / 2N) read at k(p1, p2)."""
    N = 1 << lg
    x = np.random.default_rng(lg).standard_normal(N)
    v = np.empty(N)
    v[:N // 2] = x[0::2]
    v[N - 1 - np.arange(N // 2)] = x[1::2]
    c = lc.two_pass_forward(v, lg)
    lg1, lg2 = lc.split(lg)
    p1, p2 = np.meshgrid(np.arange(1 << lg1), np.arange(1 << lg2), indexing="ij")
    k = lc.bin_of(p1, p2, lg)
    y = np.empty(N)
    y[k] = 2 * (c * np.exp(-1j * np.pi * k / (2 * N))).real
    ref = scipy.fft.dct(x, type=2)
    assert np.max(np.abs(y - ref)) < 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("kind", lc.GATE_KINDS)
@pytest.mark.parametrize("case", lc.GATE_CASES, ids=lambda c: c.id)
def test_gate_input_conditions(case, kind):
    ref = lc.gate_run(case, kind)
    print(f"{case.id} {kind}: margin {ref.margin:.2e}, {len(ref.starts)} frames")
    assert ref.margin >= sp.MARGIN_MIN
    assert len(ref.starts) >= 16   # sp.gate_cuts cuts after frames 0 and 15
    cuts = sp.gate_cuts(case.n, case.N, case.laps)
    assert cuts == sorted(set(cuts)) and cuts[-1] == case.n
    kept = ref.keep.sum(axis=1)
    assert np.all(kept > 0) and np.all(kept < case.N)   # every frame: the gate passes and stops bins
    assert np.all(np.any(ref.keep[1:] != ref.keep[:-1], axis=1))   # the kept set changes every frame
    assert np.max(np.abs(ref.y)) > 0
