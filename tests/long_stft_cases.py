"""Inputs and numpy models shared by tests/test_long_stft_cpu.py and tests/test_long_stft_gpu.py.
TEST INFRASTRUCTURE: numpy only, built on tests/stft_spec.py; nothing here is shared with the engine.

  * two_pass_forward / two_pass_inverse: the four-step transform of huygens_amd/csrc/hz_fft_long.h
    as array operations (numpy.fft for the sub-transforms, decimation in frequency modelled as
    "bin bitrev(p) ends up at position p"), so the bin-index map k(p1, p2) = bitrev_lg1(p1) +
    N1 bitrev_lg2(p2) can be checked without a GPU;
  * the gate cases for frames of 16,384 to 262,144 points and the 10 x keep gate (a reference
    program zeroes the bins with |X|^2 < 10 average^2; the engine's keep gate zeroes a bin unless
    |X|^2 > thr: the two differ at equality only, which a margin >= MARGIN_MIN excludes).
"""
from __future__ import annotations

import functools

import numpy as np

import stft_spec as sp

LONG_LGS = list(range(14, 19))


def split(lg):
    lg1 = lg // 2
    return lg1, lg - lg1


def bitrev(p, lg):
    p = np.asarray(p)
    r = np.zeros_like(p)
    for b in range(lg):
        r |= ((p >> b) & 1) << (lg - 1 - b)
    return r


def bin_of(p1, p2, lg):
    """The bin stored in workspace row p1, column p2 after the forward row pass."""
    lg1, lg2 = split(lg)
    return bitrev(p1, lg1) + (bitrev(p2, lg2) << lg1)


def two_pass_forward(x, lg):
    """[N1][N2] array of the forward transform's stored positions."""
    lg1, lg2 = split(lg)
    N1, N2, N = 1 << lg1, 1 << lg2, 1 << lg
    a = np.asarray(x, dtype=np.complex128).reshape(N1, N2)        # a[n1, n2] = x[N2 n1 + n2]
    k1 = bitrev(np.arange(N1), lg1)
    b = np.fft.fft(a, axis=0)[k1, :]                              # column pass: position p1 holds k1 = bitrev(p1)
    e = (k1[:, None] * np.arange(N2)[None, :]) % N
    b = b * np.exp(-2j * np.pi * e / N)                           # inter-pass twiddle W_N^(n2 k1)
    return np.fft.fft(b, axis=1)[:, bitrev(np.arange(N2), lg2)]   # row pass: position p2 holds k2 = bitrev(p2)


def two_pass_inverse(c, lg):
    """Stored positions -> N-point unnormalised inverse transform, natural order."""
    lg1, lg2 = split(lg)
    N1, N2, N = 1 << lg1, 1 << lg2, 1 << lg
    k1 = bitrev(np.arange(N1), lg1)
    nat2 = np.empty_like(c)
    nat2[:, bitrev(np.arange(N2), lg2)] = c                       # decimation in time reads bit-reversed
    d = np.fft.ifft(nat2, axis=1) * N2
    e = (k1[:, None] * np.arange(N2)[None, :]) % N
    d = d * np.exp(2j * np.pi * e / N)
    nat1 = np.empty_like(d)
    nat1[k1, :] = d
    return (np.fft.ifft(nat1, axis=0) * N1).reshape(N)


# ---- gates ----------------------------------------------------------------------------------------

GATE_CASES = [
    sp._gc(16384, 4, False),
    sp._gc(16384, 4, True),
    sp._gc(32768, 2, False),
    sp._gc(65536, 8, True, n=3 * 65536 + 1),
    sp._gc(262144, 16, False, n=2 * 262144 + 40),
]
GATE_KINDS = ["static", "keep", "keep10"]


def proc_keep10(X, N):
    """make_golden_stft.proc_gate_keep with the threshold 10 average^2 (sequential long double sum)."""
    average = np.add.accumulate(np.hypot(X.real, X.imag).astype(np.longdouble))[-1] / N
    nrm = (X.real * X.real + X.imag * X.imag).astype(np.longdouble)
    thr = 10 * average * average
    return np.where(nrm > thr, X, 0), float(np.min(np.abs(nrm - thr) / thr))


@functools.lru_cache(maxsize=None)
def gate_run(case, kind):
    if kind == "keep10":
        return sp.run(sp.gate_input(case), case.N, case.laps, 0, proc_keep10)
    return sp.gate_run(case, kind)
