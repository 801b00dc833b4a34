"""numpy spec of Fourier / StaticSTFT at the level of one frame's spectrum.  TEST INFRASTRUCTURE.

Built on tests/golden/make_golden_stft.py (its `window`, its `proc_*` and the closed-form schedule
s = stride*i + c*(2N-1)); nothing here is shared with the C oracle or the engine.  Where the
fixtures' `stft_run` only returns the overlap-added output, this module also names what the
processor is handed -- frame j of `frame_starts` is np.fft.fft(w * x[s:s+N]): FFTW order,
unnormalised, forward sign e^{-} -- and what a gate decided for it (the per-frame keep masks), so
a test can state conditions on its input from the spec alone.

The signal builders and the case tables at the end are the inputs of tests/test_stft_spectrum_gpu.py;
tests/test_stft_spectrum_cpu.py proves their conditions without a GPU.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from golden.make_golden_stft import proc_gate_keep, proc_hilbert, proc_static_gate, window as _window

WIN_NAMES = {0: "halfhann", 1: "hann", "halfhann": "halfhann", "hann": "hann"}


def window(kind, N):
    """kind: 0 / "halfhann" (Fourier) or 1 / "hann" (StaticSTFT), as huygens_amd.stft.WIN_*."""
    return _window(WIN_NAMES[kind], N)


def frame_starts(n, N, laps):
    """Start sample of every frame completing within n samples, in frame order f = c*2*laps + i:
    the order in which the reference calls the processor."""
    stride, S, P = N // laps, 2 * laps, 2 * N - 1
    starts = []
    c = 0
    while c * P + N - 1 < n:
        starts += [stride * i + c * P for i in range(S) if stride * i + c * P + N - 1 < n]
        c += 1
    return np.array(starts, dtype=np.int64)


def frame_spectra(x, N, laps, wkind):
    """[frames][N] complex: what the processor receives for each frame, in frame order."""
    x = np.asarray(x)
    w = window(wkind, N)
    starts = frame_starts(len(x), N, laps)
    return np.array([np.fft.fft(w * x[s:s + N]) for s in starts]).reshape(len(starts), N)


def proc_identity(X, N):
    return X, np.inf


class Run(NamedTuple):
    y: np.ndarray        # complex128 output, one sample per input sample
    starts: np.ndarray   # frame_starts
    keep: np.ndarray     # [frames][N] bool: bins the processor passed on unchanged
    margin: float        # smallest relative distance of any bin from its gate threshold


def run(x, N, laps, wkind, proc):
    """make_golden_stft.stft_run for any proc(X, N) -> (Y, margin), called in frame order (a
    processor may keep state).  Frame j's IFFT sample k, windowed, lands at t = starts[j] + N-1 + k;
    the slots are summed in slot order in long double and divided by the int N*laps/2."""
    x = np.asarray(x)
    n, S = len(x), 2 * laps
    w = window(wkind, N)
    starts = frame_starts(n, N, laps)
    ys = np.empty((len(starts), N), dtype=np.complex128)
    keep = np.empty((len(starts), N), dtype=bool)
    margin = np.inf
    for j, s in enumerate(starts):
        X = np.fft.fft(w * x[s:s + N])
        Y, m = proc(X, N)
        margin = min(margin, float(m))
        keep[j] = np.asarray(Y) == X
        ys[j] = np.fft.ifft(Y) * N
    tot = np.zeros(n, dtype=np.clongdouble)
    # every period but the last holds all S frames, so frame j is slot j % S; a slot's frames
    # never overlap in time, so adding them slot by slot is the sum in slot order
    for i in range(S):
        for j in range(i, len(starts), S):
            t0 = starts[j] + N - 1
            m = min(N, n - t0)
            tot[t0:t0 + m] += (w[:m] * ys[j].real[:m]) + 1j * (w[:m] * ys[j].imag[:m])
    tot /= (N * laps // 2)
    return Run(tot.astype(np.complex128), starts, keep, margin)


def launch_first_frames(cuts, N, laps):
    """Index of the first frame of each call when the input is split at `cuts` (a frame belongs
    to the call in which its last input sample arrives)."""
    ends = frame_starts(cuts[-1], N, laps) + N - 1
    return [int(np.sum(ends < c)) for c in cuts[:-1]]


# ---- inputs ---------------------------------------------------------------------------------------

def noise(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def ragged(n, N):
    """Call boundaries: a one-sample call, a call shorter than a frame, one of several frames."""
    cuts = sorted({0, 1, min(N // 2 + 2, n), min(2 * N + 3, n), n})
    return cuts


def hilbert_bins(N):
    """(negative-frequency bin index, positive-frequency bin index) of hilbert_signal."""
    kpos = max(1, N // 8)
    kneg = max(1, 3 * N // 16)
    return N - kneg, kpos


def hilbert_signal(n, N, seed):
    """e^{-2 pi i kneg t/N} + 0.6 e^{+2 pi i kpos t/N} + 0.05 complex noise: the Hilbert half-band
    removes the stronger, negative-frequency tone, which no position-blind processor would."""
    kneg, kpos = hilbert_bins(N)
    t = np.arange(n)
    return np.exp(2j * np.pi * kneg * t / N) + 0.6 * np.exp(2j * np.pi * kpos * t / N) + 0.05 * noise(n, seed)


def gate_bins(N):
    return [N // 8, 3 * N // 8, N // 4, N // 16 + 1]


GATE_AMPS = (1.0, 0.5, 0.25, 0.5)


def gate_signal(n, N, seed, cplx, hop=None, shift=0):
    """Non-stationary gate input: one tone whose bin steps through gate_bins(N) and whose amplitude
    steps through GATE_AMPS every `hop` samples (N/2 by default; the phase restarts with each
    segment), plus 1e-3 noise.  Real input is a sine, complex input the one-sided exponential with
    complex noise.  Consecutive frames see different tone mixes at different levels, so their
    averages, thresholds and kept bins all differ: both gates are scale-invariant, and a frame
    gated with its neighbour's threshold keeps other bins.  `shift` shortens the first segment."""
    hop = hop or N // 2
    t = np.arange(n) + shift
    seg = (t // hop) % 4
    k = np.array(gate_bins(N))[seg]
    a = np.array(GATE_AMPS)[seg]
    ph = 2 * np.pi * k * (t % hop) / N
    rng = np.random.default_rng(seed)
    if cplx:
        return a * np.exp(1j * ph) + 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return a * np.sin(ph) + 1e-3 * rng.standard_normal(n)


def gate_threshold(gate, X, N):
    """The |X|^2 threshold of make_golden_stft.proc_static_gate / proc_gate_keep for one frame."""
    if gate == "static":
        average = np.add.accumulate(np.sqrt(X.real * X.real + X.imag * X.imag) / N)[-1]
        return 100 * average * average
    average = np.add.accumulate(np.hypot(X.real, X.imag).astype(np.longdouble))[-1] / N
    return 625 * average * average


def gate_mask(gate, X, thr):
    """Bins a gate with threshold thr passes unchanged."""
    nrm = X.real * X.real + X.imag * X.imag
    return ~(nrm < thr) if gate == "static" else nrm.astype(np.longdouble) > thr


def gate_cuts(n, N, laps):
    """Call boundaries after frames 0 and 15: the launches begin at frames 0, 1 and 16, so the
    frames that share a transform are (1,2) ... (13,14) and (16,17) ..., both parities, and the
    first two launches end on a lone frame."""
    starts = frame_starts(n, N, laps)
    return [0, int(starts[0]) + N, int(starts[15]) + N, n]


def launched_pairs(cuts, N, laps):
    """(f, f + 1) for every two frames that share one transform when real input is split at
    `cuts`: each call pairs its frames from its first one on."""
    first = launch_first_frames(cuts, N, laps) + [len(frame_starts(cuts[-1], N, laps))]
    return [(f, f + 1) for a, b in zip(first[:-1], first[1:]) for f in range(a, b - 1, 2)]


class GateCase(NamedTuple):
    N: int
    laps: int
    cplx: bool
    n: int
    seed: int
    hop: int
    shift: int

    @property
    def id(self):
        return f"N{self.N}-l{self.laps}-{'cplx' if self.cplx else 'real'}"


def _gc(N, laps, cplx, n=None, seed=1, hop=None, shift=0):
    return GateCase(N, laps, cplx, n if n is not None else 9 * N, seed, hop or N // 2, shift)


# real input: the pair kernels (generic radix 8, the 4096 kernel, radix 16); complex input: the
# one-frame kernel with a gate.  N = 256 changes tone once per frame length.  8192 / 32 runs
# 3 N + 1 samples, 65 frames.  N = 512 real changes tone every 3 N / 4: in a frame split evenly
# between two sines the strongest bin stays below 25 x the mean magnitude and the keep gate passes
# nothing; with the longer segments every frame has one tone across its middle.
GATE_CASES = [
    _gc(16, 4, False), _gc(256, 4, False, hop=256), _gc(512, 4, False, hop=384), _gc(1024, 4, False), _gc(4096, 4, False),
    _gc(8192, 4, False), _gc(8192, 32, False, n=3 * 8192 + 1),
    _gc(8, 4, True), _gc(512, 4, True), _gc(4096, 4, True), _gc(8192, 4, True),
]
GATES = {"static": (1, proc_static_gate), "keep": (0, proc_gate_keep)}   # window, spec processor
MARGIN_MIN = 1e-6   # the fixtures' convention (tests/test_stft_cpu.py)


@functools.lru_cache(maxsize=None)
def gate_input(case):
    x = gate_signal(case.n, case.N, case.seed, case.cplx, case.hop, case.shift)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def gate_run(case, gate):
    wkind, proc = GATES[gate]
    return run(gate_input(case), case.N, case.laps, wkind, proc)


HILBERT_LGS = list(range(2, 14))


def hilbert_case(lg):
    """(N, laps, n): laps 4 (2 at N = 4, where laps 4 would start two frames on one sample)."""
    N = 1 << lg
    return N, (4 if N >= 8 else 2), 4 * N + 3


@functools.lru_cache(maxsize=None)
def hilbert_input(lg):
    N, _, n = hilbert_case(lg)
    x = hilbert_signal(n, N, 40 + lg)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def hilbert_run(lg):
    N, laps, _ = hilbert_case(lg)
    return run(hilbert_input(lg), N, laps, 0, proc_hilbert)


def bin_gains(N, seed=77):
    """A fixed complex gain per bin, not conjugate-symmetric: out[k] = g[k] inp[k] moves if bins
    are permuted or mirrored on the way in or out."""
    rng = np.random.default_rng(seed + N)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)
