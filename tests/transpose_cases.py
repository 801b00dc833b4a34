"""numpy model of the spectral transposer (HZ_PROC_TRANSPOSE; the reference's tests/demo.cpp:49-81)
shared by tests/test_stft_transpose_cpu.py, tests/test_stft_transpose_gpu.py and
tests/test_cpp_transpose_gpu.py.  TEST INFRASTRUCTURE: numpy only, built on tests/stft_spec.py;
nothing here is shared with the engine.

The model is the literal scatter loop, not the engine's gather:

    out[*] = 0
    for i in 0 .. N/2-1:  ix = int(i * r);  if ix < N: out[ix] += in[i]
    for i in N/2 .. N-1:  out[i] = out[N - i]

np.add.at adds unbuffered, in index order, so `scatter` is that loop; tests/test_stft_transpose_cpu.py
shows it bit for bit against `scatter_loop` (plain Python) at N = 64.
"""
from __future__ import annotations

import numpy as np

RATIOS = [0.0, 2.0 ** -10, 0.1, 1 / 3, 0.5, 2 / 3, 0.7, float(np.nextafter(1.0, 0.0)), 1.0,
          float(np.nextafter(1.0, 2.0)), 1.5, 2.0, 2.5, 3.0, 1000.3, 8192.0]
SIZES = [4, 8, 64, 4096, 8192, 16384, 32768, 262144]


def targets(N, r):
    """ix[i] = int(i * r) for i < N/2: one FP64 product, truncated (the products are >= 0)."""
    return (np.arange(N // 2, dtype=np.float64) * np.float64(r)).astype(np.int64)


def scatter(X, N, r):
    X = np.asarray(X, dtype=np.complex128)
    ix = targets(N, r)
    ok = ix < N
    out = np.zeros(N, dtype=np.complex128)
    np.add.at(out, ix[ok], X[:N // 2][ok])
    out[N // 2:] = out[N - np.arange(N // 2, N)]
    return out


def scatter_loop(X, N, r):
    """The same, as the plain loop (slow; small N only)."""
    out = [0j] * N
    for i in range(N // 2):
        ix = int(float(i) * float(r))
        if ix < N:
            out[ix] = complex(out[ix].real + X[i].real, out[ix].imag + X[i].imag)
    for i in range(N // 2, N):
        out[i] = out[N - i]
    return np.array(out, dtype=np.complex128)


def proc_transpose(r):
    """proc(X, N) -> (Y, inf) for stft_spec.run."""
    def proc(X, N):
        return scatter(X, N, r), np.inf
    return proc


def host_transpose(r):
    """The literal loop as a Fourier(callable, ...) host processor f(inp, out)."""
    def host(inp, out):
        out[:] = scatter(inp, len(inp), r)
        return 0
    return host


def source_runs(N, r):
    """(first, count) of every output bin k < N, read off the scatter's own target array: bin
    t <= N/2 receives the i with ix[i] == t (ix is non-decreasing, so they are consecutive; `first`
    of an empty run is where it would be inserted), bin k > N/2 mirrors bin N - k."""
    ix = targets(N, r)
    assert np.all(np.diff(ix) >= 0)
    k = np.arange(N)
    t = np.where(k <= N // 2, k, N - k)
    first = np.searchsorted(ix, t, side="left")
    count = np.searchsorted(ix, t, side="right") - first
    return first.astype(np.int32), count.astype(np.int32)
