"""CPU: the spectral transposer's source runs, its argument validation and its ABI, without a GPU.

The kernels gather: output bin k adds the contiguous run of source bins that the reference's
scatter loop (tests/demo.cpp:49-81) would add into it, in ascending order.  The run comes from one
__host__ __device__ function (huygens_amd/csrc/hz_transpose.h), which hz_stft_transpose_sources
exposes; here it is compared, for every bin, with the runs read off the literal scatter's own
target array (tests/transpose_cases.py) -- exactly, for every size and ratio of the table.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import transpose_cases as tc
from test_abi_cpu import ROOT

HZ_E_INVALID = -1
PROC_TRANSPOSE = 5


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "huygens_amd", "lib", "libhuygens_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-j8", "-C", ROOT, "lib"], check=True)
    from huygens_amd import load
    return load()


def test_add_at_is_the_loop():
    """np.add.at is the reference's loop, bit for bit (N = 64; signed zeros and collisions included)."""
    N = 64
    rng = np.random.default_rng(5)
    X = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    X[0] = complex(-0.0, -0.0)
    X[3] = complex(-0.0, 1.0)
    for r in tc.RATIOS:
        a, b = tc.scatter(X, N, r), tc.scatter_loop(X, N, r)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), r
    # a -0.0 alone in its bin comes out as +0.0: the sum starts from the memset's +0.0
    assert not np.signbit(tc.scatter(X, N, 1.0)[0].real)


@pytest.mark.parametrize("N", tc.SIZES)
def test_source_runs_match_the_scatter(lib, N):
    from huygens_amd.stft import transpose_sources
    for r in tc.RATIOS:
        first, count = transpose_sources(N, r)
        want_first, want_count = tc.source_runs(N, r)
        assert np.array_equal(count, want_count), (N, r)
        assert np.array_equal(first, want_first), (N, r)
        # the single-bin call is the same function
        for k in (0, 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1):
            assert transpose_sources(N, r, k) == (int(want_first[k]), int(want_count[k])), (N, r, k)


def test_gather_of_runs_is_the_scatter(lib):
    """Summing each bin's run in ascending order from +0.0 reproduces the scatter bit for bit."""
    from huygens_amd.stft import transpose_sources
    N = 64
    rng = np.random.default_rng(6)
    X = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    X[1] = complex(-0.0, -0.0)
    for r in tc.RATIOS:
        first, count = transpose_sources(N, r)
        out = np.zeros(N, dtype=np.complex128)
        for k in range(N):
            sr = si = 0.0
            for i in range(first[k], first[k] + count[k]):
                sr, si = sr + X[i].real, si + X[i].imag
            out[k] = complex(sr, si)
        assert np.array_equal(out.view(np.uint64), tc.scatter(X, N, r).view(np.uint64)), r


def test_sources_arguments(lib):
    a, b = C.c_int(), C.c_int()
    for N, r, k in [(64, 2.0, 64), (64, 2.0, -1), (48, 2.0, 0), (524288, 2.0, 0), (64, -1.0, 0),
                    (64, float("nan"), 0), (64, float("inf"), 0), (64, 8192.5, 0)]:
        assert lib.hz_stft_transpose_sources(N, r, k, C.byref(a), C.byref(b)) == HZ_E_INVALID, (N, r, k)
    assert lib.hz_stft_transpose_sources(64, 2.0, 0, None, C.byref(b)) == HZ_E_INVALID


@pytest.mark.parametrize("create", ["hz_stft_create", "hz_stft_create_long"])
def test_ratio_validated_before_the_device(lib, create):
    """A bad ratio is HZ_E_INVALID whether or not a GPU is present: it is checked first."""
    fn = getattr(lib, create)
    h = C.c_void_p()
    for r in (-1.0, float("nan"), float("inf"), 8192.5):
        assert fn(4096, 4, 0, PROC_TRANSPOSE, r, 0.0, 0, C.byref(h)) == HZ_E_INVALID, r
        assert not h.value
        assert b"ratio" in lib.hz_last_error()
    # a good ratio passes the argument checks (and then needs a device)
    rc = fn(4096, 4, 0, PROC_TRANSPOSE, 2.0, 0.0, 0, C.byref(h))
    assert rc != HZ_E_INVALID
    if rc == 0:
        lib.hz_stft_destroy(h)


@pytest.mark.parametrize("create", ["hz_stft_create", "hz_stft_create_long"])
def test_processor_id_6_rejected(lib, create):
    h = C.c_void_p()
    assert getattr(lib, create)(4096, 4, 0, 6, 2.0, 0.0, 0, C.byref(h)) == HZ_E_INVALID


def test_set_params_null_handle(lib):
    assert lib.hz_stft_set_params(None, 2.0, 0.0) == HZ_E_INVALID


def test_header_symbols(lib):
    from huygens_amd import header_symbols
    from huygens_amd._lib import _SIGS
    from huygens_amd.stft import PROC_TRANSPOSE as P, _PARAMS
    syms = header_symbols()
    for s in ("hz_stft_set_params", "hz_stft_transpose_sources", "hz_stft_transpose_sources_range"):
        assert s in syms and s in _SIGS
    assert P == PROC_TRANSPOSE and _PARAMS[P] == (2.0, 0.0)
    hdr = open(__import__("huygens_amd._lib", fromlist=["HEADER_PATH"]).HEADER_PATH).read()
    assert "#define HZ_PROC_TRANSPOSE 5" in hdr and "#define HZ_PROC_HOST 4" in hdr
