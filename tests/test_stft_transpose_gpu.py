"""GPU: the spectral transposer as a device processor (PROC_TRANSPOSE; the reference's
tests/demo.cpp:49-81) in the LDS-resident engine (N <= 8192), the four-step engine (N = 16384 ..
262144) and the per-sample path, with the staged parameter setter (Fourier.set_params).

The reference is tests/stft_spec.py::run with tests/transpose_cases.py::proc_transpose, the literal
scatter loop in numpy.  The bound is the project's own STFT bound, TOL = 1e-10 of the reference's
peak (tests/test_long_stft_gpu.py).  Bin 0 always maps to bin 0, so the reference is never
identically zero for noise input.  The bound cannot see the order of a bin's sum; that the order
is ascending is the business of tests/test_stft_transpose_cpu.py (the shared source-run function)
and of the determinism test here.

Host-callable cross-check, largest |device - host| of the output as measured on an MI355X:
(64, 4) 2.3e-16, (4096, 4) 4.7e-16, (16384, 4) exactly 0 (DESIGN.md section 4.11 says why the
LDS-resident sizes differ by a rounding: the transform code of the two paths, not the sum).
"""
import functools

import numpy as np
import pytest

import long_stft_cases as lc
import stft_spec as sp
import transpose_cases as tc
from test_long_stft_gpu import sizes
from test_stft_spectrum_gpu import in_calls, peak_err, per_sample

pytestmark = pytest.mark.gpu
TOL = 1e-10
THIRD = 1 / 3


@functools.lru_cache(maxsize=None)
def noise_input(n, seed, real=False):
    x = sp.noise(n, seed)
    if real:
        x = x.real.copy()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def transpose_ref(n, seed, real, N, laps, r):
    return sp.run(noise_input(n, seed, real), N, laps, 0, tc.proc_transpose(r))


def transposer(N, laps, r):
    from huygens_amd.stft import PROC_TRANSPOSE, Fourier
    return Fourier(PROC_TRANSPOSE, N, laps, long_frames=N > 8192, params=(r, 0.0))


def check_blocks(N, laps, n, seed, r, real=False):
    x = noise_input(n, seed, real)
    ref = transpose_ref(n, seed, real, N, laps, r)
    f = transposer(N, laps, r)
    y = in_calls(f, x, sp.ragged(n, N))
    err = peak_err(y, ref.y)
    print(f"transpose N={N} laps={laps} r={r:.6g}: {err:.2e} of the peak")
    assert np.max(np.abs(ref.y)) > 0
    assert err < TOL
    assert f.frames()[0] == len(ref.starts)


# ---- a. LDS-resident engine ---------------------------------------------------------------------------

ALL_R = [2.0, 0.5, THIRD, 1.5, 3.0, 0.0, 1.0]
LDS_CASES = [(lg, r) for lg in (2, 3, 6, 9, 12, 13) for r in (ALL_R if lg in (6, 12) else [2.0, THIRD])]


@pytest.mark.parametrize("lg,r", LDS_CASES, ids=lambda v: f"{v:.4g}")
def test_lds_engine(gpu_lib, lg, r):
    """N = 4 (frame_middle's default branch), 8 and 64 (one wave, idle threads), 512 and 4096
    (radix 8), 8192 (radix 16); complex noise of 4N + 3 samples through ragged call boundaries."""
    N, laps, n = sp.hilbert_case(lg)
    check_blocks(N, laps, n, 900 + lg, r)


def test_default_ratio_is_the_programs(gpu_lib):
    """Fourier(PROC_TRANSPOSE, ...) without params runs the program's transp = 2."""
    from huygens_amd.stft import PROC_TRANSPOSE, Fourier
    N, laps, n = sp.hilbert_case(6)
    x = noise_input(n, 906)
    y = in_calls(Fourier(PROC_TRANSPOSE, N, laps), x, sp.ragged(n, N))
    assert peak_err(y, transpose_ref(n, 906, False, N, laps, 2.0).y) < TOL


# ---- b. four-step engine ------------------------------------------------------------------------------

LONG_CASES = [(lg, r) for lg in (14, 15, 18) for r in ([2.0, THIRD, 0.5, 3.0, 0.0] if lg == 14 else [2.0, THIRD])]


@pytest.mark.parametrize("lg,r", LONG_CASES, ids=lambda v: f"{v:.4g}")
def test_long_engine(gpu_lib, lg, r):
    """lg 14 (128 x 128), 15 (128 x 256, the non-square split) and 18 (512 x 512)."""
    N = 1 << lg
    for laps, n in sizes(lg):
        check_blocks(N, laps, n, 920 + lg, r)


def test_demo_shape_real_input(gpu_lib):
    """The program's own Fourier(32768, 2) on real input with transp = 2: the output is complex
    (the mirror is not a conjugate)."""
    N, laps = 32768, 2
    n = 3 * N + 5
    check_blocks(N, laps, n, 935, 2.0, real=True)
    assert np.max(np.abs(transpose_ref(n, 935, True, N, laps, 2.0).y.imag)) > 0


# ---- c. per sample --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 16384])
def test_per_sample(gpu_lib, N):
    laps, r = 2, 2.0
    n = 3 * N if N <= 1024 else 2 * N + 40
    x = noise_input(n, 940)
    err = peak_err(per_sample(transposer(N, laps, r), x), transpose_ref(n, 940, False, N, laps, r).y)
    print(f"transpose per sample N={N}: {err:.2e}")
    assert err < TOL


# ---- d. against the host path with the literal loop ---------------------------------------------------

@pytest.mark.parametrize("N", [64, 4096, 16384])
def test_host_callable_cross_check(gpu_lib, N):
    from huygens_amd import Fourier
    laps, r = 4, THIRD
    n = 4 * N + 3 if N <= 8192 else 3 * N + 5
    x = noise_input(n, 950)
    cuts = sp.ragged(n, N)
    dev = in_calls(transposer(N, laps, r), x, cuts)
    host = in_calls(Fourier(tc.host_transpose(r), N, laps, long_frames=N > 8192), x, cuts)
    diff = float(np.max(np.abs(dev - host)))
    print(f"transpose device against host callable, N={N}: largest difference {diff:.3e} "
          f"({diff / np.max(np.abs(host)):.2e} of the peak)")
    assert np.max(np.abs(host)) > 0
    assert peak_err(dev, host) < TOL


# ---- e. determinism -----------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [THIRD, 0.0])
@pytest.mark.parametrize("N", [4096, 16384])
def test_deterministic(gpu_lib, N, r):
    """Every bin's sum runs in one thread, in ascending source order: two fresh handles on the same
    input give the same bits."""
    laps = 4
    x = noise_input(3 * N + 5, 960)
    outs = [transposer(N, laps, r).process_block(x.real.copy(), x.imag.copy()) for _ in range(2)]
    assert np.max(np.abs(outs[0][0])) > 0
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- f. set_params ------------------------------------------------------------------------------------

def switching(procs, starts, N, cut):
    """A spec processor that hands frame j to procs[0] while its last sample starts[j] + N - 1 comes
    before `cut`, to procs[1] from then on (stft_spec.run calls it in frame order)."""
    state = {"j": 0}

    def proc(X, n):
        j = state["j"]
        state["j"] += 1
        return procs[0 if starts[j] + N - 1 < cut else 1](X, n)
    return proc


@pytest.mark.parametrize("N", [64, 16384])
def test_set_params_ratio(gpu_lib, N):
    """r = 2, then set_params(0.5) between two calls; the cut is not a multiple of the stride, so
    frames straddle it: a frame belongs to the call in which its last sample arrives."""
    laps = 4
    n, cut = 4 * N + 3, 2 * N + 3
    assert cut % (N // laps)
    x = noise_input(n, 970)
    starts = sp.frame_starts(n, N, laps)
    before = int(np.sum(starts + N - 1 < cut))
    assert 0 < before < len(starts)
    ref = sp.run(x, N, laps, 0, switching([tc.proc_transpose(2.0), tc.proc_transpose(0.5)], starts, N, cut))
    f = transposer(N, laps, 2.0)
    a = f.process_block(x[:cut].real.copy(), x[:cut].imag.copy())
    f.set_params(0.5)
    b = f.process_block(x[cut:].real.copy(), x[cut:].imag.copy())
    y = np.concatenate([a[0], b[0]]) + 1j * np.concatenate([a[1], b[1]])
    err = peak_err(y, ref.y)
    print(f"set_params 2 -> 0.5 at N={N}: {err:.2e}")
    assert err < TOL
    # and the change is visible: the unswitched run differs
    assert peak_err(transpose_ref(n, 970, False, N, laps, 2.0).y, ref.y) > 1e-3


def test_set_params_per_sample(gpu_lib):
    """Per sample the new ratio holds from the next completed frame on."""
    N, laps = 64, 2
    n, cut = 3 * N, N + N // 2 + 3
    x = noise_input(n, 975)
    starts = sp.frame_starts(n, N, laps)
    ref = sp.run(x, N, laps, 0, switching([tc.proc_transpose(2.0), tc.proc_transpose(0.5)], starts, N, cut))
    f = transposer(N, laps, 2.0)
    y = np.empty(n, dtype=np.complex128)
    for t, v in enumerate(x):
        if t == cut:
            f.set_params(0.5)
        f.write(v.real, v.imag)
        y[t] = complex(*f.read())
    assert peak_err(y, ref.y) < TOL


def test_set_params_keep_gate(gpu_lib):
    """A PROC_GATE_KEEP handle from 625 to 10: from the cut on it is long_stft_cases.proc_keep10."""
    from golden.make_golden_stft import proc_gate_keep
    from huygens_amd.stft import PROC_GATE_KEEP, Fourier
    case = lc.GATE_CASES[0]
    N, laps = case.N, case.laps
    x = sp.gate_input(case)
    cut = 4 * N + 5
    starts = sp.frame_starts(case.n, N, laps)
    ref = sp.run(x, N, laps, 0, switching([proc_gate_keep, lc.proc_keep10], starts, N, cut))
    assert ref.margin >= sp.MARGIN_MIN
    f = Fourier(PROC_GATE_KEEP, N, laps, long_frames=True)
    a = f.process_block(x[:cut])
    f.set_params(10.0)
    b = f.process_block(x[cut:])
    y = np.concatenate([a[0], b[0]]) + 1j * np.concatenate([a[1], b[1]])
    err = peak_err(y, ref.y)
    print(f"set_params keep gate 625 -> 10: {err:.2e}")
    assert err < TOL
    assert peak_err(lc.gate_run(case, "keep").y, ref.y) > 1e-3   # the two gates differ on this input


def test_set_params_errors(gpu_lib):
    from huygens_amd import Fourier, HZError
    from huygens_amd._lib import HZ_E_INVALID
    from huygens_amd.stft import PROC_HILBERT
    for f in (Fourier(0, 64, 4), Fourier(PROC_HILBERT, 64, 4), Fourier(lambda i, o: 0, 64, 4)):
        with pytest.raises(HZError) as ei:
            f.set_params(2.0)
        assert ei.value.code == HZ_E_INVALID
    f = transposer(64, 4, 2.0)
    for bad in (-1.0, float("nan"), float("inf"), 8192.5):
        with pytest.raises(HZError) as ei:
            f.set_params(bad)
        assert ei.value.code == HZ_E_INVALID
    f.set_params(8192.0)


# ---- g. time-range shards -----------------------------------------------------------------------------

def test_shards_sum_to_the_whole(gpu_lib):
    N, laps, r = 4096, 4, THIRD
    n = 4 * N + 3
    x = noise_input(n, 980)
    cuts = sp.ragged(n, N)
    whole = in_calls(transposer(N, laps, r), x, cuts)
    parts = []
    for rank in range(2):
        f = transposer(N, laps, r)
        f.set_frame_shard(rank, 2, 3)
        parts.append(in_calls(f, x, cuts))
    assert np.max(np.abs(parts[0])) > 0 and np.max(np.abs(parts[1])) > 0
    assert peak_err(parts[0] + parts[1], whole) < TOL
    assert peak_err(whole, transpose_ref(n, 980, False, N, laps, r).y) < TOL


def test_long_handle_shards_unsupported(gpu_lib):
    from huygens_amd import HZError
    from huygens_amd._lib import HZ_E_UNSUPPORTED
    f = transposer(16384, 4, 2.0)
    with pytest.raises(HZError) as ei:
        f.set_frame_shard(0, 2, 3)
    assert ei.value.code == HZ_E_UNSUPPORTED


# ---- h. device pointers -------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [4096, 16384])
def test_device_pointers(gpu_lib, N):
    import torch
    laps, r = 4, 2.0
    n = 3 * N + 5
    x = noise_input(n, 990)
    f = transposer(N, laps, r)
    xr, xi = torch.from_numpy(x.real.copy()).cuda(), torch.from_numpy(x.imag.copy()).cuda()
    yr, yi = torch.full_like(xr, np.nan), torch.full_like(xr, np.nan)
    torch.cuda.synchronize()   # the handle runs on its own non-blocking stream
    f.process_block_device(xr.data_ptr(), xi.data_ptr(), yr.data_ptr(), yi.data_ptr(), n)
    f.synchronize()
    y = yr.cpu().numpy() + 1j * yi.cpu().numpy()
    assert peak_err(y, transpose_ref(n, 990, False, N, laps, r).y) < TOL
