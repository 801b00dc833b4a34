"""GPU: Fourier / StaticSTFT / Cosine with frames of 16,384 to 262,144 points (hz_fft_long.h: a
four-step transform through a device workspace) against tests/stft_spec.py (numpy) and scipy.fft.

Tolerances are the project's own: TOL = 1e-10 of the peak for the STFT, 1e-13 for Cosine (two
independent FP64 transforms differ by ~5e-16 of the peak at these sizes).  Every condition on a
gate input is proved in tests/test_long_stft_cpu.py; the margin is asserted again here, never used
to skip.
"""
import functools

import numpy as np
import pytest
import scipy.fft

import long_stft_cases as lc
import stft_spec as sp
from test_stft_spectrum_gpu import capture_into, check_spectra, gain_procs, in_calls, peak_err, per_sample

pytestmark = pytest.mark.gpu
TOL = 1e-10


def sizes(lg):
    """(laps, samples): lg 14, 15 run laps 1 and 4 over 3N + 5 samples, lg 16..18 laps 4 over
    2N + 40 (5 frames)."""
    N = 1 << lg
    return [(1, 3 * N + 5), (4, 3 * N + 5)] if lg <= 15 else [(4, 2 * N + 40)]


@functools.lru_cache(maxsize=None)
def noise_input(n, seed):
    x = sp.noise(n, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def identity_ref(n, seed, N, laps, window):
    return sp.run(noise_input(n, seed), N, laps, window, sp.proc_identity).y


# ---- a. the spectra a host processor receives, and the output ------------------------------------

@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("lg", lc.LONG_LGS)
def test_block_spectra_vs_numpy(gpu_lib, lg, window):
    from huygens_amd import Fourier
    N = 1 << lg
    for laps, n in sizes(lg):
        x = noise_input(n, 100 + lg)
        caps = []
        f = Fourier(capture_into(caps), N, laps, window, long_frames=True)
        y = in_calls(f, x, sp.ragged(n, N))
        worst = check_spectra(caps, x, N, laps, window)
        print(f"block spectrum N={N} laps={laps} window={window}: {worst:.2e} of the frame's peak")
        assert worst < TOL
        assert f.frames()[0] == len(caps)
        assert peak_err(y, identity_ref(n, 100 + lg, N, laps, window)) < TOL


# ---- b. fused identity ------------------------------------------------------------------------------

@pytest.mark.parametrize("lg", lc.LONG_LGS)
def test_identity_fused(gpu_lib, lg):
    from huygens_amd import Fourier
    N = 1 << lg
    for laps, n in sizes(lg):
        x = noise_input(n, 100 + lg)
        f = Fourier(0, N, laps, lg & 1, long_frames=True)
        y = in_calls(f, x, sp.ragged(n, N))
        err = peak_err(y, identity_ref(n, 100 + lg, N, laps, lg & 1))
        print(f"fused identity N={N} laps={laps}: {err:.2e}")
        assert err < TOL
        assert f.frames()[0] == len(sp.frame_starts(n, N, laps))


def test_identity_one_long_call(gpu_lib):
    """One call longer than the internal block (2^20 samples): several blocks, the history and
    the ring carried between them."""
    from huygens_amd import Fourier
    N, laps = 16384, 4
    n = (1 << 20) + 3 * N + 7
    x = noise_input(n, 160)
    f = Fourier(0, N, laps, 0, long_frames=True)
    yr, yi = f.process_block(x.real.copy(), x.imag.copy())
    err = peak_err(yr + 1j * yi, identity_ref(n, 160, N, laps, 0))
    print(f"one call of {n} samples: {err:.2e}")
    assert err < TOL
    assert f.frames()[0] == len(sp.frame_starts(n, N, laps))


# ---- c. bin order, sign and scale of the inverse ----------------------------------------------------

@pytest.mark.parametrize("lg", [14, 15, 18])
def test_block_bin_gains(gpu_lib, lg):
    from huygens_amd import Fourier
    N = 1 << lg
    host, spec = gain_procs(N)
    for laps, n in sizes(lg):
        x = noise_input(n, 100 + lg)
        y = in_calls(Fourier(host, N, laps, lg & 1, long_frames=True), x, sp.ragged(n, N))
        err = peak_err(y, sp.run(x, N, laps, lg & 1, spec).y)
        print(f"block gains N={N} laps={laps}: {err:.2e}")
        assert err < TOL


def test_unit_bin_inverse(gpu_lib):
    """A processor that writes one unit bin k0: every frame is e^{+2 pi i k0 t/N}, unnormalised."""
    from huygens_amd import Fourier
    lg = 15
    N, laps = 1 << lg, 2
    k0 = N // 8 + 3

    def host(inp, out):
        out[:] = 0
        out[k0] = 1
        return 0

    def spec(X, n):
        Y = np.zeros(n, dtype=np.complex128)
        Y[k0] = 1
        return Y, np.inf

    x = noise_input(2 * N + 40, 500 + lg)
    y = in_calls(Fourier(host, N, laps, 0, long_frames=True), x, sp.ragged(len(x), N))
    ref = sp.run(x, N, laps, 0, spec).y
    k = np.arange(N)
    first = sp.window(0, N) * np.exp(2j * np.pi * ((k0 * k) % N) / N) / (N * laps // 2)
    assert np.max(np.abs(ref[N - 1:N - 1 + N // laps] - first[:N // laps])) < 1e-13 * np.max(np.abs(first))
    assert peak_err(y, ref) < TOL


# ---- d. Hilbert -------------------------------------------------------------------------------------

@pytest.mark.parametrize("lg", [14, 15, 18])
def test_hilbert(gpu_lib, lg):
    from huygens_amd.stft import PROC_HILBERT, Fourier
    N, laps, n = sp.hilbert_case(lg)
    x = sp.hilbert_signal(n, N, 40 + lg)
    ref = sp.run(x, N, laps, 0, sp.proc_hilbert)
    f = Fourier(PROC_HILBERT, N, laps, long_frames=True)
    y = in_calls(f, x, sp.ragged(n, N))
    err = peak_err(y, ref.y)
    print(f"hilbert N={N} laps={laps}: {err:.2e}")
    assert err < TOL
    assert f.frames()[0] == len(ref.starts)


# ---- e. gates ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", lc.GATE_KINDS)
@pytest.mark.parametrize("case", lc.GATE_CASES, ids=lambda c: c.id)
def test_gates(gpu_lib, case, kind):
    from huygens_amd.stft import PROC_GATE_KEEP, Fourier, StaticSTFT
    N, laps = case.N, case.laps
    x = sp.gate_input(case)
    ref = lc.gate_run(case, kind)
    assert ref.margin >= sp.MARGIN_MIN
    if kind == "static":
        f = StaticSTFT(N, laps, long_frames=True)
    elif kind == "keep":
        f = Fourier(PROC_GATE_KEEP, N, laps, long_frames=True)
    else:
        f = Fourier(PROC_GATE_KEEP, N, laps, long_frames=True, params=(10.0, 0.0))
    y = in_calls(f, x, sp.gate_cuts(case.n, N, laps))
    assert f.frames()[0] == len(ref.starts)
    err = peak_err(y, ref.y)
    print(f"gate {kind} {case.id}: {err:.2e}")
    assert err < TOL


# ---- f. per sample ----------------------------------------------------------------------------------

@pytest.mark.parametrize("proc", ["identity", "gains"])
def test_per_sample(gpu_lib, proc):
    from huygens_amd import Fourier
    N, laps = 16384, 2
    x = noise_input(2 * N + 40, 214)
    if proc == "identity":
        f, spec = Fourier(0, N, laps, 0, long_frames=True), sp.proc_identity
    else:
        host, spec = gain_procs(N)
        f = Fourier(host, N, laps, 0, long_frames=True)
    err = peak_err(per_sample(f, x), sp.run(x, N, laps, 0, spec).y)
    print(f"per sample {proc}: {err:.2e}")
    assert err < TOL


# ---- g. Cosine --------------------------------------------------------------------------------------

@pytest.mark.parametrize("lg", lc.LONG_LGS)
def test_cosine(gpu_lib, lg):
    from huygens_amd import Cosine
    N = 1 << lg
    c = Cosine(N)
    x = np.random.default_rng(600 + lg).standard_normal(N)
    c.inp[:] = x
    c.forward()
    assert peak_err(c.out, scipy.fft.dct(x, type=2)) < 1e-13
    z = np.random.default_rng(700 + lg).standard_normal(N)   # backward on its own input, not a round trip
    c.out[:] = z
    c.backward()
    assert peak_err(c.inp, scipy.fft.dct(z, type=3)) < 1e-13


@pytest.mark.parametrize("N,batch", [(16384, 3), (32768, 1)])
def test_cosine_device_batches(gpu_lib, N, batch):
    import torch
    from huygens_amd import Cosine
    c = Cosine(N)
    x = np.random.default_rng(N + batch).standard_normal((batch, N))
    xs = torch.from_numpy(x).cuda()
    ys, zs = torch.full_like(xs, np.nan), torch.full_like(xs, np.nan)
    torch.cuda.synchronize()   # the handle runs on its own non-blocking stream
    c.forward_device(xs.data_ptr(), ys.data_ptr(), batch)
    assert peak_err(ys.cpu().numpy(), scipy.fft.dct(x, type=2, axis=1)) < 1e-13
    c.backward_device(xs.data_ptr(), zs.data_ptr(), batch)
    assert peak_err(zs.cpu().numpy(), scipy.fft.dct(x, type=3, axis=1)) < 1e-13


# ---- h. determinism ---------------------------------------------------------------------------------

def test_keep_gate_deterministic(gpu_lib):
    """The frame-wide sums are combined in one fixed order, without atomics: two fresh handles on
    the same input give the same bits."""
    from huygens_amd.stft import PROC_GATE_KEEP, Fourier
    case = lc.GATE_CASES[0]
    x = sp.gate_input(case)
    outs = [Fourier(PROC_GATE_KEEP, case.N, case.laps, long_frames=True).process_block(x)[0] for _ in range(2)]
    assert np.max(np.abs(outs[0])) > 0
    assert np.array_equal(outs[0], outs[1])


# ---- i. the same engine below the limit -------------------------------------------------------------

def test_long_flag_below_limit_same_bits(gpu_lib):
    from huygens_amd import StaticSTFT
    case = sp._gc(4096, 4, False)
    x = sp.gate_input(case)
    a = StaticSTFT(4096, 4).process_block(x)
    b = StaticSTFT(4096, 4, long_frames=True).process_block(x)
    assert np.max(np.abs(a[0])) > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- j. errors --------------------------------------------------------------------------------------

def test_errors(gpu_lib):
    from huygens_amd import Fourier, HZError
    from huygens_amd._lib import HZ_E_UNSUPPORTED
    with pytest.raises(HZError):
        Fourier(0, 524288, 4, long_frames=True)
    f = Fourier(0, 16384, 4, long_frames=True)
    with pytest.raises(HZError) as ei:
        f.set_frame_shard(0, 2, 5)
    assert ei.value.code == HZ_E_UNSUPPORTED
    f.set_frame_shard(0, 1, 5)   # one rank: every frame, allowed
