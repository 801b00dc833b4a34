"""GPU: Fourier / StaticSTFT / Cosine against numpy.fft / scipy.fft at the level of the spectrum.

tests/test_stft_gpu.py and tests/test_stft_slots_gpu.py compare time-domain outputs with the C
oracle.  These tests compare with tests/stft_spec.py (numpy only) and look at what those cannot
see: the bins a host processor is handed (order, sign, scale), the inverse on its own, a
bin-index-dependent processor at every frame size, and gates whose decisions change from one
frame to the next.  Every condition on an input is proved in tests/test_stft_spectrum_cpu.py;
the few repeated here are asserted, never used to skip.

Tolerance: TOL = 1e-10 of the peak, as the other STFT tests (FP64 FFT against numpy's, ~1e-15).
Below N ~ 64 neither gate can open with these windows (the keep gate needs one bin above 25 x the
mean magnitude): the gated cases at N = 8 and 16 are plain parity cases.
"""
import numpy as np
import pytest
import scipy.fft

import stft_spec as sp

pytestmark = pytest.mark.gpu
TOL = 1e-10
LGS = list(range(2, 14))
SLOT_LGS = list(range(2, 11)) + [13]


def laps_pair(N):
    """laps 1 takes the per-sample overlap-add, laps 2 / 4 the segment overlap-add."""
    return (1, 4 if N >= 8 else 2)


def slot_len(N):
    return 3 * N if N <= 1024 else 2 * N + 40


def in_calls(f, x, cuts):
    parts = [f.process_block(x[a:b].real.copy(), x[a:b].imag.copy() if np.iscomplexobj(x) else None)
             for a, b in zip(cuts[:-1], cuts[1:])]
    return np.concatenate([p[0] for p in parts]) + 1j * np.concatenate([p[1] for p in parts])


def per_sample(f, x):
    y = np.empty(len(x), dtype=np.complex128)
    for t, v in enumerate(x):
        f.write(v.real, v.imag)
        r, i = f.read()
        y[t] = complex(r, i)
    return y


def peak_err(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def capture_into(caps):
    def proc(inp, out):
        caps.append(inp.copy())
        out[:] = inp
        return 0
    return proc


def check_spectra(caps, x, N, laps, window):
    """frame count, frame order and every bin of every frame; returns the largest error"""
    ref = sp.frame_spectra(x, N, laps, window)
    assert len(caps) == len(ref) >= 2
    worst = 0.0
    for got, want in zip(caps, ref):
        assert got.shape == (N,)
        worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    return worst


# ---- a. the spectrum a host processor receives, by blocks (stft_frame_kernel<IDENTITY, 1, RMAX>) ----

@pytest.mark.parametrize("window", [0, 1])
@pytest.mark.parametrize("lg", LGS)
def test_block_spectra_vs_numpy(gpu_lib, lg, window):
    from huygens_amd import Fourier
    N = 1 << lg
    for laps in laps_pair(N):
        x = sp.noise(3 * N + 5, 100 + lg)
        caps = []
        f = Fourier(capture_into(caps), N, laps, window)
        y = in_calls(f, x, sp.ragged(len(x), N))
        worst = check_spectra(caps, x, N, laps, window)
        print(f"block spectrum N={N} laps={laps} window={window}: {worst:.2e} of the frame's peak")
        assert worst < TOL
        assert f.frames()[0] == len(caps)
        assert peak_err(y, sp.run(x, N, laps, window, sp.proc_identity).y) < TOL


@pytest.mark.parametrize("lg", LGS)
def test_identity_fused_every_size(gpu_lib, lg):
    """the fused identity path (stft_frame_kernel<IDENTITY, 0, RMAX>) at every frame size"""
    from huygens_amd import Fourier
    N = 1 << lg
    for laps in laps_pair(N):
        x = sp.noise(3 * N + 5, 150 + lg)
        y = in_calls(Fourier(0, N, laps, lg & 1), x, sp.ragged(len(x), N))
        assert peak_err(y, sp.run(x, N, laps, lg & 1, sp.proc_identity).y) < TOL


# ---- b. the same through write() / read() (slot_fft_kernel<RMAX, false>) -----------------------------

@pytest.mark.parametrize("lg", SLOT_LGS)
def test_slot_spectra_vs_numpy(gpu_lib, lg):
    from huygens_amd import Fourier
    N, laps, window = 1 << lg, (4 if lg % 2 else 2), lg & 1
    x = sp.noise(slot_len(N), 200 + lg)
    caps = []
    f = Fourier(capture_into(caps), N, laps, window)
    y = per_sample(f, x)
    worst = check_spectra(caps, x, N, laps, window)
    print(f"slot spectrum N={N} laps={laps} window={window}: {worst:.2e} of the frame's peak")
    assert worst < TOL
    assert peak_err(y, sp.run(x, N, laps, window, sp.proc_identity).y) < TOL


# ---- c. inverse path and bin order together ----------------------------------------------------------

def gain_procs(N):
    g = sp.bin_gains(N)

    def host(inp, out):
        out[:] = g * inp
        return 0

    return host, (lambda X, n: (g * X, np.inf))


@pytest.mark.parametrize("lg", LGS)
def test_block_bin_gains(gpu_lib, lg):
    """out[k] = g[k] inp[k], g not conjugate-symmetric: forward order, inverse order (MODE 2's
    bit-reversed load), sign and scale all show in the output."""
    from huygens_amd import Fourier
    N = 1 << lg
    host, spec = gain_procs(N)
    for laps in laps_pair(N):
        x = sp.noise(3 * N + 5, 300 + lg)
        y = in_calls(Fourier(host, N, laps, lg & 1), x, sp.ragged(len(x), N))
        err = peak_err(y, sp.run(x, N, laps, lg & 1, spec).y)
        print(f"block gains N={N} laps={laps}: {err:.2e}")
        assert err < TOL


@pytest.mark.parametrize("lg", SLOT_LGS)
def test_slot_bin_gains(gpu_lib, lg):
    """the same per sample (slot_fft_kernel<RMAX, true> for the inverse)"""
    from huygens_amd import Fourier
    N, laps = 1 << lg, (2 if lg % 2 else 4 if lg > 2 else 1)
    host, spec = gain_procs(N)
    x = sp.noise(slot_len(N), 400 + lg)
    err = peak_err(per_sample(Fourier(host, N, laps, 0), x), sp.run(x, N, laps, 0, spec).y)
    print(f"slot gains N={N} laps={laps}: {err:.2e}")
    assert err < TOL


@pytest.mark.parametrize("mode", ["block", "slot"])
@pytest.mark.parametrize("lg", [6, 13])
def test_unit_bin_inverse(gpu_lib, lg, mode):
    """A processor that ignores its input and writes one unit bin k0 (not 0, not N/2): every frame
    is e^{+2 pi i k0 t/N}, unnormalised -- the inverse's sign and scale with no forward in play."""
    from huygens_amd import Fourier
    N, laps = 1 << lg, 2
    k0 = N // 8 + 3
    assert k0 not in (0, N // 2) and k0 != N - k0

    def host(inp, out):
        out[:] = 0
        out[k0] = 1
        return 0

    def spec(X, n):
        Y = np.zeros(n, dtype=np.complex128)
        Y[k0] = 1
        return Y, np.inf

    x = sp.noise(2 * N + 40, 500 + lg)
    f = Fourier(host, N, laps, 0)
    y = in_calls(f, x, sp.ragged(len(x), N)) if mode == "block" else per_sample(f, x)
    ref = sp.run(x, N, laps, 0, spec).y
    # the spec's frame, stated outright: w(k) e^{+2 pi i k0 k/N} / (N laps / 2) at t = N-1+k
    k = np.arange(N)
    first = sp.window(0, N) * np.exp(2j * np.pi * ((k0 * k) % N) / N) / (N * laps // 2)   # phase reduced exactly
    assert np.max(np.abs(ref[N - 1:N - 1 + N // laps] - first[:N // laps])) < 1e-13 * np.max(np.abs(first))
    assert peak_err(y, ref) < TOL


# ---- d. Hilbert at every size, fused path (frame_middle<2|3|4, HILBERT>) ------------------------------

@pytest.mark.parametrize("lg", sp.HILBERT_LGS)
def test_hilbert_every_size(gpu_lib, lg):
    from huygens_amd.stft import PROC_HILBERT, Fourier
    N, laps, n = sp.hilbert_case(lg)
    x = sp.hilbert_input(lg)
    ref = sp.hilbert_run(lg)
    f = Fourier(PROC_HILBERT, N, laps)
    y = in_calls(f, x, sp.ragged(n, N))
    err = peak_err(y, ref.y)
    print(f"hilbert N={N} laps={laps}: {err:.2e}")
    assert err < TOL
    assert f.frames()[0] == len(ref.starts)


# ---- e. gates on non-stationary input ----------------------------------------------------------------

@pytest.mark.parametrize("gate", list(sp.GATES))
@pytest.mark.parametrize("case", sp.GATE_CASES, ids=lambda c: c.id)
def test_gates_nonstationary(gpu_lib, case, gate):
    """Real input: two frames per transform, each gated on its own average (pair_gate, the 4096
    kernel's mirrored walk, radix 16 at 8192); complex input: stft_frame_kernel<gate, 0, RMAX>.
    The kept bins change from frame to frame, launches begin on even and on odd frames
    (test_stft_spectrum_cpu.py::test_gate_input_conditions)."""
    from huygens_amd.stft import PROC_GATE_KEEP, Fourier, StaticSTFT
    N, laps = case.N, case.laps
    x = sp.gate_input(case)
    ref = sp.gate_run(case, gate)
    assert ref.margin >= sp.MARGIN_MIN
    f = StaticSTFT(N, laps) if gate == "static" else Fourier(PROC_GATE_KEEP, N, laps)
    y = in_calls(f, x, sp.gate_cuts(case.n, N, laps))
    assert f.frames()[0] == len(ref.starts)
    scale = np.max(np.abs(ref.y))
    if scale == 0.0:   # N = 8, 16 with the keep gate: nothing passes, on either side
        assert np.max(np.abs(y)) == 0.0
        return
    err = peak_err(y, ref.y)
    print(f"gate {gate} {case.id}: {err:.2e}")
    assert err < TOL


# ---- f. Cosine ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("lg", range(2, 14))
def test_cosine_every_size(gpu_lib, lg):
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


@pytest.mark.parametrize("batch", [1, 3, 7])
@pytest.mark.parametrize("N", [8, 512, 4096])
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
