"""The stationary engine's stores and the modal phase 2's LDS layout (hz_fb_resp.hip, hz_fb_modal.h).

The window spectra, the output spectra and the call's output are written with 16-byte buffer
stores from a per-workgroup base (write-through where it measured faster), the
modal phase 2 reads padded LDS tables.  Neither changes a value, so the checks are the project's
own: the mix against the CPU restatement (1e-9 of the mix), the band states against a twin handle
on the per-band LTI engine (1e-9), which engine ran -- and that nothing outside the call's n
outputs is written, for every alignment of the device pointers.
"""
import numpy as np
import pytest

from golden.spec_numpy import resonant_coefficients
from oracle import OracleFilterbank, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9
SENTINEL = 7.0
PAD = 4096   # sentinel elements on each side of a call's output


def lib():
    from huygens_amd import _lib
    return _lib


def gpu_handle(N, fwd, back, response):
    from huygens_amd import Filterbank
    fb = Filterbank(2, N, 0.001, 0.001)
    fb.set_response(response)
    if response != lib().HZ_FB_RESP_OFF:
        fb.tune_response(0, 1)
    return configure(fb, N, fwd, back)


def configure(fb, N, fwd, back):
    for n in range(N):
        fb.coefficients(n, fwd[n], back[n])
    fb.boost(np.ones(N))
    fb.open()
    return fb


def make(N, fwd, back):
    """(GPU handle, stationary whenever legal; CPU restatement; GPU twin on the per-band engines)"""
    L = lib()
    g = gpu_handle(N, fwd, back, L.HZ_FB_RESP_EAGER)
    t = gpu_handle(N, fwd, back, L.HZ_FB_RESP_OFF)
    o = configure(OracleFilterbank(2, N, 0.001, 0.001), N, fwd, back)
    return g, o, t


def states_close(a, b, tol=1e-9):
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


def check_states_against_restatement(sg, so, N):
    """the bounds of tests/test_fb_modal_gpu.py::test_modal_states_against_restatement: the regular
    bands at 1e-10 of the largest regular state, the Nyquist double pole (the last band; the
    restatement's own recurrence carries ~1e-9 of its state there) at 1e-8 of its own"""
    d = np.abs(sg[2:2 + 2 * N] - so[2:2 + 2 * N])
    assert d[:-2].max() <= 1e-10 * np.abs(so[2:2 * N]).max(), d[:-2].max()
    assert d[-2:].max() <= 1e-8 * np.abs(so[2 * N:2 + 2 * N]).max(), d[-2:]


def report_twin(n, sg, st):
    d = np.abs(sg - st)
    i = int(np.argmax(d))
    print(f"n={n}: |g - twin| max {d[i]:.3e} at state {i}, bound {1e-9 * max(1.0, np.max(np.abs(st))):.3e}")


def prime(objs, rng, lengths):
    for n in lengths:
        x = rng.uniform(-1, 1, n)
        ys = [fb.process(x) for fb in objs]
        assert rel_err(ys[0], ys[1]) < TOL, n


PRIME = (4000, 60000)
CALLS = (70001, 52000)


@pytest.fixture(scope="module")
def bank512(gpu_lib):
    """512 bands on the R = 0.999 circle (grid angles, the last band the Nyquist double pole: the
    modal pass with an exceptional band).  The references of one sequence -- two priming calls, then
    the two calls under test -- computed once and left unchanged: the inputs, the restatement's mix
    and states and the LTI twin's states after every call.  Each case runs the same sequence on a
    handle of its own, so no case depends on which cases ran before it."""
    fwd, back = resonant_coefficients(512, 0.999, 1.0)
    L = lib()
    t = gpu_handle(512, fwd, back, L.HZ_FB_RESP_OFF)
    o = configure(OracleFilterbank(2, 512, 0.001, 0.001), 512, fwd, back)
    rng = np.random.default_rng(21)
    steps = []
    for n in PRIME + CALLS:
        x = rng.uniform(-1, 1, n)
        ref = o.process(x)
        t.process(x)
        steps.append((x, ref, o.get_state(), t.get_state()))
    return fwd, back, steps


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_pointer_alignment_and_bounds(bank512, in_off, out_off):
    """Two stationary calls through device pointers 0 or 8 bytes off a 16-byte boundary (ragged
    and whole lengths), on a handle primed to stationary with host calls: mix, states, and every
    sentinel element around the n outputs untouched."""
    import torch
    L = lib()
    fwd, back, steps = bank512
    g = gpu_handle(512, fwd, back, L.HZ_FB_RESP_EAGER)
    for x, ref, _, _ in steps[:len(PRIME)]:
        assert rel_err(g.process(x), ref) < TOL, len(x)
    for x, ref, so, st in steps[len(PRIME):]:
        n = len(x)
        xbuf = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device="cuda")
        ybuf = torch.full((n + 2 * PAD + 2,), SENTINEL, dtype=torch.float64, device="cuda")
        assert xbuf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0
        xd = xbuf[in_off:in_off + n]
        xd.copy_(torch.from_numpy(x))
        yd = ybuf[PAD + out_off:PAD + out_off + n]
        assert xd.data_ptr() % 16 == 8 * in_off and yd.data_ptr() % 16 == 8 * out_off
        torch.cuda.synchronize()
        g.process_device(xd.data_ptr(), yd.data_ptr(), n)
        g.synchronize()
        got = ybuf.cpu().numpy()
        assert g.last_path() == L.HZ_FB_PATH_RESPONSE, (n, g.last_path(), g.response_info())
        assert g.modal_info()[3], g.modal_info()
        lo, hi = PAD + out_off, PAD + out_off + n
        assert np.all(got[:lo] == SENTINEL), (n, np.flatnonzero(got[:lo] != SENTINEL)[:8])
        assert np.all(got[hi:] == SENTINEL), (n, hi + np.flatnonzero(got[hi:] != SENTINEL)[:8])
        e = rel_err(got[lo:hi], ref)
        assert e < TOL, (n, e)
        sg = g.get_state()
        check_states_against_restatement(sg, so, 512)
        report_twin(n, sg, st)
        assert states_close(sg, st), n


def test_every_modal_bin_group(gpu_lib):
    """4096 bands at R = 0.995 (horizon 8192): the band angles m = i + 1 take every k1 = m mod 64
    and every k2 = m / 64 < 64, odd and even -- every phase-2 workgroup and every twiddle stride of
    the padded tables; ragged and whole call lengths."""
    L = lib()
    N = 4096
    fwd, back = resonant_coefficients(N, 0.995, 1.0)
    g, o, t = make(N, fwd, back)
    rng = np.random.default_rng(22)
    prime((g, o, t), rng, [3000, 20000])
    for n in (20000, 16385):
        x = rng.uniform(-1, 1, n)
        yg, yo = g.process(x), o.process(x)
        t.process(x)
        assert g.last_path() == L.HZ_FB_PATH_RESPONSE, (n, g.last_path(), g.response_info())
        assert g.modal_info()[3], g.modal_info()
        e = rel_err(yg, yo)
        assert e < TOL, (n, e)
        sg = g.get_state()
        check_states_against_restatement(sg, o.get_state(), N)
        report_twin(n, sg, t.get_state())
        assert states_close(sg, t.get_state()), n
