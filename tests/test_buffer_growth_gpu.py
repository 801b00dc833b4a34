"""Scratch buffers that grow on demand (hz::DevBuf / hz::PinBuf, huygens_amd/csrc/hz_buf.h): one
handle per object type takes host-buffer calls whose lengths go small -> large -> small, so every
staging and scratch buffer starts below its later need, grows once, and is reused (not re-grown)
on the way down.  The concatenated output is compared with the CPU restatement driven through
the same calls, at the tolerance of that object's own GPU test."""
import numpy as np
import pytest

from oracle import OracleFilterbank, OracleOscbank, rel_err

pytestmark = pytest.mark.gpu

LENGTHS = (64, 20000, 64)


def cat(parts):
    return np.concatenate(parts)


@pytest.mark.parametrize("order", [2, 4])
def test_filterbank(gpu_lib, order):
    """Unconverged at first (general engine), then converged (LTI engine): d_partial grows in the
    one and again in the other; d_in / d_out / d_seg grow with the long calls."""
    from huygens_amd import Filterbank
    from huygens_amd._lib import HZ_FB_PATH_GENERAL, HZ_FB_PATH_LTI, HZ_FB_RESP_OFF
    from test_filterbank_lti_gpu import TOL, random_bank
    N = 128
    fwd, back = random_bank(order, N, seed=order)
    g, o = Filterbank(order, N, 0.01, 0.01), OracleFilterbank(order, N, 0.01, 0.01)   # ~550 samples to converge
    g.set_response(HZ_FB_RESP_OFF)   # long converged calls take the per-band LTI engine
    for fb in (g, o):
        for n in range(N):
            fb.coefficients(n, fwd[n], back[n])
        fb.boost(np.ones(N))
        fb.open()
    rng = np.random.default_rng(order)
    yg, yo, paths = [], [], []
    for n in LENGTHS + (20000, 64):
        x = rng.uniform(-1, 1, n).astype(np.float32).astype(np.float64)
        yg.append(g.process(x))
        yo.append(o.process(x))
        paths.append(g.last_path())
    assert paths[0] == HZ_FB_PATH_GENERAL and paths[1] == HZ_FB_PATH_GENERAL, paths
    assert paths[3] == HZ_FB_PATH_LTI, paths
    assert rel_err(cat(yg), cat(yo)) < TOL


def test_oscbank(gpu_lib):
    from huygens_amd import Oscbank
    from test_oscbank_gpu import TOL, rel
    N = 128
    rng = np.random.default_rng(1)
    g, o = Oscbank(N), OracleOscbank(N)
    f = rng.uniform(20, 20000, N)
    for b in (g, o):
        for i in range(N):
            b.freqmod(i, f[i])
        b.activate(list(range(0, N, 2)))
    mg, pg, mo, po = [], [], [], []
    for n in LENGTHS:
        for b, m, p in ((g, mg, pg), (o, mo, po)):
            mix, pb = b.fill(n, per_band=True)
            m.append(mix)
            p.append(pb)
    assert rel(cat(mg), cat(mo)) < TOL
    assert np.max(np.abs(cat(pg) - cat(po))) < 1e-9


def test_additive(gpu_lib):
    from huygens_amd import Additive
    from oracle_osc import OracleAdditive
    from test_additive_gpu import TOL
    V, O = 8, 32
    g, o = Additive(V, O, 0.75, 1.0), OracleAdditive(V, O, 0.75, 1.0)
    for b in (g, o):
        for v in range(V):
            b.makenote(40 + 3 * v, 1.0)
    assert rel_err(cat([g.fill(n) for n in LENGTHS]), cat([o.fill(n) for n in LENGTHS])) < TOL


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bowl(gpu_lib, dtype):
    from huygens_amd import Bowl
    from oracle_bowl import OracleBowl
    from test_bowl_gpu import NORTH_STAR
    M = 128
    rng = np.random.default_rng(M)
    f = np.exp(rng.uniform(np.log(20.0), np.log(16000.0), M))
    a = rng.uniform(1e-4, 5e-2, M)
    d = rng.uniform(0.05, 15.0, M)
    g, o = Bowl(M, f, a, d, dtype), OracleBowl(M, f, a, d, dtype)
    if dtype == np.float64:
        # double samples (render): fill() rounds to float, and one rounding that falls the other
        # way is already 6e-8 of the sample, above the double engine's bound
        # (test_bowl_gpu.test_golden / test_bowl_render_double_precision: 1e-9)
        assert rel_err(cat([g.render(n) for n in LENGTHS]), cat([o.render(n) for n in LENGTHS])) < 1e-9
    else:
        assert rel_err(cat([g.fill(n) for n in LENGTHS]), cat([o.fill(n) for n in LENGTHS])) < NORTH_STAR


def test_delaybank(gpu_lib):
    """Mixed calls: the per-line scratch (d_y) grows next to the staging buffers.  Bit-exact."""
    from huygens_amd import Delaybank
    from oracle_delay import OracleDelaybank
    rng = np.random.default_rng(11)
    N, S, time = 64, 3, 3000
    g, o = Delaybank(N, S, time, np.float64), OracleDelaybank(N, S, time, np.float64)
    for k in range(N):
        fwd = [(int(rng.integers(0, 1800)), float(rng.uniform(-1, 1))) for _ in range(S)]
        back = [(int(rng.integers(1100, 1900)), float(rng.uniform(-0.3, 0.3))) for _ in range(S - 1)]
        g.coefficients(k, fwd, back)
        o.coefficients(k, fwd, back)
    yg, yo = [], []
    for n in LENGTHS:
        x = rng.standard_normal(n)
        yg.append(g.process(x, mix=True))
        yo.append(o.process(x, mix=True))
    assert np.array_equal(cat(yg), cat(yo))
    x = rng.standard_normal((N, 100))   # per-line input and output: larger staging for a short call
    assert np.array_equal(g.process(x), o.process(x))
    assert g.origin() == o.origin()


def test_granulator(gpu_lib):
    """The grain tables (pinned staging and device copy) grow with the requests of the long call."""
    from huygens_amd import Granulator
    from oracle_gran import OracleGranulator
    from test_granulator_gpu import close, random_requests
    size, P = 4000, 16
    rng = np.random.default_rng(0)
    g, o = Granulator(size, P), OracleGranulator(size, P)
    yg, yo = [], []
    for n, count in zip(LENGTHS, (2, 300, 2)):
        x = rng.standard_normal(n)
        reqs = random_requests(rng, n, count, size)
        gy, gv = g.process(x, reqs)
        oy, ov = o.process(x, reqs)
        assert list(gv) == list(ov)
        assert g.activity() == o.activity()
        yg.append(gy)
        yo.append(oy)
    assert close(cat(yg), cat(yo))


def test_freezer(gpu_lib):
    """Freezes in the long call: the chunk tables, the new-period frames and the snapshot buffer
    (which keeps snapshot 0 when it grows) all exceed what the first short call allocated."""
    from huygens_amd import Freezer
    from oracle_frz import OracleFreezer, libc_srand
    from test_freezer_gpu import peak_close
    N, laps = 64, 4
    rng = np.random.default_rng(N + laps)
    t = np.arange(sum(LENGTHS))
    x = 0.3 * np.sin(2 * np.pi * 440 * t / 48000) + 0.05 * rng.standard_normal(t.size)
    events = ([], [(3000, 1), (7000, 0), (7001, 1), (12000, 0), (15000, 1)], [(10, 0)])
    outs = []
    for make in (Freezer, OracleFreezer):
        b, pos, ys = make(N, laps, 1.0), 0, []
        libc_srand(N)
        for n, ev in zip(LENGTHS, events):
            ys.append(b.process(x[pos:pos + n], ev))
            pos += n
        outs.append(cat(ys))
    assert np.max(np.abs(outs[1])) > 0
    assert peak_close(outs[0], outs[1])
    assert np.array_equal(outs[0][:3064], outs[1][:3064])   # the dry path before any freeze: exact


def test_heterodyne(gpu_lib):
    from test_heterodyne_gpu import assert_close, assert_states_equal, bursty, make_pair
    g, o = make_pair(96, order=4, width=240, seed=96)
    x = bursty(sum(LENGTHS), 96)
    yg, yo, pos = [], [], 0
    for n in LENGTHS:
        yg.append(g.process(x[pos:pos + n]))
        yo.append(o.process(x[pos:pos + n]))
        pos += n
    assert_close(cat(yg), cat(yo))
    assert_states_equal(g, o)


@pytest.mark.parametrize("host_proc", [False, True])
def test_stft(gpu_lib, host_proc):
    """Device processor: the [Re | Im] staging grows.  Host processor: the frame spectra buffer
    grows with the frames of the long call as well."""
    from huygens_amd import Fourier
    from oracle_stft import OracleSTFT
    from test_stft_gpu import TOL, peak_err
    N, laps = 64, 4

    def identity(inp, out):
        out[:] = inp
        return 0

    g = Fourier(identity if host_proc else 0, N, laps, 0)
    o = OracleSTFT(N, laps, 0, 0, callback=None)
    rng = np.random.default_rng(N + laps)
    gr, gi, orr, oi = [], [], [], []
    for n in LENGTHS:
        re, im = rng.standard_normal(n), rng.standard_normal(n)
        a, b = g.process_block(re, im)
        c, d = o.process_block(re, im)
        gr.append(a), gi.append(b), orr.append(c), oi.append(d)
    assert peak_err(cat(gr), cat(orr)) < TOL and peak_err(cat(gi), cat(oi)) < TOL
    assert g.frames()[0] == o.frames()
