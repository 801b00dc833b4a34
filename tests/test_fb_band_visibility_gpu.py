"""Every band counts: the Filterbank engines on banks whose mix shows each band.

On the reference recipe the Nyquist band is 1 - 1e-8 of the mix, so the mix-relative tests of the
recipe bank (1e-7 of the block peak, states against 1e-7 max|state|) pass for an engine that
outputs that band alone (tests/test_visibility_cpu.py proves it with mutants of the restatement).
Here the same recipe runs with that band's gain held at exactly 0 (visibility.recipe_bank_muted:
the band still runs, through the modal exception path and the direct sum), or with a one-hot mix:

  outputs  1e-9 of the block peak per 1024-sample block (the project's TOL), every engine;
  states   every regular band within 1e-8 of ITS OWN output peak (scipy.signal.lfilter); the
           Nyquist band within 1e-7 of its own state, as the recipe-bank tests hold it.

That each band is at least 1000 x 1e-9 of these mixes is proved from the restatement alone in
tests/test_visibility_cpu.py (weakest band: 6.3e-2, 3.8e-2, 1.0e-2 and 9.6e-3 of the mix).
"""
import numpy as np
import pytest

import visibility as vz
from oracle import OracleFilterbank
from test_c2_pinned_gpu import TIGHT, ThreadedOracle, block_errors

pytestmark = pytest.mark.gpu

B = vz.B


def _paths():
    from huygens_amd import _lib
    return _lib


def _pair(N, R, k=vz.K_SMOOTH):
    from huygens_amd import Filterbank
    g, o = Filterbank(2, N, k, k), OracleFilterbank(2, N, k, k)
    fwd, back = vz.recipe_bank_muted(N, R, [g, o])
    g.tune_response(0, 1)   # small bank: stationary whenever legal (cost model off)
    return g, o, fwd, back


class _Run:
    """drives engine and restatement through the same calls; every 1024-sample block of every call
    within TOL_OUT of the block's peak"""

    def __init__(self, g, o, seed):
        self.g, self.o, self.rng = g, o, np.random.default_rng(seed)
        self.xs, self.worst, self.worst_state = [], 0.0, 0.0

    def __call__(self, n):
        x = vz.noise(self.rng, n)
        self.xs.append(x)
        yg, yo = self.g.process(x), self.o.process(x)
        err, peak = block_errors(yg, yo)
        assert peak.min() > 0
        self.worst = max(self.worst, float(err.max()))
        assert err.max() <= vz.TOL_OUT, (n, self.g.last_path(), err.max(), int(err.argmax()))
        return self.g.last_path()

    def window(self, n=vz.STATE_WINDOW):
        return np.concatenate(self.xs)[-n:]

    def states(self, scale, st_ref=None):
        N = len(scale)
        st_g = self.g.get_state()
        st_o = self.o.get_state() if st_ref is None else st_ref
        reg, nyq = vz.assert_band_states(st_g, st_o, N, scale, vz.TOL_STATE, TIGHT)
        self.worst_state = max(self.worst_state, reg)
        assert np.array_equal(st_g[:2], st_o[:2])                            # x history: exact
        assert np.max(np.abs(st_g[2 + 2 * N:] - st_o[2 + 2 * N:])) <= 1e-12   # smoothers
        assert st_g[2 + 2 * N + 2 * (N - 1) + 1] == 0.0                       # the muted gain: exactly 0
        return reg, nyq


@pytest.mark.parametrize("column_split", [False, True], ids=["three_kernel", "column_split"])
@pytest.mark.parametrize("N,R,seed", vz.MUTED_SMALL)
def test_muted_recipe_every_engine(gpu_lib, N, R, seed, column_split):
    """general -> LTI -> stationary -> 40 streamed blocks -> a long call -> a ragged call -> 64
    per-sample operator()/tick() -> a block call, each block at 1e-9 and the per-band states after
    each phase.  Measured on MI355X: worst block 7.4e-14 (N = 256) and 5.0e-12
    (N = 1024), worst regular-band state 3.4e-13 and 2.9e-11 of the band's peak, the same on both
    stationary engines (the column split runs at N = 1024, K = 49,152 = 24 partitions)."""
    L = _paths()
    g, o, fwd, back = _pair(N, R)
    g.tune_response_engine(column_split)
    run = _Run(g, o, seed)
    assert run(3000) == L.HZ_FB_PATH_GENERAL          # smoothers moving
    assert run(70_000) == L.HZ_FB_PATH_LTI            # converged; the history fills
    scale = vz.band_peaks(fwd, back, run.window())    # each band's own peak on this noise
    run.states(scale)
    assert run(60_000) == L.HZ_FB_PATH_RESPONSE
    assert g.response_engine()[0] == column_split
    K = g.response_info()[0]
    assert 0 < K <= vz.STATE_WINDOW, K
    run.states(scale)
    assert [run(B) for _ in range(40)] == [L.HZ_FB_PATH_STREAM] * 40
    assert g.stream_info()[3]                         # history in the ring
    run.states(scale)                                 # materialised on demand
    assert run(B) == L.HZ_FB_PATH_STREAM              # streaming resumes without a gap
    assert run(40_000) == L.HZ_FB_PATH_RESPONSE       # from the ring's history
    run.states(scale)
    assert [run(B) for _ in range(3)] == [L.HZ_FB_PATH_STREAM] * 3
    assert run(1000) != L.HZ_FB_PATH_STREAM           # a ragged call restarts the history
    run.states(scale)
    xs = vz.noise(run.rng, 64)                        # per-sample path after it
    yg = np.array([(g(v), g.tick())[0] for v in xs])
    yo = np.array([(o(v), o.tick())[0] for v in xs])
    assert np.max(np.abs(yg - yo)) <= vz.TOL_OUT * np.max(np.abs(yo))
    assert run(B) != L.HZ_FB_PATH_STREAM
    run.states(scale)
    print("muted recipe N %d R %g %s: worst block %.3e, worst regular-band state %.3e (K %d, column split ran %s)"
          % (N, R, "column split" if column_split else "three-kernel", run.worst, run.worst_state, K,
             g.response_engine()[1]))
    g.close()


def test_muted_recipe_c2_geometry(gpu_lib):
    """bench.py's geometry -- 4096 bands, R = 0.999, k_p 0.1, k_g 1 -- with the Nyquist band muted:
    calls of 100,000 samples until stationary, then 40 streamed blocks, against the restatement
    split over host threads.  Measured on MI355X: general, LTI, stationary after three calls; worst
    block 1.4e-11, worst regular-band state 4.1e-10 of the band's peak."""
    from huygens_amd import Filterbank
    L = _paths()
    N, R, seed, S = vz.MUTED_C2
    g = Filterbank(2, N, 0.1, 1.0)
    fwd, back = vz.recipe_bank_muted(N, R, [g])
    o = ThreadedOracle(fwd, back)
    b0, cnt, last = o.shards[-1]
    assert b0 + cnt == N
    last.mix(cnt - 1, 0.0)
    run = _Run(g, o, seed)
    paths = []
    for _ in range(5):
        paths.append(run(S))
        if paths[-1] == L.HZ_FB_PATH_RESPONSE:
            break
    assert paths[-1] == L.HZ_FB_PATH_RESPONSE and len(paths) >= 3, paths
    assert g.modal_info()[1:] == (True, 1, True)      # the Nyquist band: the direct sum
    scale = vz.band_peaks(fwd, back, run.window(16384))
    run.states(scale, o.state())
    assert [run(B) for _ in range(40)] == [L.HZ_FB_PATH_STREAM] * 40
    run.states(scale, o.state())
    print("muted C2 geometry: paths %s, worst block %.3e, worst regular-band state %.3e"
          % (paths, run.worst, run.worst_state))
    g.close()


def test_one_hot_gains(gpu_lib):
    """mix one-hot at bands 0, 1, N - 2 and either side of every boundary of the engines' geometry
    at N = 256 (visibility.ONE_HOT_BANDS names them): the output is that one band, so the reference
    is lfilter of it with the smoothed pre-amp and gain, and the bound 1e-9 of ITS peak -- through
    general, LTI and stationary calls, then 20 streamed blocks.  Measured on MI355X: worst block over
    the 18 bands 1.2e-12."""
    from huygens_amd import Filterbank
    L = _paths()
    N, R, seed = vz.ONE_HOT
    calls = [2000, 60_000, 20_000] + [B] * 20
    x = vz.noise(np.random.default_rng(seed), sum(calls))
    worst, fails = 0.0, []
    for b in vz.ONE_HOT_BANDS:
        g = Filterbank(2, N, vz.K_SMOOTH, vz.K_SMOOTH)
        fwd, back = vz.recipe_bank_muted(N, R, [g])
        g.tune_response(0, 1)
        hot = np.zeros(N)
        hot[b] = 1.0
        g.mix(hot)
        ref = vz.one_band_reference(fwd[b], back[b], x, vz.K_SMOOTH, vz.K_SMOOTH)
        pos, paths = 0, []
        for n in calls:
            y = g.process(x[pos:pos + n])
            paths.append(g.last_path())
            err, peak = block_errors(y, ref[pos:pos + n])
            assert peak.min() > 0
            worst = max(worst, float(err.max()))
            if err.max() > vz.TOL_OUT:
                fails.append((b, n, paths[-1], float(err.max())))
            pos += n
        assert paths[0] == L.HZ_FB_PATH_GENERAL and paths[2] == L.HZ_FB_PATH_RESPONSE, (b, paths[:3])
        assert paths[3:] == [L.HZ_FB_PATH_STREAM] * 20, (b, paths)
        g.close()
    print("one-hot gains: worst block over %d bands %.3e" % (len(vz.ONE_HOT_BANDS), worst))
    assert not fails, fails


def test_churn_on_muted_bank(gpu_lib):
    """test_mix_churn_streams' schedule (9 bands every 5 blocks, one all-band setter) on the muted
    512-band bank, band N - 1 held at 0 throughout: every one of the 150 blocks streams and is
    within 1e-9 -- the streaming gain-setter transient with every retuned band in sight -- then a
    boost() (per-band engines) and a long call, with the per-band states.  Measured on MI355X: worst
    block 1.1e-12, worst regular-band state 8.2e-12 of the band's peak."""
    L = _paths()
    N, R, seed = vz.CHURN
    g, o, fwd, back = _pair(N, R)
    run = _Run(g, o, seed)
    warm = [run(60_000) for _ in range(3)]
    assert warm[-1] == L.HZ_FB_PATH_RESPONSE, warm
    scale = vz.band_peaks(fwd, back, run.window())
    ev = vz.churn_events(N, seed + 1)
    calls0 = g.stream_info()[2]
    streamed = 0
    for blk in range(vz.CHURN_BLOCKS):
        for fb in (g, o):
            vz.apply_setters(fb, ev[blk])
        streamed += run(B) == L.HZ_FB_PATH_STREAM
    assert streamed == vz.CHURN_BLOCKS and g.stream_info()[2] - calls0 == vz.CHURN_BLOCKS
    run.states(scale)
    for fb in (g, o):
        fb.boost(20, 1.5)
    for _ in range(20):
        run(B)
    run(30_000)
    run.states(scale)
    print("churn on the muted bank: worst block %.3e, worst regular-band state %.3e" % (run.worst, run.worst_state))
    g.close()
