"""What the parity tests can see, proved on the CPU (tests/visibility.py).

The restatement stands in for the engine, so that the ASSERTIONS of the GPU tests are themselves
under test:

  1. the figures that motivate the rule, as asserted inequalities: on the reference recipe every
     band but the Nyquist one is below the bound the mix-relative tests assert, and most partials of
     the C3 Additive shape are too;
  2. assert_visible for every case of tests/test_fb_band_visibility_gpu.py and the new Additive
     shapes, with the N, R, gains, seeds and tolerances those tests use;
  3. mutants of the restatement -- an engine that is wrong in one band or partial -- which PASS the
     mix-relative check on the recipe bank and FAIL the checks of the new tests.  Relaxing a new
     assertion to the old form makes these tests fail.
"""
import numpy as np
import pytest

import visibility as vz
from golden.spec_numpy import resonant_coefficients
from oracle import OracleFilterbank, rel_err
from oracle_osc import OracleAdditive
from test_c2_pinned_gpu import TIGHT, block_errors

OLD_TOL = TIGHT   # 1e-7: what the recipe-bank tests assert per block and on bank-wide states


# ---- helpers ---------------------------------------------------------------------------------

def recipe_bank(N, R, k_p, k_g, cls=OracleFilterbank, **kw):
    """the unmuted reference recipe, as tests/test_fb_stream_gpu.py::_bank sets it up"""
    o = cls(2, N, k_p, k_g, **kw)
    fwd, back = resonant_coefficients(N, R, 1.0)
    for n in range(N):
        o.coefficients(n, fwd[n], back[n])
    o.boost(np.ones(N))
    o.open()
    return o


def muted_bank(N, R, k_p=vz.K_SMOOTH, k_g=vz.K_SMOOTH, cls=OracleFilterbank, **kw):
    o = cls(2, N, k_p, k_g, **kw)
    vz.recipe_bank_muted(N, R, [o])
    return o


class Mutant(OracleFilterbank):
    """The restatement, wrong in one way:
      nyquist_only    only band N - 1 sounds (every other gain target is 0)
      ignore_setters  mix(b, v) with b != N - 1 is ignored
      detune          band `band`'s back[0] is off by 1e-6 relative"""

    def __init__(self, order, N, k_p, k_g, kind, band=100):
        super().__init__(order, N, k_p, k_g)
        self.kind, self.band = kind, band

    def coefficients(self, n, fwd, back):
        if self.kind == "detune" and n == self.band:
            back = np.array(back) * [1 + 1e-6, 1.0]
        super().coefficients(n, fwd, back)

    def _only_last(self, v):
        w = np.zeros(self.N)
        w[-1] = v[-1]
        return w

    def open(self):
        super().open()
        if self.kind == "nyquist_only":
            super().mix(self._only_last(np.ones(self.N)))

    def mix(self, n_or_values, value=None):
        if value is None:
            v = np.asarray(n_or_values, dtype=np.float64)
            super().mix(self._only_last(v) if self.kind == "nyquist_only" else v)
        elif n_or_values == self.N - 1 or self.kind not in ("nyquist_only", "ignore_setters"):
            super().mix(n_or_values, value)


def stream_blocks(banks, seed, blocks=24):
    """the same float32 noise through every bank, in 1024-sample calls -> one output each"""
    rng = np.random.default_rng(seed)
    outs = [[] for _ in banks]
    for _ in range(blocks):
        x = vz.noise(rng, vz.B)
        for o, acc in zip(banks, outs):
            acc.append(o.process(x))
    return [np.concatenate(a) for a in outs]


def worst_block(y, ref):
    return float(block_errors(y, ref)[0].max())


def churn_run(bank, N, seed, warm=60_000, tail=True, mute_last=True):
    """tests/test_fb_band_visibility_gpu.py::test_churn_on_muted_bank's sequence on one bank: a
    long call, the 150 churned blocks, then boost(20, 1.5) and 20 more blocks"""
    rng = np.random.default_rng(seed)
    ev = vz.churn_events(N, seed + 1, mute_last)
    out = [bank.process(vz.noise(rng, warm))]
    for blk in range(vz.CHURN_BLOCKS):
        vz.apply_setters(bank, ev[blk])
        out.append(bank.process(vz.noise(rng, vz.B)))
    if tail:
        bank.boost(20, 1.5)
        for _ in range(20):
            out.append(bank.process(vz.noise(rng, vz.B)))
    return np.concatenate(out)


# ---- 1. the figures, as inequalities ------------------------------------------------------------

# the (N, R) of the recipe-bank tests: test_fb_stream_gpu.py, test_fb_churn_gpu.py,
# test_c2_pinned_gpu.py, test_fullsize_gpu.py, test_filterbank_resp_gpu.py
RECIPE_SHAPES = [(128, 0.99), (256, 0.99), (128, 0.999), (256, 0.999), (512, 0.999), (1024, 0.999), (4096, 0.999)]


@pytest.mark.parametrize("N,R", RECIPE_SHAPES)
def test_recipe_bank_hides_every_band_but_nyquist(N, R):
    """rest / mix < 1e-7 = the bound those tests assert: a bank with only its Nyquist band passes
    them.  Measured 2.9e-10 (128, 0.99) to 3.2e-8 (4096, 0.999); a single band is below 1e-8."""
    n = 32768
    x = vz.noise(np.random.default_rng(5), n)
    full = recipe_bank(N, R, vz.K_SMOOTH, vz.K_SMOOTH).process(x)
    rest = muted_bank(N, R).process(x)
    ratio = np.max(np.abs(rest)) / np.max(np.abs(full))
    print("recipe N %d R %g: rest / mix %.3e" % (N, R, ratio))
    assert ratio < OLD_TOL
    fwd, back = resonant_coefficients(N, R, 1.0)
    assert fwd[-1, 0] > 1e5                      # its forward gain (2.4e6 at R = 0.999)
    # the Nyquist band alone, against the whole bank, per block
    errs = block_errors(full - rest, full)[0]
    print("   Nyquist band alone, worst block: %.3e" % errs.max())
    some = range(N - 1) if N <= 1024 else range(0, N - 1, 64)
    pk = np.array([np.max(np.abs(y)) for y in vz.band_outputs(fwd, back, x, some)])
    vis = vz.component_visibility(pk, np.max(np.abs(full)))
    assert vis.max() < 1e-8                      # no regular band is visible at 1e-7 (needs 1e-4)
    assert len(vz.hidden(vis, OLD_TOL)) == len(pk)
    with pytest.raises(AssertionError):
        vz.assert_visible(vis, OLD_TOL)
    if N <= 1024:
        assert errs.max() < OLD_TOL              # ... and passes the old bound in every block
    else:
        # 4096 bands: the rest of the bank together reaches 1.04e-7 of one block, so a bank that
        # loses ALL of them would be seen there -- one that loses 2000 of them would not
        assert errs.max() < 2 * OLD_TOL and np.median(errs) < OLD_TOL


def test_c3_additive_shape_hides_most_partials():
    """V = 64, O = 256, decay 0.75 at TOL 1e-8: partial j weighs 0.75^j; 228 of 256 per voice are
    below the 1e-5 of the mix that the rule asks, and a bank cut to 80 partials passes (rel_err
    7.3e-11; cut to 96: 7.4e-13)."""
    V, O, decay, tol = 64, 256, 0.75, 1e-8
    full, cut80, cut96 = (_additive(V, p, O, decay, 1000) for p in (O, 80, 96))
    vis = vz.component_visibility(vz.partial_weights(V, O, decay), np.max(np.abs(full)))
    print("C3 shape: %d of %d partials per voice hidden" % (len(vz.hidden(vis, tol)), O))
    assert len(vz.hidden(vis, tol)) >= 228
    e80, e96 = rel_err(cut80, full), rel_err(cut96, full)
    print("C3 shape truncated to 80 / 96 partials: rel_err %.3e / %.3e" % (e80, e96))
    assert 1e-11 < e80 < tol and e96 < 1e-11    # tasks 2 to 4 of every voice: unverified


# ---- 2. every new GPU case is visible -------------------------------------------------------

def _muted_visibility(N, R, seed, n=vz.STATE_WINDOW, k_p=vz.K_SMOOTH, k_g=vz.K_SMOOTH, gain_floor=1.0):
    x = vz.noise(np.random.default_rng(seed), n)
    y = muted_bank(N, R, k_p, k_g).process(x)
    fwd, back = resonant_coefficients(N, R, 1.0)
    pk = vz.band_peaks(fwd, back, x)
    _, bpeak = block_errors(y, y)
    return vz.component_visibility(gain_floor * pk[:-1], bpeak.max())


@pytest.mark.parametrize("N,R,seed", vz.MUTED_SMALL)
def test_muted_small_cases_visible(N, R, seed):
    """measured weakest band / largest block peak: 6.3e-2 (256, 0.99), 3.8e-2 (1024, 0.999)"""
    weakest = vz.assert_visible(_muted_visibility(N, R, seed), vz.TOL_OUT)
    print("muted recipe N %d R %g: weakest band %.3e of the mix" % (N, R, weakest))
    assert weakest > 1e-2


def test_muted_c2_geometry_visible():
    """N = 4096, R = 0.999: measured 1.0e-2 (a window of 32768 samples)"""
    N, R, seed, _ = vz.MUTED_C2
    weakest = vz.assert_visible(_muted_visibility(N, R, seed, n=32768, k_p=0.1, k_g=1.0), vz.TOL_OUT)
    print("muted recipe N %d: weakest band %.3e of the mix" % (N, weakest))
    assert weakest > 5e-3


def test_one_hot_cases_visible():
    """a one-hot mix is its band: visibility 1 by construction; the band's peak is what the bound
    is relative to, and every block of it sounds"""
    N, R, seed = vz.ONE_HOT
    assert vz.ONE_HOT_BANDS == sorted(set(vz.ONE_HOT_BANDS)) and vz.ONE_HOT_BANDS[-1] == N - 2
    fwd, back = resonant_coefficients(N, R, 1.0)
    x = vz.noise(np.random.default_rng(seed), 20 * vz.B)
    for b in vz.ONE_HOT_BANDS:
        y = vz.one_band_reference(fwd[b], back[b], x, vz.K_SMOOTH, vz.K_SMOOTH)
        _, bpeak = block_errors(y, y)
        vz.assert_visible(vz.component_visibility(bpeak.min(), bpeak.max()), vz.TOL_OUT)
        # the lfilter reference is the restatement's band (its own error, far below the bound)
        o = OracleFilterbank(2, N, vz.K_SMOOTH, vz.K_SMOOTH)
        vz.recipe_bank_muted(N, R, [o])
        hot = np.zeros(N)
        hot[b] = 1.0
        o.mix(hot)
        assert worst_block(y, o.process(x)) < 1e-12


def test_churn_case_visible():
    """N = 512, gains down to 0.3 (the schedule's floor): measured 9.6e-3"""
    N, R, seed = vz.CHURN
    ev = vz.churn_events(N, seed + 1)
    floor = min(min([v for b, v in e if b is not None and b != N - 1] +
                    [np.min(v[:-1]) for b, v in e if b is None] + [1.0]) for e in ev.values())
    assert 0.3 <= floor < 0.35
    for e in ev.values():   # band N - 1 stays at 0
        assert all((v == 0.0 if b == N - 1 else True) if b is not None else v[-1] == 0.0 for b, v in e)
    vis = _muted_visibility(N, R, seed, gain_floor=floor) / 1.7   # (mix peak: gains up to 1.7)
    weakest = vz.assert_visible(vis, vz.TOL_OUT)
    print("churn N %d: weakest band %.3e of the mix" % (N, weakest))


ADD_SHAPES = [(3, 130, 1.0), (3, 130, 0.97), (2, 200, 1.0)]   # tests/test_additive_gpu.py
ADD_TOL = 1e-8


def _additive(V, P, O, decay, n, amps=None, pitch0=36, step=1):
    """OracleAdditive(V, O, decay) cut to its first P partials per voice: at harmonicity 1 partial
    j sits on (1 + j) fundamental whatever O is, so the cut bank is the P-partial bank rescaled
    by the two normalizations"""
    o = OracleAdditive(V, P, decay, 1.0)
    for v in range(V):
        o.makenote(pitch0 + step * v, 1.0 if amps is None else amps[v])
    y = o.fill(n)
    return y * (vz.partial_weights(V, O, decay)[0] / vz.partial_weights(V, P, decay)[0])


@pytest.mark.parametrize("V,O,decay", ADD_SHAPES)
def test_additive_shapes_visible_and_cut_by_one_fails(V, O, decay):
    """weakest partial / mix peak, measured: 9.9e-3, 9.3e-4, 6.9e-3 (1e-5 asked); the bank with one
    partial less is 1000 x further off than TOL"""
    n = 3000
    full = _additive(V, O, O, decay, n)
    amp = 1 - 2.0 ** (-52 * (n - 1) / 4800.0)      # the attack smoother's value by the last sample
    vis = vz.component_visibility(amp * vz.partial_weights(V, O, decay), np.max(np.abs(full)))
    weakest = vz.assert_visible(vis, ADD_TOL)
    print("Additive (%d, %d, %g): weakest partial %.3e of the mix" % (V, O, decay, weakest))
    cut = _additive(V, O - 1, O, decay, n)
    assert rel_err(cut, full) > 100 * ADD_TOL      # mutant e on the new shapes: fails < TOL


def test_audit_other_families():
    """What the other decay-weighted families see (weakest partial's weight against a mix peak of
    at most the sum of the weights, which is the most pessimistic reading).
      Subtractive WIDE  O = 40, decay 0.75 at 1e-9: 0.75^39 / sum = 3.4e-6 >= 1e-6: visible
      physics / Subtractive scenarios  O <= 4, decay 0.75: 0.15 and more: visible at 1e-5 and 1e-9
      physics WIDE      O = 40 at its audio bound 1e-5: hidden past partial 11 -- that test is
                        about positions (compared bit for bit); its audio is covered by the
                        Additive shapes above, which run the same synthesis kernel."""
    w = 0.75 ** np.arange(40)
    share = w / w.sum()
    vz.assert_visible(share, 1e-9)
    assert list(vz.hidden(share, 1e-5)) == list(range(12, 40))
    for O in (3, 4):
        w = 0.75 ** np.arange(O)
        vz.assert_visible(w / w.sum(), 1e-5)
    # equal-amplitude banks: Oscbank's largest mix, N = 16384 at 1e-9 -- one oscillator is 1 / N
    # of the sum of the amplitudes
    vz.assert_visible(np.full(16384, 1 / 16384.0), 1e-9)


@pytest.mark.parametrize("M,n", [(2048, 5000), (303, 30000), (5, 7000)])
def test_audit_bowl_modes(M, n):
    """tests/test_bowl_gpu.py::test_c5_shape's models (the same generator): mode i is
    a_i e^(-d_i t) sin(2 pi f_i t), amplitudes 1e-4 .. 5e-2.  In double (1e-9) every mode is in
    sight -- weakest 8.2e-6, 5.0e-5, 3.0e-2 of the mix (1e-6 asked).  The float engine is held to
    1e-5 because the reference rounds its running sum to float after every mode; at that bound
    the rule would ask 1e-2 of the mix: no mode of the largest model reaches that, half of the 303
    do, all of the 5-mode model do -- the float cases of the larger models claim the sum, the
    double cases of the same models the modes."""
    from golden.spec_numpy import E, PI, SR
    rng = np.random.default_rng(M)
    f = np.exp(rng.uniform(np.log(20.0), np.log(16000.0), M))
    a = rng.uniform(1e-4, 5e-2, M)
    d = rng.uniform(0.05, 15.0, M)
    t = np.arange(n) / SR
    mix, peaks = np.zeros(n), np.zeros(M)
    for i in range(M):
        y = a[i] * E ** (-d[i] * t) * np.sin(2 * PI * f[i] * t)
        peaks[i] = np.max(np.abs(y))
        mix += y
    vis = vz.component_visibility(peaks, np.max(np.abs(mix)))
    weakest = vz.assert_visible(vis, 1e-9)
    print("Bowl M %d: weakest mode %.3e of the mix; hidden at 1e-5: %d of %d" % (M, weakest, len(vz.hidden(vis, 1e-5)), M))
    assert len(vz.hidden(vis, 1e-5)) >= {2048: 2000, 303: 150, 5: 0}[M]
    if M == 5:
        vz.assert_visible(vis, 1e-5)     # the float engine's visible shape


def test_audit_goldens():
    """Additive and Sinusoids fixtures at TOL 1e-8 (1e-5 of the mix asked): the weakest partial's
    weight against the fixture's own peak -- 1.1e-3 and more, visible"""
    from oracle import golden_names, load_golden
    for name in golden_names("add_") + golden_names("sin_"):
        g = load_golden(name)
        V = int(g["V"]) if "V" in g else 1
        O, decay = int(g["O"]), float(g["decay"])
        # (sin_o10_mods glides its decay from 0.8; the fixture's lowest decay target is 0.5)
        w = vz.partial_weights(V, O, min(decay, 0.5) if name == "sin_o10_mods" else decay)
        amp = 0.3 if V > 1 else 1.0      # the fixtures' quietest note
        vz.assert_visible(vz.component_visibility(amp * w, np.max(np.abs(g["y"]))), ADD_TOL)


# ---- 3. mutants: pass the old check, fail the new ones ------------------------------------------

@pytest.mark.parametrize("kind", ["nyquist_only", "detune"])
def test_mutant_passes_mix_relative_fails_muted(kind):
    """a. only band N - 1 sounding, c. one regular band's back[0] off by 1e-6"""
    N, R, seed = vz.MUTED_SMALL[0]
    # old form: the unmuted recipe, 1e-7 of the block peak (test_stream_small_bank_switches)
    ref, mut = stream_blocks([recipe_bank(N, R, 0.01, 0.01),
                              recipe_bank(N, R, 0.01, 0.01, cls=Mutant, kind=kind)], seed)
    old = worst_block(mut, ref)
    assert old <= OLD_TOL
    # new form: the muted recipe at 1e-9
    ref, mut = stream_blocks([muted_bank(N, R), muted_bank(N, R, cls=Mutant, kind=kind)], seed)
    new = worst_block(mut, ref)
    print("mutant %s: old check %.3e (passes 1e-7), new check %.3e" % (kind, old, new))
    assert new > 100 * vz.TOL_OUT


_churn_ref = {}


@pytest.mark.parametrize("kind", ["nyquist_only", "ignore_setters"])
def test_mutant_churn(kind):
    """a, b on the churn scenario: measured 2.3e-8 / 4.5e-9 under the old check (1e-7 asserted),
    1.0 / 0.26 under the new one (1e-9 asserted)"""
    N, R, seed = vz.CHURN
    if not _churn_ref:   # the two true banks, once for both mutants
        _churn_ref["old"] = churn_run(recipe_bank(N, R, 0.1, 1.0), N, seed, tail=False, mute_last=False)
        _churn_ref["new"] = churn_run(muted_bank(N, R), N, seed)
    ref = _churn_ref["old"]
    mut = churn_run(recipe_bank(N, R, 0.1, 1.0, cls=Mutant, kind=kind), N, seed, tail=False, mute_last=False)
    old = worst_block(mut, ref)
    assert old <= OLD_TOL
    ref = _churn_ref["new"]
    mut = churn_run(muted_bank(N, R, cls=Mutant, kind=kind), N, seed)
    new = worst_block(mut[60_000:], ref[60_000:])
    print("churn mutant %s: old check %.3e, new check %.3e" % (kind, old, new))
    assert new > 100 * vz.TOL_OUT


def test_mutant_state_zeroed():
    """d. one regular band's state zeroed: inside TIGHT max|state| (the Nyquist band's 1e8), far
    outside 1e-8 of the band's own peak; a Nyquist-band state off by 1e-6 is caught separately"""
    N, R, seed = vz.MUTED_SMALL[0]
    o = recipe_bank(N, R, 0.01, 0.01)
    rng = np.random.default_rng(seed)
    x = vz.noise(rng, 20 * vz.B)
    o.process(x)
    st = o.get_state()
    bad = st.copy()
    bad[2 + 2 * 100:2 + 2 * 100 + 2] = 0.0
    sc = np.max(np.abs(st[2:2 + 2 * N]))
    assert np.max(np.abs(bad[2:2 + 2 * N] - st[2:2 + 2 * N])) <= OLD_TOL * sc      # the old check
    fwd, back = resonant_coefficients(N, R, 1.0)
    scale = vz.band_peaks(fwd, back, x)
    assert vz.assert_band_states(st, st, N, scale, vz.TOL_STATE, OLD_TOL) == (0.0, 0.0)
    with pytest.raises(AssertionError, match="band 100"):
        vz.assert_band_states(bad, st, N, scale, vz.TOL_STATE, OLD_TOL)
    reg, _ = vz.per_band_state_errors(bad, st, N, scale)
    assert reg[100] > 1e-2 and np.count_nonzero(reg) == 1
    bad = st.copy()
    bad[2 * N:2 + 2 * N] *= 1 + 1e-6
    with pytest.raises(AssertionError, match="Nyquist"):
        vz.assert_band_states(bad, st, N, scale, vz.TOL_STATE, OLD_TOL)


def test_visibility_helpers():
    assert np.allclose(vz.component_visibility([1.0, 0.5], 2.0), [0.5, 0.25])
    assert vz.assert_visible([1e-5, 1.0], 1e-8) == 1e-5
    with pytest.raises(AssertionError, match="component 1"):
        vz.assert_visible([1.0, 9.9e-6], 1e-8)
    assert list(vz.hidden([1.0, 9.9e-6], 1e-8)) == [1]
    assert vz.assert_visible([1e-3], 1e-5, factor=100) == 1e-3
    s = vz.smoothed(1.0, vz.K_SMOOTH, 80)
    assert s[0] > 0.5 and abs(s[-1] - 1.0) < 1e-15 and np.all(np.diff(s) >= 0)
