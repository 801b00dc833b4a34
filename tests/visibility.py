"""Which components can a parity case see?  (TEST INFRASTRUCTURE; numpy / scipy only.)

A parity case compares a mixdown with the restatement under a bound `tol` relative to the mix's
peak.  A component (a band of a Filterbank, a partial of an Additive bank) whose own peak is a
share v of that peak can be wrong by tol / v of itself before the case notices.  The rule used
throughout the suite:

    a case with bound tol may only claim the components whose own peak is >= 1000 tol (mix peak),

so that an error of 0.1 % in that one component fails the case.  It is a condition on the test's
INPUTS, proved from the restatement alone (tests/test_visibility_cpu.py); it is never used to skip.

The reference coefficient recipe puts its last band on Nyquist with a forward gain ~1e6 (a double
pole at z = -R): that band is 1 - 1e-8 of the mix, and every other band is invisible at any bound
the engines can meet.  recipe_bank_muted() keeps the recipe's coefficients -- the Nyquist band
still runs, with its 1e8 states, through the modal exception path and the direct sum -- and holds
that band's gain at exactly 0 on both sides, which leaves a mix every band of which counts.
"""
import numpy as np
from scipy.signal import lfilter

from golden.spec_numpy import relaxation, resonant_coefficients

FACTOR = 1000          # own peak >= FACTOR * tol * mix peak: 0.1 % of the component fails the case
STATE_WINDOW = 65536   # inputs that decide a band's state at R <= 0.999 (0.999^65536 = 3e-29)


def component_visibility(peaks, mix_peak):
    """each component's own peak as a share of the mix's peak"""
    peaks = np.atleast_1d(np.asarray(peaks, dtype=np.float64))
    assert mix_peak > 0 and np.all(np.isfinite(peaks))
    return peaks / float(mix_peak)


def assert_visible(vis, tol, factor=FACTOR):
    """every component's share of the mix is at least factor * tol; returns the weakest share"""
    vis = np.atleast_1d(np.asarray(vis, dtype=np.float64))
    assert vis.size
    worst = int(np.argmin(vis))
    assert vis[worst] >= factor * tol, (
        "component %d is %.3e of the mix: a bound of %.1e only sees it above %.1e"
        % (worst, vis[worst], tol, factor * tol))
    return float(vis[worst])


def hidden(vis, tol, factor=FACTOR):
    """indices of the components a case with bound tol cannot claim"""
    return np.flatnonzero(np.atleast_1d(vis) < factor * tol)


def recipe_bank_muted(N, R, banks=()):
    """The reference recipe's coefficients, unchanged, set on every Filterbank-like object of
    `banks` with boost(1), open() and then mix(N - 1, 0.0) before the first sample: the gain
    smoother of the Nyquist band starts at 0 and its target is 0, so its gain is exactly 0 on
    engine and restatement alike while the band itself keeps running.  -> (fwd, back)"""
    fwd, back = resonant_coefficients(N, R, 1.0)
    for fb in banks:
        for n in range(N):
            fb.coefficients(n, fwd[n], back[n])
        fb.boost(np.ones(N))
        fb.open()
        fb.mix(N - 1, 0.0)
    return fwd, back


def band_outputs(fwd, back, x, bands=None):
    """band b's own output y_b = lfilter(fwd[b], [1, back[b]], x) (pre-amp 1, before the gain),
    [len(bands)][len(x)]"""
    bands = range(len(fwd)) if bands is None else bands
    x = np.asarray(x, dtype=np.float64)
    return np.stack([lfilter(fwd[b], np.concatenate([[1.0], back[b]]), x) for b in bands])


def band_peaks(fwd, back, x):
    """per-band output peak over the window x (scipy.signal.lfilter from rest; for the scale of a
    state after a long call the last STATE_WINDOW inputs suffice at R <= 0.999)"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([np.max(np.abs(lfilter(fwd[b], np.concatenate([[1.0], back[b]]), x)))
                     for b in range(len(fwd))])


def smoothed(target, k, n, start=0.0):
    """the reference's one-pole smoother (filterbank.h:172-173) over n samples: value used BY
    sample t, t < n"""
    s = relaxation(k)
    out = np.empty(n)
    v = start
    for t in range(n):
        nv = (1 - s) * target + s * v
        if nv == v:          # the recurrence's fixed point: it stays there
            out[t:] = v
            break
        out[t] = v = nv
    return out


def one_band_reference(fwd_b, back_b, x, k_p, k_g, gain=1.0):
    """One band of a bank started from rest with boost 1 and mix `gain`: the pre-amp smoother
    scales the forward sum, the gain smoother the band's output.  lfilter restatement, independent
    of the C one."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    ff = lfilter(fwd_b, [1.0], x) * smoothed(1.0, k_p, n)
    y = lfilter([1.0], np.concatenate([[1.0], back_b]), ff)
    return y * smoothed(gain, k_g, n)


def band_state_errors(y_gpu, y_ref, scale_b, order=2):
    """band states [bands * order] of any run of bands: max |d state| / scale_b per band"""
    yg = np.asarray(y_gpu).reshape(-1, order)
    yr = np.asarray(y_ref).reshape(-1, order)
    scale_b = np.asarray(scale_b, dtype=np.float64)
    assert yg.shape == yr.shape and scale_b.shape == (len(yr),) and np.all(scale_b > 0)
    return np.max(np.abs(yg - yr), axis=1) / scale_b


def per_band_state_errors(st_gpu, st_ref, N, scale_b, order=2):
    """-> (regular, nyquist) from two hz_fb_get_state buffers: for each band b < N - 1, max
    |d state| / scale_b[b] with scale_b that band's own output peak (band_peaks); the last band
    (the recipe's Nyquist double pole, states ~1e8) separately, relative to its own reference
    state, for the bound each test had."""
    yr = np.asarray(st_ref)[order:order + order * N]
    scale = np.array(scale_b, dtype=np.float64)
    scale[-1] = max(np.max(np.abs(yr[-order:])), 1e-300)
    e = band_state_errors(np.asarray(st_gpu)[order:order + order * N], yr, scale, order)
    return e[:-1], float(e[-1])


def assert_band_states(st_gpu, st_ref, N, scale_b, tol, nyquist_tol, order=2):
    """every regular band's state within tol of ITS OWN peak; the Nyquist band within nyquist_tol
    of its own state.  -> (worst regular, nyquist)"""
    reg, nyq = per_band_state_errors(st_gpu, st_ref, N, scale_b, order)
    w = int(np.argmax(reg))
    assert reg[w] <= tol, ("band %d state off by %.3e of its own peak (bound %.1e)" % (w, reg[w], tol))
    assert nyq <= nyquist_tol, ("Nyquist band state off by %.3e (bound %.1e)" % (nyq, nyquist_tol))
    return float(reg[w]), nyq


# ---- the cases of tests/test_fb_band_visibility_gpu.py, shared with the CPU proofs ----------

TOL_OUT = 1e-9      # per 1024-sample block: the project's TOL, met by balanced 4096-band banks
TOL_STATE = 1e-8    # of the band's own peak: the loosest regular-band bound of test_fb_modal_gpu.py
K_SMOOTH = 0.001    # k_p = k_g: the smoothers converge within ~60 samples
B = 1024

MUTED_SMALL = [(256, 0.99, 5), (1024, 0.999, 6)]   # N, R, seed
MUTED_C2 = (4096, 0.999, 1234, 100_000)            # N, R, seed, call length (bench.py's geometry)
ONE_HOT = (256, 0.99, 7)
# one-hot bands at N = 256: 0, 1, N - 2 and either side of
#   15 | 16         a workgroup of the general and the LTI engine: 16 waves of one band each
#                   (hz_filterbank.hip default geometry, hz_fb_lti.hip kLtiGeoms), and one 16-wide
#                   MFMA block of the matrix-core state pass
#   31 | 32         that pass's 32 band-state columns per workgroup (hz_fb_state.h kCols) and the
#                   LTI reduce's kRedRows = 32
#   63 | 64, 127 | 128, 191 | 192   later workgroup boundaries of all three (multiples of 16 and 32)
#   modal DFT       band b of a 256-band recipe bank sits on grid point m = 16 (b + 1) of the
#                   8192-point DFT (hz_fb_modal.h), m = k1 + 64 k2: k1 wraps between bands 2 | 3,
#                   and the phase-2 workgroups take 16 values of k2 each (kParts = 4), which
#                   changes hands between bands 62 | 63, 126 | 127 and 190 | 191
# The stationary and streaming convolutions see the bank only through its response h = sum_n
# gain_n r_n (response_engine(): column split or three kernels, neither indexed by band), so a
# one-hot mix checks that h is band b's response and no other's.
ONE_HOT_BANDS = [0, 1, 2, 3, 15, 16, 31, 32, 62, 63, 64, 126, 127, 128, 190, 191, 192, 254]
CHURN = (512, 0.999, 512)                          # N, R, seed
CHURN_BLOCKS = 150


def noise(rng, n):
    """uniform [-1, 1) rounded to float32 (the audio callback's format), as doubles"""
    return rng.uniform(-1, 1, n).astype(np.float32).astype(np.float64)


def churn_events(N, seed, mute_last=True):
    """test_mix_churn_streams' schedule from a generator of its own: blk -> list of setters.
    9 bands retuned every 5 blocks for 80 blocks, one all-band setter at block 40.  mute_last:
    band N - 1 is held at 0 throughout."""
    rng = np.random.default_rng(seed)
    ev = {}
    for blk in range(CHURN_BLOCKS):
        e = []
        if blk < 80 and blk % 5 == 2:
            bands = rng.choice(N, 9, replace=False)
            vals = rng.uniform(0.3, 1.7, 9)
            for b, v in zip(bands, vals):
                e.append((int(b), 0.0 if mute_last and b == N - 1 else float(v)))
        if blk == 40:
            v = rng.uniform(0.8, 1.2, N)
            if mute_last:
                v[N - 1] = 0.0
            e.append((None, v))
        ev[blk] = e
    return ev


def apply_setters(bank, setters):
    for b, v in setters:
        if b is None:
            bank.mix(v)
        else:
            bank.mix(b, v)


# ---- Additive / Sinusoids ------------------------------------------------------------------

def partial_weights(V, O, decay):
    """partial j of a voice at amplitude 1 peaks at decay^j / (V normalization) (additive.h:27,
    53-62; a sinusoid, peak 1)"""
    norm = (1 - decay ** O) / (1 - decay) if decay != 1 else O
    return decay ** np.arange(O) / (V * norm)
