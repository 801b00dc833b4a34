"""CPU: the numpy STFT spec (tests/stft_spec.py) against the long double DFT and the committed
fixtures, and the conditions that every input of tests/test_stft_spectrum_gpu.py must meet,
proved from the spec alone -- so an input that drifts fails here instead of turning a GPU test
vacuous.

Measured (numpy's pocketfft against oracle_dft's long double radix 2, complex noise through
either window, largest bin error relative to the frame's spectral peak): 8.8e-17 at N = 4,
2.3e-16 at 64, 3.4e-16 at 1024, 3.8e-16 at 4096, 3.6e-16 at 8192.  The bound below is the 1e-14
that tests/test_stft_cpu.py already holds the two to, about 7 eps log2(N) at the largest size.
"""
import numpy as np
import pytest

import stft_spec as sp
from golden.make_golden_stft import proc_gate_keep, proc_hilbert, proc_static_gate
from oracle import golden_names, load_golden
from oracle_stft import oracle_dft

LGS = list(range(2, 14))


@pytest.mark.parametrize("lg", LGS)
def test_frame_spectra_vs_long_double_dft(lg):
    N = 1 << lg
    x = sp.noise(3 * N + 5, lg)
    for wkind, laps in ((0, 1), (1, 4 if N >= 8 else 2)):
        starts = sp.frame_starts(len(x), N, laps)
        X = sp.frame_spectra(x, N, laps, wkind)
        assert X.shape == (len(starts), N) and len(starts) >= 3
        w = sp.window(wkind, N)
        worst = 0.0
        for s, Xf in zip(starts, X):
            ref = oracle_dft(w * x[s:s + N], -1)
            worst = max(worst, np.max(np.abs(Xf - ref)) / np.max(np.abs(ref)))
        print(f"N={N} window={wkind} laps={laps}: numpy vs long double DFT {worst:.2e}")
        assert worst < 1e-14


def test_frame_starts_schedule():
    """Frame order is (c, i) order; one hop in 2*laps is stride - 1; a frame counts once its last
    sample is in."""
    s = sp.frame_starts(3 * 127, 64, 4)
    assert s.tolist() == sorted(s.tolist())
    assert set(np.diff(s).tolist()) == {15, 16}
    assert len(sp.frame_starts(63, 64, 4)) == 0 and len(sp.frame_starts(64, 64, 4)) == 1
    # laps = N: stride 1, slot 2N-1 of one period and slot 0 of the next start on the same sample
    s = sp.frame_starts(40, 4, 4)
    assert s[7] == s[8] == 7


@pytest.mark.parametrize("name", golden_names("stft_"))
def test_run_reproduces_fixtures(name):
    g = load_golden(name)
    N, laps = int(g["N"]), int(g["laps"])
    proc = {0: sp.proc_identity, 1: proc_static_gate, 2: proc_gate_keep, 3: proc_hilbert}[int(g["proc"])]
    r = sp.run(g["x_re"] + 1j * g["x_im"], N, laps, int(g["window"]), proc)
    scale = max(np.max(np.abs(g["y_re"])), np.max(np.abs(g["y_im"])))
    assert np.max(np.abs(r.y.real - g["y_re"])) <= 1e-13 * scale
    assert np.max(np.abs(r.y.imag - g["y_im"])) <= 1e-13 * scale
    assert sorted(r.starts.tolist()) == g["starts"].tolist()
    if np.isfinite(float(g["margin"])):
        assert abs(r.margin - float(g["margin"])) <= 1e-9 * float(g["margin"])
    if int(g["proc"]) == 3:
        assert np.all(r.keep[:, :N // 2]) and not np.any(r.keep[:, N // 2:])


@pytest.mark.parametrize("lg", sp.HILBERT_LGS)
def test_hilbert_input_conditions(lg):
    """A tone at a negative-frequency bin, a weaker one at a positive bin: the half-band's output
    is far from what any processor blind to the bin index would give."""
    N, laps, n = sp.hilbert_case(lg)
    kneg, kpos = sp.hilbert_bins(N)
    assert N // 2 < kneg < N and 0 < kpos < N // 2
    x = sp.hilbert_input(lg)
    assert len(x) == n and np.iscomplexobj(x)
    X = sp.frame_spectra(x, N, laps, 0)
    mag = np.abs(X).mean(axis=0)
    assert np.argmax(mag) == kneg and mag[kpos] > 0.3 * mag[kneg]
    got = sp.hilbert_run(lg)
    ident = sp.run(x, N, laps, 0, sp.proc_identity)
    peak = np.max(np.abs(got.y))
    assert peak > 0.1
    assert np.max(np.abs(got.y - ident.y)) > 0.1 * peak
    assert len(got.starts) >= 2 * laps


@pytest.mark.parametrize("gate", list(sp.GATES))
@pytest.mark.parametrize("case", sp.GATE_CASES, ids=lambda c: c.id)
def test_gate_input_conditions(case, gate):
    """Every gated GPU input: no decision within 1e-6 (relative) of its threshold; from N = 512
    on every frame keeps a bin, at least half of all consecutive frames keep different bins and
    so do at least a quarter of the frame pairs that share a transform in the calls the GPU test
    makes; launches begin on even and on odd frames.  For real input from N = 256 on, gating the
    second frame of such a pair with the first frame's threshold changes its kept bins in at least
    an eighth of the pairs.  Below N ~ 64 neither gate opens with these windows (the keep gate
    wants one bin above 25 x the mean magnitude): plain parity cases."""
    N, laps = case.N, case.laps
    x = sp.gate_input(case)
    assert len(x) == case.n and np.iscomplexobj(x) == case.cplx
    r = sp.gate_run(case, gate)
    assert r.margin >= sp.MARGIN_MIN, r.margin
    cuts = sp.gate_cuts(case.n, N, laps)
    assert cuts == sorted(set(cuts))
    first = sp.launch_first_frames(cuts, N, laps)
    assert {f % 2 for f in first} == {0, 1}, first
    kept = r.keep.sum(axis=1)
    differ = np.any(r.keep[1:] != r.keep[:-1], axis=1)
    pairs = sp.launched_pairs(cuts, N, laps)
    shared = sum(bool(differ[f]) for f, _ in pairs)
    X = sp.frame_spectra(x, N, laps, sp.GATES[gate][0])
    thr = [sp.gate_threshold(gate, Xf, N) for Xf in X]
    assert all(np.array_equal(sp.gate_mask(gate, Xf, t), k) for Xf, t, k in zip(X, thr, r.keep))
    swapped = sum(not np.array_equal(sp.gate_mask(gate, X[b], thr[a]), r.keep[b]) for a, b in pairs)
    print(f"{case.id} {gate}: {len(r.starts)} frames, margin {r.margin:.2e}, kept {kept.min()}..{kept.max()}, "
          f"{int(differ.sum())} of {len(differ)} consecutive pairs differ, {shared} of {len(pairs)} launched pairs, "
          f"{swapped} change under the neighbour's threshold")
    if N >= 512:
        assert kept.min() >= 1
        assert 2 * int(differ.sum()) >= len(differ)
        assert 4 * shared >= len(pairs)
        assert np.max(np.abs(r.y)) > 0.3
    elif N >= 256:
        assert kept.max() >= 1 and 4 * int(differ.sum()) >= len(differ)
    if N >= 256 and not case.cplx:
        assert 8 * swapped >= len(pairs)


def test_gate_cases_reach_every_kernel():
    """Real input: generic radix-8 pairs (16 ... 1024), the 4096 pair kernel, radix-16 pairs at
    8192 with laps 4 and 32; complex input: the gated one-frame kernel at 8, 512, 4096, 8192."""
    real = {(c.N, c.laps) for c in sp.GATE_CASES if not c.cplx}
    cplx = {c.N for c in sp.GATE_CASES if c.cplx}
    assert real == {(16, 4), (256, 4), (512, 4), (1024, 4), (4096, 4), (8192, 4), (8192, 32)}
    assert cplx == {8, 512, 4096, 8192}
    assert all(len(sp.frame_starts(c.n, c.N, c.laps)) >= 20 for c in sp.GATE_CASES)


@pytest.mark.parametrize("N", [4, 64, 8192])
def test_bin_gains_not_symmetric(N):
    """g[k] != conj g[N-k] and no two bins share a gain: a mirrored or permuted spectrum shows."""
    g = sp.bin_gains(N)
    k = np.arange(1, N)
    assert np.min(np.abs(g[k] - np.conj(g[N - k]))) > 1e-6
    assert len(np.unique(g)) == N
