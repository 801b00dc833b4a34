"""GPU: Subtractive<double, N> on the device (hz_subtractive.hip) against the op-for-op restatement
(tests/oracle_sub.py).

Positions and envelopes are compared as uint64 (bit for bit).  Audio is held to rel_err < 1e-9 per
channel (tests/oracle.py's norm-wise measure; the project's Filterbank parity bound): the engine
differs from the restatement in device exp2 / cos / sincos against libm's (the coefficients), and in
the order in which a sample's partials are summed.  Every test prints the error it measured."""
import os
import subprocess

import numpy as np
import pytest

from oracle import rel_err
from oracle_phys import GRAV_FABS, GRAV_TRUNC, SCENARIOS
from oracle_sub import SubOracle, run_sub_scenario
from test_subtractive_cpu import EXE, build_sub_dropin

pytestmark = pytest.mark.gpu
LAWS = [GRAV_TRUNC, GRAV_FABS]
PER_STEP = (1, 64)      # tune_physics: no bank takes the single-workgroup path, 64-thread tiles
BOUND = 1e-9
RES = 0.99999           # subtractive.h:35 default

# tests/test_physics_gpu.py's wide bank: 160 particles, voices straddle the 64-lane boundaries
WIDE = dict(V=4, O=40, decay=0.75, harm=1.0, k=0.1, period=2, n=128,
            events=[(0, 0, 48.0, 1.0), (0, 0, 48.3, 0.5), (0, 0, 55.1, 0.8), (0, 0, 60.2, 0.6)])

_cache = {}


def noise(N, n, seed=7):
    return np.random.default_rng(seed).standard_normal((N, n))


def oracle_run(name, law, N=2, sc=None, res=RES):
    """(audio [N][n], final positions, final amplitudes) of a scenario's restatement, once per key"""
    key = (name, law, N, res)
    if key not in _cache:
        sc = sc or SCENARIOS[name]
        o = SubOracle(sc["V"], sc["O"], sc["decay"], res, sc["harm"], sc["k"], N=N, law=law)
        o.physics_every(sc["period"])
        audio = run_sub_scenario(sc, noise(N, sc["n"]), o)
        audio.setflags(write=False)
        _cache[key] = (audio, o.positions(), o.amplitudes())
    return _cache[key]


def engine(sc, law, N=2, tune=None, res=RES):
    from huygens_amd import Subtractive
    g = Subtractive(sc["V"], sc["O"], sc["decay"], res, sc["harm"], sc["k"], channels=N)
    if tune:
        g.tune_physics(*tune)
    g.physics_every(sc["period"], law)
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_audio(label, got, want):
    assert got.shape == want.shape
    worst = 0.0
    for k in range(want.shape[0]):
        err = rel_err(got[k], want[k])
        print(f"subtractive audio {label} channel {k}: rel_err {err:.3e}")
        worst = max(worst, err)
    assert np.max(np.abs(want)) > 0
    assert worst < BOUND
    return worst


@pytest.mark.parametrize("tune", [None, PER_STEP], ids=["one_group", "per_step"])
@pytest.mark.parametrize("law", LAWS, ids=["trunc", "fabs"])
@pytest.mark.parametrize("name", ["v3o4", "steal", "p3"])
def test_positions_bit_exact_and_audio(gpu_lib, name, law, tune):
    """rel_err < 1e-9 asked.  Measured on MI355X over these twelve cases: 4e-16 to 1.1e-14
    (the largest of the file is the drop-in's 5.2e-14)."""
    sc = SCENARIOS[name]
    g = engine(sc, law, 2, tune)
    audio = run_sub_scenario(sc, noise(2, sc["n"]), g)
    want, final, amps = oracle_run(name, law)
    assert np.array_equal(bits(g.positions()), bits(final))
    assert np.array_equal(bits(g.amplitudes()), bits(amps))
    check_audio(f"{name} law {law}", audio, want)


def test_reference_program_resonance(gpu_lib):
    """resonance = 0.999995, k = 1: the reference programs' constructor arguments."""
    sc = dict(SCENARIOS["v3o4"], k=1.0)
    want, final, _ = oracle_run("v3o4_k1", GRAV_TRUNC, 2, sc, 0.999995)
    g = engine(sc, GRAV_TRUNC, 2, None, 0.999995)
    audio = run_sub_scenario(sc, noise(2, sc["n"]), g)
    assert np.array_equal(bits(g.positions()), bits(final))
    check_audio("v3o4 R 0.999995 k 1", audio, want)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_channels(gpu_lib, N):
    """Every channel of an N-channel run equals a one-channel run on that channel's input."""
    sc = SCENARIOS["p3"]
    x = noise(N, sc["n"], seed=11 + N)
    got = run_sub_scenario(sc, x, engine(sc, GRAV_TRUNC, N))
    assert got.shape == (N, sc["n"])
    for k in range(N):
        o = SubOracle(sc["V"], sc["O"], sc["decay"], RES, sc["harm"], sc["k"], N=1, law=GRAV_TRUNC)
        o.physics_every(sc["period"])
        want = run_sub_scenario(sc, x[k:k + 1], o)
        check_audio(f"p3 N {N} restatement, channel {k} as", got[k:k + 1], want)
        single = run_sub_scenario(sc, x[k:k + 1], engine(sc, GRAV_TRUNC, 1))
        check_audio(f"p3 N {N} one-channel engine, channel {k} as", got[k:k + 1], single)
    if N > 1:
        assert not np.array_equal(got[0], got[1])


def test_several_waves_and_workgroups(gpu_lib):
    """320 filters: 3 workgroups per channel, voices straddle the 64-lane boundaries (40 does not
    divide 64); both physics paths."""
    want, final, amps = oracle_run("wide", GRAV_FABS, 2, WIDE)
    for tune in (PER_STEP, None):
        g = engine(WIDE, GRAV_FABS, 2, tune)
        audio = run_sub_scenario(WIDE, noise(2, WIDE["n"]), g)
        assert np.array_equal(bits(g.positions()), bits(final)), tune
        check_audio(f"wide tune {tune}", audio, want)


def test_state_across_calls(gpu_lib):
    """One call against calls of 1, 127, 1, 383 samples; with period 2 a physics step lands on the
    call boundary at sample 128 (and none on the odd ones)."""
    sc = dict(SCENARIOS["v3o4"], events=SCENARIOS["v3o4"]["events"][:3])
    x = noise(2, 512, seed=3)
    whole, parts = engine(sc, GRAV_TRUNC), engine(sc, GRAV_TRUNC)
    for g in (whole, parts):
        for _, _, a, b in sc["events"]:
            g.makenote(a, b)
    y = whole.process(x)
    cuts = np.cumsum([0, 1, 127, 1, 383])
    z = np.concatenate([parts.process(np.ascontiguousarray(x[:, a:b])) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
    assert np.array_equal(bits(whole.positions()), bits(parts.positions()))
    assert np.array_equal(bits(whole.amplitudes()), bits(parts.amplitudes()))
    check_audio("split 1/127/1/383 against one call", z, y)
    assert np.abs(y).max() > 1e-6


def test_unused_voice_is_gated_off(gpu_lib):
    """Three notes on four voices: the fourth voice never sounds or ticks."""
    sc = dict(SCENARIOS["v3o4"], V=4)
    want, final, amps = oracle_run("v4o4_unused", GRAV_TRUNC, 2, sc)
    g = engine(sc, GRAV_TRUNC)
    audio = run_sub_scenario(sc, noise(2, sc["n"]), g)
    assert amps[3] == 0.0 and g.amplitudes()[3] == 0.0
    assert np.array_equal(bits(g.positions()), bits(final))
    check_audio("unused fourth voice", audio, want)


def test_released_voice_keeps_sounding(gpu_lib):
    """v3o4 releases its second note at sample 200: the amplitude decays, the filters go on."""
    sc = SCENARIOS["v3o4"]
    g = engine(sc, GRAV_TRUNC)
    x = noise(2, sc["n"])
    audio = run_sub_scenario(sc, x, g)
    want, _, amps = oracle_run("v3o4", GRAV_TRUNC)
    a = g.amplitudes()
    assert np.array_equal(bits(a), bits(amps))
    assert 0.0 < a[1] < 0.5 * 0.2          # released, decaying, not zero
    check_audio("v3o4 after endnote", audio[:, 200:], want[:, 200:])


def test_stolen_voice_keeps_filter_state(gpu_lib):
    """steal: the third note takes over a sounding voice at sample 100; were its filters reset there
    the samples after it would differ from the restatement, which never calls forget()."""
    sc = SCENARIOS["steal"]
    g = engine(sc, GRAV_TRUNC)
    audio = run_sub_scenario(sc, noise(2, sc["n"]), g)
    want, final, _ = oracle_run("steal", GRAV_TRUNC)
    assert np.array_equal(bits(g.positions()), bits(final))
    check_audio("steal after the steal", audio[:, 100:], want[:, 100:])


def test_fold_above_nyquist(gpu_lib):
    """makenote(110, ...) with 8 overtones: mtof(110) 8 = 37.6 kHz folds to 18.8 kHz."""
    sc = dict(V=1, O=8, decay=0.9, harm=1.0, k=0.01, period=0, n=256, events=[(0, 0, 110.0, 1.0)])
    want, _, _ = oracle_run("fold", GRAV_TRUNC, 1, sc)
    audio = run_sub_scenario(sc, noise(1, sc["n"]), engine(sc, GRAV_TRUNC, 1))
    check_audio("pitch 110, 8 overtones", audio, want)


def test_zero_input_gives_zero_output(gpu_lib):
    sc = SCENARIOS["v3o4"]
    g = engine(sc, GRAV_TRUNC)
    audio = run_sub_scenario(sc, np.zeros((2, sc["n"])), g)
    assert np.all(audio == 0.0)
    assert g.amplitudes().max() > 0.1


def test_physics_off_stops_the_motion(gpu_lib):
    sc = SCENARIOS["v3o4"]
    g = engine(sc, GRAV_TRUNC)
    for _, _, a, b in sc["events"][:3]:
        g.makenote(a, b)
    g.process(noise(2, 64))
    moved = g.positions()
    g.physics_every(0, GRAV_TRUNC)
    y = g.process(noise(2, 64, seed=5))
    assert np.array_equal(bits(g.positions()), bits(moved))
    assert np.abs(y).max() > 0


def test_single_physics_step_between_blocks(gpu_lib):
    sc = dict(SCENARIOS["p3"], period=0)
    x = noise(2, 128, seed=9)
    o = SubOracle(sc["V"], sc["O"], sc["decay"], RES, sc["harm"], sc["k"], N=2, law=GRAV_FABS)
    g = engine(sc, GRAV_FABS)
    for b in (o, g):
        for _, _, a, amp in sc["events"]:
            b.makenote(a, amp)
    want0, got0 = o.process(x[:, :64]), g.process(np.ascontiguousarray(x[:, :64]))
    before = g.positions()
    o.physics()
    g.physics(GRAV_FABS)
    assert np.array_equal(bits(g.positions()), bits(o.positions()))
    assert not np.array_equal(bits(g.positions()), bits(before))
    want1, got1 = o.process(x[:, 64:]), g.process(np.ascontiguousarray(x[:, 64:]))
    check_audio("single step", np.concatenate([got0, got1], axis=1), np.concatenate([want0, want1], axis=1))


def test_peek_does_not_advance(gpu_lib):
    sc = dict(SCENARIOS["p3"], period=0)
    x = noise(2, 32, seed=13)
    a, b = engine(sc, GRAV_TRUNC), engine(sc, GRAV_TRUNC)
    for g in (a, b):
        for _, _, p, amp in sc["events"]:
            g.makenote(p, amp)
    y = a.process(x)
    z = np.zeros_like(y)
    for t in range(32):
        first = b.peek(x[:, t])
        assert np.array_equal(first, b.peek(x[:, t]))
        z[:, t] = b.process(np.ascontiguousarray(x[:, t:t + 1]))[:, 0]
        assert np.array_equal(first, z[:, t])
    assert np.array_equal(y, z) and np.abs(y).max() > 0


def test_argument_checks(gpu_lib):
    from huygens_amd import HZError, Subtractive
    from huygens_amd._lib import HZ_E_INVALID, HZ_E_UNSUPPORTED
    g = Subtractive(2, 3, 0.75)
    for call in (lambda: g.physics_every(2, 0), lambda: g.physics(3), lambda: g.physics_every(-1, GRAV_TRUNC)):
        with pytest.raises(HZError) as e:
            call()
        assert e.value.code == HZ_E_INVALID
    with pytest.raises(HZError) as e:
        Subtractive(2, 3, 0.75, channels=9)
    assert e.value.code == HZ_E_UNSUPPORTED
    assert g.process(np.zeros((2, 0))).shape == (2, 0)


def test_cpp_dropin(gpu_lib, tmp_path):
    """tests/cpp/subtractive_dropin.cpp: the reference programs' loop, through process() and through
    the per-sample operator() / physics() / tick()."""
    r = build_sub_dropin()
    assert r.returncode == 0, r.stderr[-3000:]
    x = noise(2, 1024, seed=21)
    x.tofile(os.path.join(tmp_path, "sub_in.bin"))
    p = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "subtractive dropin ok" in p.stdout, p.stdout + p.stderr
    o = SubOracle(7, 7, 0.7, 0.999995, 1.0, 1.0, N=2, law=GRAV_TRUNC)
    o.physics_every(32)
    o.makenote(48, 1.0)
    o.makenote(55.3, 0.6)
    o.makenote(60.1, 0.8)
    first = o.process(x[:, :512])
    o.endnote(55.3)
    want = np.concatenate([first, o.process(x[:, 512:])], axis=1)
    for name in ("sub_block", "sub_sample"):
        got = np.fromfile(os.path.join(tmp_path, name + ".bin")).reshape(2, 1024)
        check_audio(f"dropin {name}", got, want)
