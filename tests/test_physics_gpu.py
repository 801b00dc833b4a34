"""GPU: Minimizer::physics() on the device (hz_minimizer.hip) against the op-for-op restatement
(tests/oracle_phys.py) and the reference's own recorded positions (tests/golden/physics_ref.npz).

Positions are compared as uint64 (bit for bit), under both gravity laws and on both physics paths
(one workgroup running every step; one launch per step, forced with tune_physics).  Audio is held to
the project's norm-wise criterion rel_err < 1e-5; the engine differs from the
restatement only in exp2 / sinpi against libm's pow / sin and in summing before scaling."""
import os

import numpy as np
import pytest

from oracle import rel_err
from oracle_phys import GRAV_FABS, GRAV_TRUNC, SCENARIOS, PhysAdditive, run_scenario

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "physics_ref.npz")
LAWS = [GRAV_TRUNC, GRAV_FABS]
PER_STEP = (1, 64)      # tune_physics: no bank takes the single-workgroup path, 64-thread tiles

_cache = {}


def oracle_run(name, law, sc=None):
    """(audio, track, final positions) of a scenario's restatement, computed once per (name, law)"""
    if (name, law) not in _cache:
        audio, track, o = run_scenario(sc or SCENARIOS[name], law)
        for a in (audio, track):
            a.setflags(write=False)
        _cache[name, law] = (audio, track, o.positions())
    return _cache[name, law]


def engine(sc, law, tune=None):
    from huygens_amd import Additive
    g = Additive(sc["V"], sc["O"], sc["decay"], sc["harm"], sc["k"])
    if tune:
        g.tune_physics(*tune)
    g.physics_every(sc["period"], law)
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("tune", [None, PER_STEP], ids=["one_group", "per_step"])
@pytest.mark.parametrize("law", LAWS, ids=["trunc", "fabs"])
def test_positions_bit_exact(gpu_lib, law, tune):
    sc = SCENARIOS["v3o4"]
    g = engine(sc, law, tune)
    audio, _, _ = run_scenario(sc, law, g)
    ref_audio, track, final = oracle_run("v3o4", law)
    assert np.array_equal(bits(g.positions()), bits(final))
    assert np.abs(final - track[0]).max() > 0.05      # they moved
    if law == GRAV_TRUNC:
        assert np.array_equal(bits(g.positions()), bits(np.load(GOLD)["v3o4_track"][-1]))
    assert rel_err(audio, ref_audio) < 1e-5


@pytest.mark.parametrize("tune", [None, PER_STEP], ids=["one_group", "per_step"])
def test_steal_reinitialises_particles(gpu_lib, tune):
    sc = SCENARIOS["steal"]
    g = engine(sc, GRAV_TRUNC, tune)
    run_scenario(sc, GRAV_TRUNC, g)
    assert np.array_equal(bits(g.positions()), bits(oracle_run("steal", GRAV_TRUNC)[2]))
    assert np.array_equal(bits(g.positions()), bits(np.load(GOLD)["steal_track"][-1]))


WIDE = dict(V=4, O=40, decay=0.75, harm=1.0, k=0.1, period=2, n=128,
            events=[(0, 0, 48.0, 1.0), (0, 0, 48.3, 0.5), (0, 0, 55.1, 0.8), (0, 0, 60.2, 0.6)])


def test_several_waves_and_tiles(gpu_lib):
    """160 particles: 3 workgroups of 64 on the per-step path, 3 waves on the one-workgroup path, 3 groups
    of the audio kernel; voices straddle the tile boundaries (40 does not divide 64)."""
    ref_audio, track, final = oracle_run("wide", GRAV_FABS, WIDE)
    assert np.abs(final - track[0]).max() > 0.05
    for tune in (PER_STEP, None):
        g = engine(WIDE, GRAV_FABS, tune)
        audio, _, _ = run_scenario(WIDE, GRAV_FABS, g)
        assert np.array_equal(bits(g.positions()), bits(final)), tune
        assert rel_err(audio, ref_audio) < 1e-5


def test_audio_against_restatement(gpu_lib):
    """rel_err < 1e-5 asked.  Measured on MI355X: 4.7e-13 to 5.4e-13 over the three
    scenarios and both laws (v3o4 5.4e-13, steal 4.8e-13, p3 4.9e-13)."""
    for name in ("v3o4", "steal", "p3"):
        for law in LAWS:
            g = engine(SCENARIOS[name], law)
            audio, _, _ = run_scenario(SCENARIOS[name], law, g)
            err = rel_err(audio, oracle_run(name, law)[0])
            print(f"physics audio {name} law {law}: rel_err {err:.3e}")
            assert err < 1e-5


def test_call_splitting(gpu_lib):
    sc = dict(SCENARIOS["v3o4"], events=SCENARIOS["v3o4"]["events"][:3])
    whole, parts = engine(sc, GRAV_TRUNC), engine(sc, GRAV_TRUNC)
    for g in (whole, parts):
        for _, _, a, b in sc["events"]:
            g.makenote(a, b)
    y = whole.fill(512)
    z = np.concatenate([parts.fill(m) for m in (1, 7, 64, 300, 140)])
    assert np.array_equal(bits(whole.positions()), bits(parts.positions()))
    assert np.array_equal(y, z)
    assert np.abs(y).max() > 0.01


@pytest.mark.parametrize("period,n", [(3, 128), (1, 64)])
def test_schedule_periods(gpu_lib, period, n):
    sc = dict(SCENARIOS["p3"], period=period, n=n)
    o = PhysAdditive(sc["V"], sc["O"], sc["decay"], sc["harm"], sc["k"], law=GRAV_TRUNC)
    o.physics_every(period)
    g = engine(sc, GRAV_TRUNC)
    for b in (o, g):
        for _, _, a, amp in sc["events"]:
            b.makenote(a, amp)
    track = []
    ref = o.fill(n, track)
    assert len(track) == sum(1 for T in range(n) if T >= period and T % period == 0)
    got = g.fill(n)
    assert np.array_equal(bits(g.positions()), bits(o.positions()))
    assert rel_err(got, ref) < 1e-5
    if period == 3:
        assert np.array_equal(bits(g.positions()), bits(np.load(GOLD)["p3_track"][-1]))


def test_mode_switch_to_static(gpu_lib):
    """physics_every(0): the static engine renders from the positions as moved."""
    sc = SCENARIOS["p3"]
    o = PhysAdditive(sc["V"], sc["O"], sc["decay"], sc["harm"], sc["k"], law=GRAV_FABS)
    o.physics_every(2)
    g = engine(dict(sc, period=2), GRAV_FABS)
    for b in (o, g):
        for _, _, a, amp in sc["events"]:
            b.makenote(a, amp)
    assert rel_err(g.fill(100), o.fill(100)) < 1e-5
    moved = o.positions()
    g.physics_every(0, GRAV_FABS)
    o.physics_every(0)
    assert rel_err(g.fill(3000), o.fill(3000)) < 1e-8
    assert np.array_equal(bits(g.positions()), bits(moved))
    # and back on: the device state was kept
    g.physics_every(2, GRAV_FABS)
    o.physics_every(2)
    assert rel_err(g.fill(64), o.fill(64)) < 1e-5
    assert np.array_equal(bits(g.positions()), bits(o.positions()))


def test_per_sample_path_equals_block(gpu_lib):
    from huygens_amd import Additive
    sc = SCENARIOS["p3"]
    block = engine(dict(sc, period=2), GRAV_TRUNC)
    single = Additive(sc["V"], sc["O"], sc["decay"], sc["harm"], sc["k"])
    for g in (block, single):
        for _, _, a, amp in sc["events"]:
            g.makenote(a, amp)
    y = block.fill(64)
    z = np.zeros(64)
    for T in range(64):
        z[T] = single.peek()
        if T >= 2 and T % 2 == 0:
            single.physics(GRAV_TRUNC)
        assert single.fill(1)[0] == z[T]
    assert np.array_equal(y, z)
    assert np.array_equal(bits(block.positions()), bits(single.positions()))


def test_sharded_handle_unsupported(gpu_lib):
    from huygens_amd import Additive, HZError
    from huygens_amd._lib import HZ_E_INVALID, HZ_E_UNSUPPORTED
    a = Additive(2, 8, 0.75, shard=(0, 4))
    with pytest.raises(HZError) as e:
        a.physics_every(2, GRAV_TRUNC)
    assert e.value.code == HZ_E_UNSUPPORTED
    with pytest.raises(HZError) as e:
        a.physics(GRAV_FABS)
    assert e.value.code == HZ_E_UNSUPPORTED
    whole = Additive(2, 8, 0.75)
    with pytest.raises(HZError) as e:
        whole.physics_every(2, 0)
    assert e.value.code == HZ_E_INVALID
