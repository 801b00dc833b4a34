"""GPU parity: the PHASE and STICKS chains and the output stage of the heterodyne engine
(het_phase_kernel, het_sticks_kernel, het_mix_kernel) against tests/oracle_chains.py.

PHASE: analysis, synthesis, Slidebank, RMS sums, history and latch flags hold only IEEE-exact
operations and are compared bit for bit.  The smoothbank state and the output sit behind the
device's atan2 and hypot: max|gpu - oracle| / max|oracle| <= 1e-9, the project's bound for audio
behind device transcendentals.  STICKS and the output stage: 1e-12 relative (the channel sum's
order, device atan / hypot within the gate margin asserted in tests/test_het_chains_cpu.py).
The cases are tests/het_chain_cases.py; each test prints the figure it measured."""
import functools

import numpy as np
import pytest

from het_chain_cases import (PHASE_CASES, STICKS_CASES, STICKS_GATE, STICKS_RAD, TOTAL, configure,
                             phase_args, phase_oracle, pieces, signal, sticks_oracle)
from oracle_chains import OUT_LIMITER, OUT_RAW, OracleHarm

pytestmark = pytest.mark.gpu
TOL = 1e-12          # the existing chain's tolerance
TOL_DEVICE = 1e-9    # behind device atan2 / hypot
EXACT = (0, 1, 2, 3, 4, 6)   # analysis, synthesis, Slidebank, RMS sums, latch flags, history


def rel(g, o):
    return np.max(np.abs(g - o)) / np.max(np.abs(o))


@functools.lru_cache(maxsize=None)
def phase_reference(case):
    """The restatement's outputs (call by call) and final states, computed once per case."""
    o = phase_oracle(case)
    ys = [o.process(p) for p in pieces(signal(TOTAL, case[-1]))]
    return np.concatenate(ys), {w: o.state(w) for w in range(7)}


@functools.lru_cache(maxsize=None)
def sticks_reference(case, gate):
    o = sticks_oracle(case, gate=gate)
    ys = [o.process(p) for p in pieces(signal(TOTAL, case[-1]))]
    return np.concatenate(ys), {w: o.state(w) for w in (0, 1, 5)}


def gpu_phase(case):
    from huygens_amd import Heterodyne
    N, order, sorder, width, seed = case
    return configure(Heterodyne(*phase_args(N, order, sorder, width, seed), chain="phase"), N, seed)


def gpu_sticks(case, gate):
    from huygens_amd import StickChain
    N, pre, post, seed = case
    return configure(StickChain(N, pre, post, STICKS_RAD, gate, 0.1, 1.0), N, seed)


def states(g, which=range(7)):
    return {w: g.state(w) for w in which}


@pytest.mark.parametrize("case", PHASE_CASES)
def test_phase_vs_oracle(gpu_lib, case):
    from huygens_amd.heterodyne import CHAIN_PHASE
    g = gpu_phase(case)
    assert g.chain() == CHAIN_PHASE
    gy = np.concatenate([g.process(p) for p in pieces(signal(TOTAL, case[-1]))])
    oy, ost = phase_reference(case)
    for w in EXACT:
        assert np.array_equal(g.state(w), ost[w]), f"state {w}"
    assert np.isfinite(gy).all() and np.max(np.abs(oy)) > 1e-2
    e_out, e_stick = rel(gy, oy), rel(g.state(5), ost[5])
    print(f"PHASE {case}: output {e_out:.3e}, smoothbank {e_stick:.3e}")
    assert e_out <= TOL_DEVICE and e_stick <= TOL_DEVICE


@pytest.mark.parametrize("chunk", [None, "37"])
def test_phase_split_calls_equal_one_call(gpu_lib, monkeypatch, chunk):
    """Pieces of 1, 15, 16, 17 and 300 samples equal one call of 349 bit for bit (output and every
    state); likewise with the launch split forced (HZ_HET_CHUNK, as test_launch_splits does)."""
    case = PHASE_CASES[2]
    x = signal(TOTAL, case[-1])
    a = gpu_phase(case)
    ya = np.concatenate([a.process(p) for p in pieces(x)])
    if chunk:
        monkeypatch.setenv("HZ_HET_CHUNK", chunk)
    b = gpu_phase(case)
    yb = b.process(x)
    assert np.array_equal(ya, yb)
    sa, sb = states(a), states(b)
    for w in range(7):
        assert np.array_equal(sa[w], sb[w]), f"state {w}"


def test_phase_reconfigure_between_calls(gpu_lib):
    """freqmod, deactivate and Slidebank::setup between calls (setup zeroes the stages)."""
    case = PHASE_CASES[2]
    N, seed = case[0], case[-1]
    g, o = gpu_phase(case), phase_oracle(case)
    x = signal(3 * 120, seed)
    rng = np.random.default_rng(seed)
    idx, hz = rng.choice(N, 20, replace=False), rng.uniform(100, 3000, 20)
    radii = np.zeros(2 * N)
    radii[0::2], radii[1::2] = 0.7, 0.02
    errs = [rel(g.process(x[:120]), o.process(x[:120]))]
    for h in (g, o):
        h.freqmod(1, idx, hz)
        h.activate(0, idx[:8], on=False)
    errs.append(rel(g.process(x[120:240]), o.process(x[120:240])))
    for h in (g, o):
        h.setup(2, radii)
    errs.append(rel(g.process(x[240:]), o.process(x[240:])))
    for w in EXACT:
        assert np.array_equal(g.state(w), o.state(w)), f"state {w}"
    print(f"PHASE reconfigured: output {max(errs):.3e}")
    assert max(errs) <= TOL_DEVICE and rel(g.state(5), o.state(5)) <= TOL_DEVICE


@pytest.mark.parametrize("gate", [0.0, STICKS_GATE])
@pytest.mark.parametrize("case", STICKS_CASES)
def test_sticks_vs_oracle(gpu_lib, case, gate):
    from huygens_amd.heterodyne import CHAIN_STICKS
    g = gpu_sticks(case, gate)
    assert g.chain() == CHAIN_STICKS
    gy = np.concatenate([g.process(p) for p in pieces(signal(TOTAL, case[-1]))])
    oy, ost = sticks_reference(case, gate)
    for w in (0, 1):
        assert np.array_equal(g.state(w), ost[w]), f"state {w}"
    e_out, e_stick = rel(gy, oy), rel(g.state(5), ost[5])
    print(f"STICKS {case} gate {gate}: output {e_out:.3e}, Stickbanks {e_stick:.3e}")
    assert e_out <= TOL and e_stick <= TOL


def harm_pair(seed=31, N=65):
    from huygens_amd import Heterodyne
    args = phase_args(N, 2, 1, 7, seed)
    return configure(Heterodyne(*args), N, seed), configure(OracleHarm(*args), N, seed)


@pytest.mark.parametrize("shaper,drive,clip", [(OUT_LIMITER, 4.0, 0.9), (OUT_RAW, 0.0, 0.0), (OUT_RAW, 2.5, 0.125)])
def test_output_stage_vs_oracle(gpu_lib, shaper, drive, clip):
    """tests/slidebank.cpp's tail (LIMITER, drive 4, width 0.9) on a HARM handle, and RAW."""
    g, o = harm_pair()
    x = signal(TOTAL, 31)
    for h in (g, o):
        h.set_output(shaper, drive, clip)
    o.record = True
    gy, oy = g.process(x), o.process(x)
    if drive:   # both branches of the softclip are taken
        driven = np.abs(drive * np.array(o.trace["mix"]))
        assert (driven < clip).any() and (driven > clip).any()
    e = rel(gy, oy)
    print(f"output stage ({shaper}, {drive}, {clip}): {e:.3e}")
    assert np.max(np.abs(oy)) > 1e-2 and e <= TOL


def test_default_output_stage_is_the_old_expression(gpu_lib):
    """No set_output call, an explicit default and a second plain handle: the same bits."""
    x = signal(TOTAL, 31)
    a, b, c = harm_pair()[0], harm_pair()[0], harm_pair()[0]
    b.set_output(OUT_LIMITER, 0.0, 0.9)
    ya = a.process(x)
    assert np.array_equal(ya, b.process(x)) and np.array_equal(ya, c.process(x))
    assert np.max(np.abs(ya)) > 1e-2


def test_errors(gpu_lib):
    from huygens_amd import Heterodyne, HZError, StickChain
    from huygens_amd._lib import HZ_E_INVALID, HZ_E_UNSUPPORTED
    for pre, post in [(0, 0), (3, 2), (5, 0), (-1, 2)]:
        with pytest.raises(HZError):
            StickChain(4, pre, post)
    s = StickChain(4, 3, 1)
    for what in (2, 3, 4, 6):   # Slidebank, RMS, latch, history
        with pytest.raises(HZError) as e:
            s.state(what)
        assert e.value.code == HZ_E_INVALID
    with pytest.raises(HZError) as e:
        s.setup(1, np.zeros(8))
    assert e.value.code == HZ_E_UNSUPPORTED
    assert s.state(5).size == 4 * 4 * 2
    for h in (s, Heterodyne(4, 2, np.zeros(8)), Heterodyne(4, 2, np.zeros(8), chain="phase")):
        with pytest.raises(HZError):
            h.set_output(2, 0.0, 0.0)   # a bad shaper
        with pytest.raises(HZError):
            h.set_output(OUT_LIMITER, 4.0, 1.0)   # softclip's (1 - width) divides
    with pytest.raises(ValueError):
        Heterodyne(4, 2, np.zeros(8), chain="sticks")
    with pytest.raises(HZError):
        Heterodyne(4, 9, np.zeros(8), chain="phase")
    assert s.process(np.zeros(0)).size == 0
