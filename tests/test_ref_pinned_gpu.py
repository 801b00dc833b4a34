"""GPU parity: the HIP engines against the reference's own compiled output, no oracle in between.

tests/golden/ref_*.npz hold what the reference's classes computed (tests/golden/make_golden_ref.py);
every other GPU parity test compares an engine with our own restatement of the reference, so a
misreading shared by restatement and kernel would pass there.  Each engine runs the fixture's own
schedule, split into several calls at the event times.  Tolerances are those of the engine's
existing golden test: Bowl 1e-9 (double) and 1e-5 (float buffer), Delaybank exact, Additive and
Sinusoids 1e-8, Granulator 1e-12 of the peak with the voices equal.  Reads only tests/golden/.
"""
import numpy as np
import pytest

import ref_driver as R
from oracle import golden_names, load_golden, rel_err
from oracle_osc import run_note_events

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("groups", [1, 256])
@pytest.mark.parametrize("name", golden_names("ref_bowl"))
def test_bowl(gpu_lib, name, groups):
    """Bowl<double>: operator()/tick() as render(), and fill(float*), in n // 3, 1, rest with a
    trigger() mid-run"""
    from huygens_amd import Bowl
    g = load_golden(name)
    for method, key, tol in (("render", "y_render", 1e-9), ("fill", "y_fill", 1e-5)):
        b = Bowl(int(g["M"]), g["f"], g["a"], g["d"], np.float64)
        b.set_target_groups(groups)
        err = rel_err(R.run_bowl(b, g, method), g[key])
        print(f"{name} {method} groups {groups}: rel err {err:.3e}")
        assert err < tol


@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("name", golden_names("ref_delay"))
def test_delaybank(gpu_lib, name, split):
    """Delay<double> / Delay<float> lines: taps past the ring, a dropped zero-time feedback tap,
    modulate_forward / modulate_back between calls, bare tick()s -- bit for bit"""
    from huygens_amd import Delaybank

    def bank(*args):
        b = Delaybank(*args)
        b.set_split(split)
        return b

    g = load_golden(name)
    y = R.run_delay(bank, g)
    assert y.dtype == g["y"].dtype
    assert np.array_equal(y, g["y"])


@pytest.mark.parametrize("name", golden_names("ref_additive"))
def test_additive(gpu_lib, name):
    from huygens_amd import Additive
    g = load_golden(name)
    a = Additive(int(g["V"]), int(g["O"]), float(g["decay"]), float(g["harm"]), float(g["k"]))
    err = rel_err(run_note_events(a, g), g["y"])
    print(f"{name}: rel err {err:.3e}")
    assert err < 1e-8


@pytest.mark.parametrize("name", golden_names("ref_sinusoids"))
def test_sinusoids(gpu_lib, name):
    from huygens_amd import Sinusoids
    g = load_golden(name)
    s = Sinusoids(float(g["fund"]), int(g["O"]), float(g["decay"]), float(g["harm"]), float(g["k"]))
    err = rel_err(run_note_events(s, g), g["y"])
    print(f"{name}: rel err {err:.3e}")
    assert err < 1e-8


class _Chunked:
    """fill(n) as a run of shorter calls: single samples (operator()/tick(), served from the
    speculative block), calls just below and at its threshold, longer ones"""

    def __init__(self, obj, sizes=(1, 1, 1, 7, 63, 64, 1, 300, 2, 1000)):
        self.obj, self.sizes, self.i = obj, sizes, 0

    def __getattr__(self, name):
        return getattr(self.obj, name)

    def fill(self, n):
        parts = []
        while n:
            m = min(n, self.sizes[self.i % len(self.sizes)])
            self.i += 1
            parts.append(self.obj.fill(m))
            n -= m
        return np.concatenate(parts)


@pytest.mark.parametrize("name", golden_names("ref_sinusoids") + golden_names("ref_additive"))
def test_call_sizes(gpu_lib, name):
    """the same fixtures through per-sample and short calls: a modulator's relaxation (k = 0.01 s in
    ref_sinusoids_o5_slow: 480 samples) and a note's attack run across many call boundaries"""
    from huygens_amd import Additive, Sinusoids
    g = load_golden(name)
    if str(g["cls"]) == "sinusoids":
        o = Sinusoids(float(g["fund"]), int(g["O"]), float(g["decay"]), float(g["harm"]), float(g["k"]))
    else:
        o = Additive(int(g["V"]), int(g["O"]), float(g["decay"]), float(g["harm"]), float(g["k"]))
    err = rel_err(run_note_events(_Chunked(o), g), g["y"])
    print(f"{name} in short calls: rel err {err:.3e}")
    assert err < 1e-8


def test_synth_through_sinusoids(gpu_lib):
    """The oscillator / synth path on its own: no Python class fronts a bare Synth, but
    Sinusoids(f, 1, decay 1, harmonicity 1, k = 0) is one -- one overtone of weight
    pow(1, 0) / 1, relaxation(0) = 0 so fundmod(t) reaches freqmod(t * pow(1, 1)) on the same
    tick -- and must equal the reference's Synth<double>(&cycle, f) under freqmod steps."""
    from huygens_amd import Sinusoids
    g = load_golden("ref_synth_freqsteps")
    assert float(g["phi"]) == 0.0 and float(g["k"]) == 2.0 / 48000 and set(g["ev_kind"].tolist()) == {R.FREQMOD}
    s = Sinusoids(float(g["f"]), 1, 1.0, 1.0, 0.0)
    as_fundmod = dict(g, ev_kind=np.full_like(g["ev_kind"], R.FUNDMOD))
    err = rel_err(run_note_events(s, as_fundmod), g["y"])
    print(f"ref_synth_freqsteps: rel err {err:.3e}")
    assert err < 1e-8


@pytest.mark.parametrize("name", golden_names("ref_granulator"))
def test_granulator(gpu_lib, name):
    """polyphony 4: a refused request, size == 0, the offset clamp, speeds 1, 2, -1, a grain ending
    at ticks == sizes; one call per stretch between request times"""
    from huygens_amd import Granulator
    g = load_golden(name)
    n = int(g["n"])
    cuts = [0] + [t for t in R.split_points(g) if t > 0] + [n]
    y, voices = R.run_granulator(Granulator(int(g["size"]), int(g["P"])), g, np.diff(cuts).tolist())
    assert voices.tolist() == g["voices"].tolist()
    peak = float(np.max(np.abs(g["y"])))
    err = float(np.max(np.abs(y - g["y"]))) / peak
    print(f"{name}: max err / peak {err:.3e}")
    assert err <= 1e-12
