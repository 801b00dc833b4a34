"""The restatements against the reference's own compiled output (CPU).

tests/golden/ref_*.npz were written by the reference's classes themselves (oracle/_ref/hz_ref_dump,
see tests/golden/make_golden_ref.py); everything else in tests/golden/ comes from our own
restatements.  Here the C oracle, driven through the Oracle* bindings over each fixture's own
schedule, must reproduce the reference BIT FOR BIT: both are scalar code built with FP
contraction off against the same libm, and every class measured so (largest |oracle - reference|
over all fixtures: 0.0), so no class needs a bound.

The numpy spec (tests/golden/spec_additive.py) is vectorised: numpy's own sin, `**` and pairwise
np.sum stand where the reference calls libm and adds in index order, a legitimate libm and
ordering effect, so it cannot be bit-equal.  Largest |spec - reference| measured over the
Additive and Sinusoids fixtures: 2.387e-15 (ref_sinusoids_o7_inharm; the others 1.4e-16 to
4.4e-16, outputs of magnitude <= 1); the bound is 8 x that, SPEC_TOL = 1.91e-14.  The spec's
scalar functions (relaxation, mtof, ftom) are bit-equal.
"""
import os
import sys

import numpy as np
import pytest

import ref_driver as R
from oracle import ROOT, golden_names, load_golden

NAMES = golden_names("ref_")
SPEC_TOL = 8 * 2.387e-15
LARGEST_FIXTURE = 163 * 1024   # dly_bank_f.npz
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))   # spec_additive imports spec_numpy as a sibling


def test_fixture_set():
    """every class of the pin has its fixture, tagged and data only"""
    classes = {str(load_golden(n)["cls"]) for n in NAMES}
    assert classes == {"scalars", "wave", "oscillator", "synth", "sinusoids", "additive", "delay", "bowl", "granulator"}
    for n in NAMES:
        g = load_golden(n)   # allow_pickle=False: arrays and names only
        assert str(g["made_by"]) == "reference"
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) <= LARGEST_FIXTURE


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_reference(name):
    g = load_golden(name)
    got = R.oracle_outputs(g)
    assert got
    for key, val in got.items():
        print(f"{name} {key}: max |oracle - reference| = {R.max_abs_diff(val, g[key]):.3e}")
        assert R.bit_equal(val, g[key]), (name, key, R.max_abs_diff(val, g[key]))


def test_fixtures_reach_their_branches():
    """known answers that show the table's cases do what their comments say"""
    g = load_golden("ref_granulator_p4")
    assert g["voices"].tolist() == [0, 1, 2, 3, -1, -1, 0]    # refused, size == 0, voice 0 reused
    assert np.all(g["y"][:11] == 0) and np.any(g["y"][11:] != 0)
    g = load_golden("ref_scalars_all")
    assert g["relaxation_y"][0] == 0.0 and g["relaxation_y"][-1] == 0.0 and g["mtof_y"][4] == 440.0
    g = load_golden("ref_wave_shapes")
    p = g["phase"]
    assert g["y"][2][p == 0.5] == 0.0 and np.all(np.abs(g["y"][2][p != 0.5]) == 1.0)   # square
    assert np.all(g["y"][1] >= -1.0) and np.any(g["y"][1] > 0.0)                      # triangle: the floating abs
    for name in ("ref_delay_l1_d", "ref_delay_l3_f"):
        g = load_golden(name)
        assert g["bt"][0][0] == 0 and g["bg"][0][0] != 0           # a zero-time feedback tap is asked for ...
        x, y = g["x"][0].astype(np.float64), g["y"][0].astype(np.float64)
        assert y[0] == x[0] * g["fg"][0][0]                        # ... and dropped: y[0] = 1.0 x[0], no 0.4 y[0]
    for name in golden_names("ref_additive"):
        g = load_golden(name)
        assert np.all(g["y"][0] == 0) and np.any(g["y"][2100:2600] != 0) and np.any(g["y"][4000:] != 0)
    for name in golden_names("ref_bowl"):
        g = load_golden(name)
        assert np.array_equal(g["y_render"][1700:1800], g["y_render"][:100])   # trigger() restarts the strike
        assert np.array_equal(g["y_fill"], g["y_render"].astype(np.float32))


def _spec_events(g, table):
    return [(int(t), table[int(k)], (float(a), float(b))) for t, k, a, b in
            zip(g["ev_t"], g["ev_kind"], g["ev_a"], g["ev_b"])]


@pytest.mark.parametrize("name", golden_names("ref_additive") + golden_names("ref_sinusoids"))
def test_numpy_spec_reproduces_reference(name):
    from spec_additive import additive_run, sinusoids_run
    g = load_golden(name)
    n = int(g["n"])
    if str(g["cls"]) == "additive":
        ev = _spec_events(g, {R.MAKENOTE: "makenote", R.ENDNOTE: "endnote", R.REQUEST: "request", R.RELEASE: "release"})
        ev = [(t, kind, (int(a[0]),) if kind == "release" else a) for t, kind, a in ev]
        y = additive_run(int(g["V"]), int(g["O"]), float(g["decay"]), float(g["harm"]), float(g["k"]), ev, n)
    else:
        ev = _spec_events(g, {R.FUNDMOD: "fundmod", R.DECAYMOD: "decaymod", R.HARMMOD: "harmmod"})
        ev = [(t, kind, a[0]) for t, kind, a in ev]
        y = sinusoids_run(float(g["fund"]), int(g["O"]), float(g["decay"]), float(g["harm"]), float(g["k"]), ev, n)
    err = R.max_abs_diff(y, g["y"])
    print(f"{name}: max |spec - reference| = {err:.3e}")
    assert err < SPEC_TOL


def test_numpy_spec_scalars():
    from spec_additive import ftom, mtof
    from spec_numpy import relaxation
    g = load_golden("ref_scalars_all")
    assert R.bit_equal(np.array([relaxation(float(k)) for k in g["relaxation_x"][:-1]]), g["relaxation_y"][:-1])
    assert R.bit_equal(np.array([mtof(float(m)) for m in g["mtof_x"]]), g["mtof_y"])
    assert R.bit_equal(np.array([ftom(float(f)) for f in g["ftom_x"]]), g["ftom_y"])


def test_oracle_builds_without_the_reference(tmp_path):
    """a machine without the reference's sources (the GPU machine): `make -C oracle` says so in one
    line, succeeds, still builds the oracle library and leaves no _ref/ behind"""
    import shutil
    import subprocess
    src = os.path.join(ROOT, "oracle")
    dst = tmp_path / "oracle"
    dst.mkdir()
    for f in os.listdir(src):
        if f == "Makefile" or f.endswith((".c", ".h")):
            shutil.copy(os.path.join(src, f), dst / f)
    shutil.copytree(os.path.join(src, "ref"), dst / "ref")
    r = subprocess.run(["make", "-s", "-C", str(dst), f"REF_SRC={tmp_path / 'absent'}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len(r.stdout.strip().splitlines()) == 1 and "no reference sources" in r.stdout
    assert (dst / "_build" / "libhz_oracle.so").exists() and not (dst / "_ref").exists()
    for stub in ("portaudio.h", "RtMidi.h", os.path.join("Eigen", "Dense")):
        assert os.path.getsize(dst / "ref" / "stubs" / stub) == 0
