"""GPU: tests/cpp/octave_dropin.cpp -- long frames through include/soundmath/fourier.h as a reference
program would use them: Fourier(host gate, 16384, 4) driven with write() / read() per sample, and
Cosine(32768) forward then backward.  The program dumps its input; the outputs are compared with
tests/stft_spec.py (the 10 x keep gate of tests/long_stft_cases.py) at 1e-10 of the peak and with
scipy.fft.dct at 1e-13."""
import os
import subprocess

import numpy as np
import pytest
import scipy.fft

import long_stft_cases as lc
import stft_spec as sp
from test_cpp_cpu import LIB, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tests", "cpp", "octave_dropin")
N, LAPS, SAMPLES, DCT = 16384, 4, 2 * 16384 + 40, 32768
TOL = 1e-10


def build_octave():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "octave_dropin.cpp"), "-o", EXE, "-L", LIB, "-lhuygens_hip",
           f"-Wl,-rpath,{LIB}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_octave_dropin(gpu_lib, tmp_path):
    r = build_octave()
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "octave_dropin ok" in p.stdout, p.stdout + p.stderr

    def load(name, n):
        a = np.fromfile(os.path.join(tmp_path, name + ".bin"), dtype=np.float64)
        assert a.shape == (n,)
        return a
    x = load("octave_x", SAMPLES)
    y = load("octave_yr", SAMPLES) + 1j * load("octave_yi", SAMPLES)
    ref = sp.run(x, N, LAPS, 0, lc.proc_keep10)
    assert ref.margin >= sp.MARGIN_MIN and len(ref.starts) == 5
    kept = ref.keep.sum(axis=1)
    assert np.all(kept > 0) and np.all(kept < N)   # the gate passes and stops bins in every frame
    assert np.max(np.abs(ref.y)) > 0.1
    err = float(np.max(np.abs(y - ref.y)) / np.max(np.abs(ref.y)))
    print(f"octave drop-in: {err:.2e} of the peak, margin {ref.margin:.2e}")
    assert err < TOL

    c = load("cosine_x", DCT)
    fwd = scipy.fft.dct(c, type=2)
    back = scipy.fft.dct(fwd, type=3)
    assert np.max(np.abs(load("cosine_fwd", DCT) - fwd)) < 1e-13 * np.max(np.abs(fwd))
    assert np.max(np.abs(load("cosine_back", DCT) - back)) < 1e-13 * np.max(np.abs(back))
