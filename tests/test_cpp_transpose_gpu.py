"""GPU: tests/cpp/demo_dropin.cpp -- the audio callback of the reference's tests/demo.cpp through
include/soundmath/fourier.h: Fourier(HZ_PROC_TRANSPOSE, 32768, 2, 2, 0) driven with write() / read()
per sample over 3N + 5 samples.  The program dumps its input; the output is compared with
tests/stft_spec.py under tests/transpose_cases.py's literal scatter at 1e-10 of the peak."""
import os
import subprocess

import numpy as np
import pytest

import stft_spec as sp
import transpose_cases as tc
from test_cpp_cpu import LIB, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tests", "cpp", "demo_dropin")
N, LAPS, SAMPLES, RATIO = 32768, 2, 3 * 32768 + 5, 2.0
TOL = 1e-10


def build_demo():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "demo_dropin.cpp"), "-o", EXE, "-L", LIB, "-lhuygens_hip",
           f"-Wl,-rpath,{LIB}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_demo_dropin(gpu_lib, tmp_path):
    r = build_demo()
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "demo_dropin ok" in p.stdout, p.stdout + p.stderr

    def load(name):
        a = np.fromfile(os.path.join(tmp_path, name + ".bin"), dtype=np.float64)
        assert a.shape == (SAMPLES,)
        return a
    x = load("demo_x")
    y = load("demo_yr") + 1j * load("demo_yi")
    ref = sp.run(x, N, LAPS, 0, tc.proc_transpose(RATIO))
    assert len(ref.starts) >= 4
    assert np.max(np.abs(ref.y)) > 0.01
    err = float(np.max(np.abs(y - ref.y)) / np.max(np.abs(ref.y)))
    print(f"demo drop-in: {err:.2e} of the peak")
    assert err < TOL
