"""GPU: tests/cpp/phasebank_dropin.cpp -- the reference's phase vocoder (tests/phasebank.cpp: 48
channels, multiplicity 1, both banks open) over include/soundmath/harmbank.h, twelve blocks of
BSIZE = 32 once through operator() and once through process().  The program dumps its
configuration and input; both outputs are compared with the restatement (tests/oracle_chains.py)
at the PHASE chain's bound (device atan2 / hypot), and with each other bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from huygens_amd.heterodyne import phasebank
from oracle_chains import OraclePhase
from test_cpp_cpu import LIB, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tests", "cpp", "phasebank_dropin")
TOL_DEVICE = 1e-9


def build_phasebank():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "phasebank_dropin.cpp"), "-o", EXE, "-L", LIB, "-lhuygens_hip",
           f"-Wl,-rpath,{LIB}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_phasebank_dropin(gpu_lib, tmp_path):
    r = build_phasebank()
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "phasebank_dropin ok" in p.stdout, p.stdout + p.stderr

    def load(name):
        return np.fromfile(os.path.join(tmp_path, "phase_" + name + ".bin"), dtype=np.float64)
    fa, fs, radii, x, y_op, y_blk = (load(k) for k in ("fa", "fs", "radii", "x", "y_op", "y_blk"))
    # the program's configuration is phasebank()'s
    n, pfa, pfs, pradii = phasebank()
    assert fa.size == n == 48
    assert np.allclose(fa, pfa, rtol=1e-14) and np.allclose(fs, pfs, rtol=1e-14)
    assert np.allclose(radii, pradii, rtol=1e-14)
    o = OraclePhase(n, 1, radii, 0.0005, 0.2, 2400, 1, -0.9, 0.0, 3.0, record=True)
    o.freqmod(0, np.arange(n), fa)
    o.freqmod(1, np.arange(n), fs)
    o.open(0)
    o.open(1)
    want = o.process(x)
    # every latch opens.  This instrument's +-partial pairs cancel in the mix for a real input
    # (conjugate Slidebank outputs, opposite angles), so its output is small; the smoothbank taps,
    # which do not cancel, are compared as well
    assert np.array(o.trace["engaged"])[-1].all() and np.max(np.abs(want)) > 1e-5
    assert np.array_equal(y_op, y_blk)
    err = np.max(np.abs(y_blk - want)) / np.max(np.abs(want))
    stick, ostick = load("stick"), o.state(5)
    err_stick = np.max(np.abs(stick - ostick)) / np.max(np.abs(ostick))
    print(f"phasebank drop-in: output {err:.3e}, smoothbank {err_stick:.3e}")
    assert np.max(np.abs(ostick)) > 0.1
    assert err <= TOL_DEVICE and err_stick <= TOL_DEVICE
