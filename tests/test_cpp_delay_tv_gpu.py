"""GPU: tests/cpp/ambi_dropin.cpp -- the reference's ambisonic demo (tests/ambi.cpp: twelve
Delay<double>(1, SR) lines whose tap moves every sample) over include/soundmath/delay.h, 2048
samples in blocks of 32 through Delaybank::process_stream.  The program dumps the tap stream it
computed; the stream is replayed through the oracle per sample (modulate_forward, one sample), so
no sqrt or cos is recomputed here, and the twelve line outputs are compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from delay_tv_model import oracle_tv
from oracle_delay import OracleDelaybank
from test_cpp_cpu import LIB, ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tests", "cpp", "ambi_dropin")
LINES, SAMPLES, SR = 12, 2048, 48000


def build_ambi():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "ambi_dropin.cpp"), "-o", EXE, "-L", LIB, "-lhuygens_hip",
           f"-Wl,-rpath,{LIB}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_ambi_dropin_bit_exact(gpu_lib, tmp_path):
    r = build_ambi()
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ambi_dropin ok" in p.stdout, p.stdout + p.stderr

    def load(name, dtype):
        return np.fromfile(os.path.join(tmp_path, name + ".bin"), dtype=dtype).reshape(LINES, SAMPLES)
    x, y, fg = load("ambi_x", np.float64), load("ambi_y", np.float64), load("ambi_fg", np.float64)
    ft = load("ambi_ft", np.uint32)
    # the taps move (Doppler): a static bank could not pass
    assert all(np.unique(ft[l]).size > 50 for l in range(LINES))
    assert int(ft.max()) < SR and np.all(fg > 0)
    o = OracleDelaybank(LINES, 1, SR, np.float64)
    want = oracle_tv(o, x, ft[:, None, :], fg[:, None, :])
    assert np.all(np.abs(want).max(axis=1) > 1e-4)   # every line sounds within the run
    assert np.array_equal(y, want)
