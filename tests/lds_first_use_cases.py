"""The child side of tests/test_lds_first_use_gpu.py: `python lds_first_use_cases.py CASE` builds
one library object as the first in its process, runs it against its reference and prints one
`err <value>` line per comparison.  Inputs, references and comparisons are those of the tests that
already cover the objects (named per case); the bounds are asserted by the parent."""
import os
import sys

try:  # one HIP runtime per process: let torch-ROCm load it first (see huygens_amd/_lib.py)
    import torch  # noqa: F401
except Exception:
    pass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cosine():
    """test_stft_spectrum_gpu.py::test_cosine_every_size at lg = 13 (dct2_kernel / dct3_kernel, 128 KB)"""
    import scipy.fft
    from huygens_amd import Cosine
    from test_stft_spectrum_gpu import peak_err
    lg = 13
    N = 1 << lg
    c = Cosine(N)
    x = np.random.default_rng(600 + lg).standard_normal(N)
    c.inp[:] = x
    c.forward()
    yield peak_err(c.out, scipy.fft.dct(x, type=2))
    z = np.random.default_rng(700 + lg).standard_normal(N)
    c.out[:] = z
    c.backward()
    yield peak_err(c.inp, scipy.fft.dct(z, type=3))


def stft_p4():
    """test_stft_spectrum_gpu.py::test_gates_nonstationary[N4096-l4-real-static]: stft_pair4096_kernel"""
    import stft_spec as sp
    from huygens_amd.stft import StaticSTFT
    from test_stft_spectrum_gpu import in_calls, peak_err
    case, = [c for c in sp.GATE_CASES if (c.N, c.laps, c.cplx) == (4096, 4, False)]
    ref = sp.gate_run(case, "static")
    assert ref.margin >= sp.MARGIN_MIN
    f = StaticSTFT(case.N, case.laps)
    y = in_calls(f, sp.gate_input(case), sp.gate_cuts(case.n, case.N, case.laps))
    assert f.frames()[0] == len(ref.starts)
    yield peak_err(y, ref.y)


def freezer():
    """test_freezer_gpu.py::test_freeze_cycles_vs_oracle's input and events at N = 8192, the largest"""
    from test_freezer_gpu import run_both
    N, laps = 8192, 4
    rng = np.random.default_rng(N + laps)
    t = np.arange(40000)
    x = 0.3 * np.sin(2 * np.pi * 440 * t / 48000) + 0.05 * rng.standard_normal(t.size)
    blocks = [(5000, [(0, 0), (3000, 1)]), (7000, [(2500, 0), (2501, 1), (6000, 1)]), (1, [(0, 0)]),
              (12000, [(4000, 1), (9000, 0)]), (15999, [])]
    gy, oy = run_both(N, laps, 1.0, x, blocks, seed=N)
    assert np.max(np.abs(oy)) > 0
    yield float(np.max(np.abs(gy - oy)) / np.max(np.abs(oy)))   # peak_close's ratio


def bowl():
    """test_bowl_gpu.py::test_c5_shape's model at M = 303, T = double: one fill of 2048 samples (float
    samples), then a render of as many (double samples, test_golden's bound)"""
    from huygens_amd import Bowl
    from oracle import rel_err
    from oracle_bowl import OracleBowl
    M, n = 303, 2048
    rng = np.random.default_rng(M)
    f = np.exp(rng.uniform(np.log(20.0), np.log(16000.0), M))
    a = rng.uniform(1e-4, 5e-2, M)
    d = rng.uniform(0.05, 15.0, M)
    g, o = Bowl(M, f, a, d, np.float64), OracleBowl(M, f, a, d, np.float64)
    yield rel_err(g.fill(n), o.fill(n))
    yield rel_err(g.render(n), o.render(n))


if __name__ == "__main__":
    for err in {"cosine": cosine, "stft_p4": stft_p4, "freezer": freezer, "bowl": bowl}[sys.argv[1]]():
        print(f"err {float(err)!r}", flush=True)
