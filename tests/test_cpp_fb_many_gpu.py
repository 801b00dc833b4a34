"""The C++ drop-in's block call over several banks (tests/cpp/multichannel_block.cpp): the loop of
tests/filterbanks.cpp:191-211 with soundmath::process_many_frames on the callback's interleaved float
buffers (non-zero input and output offsets, a ragged last block), against the same program through
soundmath::sample_many.

Bound: test_rt_server_gpu.py::test_sample_many_cpp_multichannel holds multichannel.cpp's double
outputs to 1e-8 per element.  Here the block route's outputs pass through the callback's float
buffer, which rounds each to 24 bits: at most 2^-24 of its magnitude on top (the per-sample route's
doubles are compared as they are), so |y_block - y_sample| <= (1e-8 + 2^-24) |y_sample|."""
import os
import subprocess

import numpy as np
import pytest

from golden.spec_numpy import resonant_coefficients

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_process_many_frames_cpp_multichannel(gpu_lib, tmp_path):
    H, N, T = 8, 864, 3 * 512 + 300
    fwd, back = resonant_coefficients(N, 0.999, 1.0)
    np.concatenate([np.asarray(fwd)[:, :3], np.asarray(back)[:, :2]], axis=1).astype(np.float64).tofile(tmp_path / "coef.bin")
    x = np.random.default_rng(23).uniform(-1, 1, (T, H))
    x.tofile(tmp_path / "x.bin")
    lib = os.path.join(ROOT, "huygens_amd", "lib")
    exe = str(tmp_path / "multichannel_block")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "multichannel_block.cpp"), "-o", exe, "-L", lib,
                        "-lhuygens_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "multichannel block ok" in p.stdout, p.stdout + p.stderr
    yb = np.fromfile(tmp_path / "y_block.bin").reshape(T, H)
    ys = np.fromfile(tmp_path / "y_sample.bin").reshape(T, H)
    assert np.max(np.abs(ys)) > 1e-3
    worst = float(np.max(np.abs(yb - ys) / np.maximum(1e-30, np.abs(ys))))
    print(f"process_many_frames vs sample_many, 8x864 softclip, {T} frames: worst relative difference {worst:.3e}")
    assert worst <= 1e-8 + 2.0 ** -24, worst
