"""GPU: tests/cpp/mac_bits.cpp -- the stationary engine's MAC kernels (huygens_amd/csrc/hz_fb_mac.h)
launched on their own: resp_mac_kernel<8, QP> (operands in registers) and resp_mac_kernel_lds<QP>
(operands staged through LDS, in the stages the library builds) on seeded random H and Z, QP in {8,
16, 24} x Q in {QP - 7, QP - 1, QP} x B in {1, 8, 31, 32, 33, 65}: every Y element byte-equal, no
row past B written, and a sample of bins byte-equal to the same FMAs on the host.  One program, one
run (kH = 2048 bins, at most 65 output blocks)."""
import os
import subprocess

import pytest

from test_cpp_cpu import ROOT

pytestmark = pytest.mark.gpu
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "cpp", "mac_bits.cpp")


def test_mac_kernels_agree_bit_for_bit(gpu_lib, tmp_path):
    exe = str(tmp_path / "mac_bits")
    r = subprocess.run([HIPCC, "-x", "hip", "-std=c++17", "-O3", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-Wno-pass-failed", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "mac_bits ok" in p.stdout, p.stdout + p.stderr
