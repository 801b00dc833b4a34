"""CPU: the Subtractive restatement (tests/oracle_sub.py) against plain forms of what it restates,
and the ABI / Python / C++ boundary of the device engine (no compute call is made here)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle_phys import GRAV_TRUNC, SR, mtof
from oracle_sub import Filter, SubOracle, fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "huygens_amd", "lib")
EXE = os.path.join(ROOT, "tests", "cpp", "subtractive_dropin")


def build_sub_dropin():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "subtractive_dropin.cpp"), "-o", EXE, "-L", LIB, "-lhuygens_hip",
           f"-Wl,-rpath,{LIB}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_ring_filter_equals_direct_form_biquad():
    """One gated-on voice, physics off: every filter's ring output equals the direct form
    y = (g x - b1 y1) + ((-g) x2 - b2 y2) with the coefficients of the preceding tick, bit for bit."""
    o = SubOracle(1, 3, 0.75, 0.9999, 1.0, 0.001, N=1, law=GRAV_TRUNC)
    o.makenote(57.0, 1.0)
    x = np.random.default_rng(1).standard_normal(300)
    taps = [[] for _ in range(3)]
    coefs = [[] for _ in range(3)]
    for t in range(300):
        for j in range(3):
            f = o.filters[j]
            if o.amps[0]:
                coefs[j].append((f.forward[0], f.back[1], f.back[2]))
                taps[j].append(f(float(x[t])))
        o([float(x[t])])
        o.tick()
    for j in range(3):
        y1 = y2 = x1 = x2 = 0.0
        assert len(taps[j]) == 299          # sample 0 precedes the first tick: amplitude 0, not computed
        for (g, b1, b2), xt, want in zip(coefs[j], x[1:], taps[j]):
            y = (g * xt - b1 * y1) + ((-g) * x2 - b2 * y2)
            assert y == want
            y2, y1, x2, x1 = y1, y, x1, float(xt)
    assert max(abs(v) for v in taps[0]) > 0


def test_never_activated_voice_keeps_zero_state():
    o = SubOracle(2, 3, 0.75, N=2, law=GRAV_TRUNC)
    o.makenote(60.0, 1.0)
    o.process(np.random.default_rng(2).standard_normal((2, 64)))
    for k in range(2):
        for j in range(3):
            f = o.filters[k * 6 + 3 + j]     # voice 1
            assert f.origin == 0 and not f.computed
            assert f.output == [0.0] * 4 and f.history == [0.0] * 4
            assert f.forward == [1.0, 0.0, 0.0]
            g = o.filters[k * 6 + j]         # voice 0 ran
            assert any(g.output) and g.forward[2] == -g.forward[0]


def test_frequency_above_nyquist_is_folded():
    top = mtof(110) * 8
    assert 37000 < top < 38000
    assert fold(top) == top / 2 and 18000 < fold(top) < 19000
    assert fold(24000.0) == 24000.0 and fold(24000.5) == 12000.25
    o = SubOracle(1, 8, 0.75, N=1, law=GRAV_TRUNC)
    o.makenote(110, 1.0)
    o.process(np.zeros((1, 2)))
    f = fold(mtof(o.x[7]))
    assert f < SR / 2
    assert o.filters[7].back[1] == -2 * o.resonance * math.cos(2 * 3.14159265359 * f / SR)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(LIB, "libhuygens_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-j8", "-C", ROOT, "lib"], check=True)
    from huygens_amd import load
    return load()


SUB_NAMES = ["hz_sub_create", "hz_sub_destroy", "hz_sub_request", "hz_sub_release", "hz_sub_makenote",
             "hz_sub_endnote", "hz_sub_physics_every", "hz_sub_physics", "hz_sub_process", "hz_sub_process_device",
             "hz_sub_positions", "hz_sub_amplitudes", "hz_sub_set_stream", "hz_sub_tune_physics", "hz_sub_profile",
             "hz_sub_profile_read"]


def test_sub_symbols_exported_and_bound(lib):
    from huygens_amd import header_symbols
    from huygens_amd._lib import _SIGS
    syms = [s for s in header_symbols() if s.startswith("hz_sub_")]
    assert not [s for s in SUB_NAMES if s not in syms]
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in syms if s not in exported]
    assert not [s for s in syms if s not in _SIGS]


def test_create_without_gpu_fails_loudly(lib):
    if lib.hz_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    h = C.c_void_p()
    assert lib.hz_sub_create(3, 4, 2, 0.75, 0.99999, 1.0, 0.1, 0, C.byref(h)) == -4   # HZ_E_NODEV
    assert b"no CPU fallback" in lib.hz_last_error()
    assert not h.value


def test_invalid_arguments_rejected_without_device(lib):
    h = C.c_void_p()
    args = (0.75, 0.99999, 1.0, 0.1, 0, C.byref(h))
    assert lib.hz_sub_create(0, 4, 2, *args) == -1      # voices < 1
    assert lib.hz_sub_create(3, 1, 2, *args) == -1      # overtones < 2
    assert lib.hz_sub_create(3, 4, 0, *args) == -1      # channels < 1
    assert lib.hz_sub_create(3, 4, 9, *args) == -6      # HZ_E_UNSUPPORTED: more than 8 channels
    assert not h.value
    assert lib.hz_sub_destroy(None) == 0
    assert lib.hz_sub_physics_every(None, 32, 1) == -1
    assert lib.hz_sub_physics(None, 1) == -1


def test_python_class_exported():
    import huygens_amd
    assert "Subtractive" in huygens_amd.__all__
    assert huygens_amd.Subtractive.__module__ == "huygens_amd.subtractive"


def test_cpp_dropin_builds(lib):
    r = build_sub_dropin()
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]


def test_cpp_header_standalone(tmp_path):
    src = tmp_path / "one.cpp"
    src.write_text('#include "soundmath/subtractive.h"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
