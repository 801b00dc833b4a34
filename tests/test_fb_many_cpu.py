"""CPU side of hz_fb_process_many: the three entry points are declared in include/huygens_hip.h,
exported by the library and bound in the Python mirror (as tests/test_abi_cpu.py checks the rest),
and the batch's segment plan (hz::mix_plan_batch, huygens_amd/csrc/hz_mixplan.h) holds on the host:
tests/cpp/many_plan_host.cpp, built plain and with AddressSanitizer + UBSan and run as a program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "many_plan_host.cpp")
NAMES = ["hz_fb_process_many_device", "hz_fb_process_many", "hz_fb_many_info"]


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "huygens_amd", "lib", "libhuygens_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-j8", "-C", ROOT, "lib"], check=True)
    from huygens_amd import load
    return load()


def test_symbols_declared_exported_and_bound(lib):
    from huygens_amd import header_symbols
    from huygens_amd._lib import _SIGS
    syms = header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in syms, f"{name} is not declared in include/huygens_hip.h"
        assert name in exported, f"{name} is not exported"
        assert name in _SIGS and len(_SIGS[name][1]) == (3 if name == "hz_fb_many_info" else 7)


def test_python_wrappers_present():
    import huygens_amd
    from huygens_amd import Filterbank
    assert callable(huygens_amd.process_many) and callable(huygens_amd.process_many_device)
    assert callable(Filterbank.many_info)


def test_null_arguments_rejected_without_device(lib):
    # (the checks come before any handle is touched: no GPU needed)
    assert lib.hz_fb_process_many(None, 0, None, 0, None, 0, 0) == 0
    assert lib.hz_fb_process_many(None, 2, None, 8, None, 8, 8) == -1
    assert lib.hz_fb_process_many_device(None, 300, None, 8, None, 8, 8) == -1
    assert lib.hz_fb_many_info(None, None, None) == -1


def build_and_run(exe, extra):
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + extra + [SRC, "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        return r, None
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return r, subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)


def check(r, run):
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "many plan ok: 341 plans" in run.stdout, run.stdout   # 5 named + 7 lengths x 4 targets x 3 waves x 4 shapes


def test_many_plan_host_program(tmp_path):
    check(*build_and_run(tmp_path / "many_plan_host", ["-O1"]))


def test_many_plan_host_program_sanitized(tmp_path):
    # a stand-alone host program, nothing preloaded
    r, run = build_and_run(tmp_path / "many_plan_host_san",
                           ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and any(n in r.stderr for n in ("asan", "ubsan", "sanitize")):
        pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    check(r, run)
